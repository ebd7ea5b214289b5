"""Seed-anchor cases at the 1000-occurrence rule (TEST INFRASTRUCTURE): pairs in which one k-mer of the query occurs 998, 999,
1000 or 1001 times in the reference sequence, and the match run it lies in is short enough to reason about by hand.

generate_anchors skips a query k-mer whose hash has 1000 reference positions or more (reference: src/chain.cc:61).  Every
builder below returns (q, r, same_chr, delta) pairs and asserts its own premise -- the exact number of hash-equal, N-free
windows of `r` -- with count_by_code, a restatement of the reference's rolling hash (src/chain.cc:28-40) that shares nothing
with tests/bruteforce.py.  Sizes: len(q) <= 400, len(r) <= 40,000 (the model is O(|q| * |r|)).

The layout of every pair:

    q =       xq + S + yq
    r = pad + xr + S + yr + "N" + ("N" + copy) * m

xq / xr end in different bases and yq / yr begin with different bases, so on the FOCUS diagonal (r - q = len(pad)) the match
run is exactly S, or S and yq where a builder says so.  The copies are far away and N-separated: a copy adds exactly the windows
it was written for.  `focus` of a case lists the anchors that the reasoning in the builder's comment expects on that diagonal."""
import collections
import functools
import random

K_VALUES = (8, 11, 15)
COUNTS = (998, 999, 1000, 1001)
CAP = 1000  # src/chain.cc:61
PAD, FLANK = 30, 10

Case = collections.namedtuple("Case", "family k group occ label pair diag focus")

_CODE = {"C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}  # hash_dna (src/common.h:56-69,89): everything else is 0


# ---- independent counts ---------------------------------------------------------------------------------------------------------
def count_by_code(r, w, skip_n=True):
    """Windows of r whose rolling 2-bit hash equals w's, windows with an N left out (src/chain.cc:28-40).  skip_n=False: the
    count a restatement would get that hashed an N like the A it codes as."""
    k = len(w)
    mask = (1 << (2 * k)) - 1
    target = 0
    for c in w:
        target = (target << 2) | _CODE.get(c, 0)
    h, last_n, cnt = 0, -k, 0
    for i, c in enumerate(r):
        if skip_n and c in "Nn":
            last_n = i
        h = ((h << 2) | _CODE.get(c, 0)) & mask
        if i >= k - 1 and last_n < i - k + 1 and h == target:
            cnt += 1
    return cnt


def count_by_string(r, w, fold=True):
    """Windows of r equal to w as strings (fold: case-insensitively)."""
    if fold:
        r, w = r.upper(), w.upper()
    cnt, at = 0, r.find(w)
    while at >= 0:
        cnt += 1
        at = r.find(w, at + 1)
    return cnt


# ---- pieces ---------------------------------------------------------------------------------------------------------------------
def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _not(rng, *bases):
    return rng.choice([b for b in "ACGT" if b not in "".join(bases).upper()])


def _pair(rng, S, copies, tail="", first=None, last=None):
    """The layout of the module docstring.  tail: what follows S in BOTH sequences (the run goes on through it, to the end of q).
    first / last: the first and last base of S as far as the flanks must avoid them (a homopolymer S would gain a window)."""
    first, last = first or S[0], last or (tail or S)[-1]
    a = _not(rng, first)
    b = _not(rng, first, a)
    xq, xr = _seq(rng, FLANK - 1) + a, _seq(rng, FLANK - 1) + b
    if tail:
        yq = yr = tail
    else:
        c = _not(rng, last)
        d = _not(rng, last, c)
        yq, yr = c + _seq(rng, FLANK - 1), d + _seq(rng, FLANK - 1)
    q = xq + S + yq
    r = _seq(rng, PAD) + xr + S + yr + "N" + "".join("N" + c for c in copies)
    assert len(q) <= 400 and len(r) <= 40000, (len(q), len(r))
    return q, r


def _kmers(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def _on(q0, length, has_u=1):
    return (FLANK + q0, FLANK + q0 + PAD, length, has_u)


def _rng(*key):
    return random.Random(repr(key))


# ---- A1: where a run starts --------------------------------------------------------------------------------------------------------
def run_start(k, occ, same_chr=0, off=None, family="A1"):
    """S = unit * 3 and the run goes on through a unique right flank; the copies are the bare unit.  With p = len(unit), the
    k-mers of phase 0 .. p - k lie wholly inside a copy: 3 in S and occ - 3 copies.  Every other k-mer of the run occurs two or
    three times.  Below the cap the anchor starts with the run; at the cap it starts at phase p - k + 1 of the first unit, the
    run's first k-mer under the cap.  (same_chr, off): the pair is on one chromosome and delta puts the focus diagonal `off`
    from the main one -- |off| <= k excludes it, src/chain.cc:67-69.)"""
    rng = _rng("A1", k)
    p = 12 if k <= 11 else 16
    unit, tail = _seq(rng, p), _seq(rng, 2 * FLANK)
    q, r = _pair(rng, unit * 3, [unit] * (occ - 3), tail=tail)
    frequent = _kmers(unit * 2, k)[:p - k + 1]
    assert all(count_by_code(r, w) == occ and count_by_string(r, w) == occ for w in frequent)
    rest = [w for w in _kmers(unit * 3 + tail, k) if w not in frequent]
    assert rest[0] == (unit * 2)[p - k + 1:p + 1] and all(count_by_code(r, w) in (1, 2, 3) for w in rest)
    run = 3 * p + len(tail)
    skip = 0 if occ < CAP else p - k + 1
    focus = [_on(skip, run - skip)]
    delta = 0
    if same_chr:
        delta = off - PAD
        if abs(off) <= k:
            focus = []
    label = "%s k=%d occ=%d" % (family, k, occ) + (" off=%+d" % off if same_chr else "")
    group = "%s k=%d" % (family, k) + (" off=%+d" % off if same_chr else "")
    return Case(family, k, group, occ, label, (q, r, same_chr, delta), PAD, focus)


# ---- A2: frequent k-mers in the middle of a run -----------------------------------------------------------------------------------
def cap_inside_run(k, occ):
    """S = G1 + F + G2 with |F| = k + 2: the three k-mers inside F occur occ times (S and occ - 1 copies of F), the k-mers that
    reach into G1 or G2 once.  ONE anchor over all of S whatever occ is: the k-mers behind F are covered by the anchor that the
    run's first k-mer started, src/chain.cc:72,92."""
    rng = _rng("A2", k)
    G1, F, G2 = _seq(rng, k + 4), _seq(rng, k + 2), _seq(rng, k + 4)
    S = G1 + F + G2
    q, r = _pair(rng, S, [F] * (occ - 1))
    assert all(count_by_code(r, w) == occ and count_by_string(r, w) == occ for w in _kmers(F, k))
    assert all(count_by_code(r, w) == 1 for w in _kmers(S, k) if w not in _kmers(F, k))
    return Case("A2", k, "A2 k=%d" % k, occ, "A2 k=%d occ=%d" % (k, occ), (q, r, 0, 0), PAD, [_on(0, len(S))])


# ---- A3: every k-mer of a run is frequent ---------------------------------------------------------------------------------------
def whole_run_capped(k, occ):
    """S = F alone, |F| = k + 2: below the cap one anchor of length k + 2, at the cap nothing on the diagonal."""
    rng = _rng("A3", k)
    F = _seq(rng, k + 2)
    q, r = _pair(rng, F, [F] * (occ - 1))
    assert all(count_by_code(r, w) == occ and count_by_string(r, w) == occ for w in _kmers(F, k))
    focus = [_on(0, k + 2)] if occ < CAP else []
    return Case("A3", k, "A3 k=%d" % k, occ, "A3 k=%d occ=%d" % (k, occ), (q, r, 0, 0), PAD, focus)


# ---- A4 (and the frame of B and C): the run's first k-mer is frequent, its second and last is not ---------------------------------
def _first_kmer_frame(rng, W, copies, lower=False):
    """S = W + c: W occurs in S and in the copies, the run's other k-mer W[1:] + c once."""
    k = len(W)
    c = _not(rng, W[-1])
    S = (W + c).lower() if lower else W + c
    q, r = _pair(rng, S, copies, first=W[0], last=c)
    assert count_by_code(r, S[1:]) == 1 and count_by_code(q, W) == 1
    return q, r, k


def _first_kmer_focus(k, occ, has_u=1):
    return [_on(0, k + 1, has_u)] if occ < CAP else [_on(1, k, has_u)]


def uncapped_later_kmer(k, occ):
    """A run of exactly k + 1: at the cap the second k-mer alone starts an anchor of length k."""
    rng = _rng("A4", k)
    W = _seq(rng, k)
    q, r, _ = _first_kmer_frame(rng, W, [W] * (occ - 1))
    assert count_by_code(r, W) == occ and count_by_string(r, W) == occ
    return Case("A4", k, "A4 k=%d" % k, occ, "A4 k=%d occ=%d" % (k, occ), (q, r, 0, 0), PAD, _first_kmer_focus(k, occ))


# ---- B: occurrences are counted by code -------------------------------------------------------------------------------------------
def _with_a(rng, k):
    W = list(_seq(rng, k))
    W[k // 2] = "A"
    return "".join(W)


def other_letter_counts_as_a(k, letter, occ):
    """occ - 1 string-equal windows and one copy with `letter` (R, M, r, m: hash_dna codes them 0, like A) where W has an A."""
    rng = _rng("B1", k)
    W = _with_a(rng, k)
    odd = W[:k // 2] + letter + W[k // 2 + 1:]
    copies = [W] * (occ - 2)
    copies.insert(len(copies) // 2, odd)
    q, r, _ = _first_kmer_frame(rng, W, copies)
    by_string, by_code = count_by_string(r, W), count_by_code(r, W)
    assert (by_string, by_code) == (occ - 1, occ), (by_string, by_code)
    return Case("B", k, "B1 k=%d %s" % (k, letter), occ, "B1 k=%d %s by string %d by code %d" % (k, letter, by_string, by_code),
                (q, r, 0, 0), PAD, _first_kmer_focus(k, occ))


def window_with_n_is_left_out(k, copies_written):
    """copies_written windows were written, one of them with an N where W has an A: it is no window at all (src/chain.cc:32-38),
    although the N would hash as the A does."""
    rng = _rng("B2", k)
    W = _with_a(rng, k)
    odd = W[:k // 2] + "N" + W[k // 2 + 1:]
    copies = [W] * (copies_written - 2)
    copies.insert(len(copies) // 2, odd)
    q, r, _ = _first_kmer_frame(rng, W, copies)
    by_string, by_code, hashed = count_by_string(r, W), count_by_code(r, W), count_by_code(r, W, skip_n=False)
    assert (by_string, by_code, hashed) == (copies_written - 1, copies_written - 1, copies_written), (by_string, by_code, hashed)
    occ = by_code
    return Case("B", k, "B2 k=%d" % k, occ, "B2 k=%d by string %d by code %d with N hashed %d" % (k, by_string, by_code, hashed),
                (q, r, 0, 0), PAD, _first_kmer_focus(k, occ))


def both_cases_count_together(k, n_upper, n_lower):
    """n_upper upper-case copies and n_lower lower-case windows (the run itself, lower-case in both sequences, is one of them)."""
    rng = _rng("B3", k)
    W = _with_a(rng, k)
    copies = [W.lower()] * (n_lower - 1) + [W] * n_upper
    q, r, _ = _first_kmer_frame(rng, W, copies, lower=True)
    up, low, by_code = count_by_string(r, W, fold=False), count_by_string(r, W.lower(), fold=False), count_by_code(r, W)
    assert (up, low, by_code) == (n_upper, n_lower, n_upper + n_lower), (up, low, by_code)
    occ = by_code
    return Case("B", k, "B3 k=%d" % k, occ, "B3 k=%d upper %d lower %d by code %d" % (k, up, low, by_code), (q, r, 0, 0), PAD,
                _first_kmer_focus(k, occ, has_u=0))


# ---- C: the same k-mer in three neighbouring pairs of one call --------------------------------------------------------------------
def neighbours(k, kind):
    """Three pairs whose frequent k-mer is the same -- a random one, all A (hash 0) or all T (the largest hash) -- with 999,
    1000 and 999 reference occurrences: in a call that sorts the keys of all its pairs into one array, a k-mer's run of equal
    keys ends where its pair's keys end."""
    W = {"A": "A" * k, "T": "T" * k}.get(kind) or _seq(_rng("C", k), k)
    out = []
    for slot, occ in enumerate((CAP - 1, CAP, CAP - 1)):
        rng = _rng("C", k, kind, slot)
        q, r, _ = _first_kmer_frame(rng, W, [W] * (occ - 1))
        assert count_by_code(r, W) == occ and count_by_string(r, W) == occ
        out.append(Case("C", k, "C k=%d %s" % (k, kind), occ, "C k=%d %s pair %d occ=%d" % (k, kind, slot, occ), (q, r, 0, 0), PAD,
                        _first_kmer_focus(k, occ)))
    return out


# ---- D: the same chromosome --------------------------------------------------------------------------------------------------------
def same_chromosome(k, occ, off):
    return run_start(k, occ, same_chr=1, off=off, family="D")


# ---- the file's cases --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(k):
    out = []
    for build in (run_start, cap_inside_run, whole_run_capped, uncapped_later_kmer):
        out += [build(k, occ) for occ in COUNTS]
    out += [other_letter_counts_as_a(k, letter, CAP) for letter in "RMrm"] + [other_letter_counts_as_a(k, "R", CAP - 1)]
    out += [window_with_n_is_left_out(k, CAP), window_with_n_is_left_out(k, CAP + 1)]
    out += [both_cases_count_together(k, 500, 500), both_cases_count_together(k, 499, 500)]
    for kind in ("A", "random", "T"):
        out += neighbours(k, kind)
    out += [same_chromosome(k, occ, off) for off in (k, k + 1, -k, -(k + 1)) for occ in (CAP - 1, CAP)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(k):
    """The model's answer for every case of k (tests/bruteforce.py), computed once a process."""
    from bruteforce import anchors_bruteforce
    return tuple(tuple(anchors_bruteforce(q, r, k, bool(same), 0, delta)) for (q, r, same, delta) in (c.pair for c in cases(k)))


def on_diagonal(anchors, diag):
    return [a for a in anchors if a[1] - a[0] == diag]

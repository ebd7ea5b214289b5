"""The winnowed minimizers of a sequence and the index over them, as the reference computes them: a literal transcription of
get_minimizers and Index::Index (src/hash.cc:53-141) -- the deque loop with its test of window.back().loc and its pop of the
front kept as they are -- and, next to it, the closed form the device kernels implement (sedef_amd/csrc/minimizers.hip).

A sequence is a bytes object of FASTA characters below 128.  A minimizer is (hash, loc, status); status 0 HAS_UPPERCASE,
1 ALL_LOWERCASE, 2 HAS_N (src/hash.h:22)."""
from collections import deque

import numpy as np

HAS_UPPERCASE, ALL_LOWERCASE, HAS_N = 0, 1, 2
THRESHOLD_NONE = 1 << 31
INDEX_CUTOFF = 0.001  # Globals::Hash::INDEX_CUTOFF (src/globals.cc)

_HASH = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3}
_REV = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCAtgca")}


def rev_comp(s):
    """rc (src/util.cc:43) with rev_dna (src/common.h:72-93): everything that is not ACGTacgt becomes 'N'."""
    return bytes(_REV.get(c & 127, ord("N")) for c in reversed(s))


def keys(s, k, separate_lowercase):
    """(status, hash) of every k-mer start, by definition."""
    out = []
    for j in range(len(s) - k + 1):
        kmer = s[j:j + k]
        h = 0
        for c in kmer:
            h = (h << 2) | _HASH.get(c, 0)
        if any(c in b"Nn" for c in kmer):
            st = HAS_N
        elif any(65 <= c <= 90 for c in kmer):
            st = HAS_UPPERCASE
        else:
            st = ALL_LOWERCASE if separate_lowercase else HAS_UPPERCASE
        out.append((st, h))
    return out


def get_minimizers(s, kmer_size, window_size, separate_lowercase=True):
    """src/hash.cc:53-100, line by line.  Returns [(hash, loc, status)]."""
    minimizers = []
    window = deque()  # of ((status, hash), loc)
    mask = (1 << (2 * kmer_size)) - 1
    h = 0
    last_n = -kmer_size - window_size
    last_u = last_n
    for i in range(len(s)):
        c = s[i]
        if chr(c).upper() == "N":
            last_n = i
        elif 65 <= c <= 90:  # isupper
            last_u = i
        h = ((h << 2) | _HASH.get(c, 0)) & mask
        if i < kmer_size - 1:
            continue
        if last_n >= i - kmer_size + 1:
            status = HAS_N
        elif last_u >= i - kmer_size + 1:
            status = HAS_UPPERCASE
        else:
            status = ALL_LOWERCASE
        if not separate_lowercase and status == ALL_LOWERCASE:
            status = HAS_UPPERCASE
        hh = (status, h)
        while window and not (window[-1][0] < hh):
            window.pop()
        while window and window[-1][1] < (i - kmer_size + 1) - window_size:
            window.popleft()
        window.append((hh, i - kmer_size + 1))
        if i - kmer_size + 1 < window_size:
            continue
        front = window[0]
        if not minimizers or not ((front[1], front[0]) == (minimizers[-1][1], minimizers[-1][0])):
            minimizers.append(front)
    return [(hh[1], loc, hh[0]) for hh, loc in minimizers]


def index(minimizers):
    """Index::Index (src/hash.cc:113-141) over a minimizer list.  Returns (n_groups, threshold, groups): groups as
    [((status, hash), [locs])] in ascending key order (the reference's map is unordered; the order is ours)."""
    idx = {}
    for h, loc, st in minimizers:
        idx.setdefault((st, h), []).append(loc)
    ignore = int((len(minimizers) * INDEX_CUTOFF) / 100.0)
    hist = {}
    for locs in idx.values():
        hist[len(locs)] = hist.get(len(locs), 0) + 1
    total = 0
    threshold = THRESHOLD_NONE
    for size in sorted(hist, reverse=True):
        total += hist[size]
        if total <= ignore:
            threshold = size
        else:
            break
    return len(idx), threshold, sorted(idx.items())


def closed_form_keys(key, w):
    """The closed form over a list of comparable keys: position j is a ROOT when no y in [max(0, j - w), j) has
    key[y] < key[j]; the minimizers are the largest root <= w, then every root > w; none when len(key) <= w.  Returns locs."""
    nk = len(key)
    if nk <= w:
        return []
    roots = [j for j in range(nk) if not any(key[y] < key[j] for y in range(max(0, j - w), j))]
    return [max(j for j in roots if j <= w)] + [j for j in roots if j > w]


def deque_keys(key, w):
    """The deque loop of get_minimizers over a list of keys alone.  Returns locs."""
    out, window = [], deque()
    for j, hh in enumerate(key):
        while window and not (window[-1][0] < hh):
            window.pop()
        while window and window[-1][1] < j - w:
            window.popleft()
        window.append((hh, j))
        if j < w:
            continue
        if not out or window[0] != out[-1]:
            out.append(window[0])
    return [loc for _, loc in out]


def closed_form(s, k, w, separate_lowercase=True):
    """get_minimizers by the closed form.  Returns [(hash, loc, status)]."""
    ks = keys(s, k, separate_lowercase)
    return [(ks[j][1], j, ks[j][0]) for j in closed_form_keys(ks, w)]


def closed_form_np(s, k, w, separate_lowercase=True):
    """The closed form with numpy, for long sequences: an array of (hash, loc, status) rows (int64)."""
    a = np.frombuffer(bytes(s), np.uint8) & 127
    nk = len(a) - k + 1
    if nk <= w:
        return np.zeros((0, 3), np.int64)
    u = a & 0xDF
    code = np.zeros(len(a), np.int64)
    for ch, v in ((65, 0), (67, 1), (71, 2), (84, 3)):
        code[u == ch] = v
    is_n = (u == 78).astype(np.int64)
    is_up = ((a >= 65) & (a <= 90)).astype(np.int64)
    h = np.zeros(nk, np.int64)
    for t in range(k):
        h = (h << 2) | code[t:t + nk]
    cn = np.concatenate([[0], np.cumsum(is_n)])
    cu = np.concatenate([[0], np.cumsum(is_up)])
    has_n = (cn[k:k + nk] - cn[:nk]) > 0
    has_u = (cu[k:k + nk] - cu[:nk]) > 0
    st = np.where(has_n, 2, np.where(has_u, 0, 1 if separate_lowercase else 0)).astype(np.int64)
    key = (st << 32) | h
    big = np.int64(1) << 40
    low = np.full(nk, big)  # the least key among the w positions before j
    pad = np.concatenate([np.full(w, big), key])
    for d in range(1, w + 1):
        low = np.minimum(low, pad[w - d:w - d + nk])
    root = np.flatnonzero(low >= key)
    head = root[root <= w].max()
    loc = np.concatenate([[head], root[root > w]])
    return np.stack([h[loc], loc, st[loc]], 1)

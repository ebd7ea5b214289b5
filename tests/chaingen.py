"""Anchor sets of a WANTED size for the chaining tests, and the launch classes of sdf_chain_batch (test infrastructure).

The two families of test_chain_oracle._chain_cases, each with an explicit number of anchors m:
  * lattices: coordinates on a grid of step 1, 5 or 10, lengths 11..13 -- equal coordinates and equal scores, so the
    tree's tie rules decide.  The span follows from m: an anchor links to one that ended at most ~24 bases (its weight)
    before it in q and r together, a region of ~290 positions, so m points in a span of 17 sqrt(m) have one such
    neighbour each on average; the span is 5..14 sqrt(m) (at least 20, the least _chain_cases draws; 400..1,100 at 6,000
    anchors), which gives chains AND equal coordinates at every m -- a fixed span of 400..3,000 holds no chain below a
    thousand anchors;
  * real anchors: host.anchors on mutated copies of 60-120 kb with a tandem repeat at k = 11 (thousands of anchors: the
    diagonal, the repeat's parallel diagonals and chance matches), a slice of m consecutive ones in generation order.
The launch classes restate sdf_seed_api.hip: sdf_chain_batch and extz2_geom.h: chain_wave_lds_bytes; what the device granted
for class 5 comes from the library (sdf_last_chain_classes, word 7), never from here."""
import numpy as np

import hostgen

SETTINGS = ((210, 4), (50, 3))  # (max_chain_gap, match_chain_score): the reference's, and a tight one
WAVE_CAPS = (2048, 4096, 8192, 16384, 32768)  # LDS bytes of the launch classes 0..4 of chain_wave_kernel
SPILL_PAIRS = 512  # more pairs of class 5 than this in one call: all of them on the thread-per-pair kernel


def wave_lds_bytes(m):
    """extz2_geom.h: chain_wave_lds_bytes -- 64 m + 32 np2(m) + 640, np2 the next power of two >= m."""
    if m <= 0:
        return 16
    return 64 * m + 32 * (1 << (m - 1).bit_length()) + 640


def launch_class(m, cap5, threads_only=False):
    """0..5: the LDS class of the wavefront kernel a pair of m anchors runs in; 6: the thread-per-pair kernel."""
    if not threads_only:
        for c, cap in enumerate(WAVE_CAPS + (cap5,)):
            if wave_lds_bytes(m) <= cap:
                return c
    return 6


def class_counts(sizes, cap5, threads_only=False):
    """What sdf_last_chain_classes reports (words 0..6) for one call over pairs of these sizes."""
    n = [0] * 7
    for m in sizes:
        n[launch_class(m, cap5, threads_only)] += 1
    if n[5] > SPILL_PAIRS:
        n[6] += n[5]
        n[5] = 0
    return n


def class_tops(cap5):
    """The largest m of each of the classes 0..5."""
    tops, m = [], 0
    for c in range(6):
        while launch_class(m + 1, cap5) <= c:
            m += 1
        tops.append(m)
    return tops


def edge_sizes(cap5):
    """Both sides of every class boundary, 2^k - 1, 2^k, 2^k + 1 for k = 1..11 (the bitonic network's ragged tail and the
    tree's shape change there), and 0, 1, 2."""
    s = {0, 1, 2}
    for t in class_tops(cap5):
        s |= {t, t + 1}
    for k in range(1, 12):
        s |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(s)


def lattice(rng, m, step=None, span=None):
    if step is None:
        step = int(rng.choice([1, 5, 10]))
    if span is None:
        span = min(3000, max(20, int(np.sqrt(max(m, 1)) * rng.uniform(5, 14))))
    side = span // step + 1
    return np.stack([rng.integers(0, side, m) * step, rng.integers(0, side, m) * step, rng.integers(11, 14, m),
                     rng.integers(0, 2, m)], 1).astype(np.int32)


class RealAnchors:
    """Pools of real anchors; take(rng, m): m consecutive ones of a pool that holds as many."""

    def __init__(self, host, rng, lengths=(60_000, 90_000, 120_000)):
        self.pools = []
        for it, n in enumerate(lengths):
            q = hostgen.rseq(rng, n, 0.004 if it % 2 else 0.0)
            r = hostgen.rseq(rng, int(rng.integers(0, 300))) + hostgen.mut(rng, q, 0.04 + 0.02 * it) + \
                hostgen.rseq(rng, int(rng.integers(0, 300)))
            rep = hostgen.rseq(rng, int(rng.integers(6, 15))) * 30
            q, r = q[:200] + rep + q[200:], r[:100] + rep + r[100:]
            self.pools.append(np.array(host.anchors(q, r, 11), np.int32).reshape(-1, 4))
        self.pools.sort(key=len)

    def take(self, rng, m):
        pool = next(p for p in self.pools if len(p) >= m)
        # (every other slice from the pool's start: the tandem repeat's parallel diagonals lie there)
        s = 0 if rng.random() < 0.5 else int(rng.integers(0, len(pool) - m + 1))
        return pool[s:s + m].copy()


def cases_of(rng, real, sizes, shuffle=True, accept=None):
    """One lattice and one slice of real anchors per size, in an order that is not the order of their sizes.  accept(a):
    what the caller wants of a SMALL set (3..32 anchors seldom hold a chain of three by chance): drawn again, up to 64
    times, until it says yes -- a choice of inputs by the oracle's answer, made before anything else sees them."""
    out = []
    for m in sizes:
        for draw in (lambda: lattice(rng, m), lambda: real.take(rng, m)):
            a = draw()
            for _ in range(64 if accept is not None and 3 <= m <= 32 else 0):
                if accept(a):
                    break
                a = draw()
            out.append(a)
    if shuffle:
        out = [out[i] for i in rng.permutation(len(out))]
    return out


def edge_cases(rng, real, cap5, accept=None):
    """The class-edge list: edge_sizes() in both families, shuffled, with further pairs of 0, 1 and 2 anchors in between
    (the launch order -- by class, largest first -- then differs from the pair order everywhere)."""
    out = cases_of(rng, real, edge_sizes(cap5), accept=accept)
    for k, m in enumerate((0, 1, 2, 0, 2, 1, 0, 1)):
        out.insert(3 + 9 * k, lattice(rng, m))
    return out


def check_inputs(cases, results, cap5):
    """The conditions on a list of anchor sets, on the ORACLE's results alone (before the GPU is asked anything).  Size
    groups: the launch classes of a default engine; a pair of fewer than three anchors has no chain of three and
    belongs to no group."""
    groups = {}
    for a, res in zip(cases, results):
        if len(a) >= 3:
            groups.setdefault(launch_class(len(a), cap5), []).append(res)
    assert groups
    for c, rs in sorted(groups.items()):
        long_chain = sum(int(np.diff(r["bounds"][:, 0]).max()) >= 3 for r in rs)
        assert 2 * long_chain >= len(rs), ("chains of three anchors in fewer than half of the pairs", c, long_chain, len(rs))
        assert any(len(np.unique(r["dp"])) < len(r["dp"]) for r in rs), ("no pair with two anchors of equal dp", c)
    linked = sum(int((r["prev"] != -1).sum()) for r in results)
    total = sum(len(a) for a in cases)
    assert 4 * linked >= total, ("fewer than a quarter of the anchors have a predecessor", linked, total)


def shifted(cases, dq, dr):
    out = []
    for a in cases:
        b = a.copy()
        b[:, 0] += dq
        b[:, 1] += dr
        out.append(b)
    return out


def signed_variants(cases):
    """name -> (anchor sets, max_chain_gap, match_chain_score): what only an ordering of the keys as `int` gets right.
    a: every q shifted by -1,000 and every r by -700 (negative and non-negative coordinates side by side); b: a negative
    match_chain_score (every dp negative: each anchor a chain of its own, ordered by dp); b1: a score of -1, whose half is
    0 in C (dp is 0 for an anchor without upper case and -1 with: negative and non-negative SCORES side by side -- among
    negative numbers alone the unsigned order is the signed one); c: coordinates near 10^9 (every sum below 2^31)."""
    return {"a": (shifted(cases, -1000, -700), 210, 4), "b": (cases, 210, -4), "b1": (cases, 210, -1),
            "c": (shifted(cases, 1_000_000_000, 999_000_000), 210, 4)}


def mixed_signs(cases):
    """Pairs whose start coordinates q, or whose tree keys r + l - 1, are negative for some anchors and not for others."""
    n = 0
    for a in cases:
        a = a.astype(np.int64)
        for v in (a[:, 0], a[:, 1] + a[:, 2] - 1):
            n += int(len(v) > 0 and v.min() < 0 <= v.max())
    return n


def has_chain_of_three(oracle):
    """accept() for cases_of: the oracle finds a chain of three anchors under the reference's settings."""
    return lambda a: int(np.diff(oracle.chain_anchors(a, *SETTINGS[0])["bounds"][:, 0]).max()) >= 3


def same(got, res):
    return np.array_equal(got[0], res["path"]) and np.array_equal(got[1], res["bounds"])

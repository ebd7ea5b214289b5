#!/usr/bin/env python3
"""Generates tests/golden/plan_digests.json: what the batch planner (sedef_amd/csrc/sdf_plan.hip: cut_batch + plan_chunk)
plans for a corpus of batches, as the six digests of the library's sdf_debug_plan_dump hook -- the cut's figures, every
PlanTask field, the launch order, the chunks, their launches, the lane figures and records: everything the launcher reads.
No GPU and no reference: the planner is host code and the batches are made here from fixed seeds.

A case is (name, batch, settings): the environment's SDF_* settings, the request, the scoring, the workspace, the LDS limit
and whether the scan gets lane records.  Every case is planned with 0 and with 3 planning threads; the file holds one digest
per (case, threads).  The two are equal except where the case says `two_pass` (the cut in two passes needs scan threads:
other chunk counts and upper bounds, by design).

tests/test_plan_same.py regenerates every batch and asserts its digests: a change of the planner that is meant to leave
every plan as it is must pass it WITHOUT this script being run again.

usage: make_golden_plans.py [--lib PATH] [--check] [--only SUBSTRING] [--dump DIR]
  --lib    another build of the library (to compare two builds)
  --check  compare with the file instead of writing it
  --dump   write every word that goes into the digests of each case into DIR (one file per case and thread count)"""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
THREADS = (0, 3)

SCORE_ONLY, RIGHT, GENERIC_SC, APPROX_MAX, EXTZ_ONLY, REV_CIGAR = 0x01, 0x02, 0x04, 0x08, 0x40, 0x80
# extz2_geom.h / sdf_config.hip: the thresholds the boundary batches stand on
STRIPE_MIN, STRIP_MAX_T, STRIPE_MAX_T, CHAIN_MAX_T, MIXED_MAX_NEED = 400, 512, 254 * 128, 65536, 576


def tasks(qlen, tlen, w=-1, flag=0, zdrop=-1, q_off=0, t_off=0):
    from sedef_amd.extz2 import TASK_DTYPE
    t = np.zeros(len(qlen), TASK_DTYPE)
    t["qlen"], t["tlen"], t["w"], t["flag"], t["zdrop"], t["q_off"], t["t_off"] = qlen, tlen, w, flag, zdrop, q_off, t_off
    return t


def cat(*parts):
    return np.concatenate(parts)


# ---- the batches of tests/test_planner.py ------------------------------------------------------------------------------
def headline(n=100000):
    rng = np.random.default_rng(1)
    return tasks(np.full(n, 1000), 1000 + rng.integers(-25, 25, n), w=128)


def mixture():  # small tasks + 60 heavy + 50 empty
    rng = np.random.default_rng(2)
    n = 80000
    q = rng.integers(1, 220, n)
    tl = np.maximum(1, q + rng.integers(-8, 8, n))
    big = rng.choice(n, 60, replace=False)
    q[big] = rng.integers(1500, 9000, 60)
    tl[big] = q[big] + rng.integers(-100, 100, 60)
    q[rng.choice(n, 50, replace=False)] = 0
    return tasks(q, tl)


def by_request():
    return tasks([500, 500, 500, 500, 3000, 70000], [500, 500, 500, 500, 3000, 300], w=[-1, -1, 64, 64, -1, -1],
                 zdrop=[-1, 100, -1, -1, -1, -1], flag=[0, 0, 0, 2, 0, 0])


def four_for_scorings():
    return tasks([300, 300, 1000, 1000], [300, 300, 1000, 1000], w=[-1, -1, 128, 128])


def banded_eight():
    return tasks([7000, 7000, 3000, 20000, 33000, 1000, 2500, 12000], [7000, 7100, 3100, 20000, 33000, 1000, 2700, 11000],
                 w=[64, 128, 16, 200, 200, 128, 100, 300])


def two_pass():
    rng = np.random.default_rng(5)
    n = 420000
    q = rng.integers(1, 210, n)
    tl = np.maximum(1, q + rng.integers(-6, 6, n))
    big = rng.choice(n, 700, replace=False)
    q[big[:300]] = rng.integers(1200, 6000, 300)
    tl[big[:300]] = q[big[:300]] + rng.integers(-60, 60, 300)
    q[big[300:]] = 500
    tl[big[300:]] = 500 + rng.integers(-10, 10, 400)
    q[rng.choice(n, 40, replace=False)] = 0
    return tasks(q, tl)


def settings_batch():
    rng = np.random.default_rng(7)
    q = np.r_[np.full(2000, 1000), np.full(20, 6000)]
    tl = np.r_[1000 + rng.integers(-25, 25, 2000), np.full(20, 6000)]
    return tasks(q, tl, w=np.r_[np.full(2000, 128), np.full(20, -1)])


def _mm8_like(rng, n):
    q = np.exp(rng.uniform(np.log(200), np.log(20000), n)).astype(np.int64)
    t = np.maximum(1, q + (rng.normal(0, 1, n) * np.sqrt(0.04 * q)).astype(np.int64))
    cut = (np.arange(n) % 20 == 0) & (t > 6000)
    t = np.where(cut, t - rng.integers(1000, 5001, n), t)
    return tasks(q, t, w=rng.choice([64, 128, 256, 512], n))


def mm8_40k():
    return _mm8_like(np.random.default_rng(11), 40000)


def mm8_3k():
    rng = np.random.default_rng(11)
    _mm8_like(rng, 40000)
    return _mm8_like(rng, 3000)


def strip_pairs(cols, trial):  # (the generator's state after `trial` rounds, as the test draws them)
    rng = np.random.default_rng(66 + cols)
    for tr in range(trial + 1):
        n = 6000
        tl = np.exp(rng.uniform(np.log(257), np.log(7000), n)).astype(np.int64)
        if tr % 3 == 0:
            ql = np.exp(rng.uniform(np.log(64), np.log(7000), n)).astype(np.int64)
        elif tr % 3 == 1:
            ql = np.maximum(64, tl + rng.integers(-200, 200, n))
        else:
            ql = np.array([64, 137, 219, 311, 414, 530, 661, 808, 973, 1159])[rng.integers(0, 10, n)]
    return tasks(ql, tl)


# ---- a boundary batch per rule -----------------------------------------------------------------------------------------
def window_needs():
    """Every window need there is, on every route that reads it: bands 1 .. 1100 on tasks whose band reaches the corner
    (wave, exact and mixed pairs: 128/129 .. 1024/1025 slots, kMixedMaxNeed), whose band runs out (TRACK: 192/193, 384/385),
    long ones of both (banded stripes: 192/193), each geometry twice so that it finds its partner and once more alone; and
    full-band tasks whose target, not their band, bounds the window."""
    w = np.arange(1, 1101)
    parts = []
    for q, dt in ((1500, 0), (1500, 40), (5000, 0), (5000, 40)):
        for rep in range(2):
            parts.append(tasks(np.full(len(w), q), q + (w + dt if dt else 0), w=w))
    parts.append(tasks(np.full(len(w), 1501), np.full(len(w), 1501), w=w))
    tl = np.arange(100, 1101)
    parts.append(tasks(np.full(len(tl), 2000), tl))
    parts.append(tasks(np.full(len(tl), 2000), tl, w=2000))
    return cat(*parts)


def target_lengths():
    """Full-band targets on either side of 256, stripe_min (400 and 600), kStripMaxT, kStripeMaxT and kStripChainMaxT, queries of
    63 / 64 / 65 (the strips' shortest) and longer ones, each twice; a banded target of more than 254 stripes of 128."""
    tl = [255, 256, 257, 258, 399, 400, 401, 402, 599, 600, 601, STRIP_MAX_T - 1, STRIP_MAX_T, STRIP_MAX_T + 1, STRIP_MAX_T + 2,
          STRIPE_MAX_T - 1, STRIPE_MAX_T, STRIPE_MAX_T + 1, CHAIN_MAX_T - 1, CHAIN_MAX_T, CHAIN_MAX_T + 1]
    q, t = [], []
    for ql in (63, 64, 65, 300, 3000):
        for x in tl:
            q += [ql, ql]
            t += [x, x]
    full = tasks(q, t)
    banded = tasks([33000, 33000, 32513, 32512], [33000, 32600, 32513, 32512], w=[200, 200, 300, 300])
    return cat(full, banded)


def many_strips(n, seed=21):
    """`n` one-wavefront strip tasks (std::sort below 2,048 keys, the radix sort from there) and enough chains for a launch."""
    rng = np.random.default_rng(seed)
    return tasks(rng.integers(64, 700, n), rng.integers(257, STRIP_MAX_T + 1, n))


def antidiagonals():
    """Banded tasks of 3,999 / 4,000 / 4,001 anti-diagonals (bstripe_min_rows), wide and narrow windows, bands that run out by
    one, just reach the corner, and are wider than needed."""
    q, t, w = [], [], []
    for rows in (3998, 3999, 4000, 4001, 4002):
        for band in (16, 64, 160, 200, 512):
            for d in (0, band - 1, band, band + 1, band + 40):
                ql = (rows + 1 - d) // 2
                q += [ql, ql]
                t += [rows + 1 - ql] * 2
                w += [band, band]
    for d in (63, 64, 65, 66):  # short ones: the band runs out / just reaches the corner
        q += [1000, 1000, 1000 + d]
        t += [1000 + d, 1000 + d, 1000]
        w += [64, 64, 64]
    return tasks(q, t, w=w)


def long_among_chains(n_long):
    """4,000 full-band 1000 x 1000 tasks (chains) and `n_long` of 12,000 rows + columns and more, one of 11,999: up to 64 take
    the stripe kernel."""
    q = np.r_[np.full(4000, 1000), np.full(n_long - 1, 6000), [5999, 5999]]
    t = np.r_[np.full(4000, 1000), np.full(n_long - 1, 6000), [6000, 6001]]
    return tasks(q, t)


def unpaired(n_geom):
    """`n_geom` banded geometries, one task each (self_pair_max), among 1,000 pairs."""
    g = np.arange(n_geom)
    return cat(tasks(600 + g, 600 + g, w=64), tasks(np.full(2000, 500), np.full(2000, 500), w=64))


def class_sizes(n_a, w=128, n_b=100):
    """Two launch classes of one kernel, `n_a` and `n_b` tasks (classes below 2,048 merge when they differ by their LDS size
    alone: the stripe kernel's, w = -1 without the strip kernels), tasks of two sizes in the larger (the longest-first order
    below 8,192)."""
    half = n_a // 2
    q = np.r_[np.full(half, 1000), np.full(n_a - half, 1000), np.full(n_b, 6000)]
    t = np.r_[np.full(half, 1000), np.full(n_a - half, 450), np.full(n_b, 6000)]
    return tasks(q, t, w=w)


def batch_sizes(n, long_task=False):
    rng = np.random.default_rng(31)
    t = tasks(np.full(n, 1000), 1000 + rng.integers(-25, 25, n), w=128)
    if long_task:
        t[n // 2]["qlen"], t[n // 2]["tlen"], t[n // 2]["w"] = 1500, 1500, 128
    return t


# ---- lane batches ------------------------------------------------------------------------------------------------------
def lane_small(n, seed=41):
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 211, n)
    return tasks(q, np.maximum(1, q + rng.integers(-6, 6, n)), flag=rng.choice([0, 0, SCORE_ONLY, REV_CIGAR], n),
                 q_off=rng.integers(0, 1 << 30, n), t_off=rng.integers(0, 1 << 30, n))


def lane_too_few():  # (the scan runs -- the batch is large enough -- and finds 5,000)
    return cat(lane_small(5000), tasks(np.full(15000, 300), np.full(15000, 300)))[np.random.default_rng(42).permutation(20000)]


def lane_refused():
    t = lane_small(20000, 43)
    rng = np.random.default_rng(44)
    t["q_off"][rng.choice(20000, 300, replace=False)] += 1 << 32
    t["t_off"][rng.choice(20000, 300, replace=False)] = (1 << 32) - 1
    sel = rng.choice(20000, 600, replace=False)
    t["w"][sel] = np.maximum(t["qlen"][sel], t["tlen"][sel]) - rng.integers(0, 3, 600)
    t["zdrop"][rng.choice(20000, 300, replace=False)] = rng.integers(0, 200, 300)
    t["flag"][rng.choice(20000, 100, replace=False)] |= RIGHT
    return t


def lane_with_heavy():
    t = lane_small(40000, 45)
    big = np.random.default_rng(46).choice(40000, 60, replace=False)
    t["qlen"][big] = 1500 + 100 * np.arange(60)
    t["tlen"][big] = t["qlen"][big] + 7
    return t


def with_flag(build, flag=0, zdrop=None, every=3):
    def f():
        t = build().copy()
        t["flag"][::every] |= flag
        if zdrop is not None:
            t["zdrop"][::every] = zdrop
        return t
    f.__name__ = "%s+flag%x%s" % (build.__name__, flag, "" if zdrop is None else "z%d" % zdrop)
    return f


ONE_SETTING = [("SDF_FORCE_GENERAL", 1), ("SDF_NO_PAIR", 1), ("SDF_NO_MIXED", 1), ("SDF_NO_STRIPE", 1), ("SDF_NO_STRIP", 1),
               ("SDF_STRIP_ALWAYS", 1), ("SDF_STRIP_COLS", 4), ("SDF_STRIP_COLS", 8), ("SDF_STRIPE_NREG", 1), ("SDF_STRIPE_NREG", 2),
               ("SDF_STRIPE_NREG", 4), ("SDF_STRIPE_MIN", 600), ("SDF_BSTRIPE_ALL", 1), ("SDF_BSTRIPE_NREG", 2),
               ("SDF_BSTRIPE_NREG", 4), ("SDF_BSTRIPE_MIN_ROWS", 0), ("SDF_MIXED_MIN", 0), ("SDF_SELF_PAIR_MAX", 0),
               ("SDF_CHAIN_MIN", 0), ("SDF_CUT_NCH", 3), ("SDF_HEAVY_BYTES", 65536)]
GENERAL_SCORING = dict(mat=(5, -11), gapo=10, gape=0)  # (fresh score bytes out of q .. 127: sdf_api.hip, plan_env)
DEGENERATE = dict(mat="degenerate", gapo=1, gape=1)
GIB = 1 << 30


def corpus():
    """[(name, builder, args of the builder, settings)]; settings: env, want, ws, lds, scoring, lane, two_pass."""
    out = []

    def add(name, build, *args, **kw):
        out.append((name, build, args, kw))

    # tests/test_planner.py, test by test
    add("headline", headline)
    add("mixture", mixture)
    add("request", by_request)
    add("request/pair", lambda: tasks([300, 390], [300, 390]))
    add("request/want7", by_request, want=7)
    add("request/flags", lambda: tasks([300, 300], [300, 300], flag=[4, 8]))
    add("request/degenerate", lambda: tasks([300, 0], [300, 5]), scoring=DEGENERATE)
    for ma, mi, go, ge in ((5, -10, 10, 0), (5, -11, 10, 0), (5, -4, 60, 1), (5, -4, 61, 1), (5, -4, 40, 1)):
        add("request/scoring%d_%d_%d_%d" % (ma, mi, go, ge), four_for_scorings, scoring=dict(mat=(ma, mi), gapo=go, gape=ge))
    add("stripe/one", lambda: tasks([6000], [6000]))
    add("stripe/6000", lambda: tasks([1000] * 6000, [1000] * 6000))
    add("stripe/4000", lambda: tasks([1000] * 4000, [1000] * 4000))
    add("stripe/4000/no_strip", lambda: tasks([1000] * 4000, [1000] * 4000), env={"SDF_NO_STRIP": 1})
    add("stripe/banded", banded_eight)
    add("two_pass", two_pass)
    add("two_pass/early", two_pass, env={"SDF_DEBUG_PLAN_EARLY": 1}, two_pass=True)
    add("settings", settings_batch)
    for var in ("SDF_FORCE_GENERAL", "SDF_NO_PAIR", "SDF_NO_STRIPE"):
        add("settings/" + var, settings_batch, env={var: 1})
    add("mm8_40k", mm8_40k)
    add("mm8_3k", mm8_3k)
    for cols in (0, 4, 8):
        for trial in range(6):
            for ws in (64 * GIB, 2 * GIB, 600 << 20):
                add("strip_pairs/cols%d/trial%d/ws%d" % (cols, trial, ws >> 20), strip_pairs, cols, trial, ws=ws,
                    env={"SDF_STRIP_COLS": cols, "SDF_STRIP_ALWAYS": 1})
    # one setting at a time
    for build in (mm8_40k, mm8_3k, mixture):
        for var, val in ONE_SETTING:
            add("%s/%s=%d" % (build.__name__, var, val), build, env={var: val})
    # requests
    for build in (mm8_3k, mixture, window_needs):
        for want in (2, 3, 7):
            add("%s/want%d" % (build.__name__, want), build, want=want)
        for flag in (SCORE_ONLY, REV_CIGAR, RIGHT, EXTZ_ONLY, GENERIC_SC, APPROX_MAX):
            add("%s/flag%02x" % (build.__name__, flag), with_flag(build, flag))
        add("%s/zdrop100" % build.__name__, with_flag(build, 0, 100))
        add("%s/general_scoring" % build.__name__, build, scoring=GENERAL_SCORING)
        add("%s/degenerate" % build.__name__, build, scoring=DEGENERATE)
    # workspace and LDS
    for build in (headline, mixture, mm8_40k, window_needs, target_lengths):
        for ws in (64 * GIB, 2 * GIB, 600 << 20):
            for lds in (64 << 10, 160 << 10):
                add("%s/ws%d/lds%d" % (build.__name__, ws >> 20, lds >> 10), build, ws=ws, lds=lds)
    # a boundary batch per rule
    for env in ({}, {"SDF_MIXED_MIN": 0}, {"SDF_BSTRIPE_ALL": 1}, {"SDF_NO_PAIR": 1}, {"SDF_NO_MIXED": 1}, {"SDF_SELF_PAIR_MAX": 0}):
        add("window_needs/%s" % "".join("%s=%s" % kv for kv in env.items()), window_needs, env=env)
    for env in ({}, {"SDF_STRIP_ALWAYS": 1}, {"SDF_STRIPE_MIN": 600}, {"SDF_STRIPE_MIN": 600, "SDF_STRIP_ALWAYS": 1}, {"SDF_NO_STRIP": 1},
                {"SDF_NO_STRIPE": 1}, {"SDF_STRIP_ALWAYS": 1, "SDF_STRIP_COLS": 4}, {"SDF_STRIP_ALWAYS": 1, "SDF_STRIP_COLS": 8}):
        name = "".join("%s=%s" % kv for kv in env.items())
        add("target_lengths/%s" % name, target_lengths, env=env)
        add("target_lengths/score_only/%s" % name, with_flag(target_lengths, SCORE_ONLY, every=1), env=env)
    for n in (1023, 1024, 2047, 2048, 5000):
        add("many_strips/%d" % n, many_strips, n)
        add("many_strips/%d/with_chains" % n, lambda n=n: cat(many_strips(n), tasks([1000] * 4000, [1000] * 4000)))
    for env in ({}, {"SDF_MIXED_MIN": 0}, {"SDF_BSTRIPE_MIN_ROWS": 4001}):
        add("antidiagonals/%s" % "".join("%s=%s" % kv for kv in env.items()), antidiagonals, env=env)
    for n_long in (1, 64, 65):
        add("long_among_chains/%d" % n_long, long_among_chains, n_long)
    add("long_among_chains/64/heavy256k", long_among_chains, 64, ws=2 * GIB)
    for n_geom in (511, 512, 513, 514):
        add("unpaired/%d" % n_geom, unpaired, n_geom)
    for n_a in (2046, 2047, 2048, 2050, 8190, 8191, 8192, 8194):
        add("class_sizes/%d" % n_a, class_sizes, n_a)
        add("class_sizes/%d/stripes" % n_a, class_sizes, n_a, -1, env={"SDF_NO_STRIP": 1})
    for n in (2047, 2048, 32767, 32768):
        add("batch_sizes/%d" % n, batch_sizes, n)
    for n in (2047, 2048):
        add("batch_sizes/%d/long" % n, batch_sizes, n, True)
    add("batch_sizes/100/long", batch_sizes, 100, True)
    # lane batches, the scan filling lane records
    add("lane/20000", lane_small, 20000, lane=1)
    add("lane/20000/want2", lane_small, 20000, lane=1, want=2)
    add("lane/20000/want7", lane_small, 20000, lane=1, want=7)
    add("lane/20000/no_records", lane_small, 20000)
    add("lane/20000/ws64m", lane_small, 20000, lane=1, ws=64 << 20)
    add("lane/5000", lane_small, 5000, lane=1)
    add("lane/too_few", lane_too_few, lane=1)
    add("lane/refused", lane_refused, lane=1)
    add("lane/with_heavy", lane_with_heavy, lane=1)
    add("lane/mixture", mixture, lane=1)
    add("lane/two_pass", two_pass, lane=1)
    add("lane/two_pass/early", two_pass, lane=1, env={"SDF_DEBUG_PLAN_EARLY": 1}, two_pass=True)
    add("lane/two_pass/early/lane_min", two_pass, lane=1, env={"SDF_DEBUG_PLAN_EARLY": 1, "SDF_LANE_MIN": 419500}, two_pass=True)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def load(path=None):
    if path:
        lib = C.CDLL(path)
    else:
        import sedef_amd
        lib = sedef_amd.load_library()
    lib.sdf_debug_plan_dump.restype = C.c_int
    lib.sdf_debug_plan_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
    return lib


def plan_digest(lib, t, threads, env=None, want=3, ws=64 * GIB, lds=160 * 1024, scoring=None, lane=0, two_pass=False,
                dump=None, ms=None):
    """The six digests of one plan as one string (or "rc=<error>")."""
    from sedef_amd import extz2
    s = scoring or dict(mat=(5, -4), gapo=40, gape=1)
    mat = np.array([1] + [-100] * 24, np.int8) if s["mat"] == "degenerate" else extz2.sedef_mat(*s["mat"])
    sc = extz2._scoring(mat, s["gapo"], s["gape"])
    dig = np.zeros(6, np.uint64)
    took = C.c_double(0)
    with environment(env or {}):
        rc = lib.sdf_debug_plan_dump(C.byref(sc), t.ctypes.data, len(t), want, ws, lds, threads, lane, dig.ctypes.data,
                                     dump.encode() if dump else None, C.byref(took))
    if ms is not None:
        ms.append(took.value)
    return "rc=%d" % rc if rc else "-".join("%016x" % int(x) for x in dig)


def built(cache, build, args):
    key = (build.__name__, args)
    if build.__name__ == "<lambda>" or key not in cache:
        cache.clear()  # (one batch at a time: consecutive cases share theirs)
        cache[key] = build(*args)
    return cache[key]


def main():
    argv = sys.argv[1:]
    opt = lambda name: argv[argv.index(name) + 1] if name in argv else None
    lib = load(opt("--lib"))
    only, dump = opt("--only"), opt("--dump")
    got, cache = {}, {}
    for name, build, args, kw in corpus():
        if only and only not in name:
            continue
        t = built(cache, build, args)
        for threads in THREADS:
            path = os.path.join(dump, "%s.t%d.bin" % (name.replace("/", "_"), threads)) if dump else None
            got["%s|t%d" % (name, threads)] = plan_digest(lib, t, threads, dump=path, **kw)
    if "--check" in argv:
        want = json.load(open(OUT))
        bad = [k for k in got if got[k] != want.get(k)]
        for k in bad:
            print("DIFFERENT %s\n  file %s\n  now  %s" % (k, want.get(k), got[k]))
        print("%d digests, %d different" % (len(got), len(bad)))
        return 1 if bad else 0
    with open(OUT, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(got), OUT))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""A slice of the hand-run fuzz campaigns (tests/fuzz/, profiles/r0N_fuzz.txt) inside `pytest -m gpu`: 500,000 random tasks,
every kernel of the path forced in turn through the library's configuration struct, twenty scorings -- a third of them on the
edges of the condition that decides between the register-resident kernels' 32-bit differences and the general kernel
(sedef_amd/csrc/sdf_api.hip: plan_env) -- every task's score and every CIGAR word against the CPU checker: the
reference's own ksw_extz2_sse where oracle/_ref travels with the repository (extern/ksw2_extz2_sse.cc compiled unmodified),
else the scalar oracle.  VERDICT r5: the campaigns were logs of scripts run by hand; this is the part of them the driver's own
run carries (budget: about a minute)."""
import concurrent.futures as cf
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

BANDS = np.array([1, 3, 15, 16, 17, 33, 64, 100, 128, 129, 255, 256, 400, 512])


def _scoring(rng, kind):
    """(match, mismatch, gap open, gap extend); kind 0-3: on the edges of the fast kernels' condition (tests/fuzz/fuzz_scorings.py)."""
    go, ge = int(rng.integers(0, 62)), int(rng.integers(0, 6))
    ma, mi = int(rng.integers(1, 14)), -int(rng.integers(1, 16))
    if kind == 0:
        mi = -(go + 2 * ge) if go + 2 * ge > 0 else -1  # mismatch + q + 2 e = 0: the last fast one
    if kind == 1:
        mi = -(go + 2 * ge) - 1  # ... and the first on the general kernel
    if kind == 2:
        ma = 127 - 2 * (go + ge)  # cap = 127
    if kind == 3:
        ma = 128 - 2 * (go + ge)  # cap = 128: the bytes wrap
    if kind in (2, 3) and (ma < 1 or ma > 127):
        go, ge, ma = 40, 1, (45 if kind == 2 else 46)
    if -mi > 2 * (go + ge):
        mi = -min(-mi, max(1, 2 * (go + ge)))  # (else the reference returns at once)
    return ma, max(mi, -128), go, ge


def _fnv_tasks(res, cig):
    """FNV-1a over each task's CIGAR words (what ref_extz2_batch / sdfo_extz2_batch return), all tasks at once."""
    n = len(res)
    h = np.full(n, 1469598103934665603, np.uint64)
    off = res["cigar_off"].astype(np.int64)
    cnt = res["n_cigar"].astype(np.int64)
    words = cig.astype(np.uint64)
    with np.errstate(over="ignore"):
        for j in range(int(cnt.max()) if n else 0):
            live = np.nonzero(cnt > j)[0]
            h[live] = (h[live] ^ words[off[live] + j]) * np.uint64(1099511628211)
    return h


def _cpu_batch(cpu, pool, q_off, qlen, t_off, tlen, w, mat, go, ge, threads=16):
    """The checker over the batch: one call per band value and slice, on `threads` host threads (the C loop releases the GIL)."""
    n = len(qlen)
    score = np.zeros(n, np.int32)
    h = np.zeros(n, np.uint64)
    jobs = []
    for wv in np.unique(w):
        idx = np.nonzero(w == wv)[0]
        # (equal shares of cells, roughly: tasks are in random order)
        for part in np.array_split(idx, max(1, min(threads, len(idx) // 64))):
            if len(part):
                jobs.append((int(wv), part))

    def run(job):
        wv, part = job
        s, hh = cpu.batch(pool, q_off[part], qlen[part], t_off[part], tlen[part], mat=mat, gapo=go, gape=ge, w=wv)
        score[part] = s
        h[part] = hh

    with cf.ThreadPoolExecutor(threads) as ex:
        list(ex.map(run, jobs))
    return score, h


# (label, settings, shape of the batch) -- one context per entry, the settings through sdf_create_cfg
def _banded(rng, n, lo=1, hi=1400, bands=BANDS, spread=200):
    ql = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.int64)
    tl = np.maximum(1, ql + rng.integers(-spread, spread + 1, n))
    return ql, tl, rng.choice(bands, n)


def _full(rng, n, lo=1, hi=600, spread=60):
    ql = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.int64)
    tl = np.maximum(1, ql + rng.integers(-spread, spread + 1, n))
    return ql, tl, np.full(n, -1)


CASES = [
    ("default routing, banded", {}, lambda r, n: _banded(r, n)),
    ("default routing, full band", {}, lambda r, n: _full(r, n)),
    ("one task per wavefront (wave kernel)", dict(SDF_NO_PAIR=1), lambda r, n: _banded(r, n)),
    ("general kernel", dict(SDF_FORCE_GENERAL=1), lambda r, n: _banded(r, n, hi=500)),
    ("pair kernel without mixed pairs", dict(SDF_NO_MIXED=1), lambda r, n: _banded(r, n)),
    ("mixed pairs forced", dict(SDF_MIXED_MIN=2), lambda r, n: _banded(r, n, lo=100, bands=np.array([16, 64, 128, 256, 512]))),
    ("banded stripes, 1 register", dict(SDF_BSTRIPE_MIN_ROWS=100, SDF_BSTRIPE_ALL=1, SDF_BSTRIPE_NREG=1), lambda r, n: _banded(r, n, lo=60)),
    ("banded stripes, 2 registers", dict(SDF_BSTRIPE_MIN_ROWS=100, SDF_BSTRIPE_ALL=1, SDF_BSTRIPE_NREG=2), lambda r, n: _banded(r, n, lo=60)),
    ("banded stripes, 4 registers", dict(SDF_BSTRIPE_MIN_ROWS=100, SDF_BSTRIPE_ALL=1, SDF_BSTRIPE_NREG=4), lambda r, n: _banded(r, n, lo=60)),
    ("full-band stripes, 1 register", dict(SDF_NO_STRIP=1, SDF_STRIPE_MIN=128, SDF_STRIPE_NREG=1), lambda r, n: _full(r, n, lo=100, hi=1500)),
    ("full-band stripes, 2 registers", dict(SDF_NO_STRIP=1, SDF_STRIPE_MIN=128, SDF_STRIPE_NREG=2), lambda r, n: _full(r, n, lo=100, hi=1500)),
    ("full-band stripes, 4 registers", dict(SDF_NO_STRIP=1, SDF_STRIPE_MIN=128, SDF_STRIPE_NREG=4), lambda r, n: _full(r, n, lo=100, hi=1500)),
    ("strips and chains, 4 columns a lane", dict(SDF_STRIP_ALWAYS=1, SDF_STRIP_COLS=4), lambda r, n: _full(r, n, lo=200, hi=2500, spread=150)),
    ("strips and chains, 8 columns a lane", dict(SDF_STRIP_ALWAYS=1, SDF_STRIP_COLS=8), lambda r, n: _full(r, n, lo=200, hi=2500, spread=150)),
    ("lane kernel", dict(SDF_LANE_MIN=1), lambda r, n: _full(r, n, lo=1, hi=250, spread=12)),
    ("small tasks without the lane kernel", dict(SDF_NO_LANE=1), lambda r, n: _full(r, n, lo=1, hi=250, spread=12)),
    ("bands that run out (TRACK flavour)", {}, lambda r, n: _banded(r, n, lo=30, hi=900, bands=np.array([15, 33, 64, 128]), spread=500)),
    ("one chunk on one stream", dict(SDF_PIPELINE=0), lambda r, n: _banded(r, n)),
    ("three chunks forced", dict(SDF_CUT_NCH=3), lambda r, n: _banded(r, n, hi=700)),
    ("no stripe kernels of any kind", dict(SDF_NO_STRIPE=1, SDF_BSTRIPE_MIN_ROWS=0, SDF_NO_STRIP=1), lambda r, n: _banded(r, n, bands=np.array([-1, -1, 64, 256, 512]), hi=900)),
]


def test_fuzz_slice_every_forced_kernel_twenty_scorings(oracle):
    import bench
    import sedef_amd
    from oracle.binding import Reference
    from sedef_amd.extz2 import WANT_CIGAR, WANT_SCORE, sedef_mat
    try:
        cpu, checker = Reference(), "reference kernel"
    except Exception:  # noqa: BLE001  (oracle/_ref not built on this box)
        cpu, checker = oracle, "scalar oracle"
    per_case = int(os.environ.get("SDF_FUZZ_SLICE_TASKS", "25000"))
    seed = int(os.environ.get("SDF_FUZZ_SLICE_SEED", "606"))
    t0 = time.time()
    total = bad = fast = 0
    for ci, (label, settings, shape) in enumerate(CASES):
        rng = np.random.default_rng(seed * 1009 + ci)
        # a scoring per case; kinds 0-3 lie on the edges of the condition.  A case that forces a register-resident kernel draws
        # until its scoring is one those kernels take (kinds 1 and 3 never are: they go with the cases on the default routing
        # and the general kernel, which is where such a scoring runs whatever is forced)
        forced = bool(settings) and "SDF_FORCE_GENERAL" not in settings
        kind = ci % 6
        for _ in range(64):
            ma, mi, go, ge = _scoring(rng, kind)
            qe2 = 2 * (go + ge)
            is_fast = ma + qe2 <= 127 and mi + qe2 <= 127 and ma + qe2 >= go and mi + qe2 >= go
            if is_fast or not forced:
                break
            kind = (0, 2, 4, 5)[int(rng.integers(0, 4))]
        assert is_fast or not forced
        fast += is_fast
        mat = sedef_mat(ma, mi)
        ql, tl, w = shape(rng, per_case)
        div = float(rng.choice([0.02, 0.06, 0.15]))
        pool, q_off, qlen, t_off, tlen = bench.synth_ragged(rng, ql, tl, sub=div, dele=div / 3, ins=div / 3)
        # a few N runs
        for _ in range(200):
            at = int(rng.integers(0, len(pool) - 8))
            pool[at:at + int(rng.integers(1, 8))] = 4
        tasks = np.zeros(per_case, sedef_amd.TASK_DTYPE)
        tasks["q_off"], tasks["t_off"], tasks["qlen"], tasks["tlen"] = q_off, t_off, qlen, tlen
        tasks["w"], tasks["zdrop"] = w, -1
        eng = sedef_amd.Extz2Engine(0, config=settings)
        res, cig = eng.align_batch(tasks, pool, mat=mat, gapo=go, gape=ge, want=WANT_CIGAR | WANT_SCORE)
        eng.close()
        score, h = _cpu_batch(cpu, pool, q_off, qlen, t_off, tlen, np.asarray(w), mat, go, ge)
        got = _fnv_tasks(res, cig)
        wrong = np.nonzero((res["score"] != score) | (got != h))[0]
        total += per_case
        bad += len(wrong)
        assert len(wrong) == 0, "%s, scoring %s: %d of %d tasks differ from the %s, first (qlen, tlen, w) %s" % (
            label, (ma, mi, go, ge), len(wrong), per_case, checker,
            [(int(qlen[k]), int(tlen[k]), int(w[k])) for k in wrong[:5]])
    print("fuzz slice: %d tasks, %d kernel settings, %d scorings (%d on the register-resident kernels), checker = %s, %d bad, %.0f s"
          % (total, len(CASES), len(CASES), fast, checker, bad, time.time() - t0))
    assert total >= 200000 or "SDF_FUZZ_SLICE_TASKS" in os.environ

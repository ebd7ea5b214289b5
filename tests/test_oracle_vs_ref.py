"""CPU: fuzz of the oracle against the reference kernel: live where oracle/_ref/libksw2_ref.so is built, else against
its recorded answers for the same seeded cases (tests/refcalls.py)."""
import numpy as np
import pytest

from oracle.binding import NEG_INF, Reference, mutate, random_codes, sedef_mat
from refcalls import ref_calls
from util import FIELDS


def _same(a, b):
    return all(a[k] == b[k] for k in FIELDS) and np.array_equal(a["cigar"], b["cigar"])


def test_fuzz_sedef_scoring(oracle):
    with ref_calls("oracle_vs_ref_sedef_scoring", Reference) as ref:
        _fuzz_sedef_scoring(oracle, ref)


def _fuzz_sedef_scoring(oracle, ref):
    rng = np.random.default_rng(11)
    for _ in range(3000):
        q = random_codes(rng, int(rng.integers(1, 400)), 0.02 if rng.random() < 0.3 else 0.0)
        d = rng.random() * 0.12
        t = mutate(rng, q, d, d / 3, d / 3)
        if rng.random() < 0.3:
            k, L = int(rng.integers(0, len(t))), int(rng.integers(1, 80))
            t = np.concatenate([t[:k], random_codes(rng, L), t[k:]])
        kw = dict(w=int(rng.choice([-1, 0, 1, 2, 7, 15, 16, 17, 31, 32, 33, 64, 128])),
                  flag=int(rng.choice([0, 0, 0, 2, 0x40, 0x80, 1, 8, 4, 0x18])),
                  zdrop=int(rng.choice([-1, -1, 50, 200])))
        assert _same(oracle.extz2(q, t, **kw), ref.extz2(q, t, **kw)), kw


def test_fuzz_wrapping_scorings(oracle):
    with ref_calls("oracle_vs_ref_wrapping_scorings", Reference) as ref:
        _fuzz_wrapping_scorings(oracle, ref)


def _fuzz_wrapping_scorings(oracle, ref):
    rng = np.random.default_rng(12)
    for _ in range(3000):
        q = random_codes(rng, int(rng.integers(1, 300)), 0.05 if rng.random() < 0.3 else 0.0)
        d = rng.random() * 0.2
        t = mutate(rng, q, d, d / 3, d / 3)
        kw = dict(w=int(rng.choice([-1, 0, 1, 3, 8, 15, 16, 17, 40, 100])),
                  mat=sedef_mat(int(rng.integers(1, 12)), -int(rng.integers(1, 12))),
                  gapo=int(rng.integers(0, 70)), gape=int(rng.integers(0, 6)),
                  flag=int(rng.choice([0, 0, 2, 0x40])))
        assert _same(oracle.extz2(q, t, **kw), ref.extz2(q, t, **kw)), kw


def test_fuzz_generic_matrix_and_approximate_modes(oracle):
    """KSW_EZ_GENERIC_SC with a matrix whose wildcard row / column is not zero, KSW_EZ_APPROX_MAX / APPROX_DROP."""
    with ref_calls("oracle_vs_ref_generic_matrix", Reference) as ref:
        _fuzz_generic_matrix(oracle, ref)


def _fuzz_generic_matrix(oracle, ref):
    rng = np.random.default_rng(13)
    mat = np.array([6, -3, -5, -3, -1, -3, 6, -3, -5, -1, -5, -3, 6, -3, -1, -3, -5, -3, 6, -1, -1, -1, -1, -1, 1], np.int8)
    for _ in range(2000):
        q = random_codes(rng, int(rng.integers(1, 300)), 0.04)
        d = rng.random() * 0.2
        t = mutate(rng, q, d, d / 3, d / 3)
        flag = int(rng.choice([0x04, 0x08, 0x18, 0x0c, 0x1c, 0x48, 0x09, 0x05]))
        kw = dict(w=int(rng.choice([-1, -1, 3, 17, 64])), zdrop=int(rng.choice([-1, 40, 300])), flag=flag,
                  mat=mat if flag & 4 else sedef_mat(), gapo=12, gape=2)
        assert _same(oracle.extz2(q, t, **kw), ref.extz2(q, t, **kw)), kw


def test_early_returns_match_the_reference(oracle):
    """What the reference returns before it does any work (extern/ksw2_extz2_sse.cc:57: a side without a base; :81: a scoring
    with -min_sc > 2 (q + e)), live against oracle/_ref: the GPU tests of the batch entry points take the expected record of
    such a task from the oracle (tests/test_gpu_batch_contract.py).  Skips where the reference kernel was not built."""
    if not Reference.available():
        pytest.skip("oracle/_ref/libksw2_ref.so not built")
    ref = Reference()
    rng = np.random.default_rng(14)
    reset = dict(score=NEG_INF, mqe=NEG_INF, mte=NEG_INF, max=0, max_q=-1, max_t=-1, mqe_t=-1, mte_q=-1, zdropped=0)
    cases = [(random_codes(rng, ql), random_codes(rng, tl), kw) for ql, tl in ((0, 5), (5, 0), (0, 0))
             for kw in (dict(), dict(w=3, zdrop=50, flag=0x40), dict(flag=1))]
    q = random_codes(rng, 50)
    cases.append((q, mutate(rng, q)[:50], dict(mat=sedef_mat(1, -20), gapo=4, gape=2)))  # 20 > 2 (4 + 2)
    for q, t, kw in cases:
        a, b = oracle.extz2(q, t, **kw), ref.extz2(q, t, **kw)
        assert _same(a, b), (len(q), len(t), kw)
        assert all(a[k] == reset[k] for k in FIELDS) and len(a["cigar"]) == 0, (len(q), len(t), kw)

"""Seed anchors at the 1000-occurrence rule (src/chain.cc:61) on the GPU: the cases of tests/anchor_edge_cases.py through
sdf_anchors_batch, its strand form and the view / more forms, against the model (tests/bruteforce.py).  All comparisons are exact.

The rule stands twice in sedef_amd/csrc/anchors.hip: query_lookup_kernel disables a k-mer with 1000 reference positions or more,
and candidates_kernel walks back along a match run to the first k-mer under the cap -- families A1, A2 and A4 are the ones in
which that walk meets a k-mer AT the cap (tests/test_anchor_edges_cpu.py checks that the model answers them as reasoned)."""
import ctypes as C
import random

import numpy as np
import pytest

import anchor_edge_cases as aec
from test_gpu_resident_strand import rc_bytes, rev_table

pytestmark = pytest.mark.gpu


def batch(k):
    """The cases of k in the order of the call, with the model's answers: shuffled once, then family C's triples (999, 1000, 999
    occurrences of one k-mer in neighbouring pairs) moved to the ends -- the all-A k-mer (hash 0) in the call's first pairs, the
    all-T k-mer (the largest hash) in its last ones."""
    cases, exp = aec.cases(k), aec.expected(k)
    triple = {kind: [i for i, c in enumerate(cases) if c.group == "C k=%d %s" % (k, kind)] for kind in ("A", "random", "T")}
    assert all(len(t) == 3 and [cases[i].occ for i in t] == [999, 1000, 999] for t in triple.values())
    rest = [i for i, c in enumerate(cases) if c.family != "C"]
    random.Random(20).shuffle(rest)
    order = triple["A"] + triple["random"] + rest + triple["T"]
    assert sorted(order) == list(range(len(cases)))
    return [cases[i] for i in order], [list(exp[i]) for i in order]


@pytest.fixture(scope="module")
def engine():
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    yield eng
    eng.close()


def resident(cases, stored=None):
    """One pool and the pairs' descriptors; stored[i]: the bytes that lie in the pool for pair i's reference."""
    from sedef_amd.extz2 import ANCHOR_PAIR_DTYPE
    desc = np.zeros(len(cases), ANCHOR_PAIR_DTYPE)
    parts, off = [], 0
    for i, c in enumerate(cases):
        q, r, same, delta = c.pair
        qb = np.frombuffer(q.encode(), np.uint8)
        rb = np.frombuffer(r.encode(), np.uint8) if stored is None else stored[i]
        desc[i] = (off, off + len(qb), len(qb), len(rb), same, delta)
        off += len(qb) + len(rb)
        parts += [qb, rb]
    return np.concatenate(parts), desc


def as_lists(anchors, off):
    return [[tuple(int(x) for x in a) for a in anchors[off[i]:off[i + 1]]] for i in range(len(off) - 1)]


def assert_equal_the_model(cases, got, exp):
    assert len(got) == len(exp)
    for c, g, e in zip(cases, got, exp):
        assert g == e, (c.label, len(g), len(e), aec.on_diagonal(g, c.diag), c.focus)


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_one_batch_call_equals_the_model(engine, k):
    cases, exp = batch(k)
    got = engine.anchors_batch([c.pair for c in cases], k)
    assert_equal_the_model(cases, got, exp)
    assert sum(len(g) for g in got) >= 30000  # (the floor of tests/test_anchor_edges_cpu.py)


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_strand_form_equals_the_model_on_the_meant_sequences(engine, k):
    """Every reference lies reverse-complemented in the pool and is read with r_rc = 1 (kmer_at_rc, ref_char<true>); the pairs
    whose reference holds R or M -- rev_dna makes an N of them, src/common.h:72-86 -- stay forward in the same call."""
    cases, exp = batch(k)
    tab = rev_table()
    stored, r_rc = [], np.zeros(len(cases), bool)
    for i, c in enumerate(cases):
        rb = np.frombuffer(c.pair[1].encode(), np.uint8)
        r_rc[i] = not set(c.pair[1]) & set("RMrm")
        if r_rc[i]:
            rb, meant = rc_bytes(tab, rb), rb
            assert rc_bytes(tab, rb).tobytes() == meant.tobytes()
        stored.append(rb)
    assert (~r_rc).sum() == 5 and all(cases[i].group.startswith("B1") for i in np.flatnonzero(~r_rc))
    pool, desc = resident(cases, stored)
    engine.pool_upload(pool.tobytes())
    got, off = engine.anchors_batch_resident(desc, k, r_rc=r_rc)
    assert_equal_the_model(cases, as_lists(got, off), exp)


def _staged(engine, desc, k, keep=None):
    """sdf_anchors_batch_view (keep is None) or sdf_anchors_batch_more on the resident pool -> (address, anchors there, offsets)."""
    desc = np.ascontiguousarray(desc)
    p, used, offs = C.c_void_p(), C.c_size_t(0), np.zeros(len(desc) + 1, np.int64)
    if keep is None:
        rc = engine.lib.sdf_anchors_batch_view_strand(engine.ctx, desc.ctypes.data, None, len(desc), None, engine.pool_bytes(), k,
                                                      C.byref(p), offs.ctypes.data, C.byref(used))
    else:
        rc = engine.lib.sdf_anchors_batch_more_strand(engine.ctx, desc.ctypes.data, None, len(desc), engine.pool_bytes(), k, keep,
                                                      C.byref(p), offs.ctypes.data, C.byref(used))
    engine._check(rc)
    return p.value, used.value, offs


def _read(address, n):
    from sedef_amd.extz2 import ANCHOR_DTYPE
    return np.frombuffer((C.c_char * (n * 16)).from_address(address), ANCHOR_DTYPE).copy() if n else np.zeros(0, ANCHOR_DTYPE)


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_view_then_more_equals_the_single_call(engine, k):
    cases, exp = batch(k)
    pool, desc = resident(cases)
    engine.pool_upload(pool.tobytes())
    whole, off = engine.anchors_batch_resident(desc, k)
    assert_equal_the_model(cases, as_lists(whole, off), exp)
    # the cut falls between the 999 pair and the 1000 pair of a C triple: the second triple of the front, the last of the call
    for cut in (4, len(cases) - 2):
        assert (cases[cut - 1].family, cases[cut - 1].occ, cases[cut].family, cases[cut].occ) == ("C", 999, "C", 1000)
        assert cases[cut - 1].group == cases[cut].group
        at1, n1, off1 = _staged(engine, desc[:cut], k)
        first = _read(at1, n1)
        at2, n2, off2 = _staged(engine, desc[cut:], k, keep=n1)
        assert at2 == at1 + 16 * n1 and n1 > 0 and n2 > 0
        assert _read(at1, n1).tobytes() == first.tobytes()  # the first half is where and what it was
        assert _read(at1, n1 + n2).tobytes() == whole.tobytes()
        assert np.array_equal(off1, off[:cut + 1]) and np.array_equal(off2 + n1, off[cut:])

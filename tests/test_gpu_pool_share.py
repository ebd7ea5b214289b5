"""One resident pool read by several contexts of a device (sdf_pool_share), and pool offsets beyond 2^31.

A view's answers are compared byte for byte with the owner's own on the same ranges; beyond 2^31 the answers are those of a
fresh context that holds nothing but the small record the tasks, pairs and ranges name."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


def small_record(rng, tab, third=1000):
    """3 * third bases: a soft-masked stretch with N runs and IUPAC letters, a mutated copy of it, and the reverse complement
    of another mutated copy -- so that forward and reverse-strand ranges of the record are related sequences."""
    from test_gpu_resident_strand import fasta_chars, rc_bytes

    def mutated(a):
        b = a.copy()
        sub = rng.random(len(b)) < 0.03
        b[sub] = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, int(sub.sum()))]
        return b
    a = fasta_chars(rng, third)
    a[third // 2:third // 2 + 40] = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, 40)]
    a[5], a[6] = ord("R"), ord("-")
    return np.concatenate([a, mutated(a), rc_bytes(tab, mutated(a))])


def as_fasta(bases, line, end=b"\n", last_end=True):
    """(raw lines, n_bases, line_bases, line_bytes) of one record as a file has it."""
    b = bases.tobytes()
    lines = [b[i:i + line] for i in range(0, len(b), line)]
    return end.join(lines) + (end if last_end else b""), len(b), line, line + len(end)


def work_on(rng, base, n, n_tasks=400):
    """DP tasks on both strands, anchor pairs with and without r_rc and class ranges, all inside pool[base, base + n)."""
    from sedef_amd.extz2 import ANCHOR_PAIR_DTYPE, TASK_DTYPE
    t = np.zeros(n_tasks, TASK_DTYPE)
    ql = np.where(rng.random(n_tasks) < 0.9, rng.integers(1, 211, n_tasks), rng.integers(257, 900, n_tasks))
    tl = np.clip(ql + rng.integers(-6, 7, n_tasks), 1, None)
    t["qlen"], t["tlen"], t["w"], t["zdrop"] = ql, tl, -1, -1
    t["q_off"] = (rng.random(n_tasks) * (n - ql)).astype(np.int64)
    t["t_off"] = (rng.random(n_tasks) * (n - tl)).astype(np.int64)
    # half of them on related ranges: the query in the first third, the target where its mutated copy lies -- forward in the
    # second third, reverse-complemented in the last
    third = n // 3
    strand = rng.integers(0, 4, n_tasks)
    q_rc, t_rc = (strand & 1).astype(bool), (strand & 2).astype(bool)
    for k in range(0, n_tasks, 2):
        L = int(min(ql[k], tl[k], 200))
        o = int(rng.integers(0, third - L))
        t["qlen"][k] = t["tlen"][k] = L
        t["q_off"][k] = o
        q_rc[k] = False
        if k % 4 == 0:
            t["t_off"][k], t_rc[k] = third + o, False
        else:
            t["t_off"][k], t_rc[k] = 2 * third + (third - o - L), True
    t["q_off"] += base
    t["t_off"] += base
    desc = np.zeros(5, ANCHOR_PAIR_DTYPE)
    desc[0] = (base, base + third, third, third, 0, 0)
    desc[1] = (base, base + 2 * third, third, third, 0, 0)
    desc[2] = (base + 100, base + 2 * third + 50, third - 200, third - 100, 1, 7)
    desc[3] = (base, base + third, third, third, 1, third)
    desc[4] = (base + 1, base + n - 333, 500, 333, 0, 0)
    r_rc = np.array([0, 1, 1, 0, 1], np.uint8)
    ranges = [(base, n), (base + 1, 0), (base + 5, 17), (base + n - 1, 1), (base + third - 3, third + 9), (base + 16, 16)]
    return t, q_rc, t_rc, desc, r_rc, ranges


def answers(eng, work):
    """Everything the three kinds of call return, as bytes."""
    t, q_rc, t_rc, desc, r_rc, ranges = work
    res, cig = eng.align_batch_pairs(t, q_rc=q_rc, t_rc=t_rc)
    an, an_off = eng.anchors_batch_resident(desc, 11, r_rc=r_rc)
    an0, an0_off = eng.anchors_batch_resident(desc, 11)
    cls = eng.pool_range_classes(ranges)
    return dict(dp=res.tobytes(), cigar=cig.tobytes(), anchors=an.tobytes(), anchor_off=an_off.tobytes(),
                anchors_fwd=an0.tobytes(), anchor_fwd_off=an0_off.tobytes(), classes=cls.tobytes()), (res, an, an0, cls)


def check_meaningful(parts, work):
    res, an, an0, cls = parts
    t, q_rc, t_rc, desc, r_rc, ranges = work
    assert (res["n_cigar"] > 0).all() and t_rc.any() and q_rc.any()
    related = np.arange(0, len(t), 2)
    for sel in (related[0::2], related[1::2]):  # the forward and the reversed targets were found (N runs aside)
        assert (res["matches"][sel] >= 0.8 * t["qlen"][sel]).mean() > 0.5
    assert len(an) > 5 and len(an0) > 5 and an.tobytes() != an0.tobytes()
    assert int(cls["upper_acgt"][0]) + int(cls["lower_acgt"][0]) + int(cls["n_any"][0]) + int(cls["other"][0]) == ranges[0][1]
    assert cls["lower_acgt"][0] > 0 and cls["other"][0] > 0


@pytest.fixture(scope="module")
def tab():
    from test_gpu_resident_strand import rev_table
    return rev_table()


def test_view_answers_as_its_owner_and_holds_no_memory(tab):
    import sedef_amd
    from sedef_amd.extz2 import live_device_bytes
    rng = np.random.default_rng(11)
    live0 = live_device_bytes()
    a, b = sedef_amd.Extz2Engine(0), sedef_amd.Extz2Engine(0)
    try:
        first = small_record(rng, tab, 700)
        second = small_record(rng, tab, 1000)
        assert a.pool_append_fasta(*as_fasta(first, 60), reset=True) == 0
        base = a.pool_append_fasta(*as_fasta(second, 70, b"\r\n", last_end=False))
        assert base == len(first) and a.pool_bytes() == len(first) + len(second)
        held = b.device_bytes()
        assert b.pool_share(a) == a.pool_bytes()
        assert b.device_bytes() == held  # the view holds no memory
        work = work_on(rng, base, len(second))
        mine, parts = answers(a, work)
        check_meaningful(parts, work)
        theirs, _ = answers(b, work)
        for k in mine:
            assert mine[k] == theirs[k], k
        # ... and the first record through the view, against the owner
        work1 = work_on(rng, 0, len(first), 100)
        m1, t1 = answers(a, work1)[0], answers(b, work1)[0]
        assert m1 == t1
        # the view counts none of the pool: what it holds now are the buffers of its own calls
        assert a.device_bytes() >= a.pool_bytes()
        pool_cap = a.pool_bytes()
        b_now = b.device_bytes()
        b.close()
        assert live_device_bytes() == live0 + a.device_bytes()  # b's buffers are gone, the pool is not
        assert b_now > 0 and pool_cap > 0
        # the owner still answers, from the pool the view did not free
        assert answers(a, work)[0] == mine
    finally:
        b.close()
        a.close()
    assert live_device_bytes() == live0


def test_sharing_rules(tab):
    import sedef_amd
    from sedef_amd.extz2 import SdfError
    rng = np.random.default_rng(12)
    rec = small_record(rng, tab, 400)
    fa = as_fasta(rec, 50)
    a, b, c = sedef_amd.Extz2Engine(0), sedef_amd.Extz2Engine(0), sedef_amd.Extz2Engine(0)
    try:
        a.pool_append_fasta(*fa, reset=True)
        n = a.pool_bytes()
        whole = a.pool_range_classes([(0, n)]).tobytes()
        b.pool_share(a)
        # the owner neither grows nor replaces its pool while a view exists, and keeps it as it was
        with pytest.raises(SdfError, match="rc=-4.*pool is shared"):
            a.pool_append_fasta(*fa)
        with pytest.raises(SdfError, match="rc=-4.*pool is shared"):
            a.pool_append_fasta(*fa, reset=True)
        with pytest.raises(SdfError, match="rc=-4.*pool is shared"):
            a.pool_upload(rec.tobytes())
        with pytest.raises(SdfError, match="rc=-4.*pool is shared"):
            a.pool_upload(rec.tobytes(), pinned=False)
        with pytest.raises(SdfError, match="rc=-4.*pool is shared"):
            a.anchors_batch([("ACGTACGTACGTTTGACC", "ACGTACGTACGTTTGACC", 0, 0)], kmer=5)
        assert a.pool_bytes() == n and b.pool_bytes() == n
        assert a.pool_range_classes([(0, n)]).tobytes() == whole == b.pool_range_classes([(0, n)]).tobytes()
        # a view cannot be added to; nobody shares with itself, from a view, or into a pool that has views
        with pytest.raises(SdfError, match="rc=-4.*pool is shared"):
            b.pool_append_fasta(*fa)
        for dst, src in ((a, a), (c, b), (a, c)):
            with pytest.raises(SdfError, match="rc=-4"):
                dst.pool_share(src)
        assert b.pool_bytes() == n and c.pool_bytes() == 0
        # a pool of its own again on the view: the owner is free
        b.pool_upload(rec[:100].tobytes())
        assert b.pool_bytes() == 100
        assert a.pool_append_fasta(*fa) == n and a.pool_bytes() == 2 * n
        # b's own pool is replaced by a view, c views as well; both gone (one destroyed, one with an appended pool of its own)
        # before the owner may append again
        assert b.pool_share(a) == 2 * n and c.pool_share(a) == 2 * n
        assert b.pool_range_classes([(n, n)]).tobytes() == whole
        b.close()
        with pytest.raises(SdfError, match="pool is shared"):
            a.pool_append_fasta(*fa)
        assert c.pool_append_fasta(*fa, reset=True) == 0 and c.pool_bytes() == n
        assert a.pool_append_fasta(*fa) == 2 * n
        assert c.pool_range_classes([(0, n)]).tobytes() == whole
        # an owner destroyed under a view (the caller's error): the view is left with an empty pool and says so
        c.pool_share(a)
        a.close()
        assert c.pool_bytes() == 0
        rc, _, _ = c.pool_range_classes([(0, 1)], check=False)
        assert rc == -4
        assert c.pool_append_fasta(*fa, reset=True) == 0  # ... and is a context like any other afterwards
        assert c.pool_range_classes([(0, n)]).tobytes() == whole
    finally:
        for e in (b, c, a):
            e.close()


def _free_device_bytes(eng):
    # (from the HIP runtime the library itself runs on: a symbol lookup on the library's handle goes through it)
    hip = eng.lib
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free_b, total_b = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
    return int(free_b.value)


def test_offsets_beyond_2_to_31(tab):
    """A record behind 34 x 64 MiB of others: its base offset is 2,281,701,376.  DP tasks on both strands, anchor pairs with and
    without r_rc and class ranges inside it answer as they do on a fresh context that holds the record alone."""
    import sedef_amd
    rng = np.random.default_rng(13)
    small = small_record(rng, tab, 1000)
    fa = as_fasta(small, 60)
    big_n = 64 << 20
    a = sedef_amd.Extz2Engine(0)
    fresh = sedef_amd.Extz2Engine(0)
    try:
        if _free_device_bytes(a) < (8 << 30):
            pytest.skip("less than 8 GiB of device memory free")
        # one line of 64 MiB without a line end, the same host buffer every time
        big = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, 1 << 20)]
        big = np.tile(big, big_n >> 20)
        for k in range(34):
            assert a.pool_append_fasta(big, big_n, big_n, big_n, reset=(k == 0)) == k * big_n
            a.pool_sync()  # (where the buffer is reused, although its content never changes)
        base = a.pool_append_fasta(*fa)
        assert base == 34 * big_n > (1 << 31) and a.pool_bytes() == base + len(small)
        assert fresh.pool_append_fasta(*fa, reset=True) == 0
        got, parts = answers(a, work_on(np.random.default_rng(14), base, len(small)))
        work0 = work_on(np.random.default_rng(14), 0, len(small))
        exp, parts0 = answers(fresh, work0)
        check_meaningful(parts0, work0)
        for k in exp:
            assert exp[k] == got[k], k
        # the bytes in front of the record are what was appended, up to the last one
        # (2^31 is where the 33rd copy starts)
        cls = a.pool_range_classes([(base - 4096, 4096), (base - 1, 2), ((1 << 31) - 8, 16)])
        want = np.concatenate([big[-4096:], big[-1:], small[:1], big[-8:], big[:8]])
        from test_gpu_pool_classes import expected, as_rows
        exp_cls = expected(want, [(0, 4096), (4096, 2), (4098, 16)])
        assert (as_rows(cls) == exp_cls).all()
    finally:
        fresh.close()
        a.close()

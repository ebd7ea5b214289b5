"""Resident chromosomes on the GPU: strand bits on resident DP tasks (SDF_TASK_Q_RC / SDF_TASK_T_RC), a strand per anchor pair
(sdf_anchors_batch_strand and its _view / _more forms) and the FASTA-layout upload (sdf_pool_append_fasta).

Every expected value comes from what the library already did before these calls existed, on bytes prepared on the host: the
same tasks and pairs FORWARD on a pool in which the reversed ranges were written with rc_inplace semantics (the 128-entry table
is taken from sedef_amd.host, which restates the reference's rev_dna), the CPU oracle on host-coded sequences, the brute-force
anchor definition of tests/bruteforce.py, and the numpy model of the line-end arithmetic (tests/test_resident_strand_cpu.py,
which ties it to the reference's src/fasta.cc)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

# (label, settings): the forced kernels of tests/test_gpu_fuzz_slice.py that the stage's shapes meet -- only the packing changed,
# so every kernel must see the same packed words either way
FORCED = [
    ("default routing", {}),
    ("small tasks without the lane kernel", dict(SDF_NO_LANE=1)),
    ("no strips", dict(SDF_NO_STRIP=1)),
    ("one task per wavefront", dict(SDF_NO_PAIR=1)),
    ("general kernel", dict(SDF_FORCE_GENERAL=1)),
    ("lane kernel for every small batch", dict(SDF_LANE_MIN=1)),
]


# ---- host-side strand: the table behind rc() / rc_inplace ---------------------------------------------------------------------
def rev_table():
    """kDna.rev (sedef_amd/csrc/host/alignment.cc; reference: src/common.h:72-77) through the host library's Sequence ctor."""
    from sedef_amd import host
    host.build_host()
    chars = "".join(chr(c) for c in range(1, 128))
    _, rc, _ = host.sequence("t", chars, True)
    assert len(rc) == 127
    tab = np.full(128, ord("N"), np.uint8)
    tab[1:] = np.frombuffer(rc.encode("latin-1"), np.uint8)[::-1]
    tab = np.concatenate([tab, tab])  # (the table is indexed with c & 127)
    assert bytes(tab[[65, 67, 71, 84, 97, 99, 103, 116, 78, 110, 82]]) == b"TGCAtgcaNNN"
    return tab


def rc_bytes(tab, a):
    return tab[a[::-1]]


ALIGN = np.full(256, 4, np.uint8)  # align_dna (src/common.h:70,91), index c & 127
for _k, _c in enumerate(b"ACGT"):
    for _x in (_c, _c | 0x20, _c | 0x80, _c | 0xa0):
        ALIGN[_x] = _k


def fasta_chars(rng, n, iupac=True):
    """Mixed case in stretches, N runs and a few IUPAC letters."""
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    pos = 0
    while pos < n:  # soft-masked stretches
        L = int(rng.integers(20, 600))
        if rng.random() < 0.35:
            a[pos:pos + L] |= 0x20
        pos += L
    for _ in range(max(1, n // 20000)):  # N runs
        s = int(rng.integers(0, n))
        a[s:s + int(rng.integers(1, 300))] = ord("N") if rng.random() < 0.7 else ord("n")
    if iupac:
        k = max(1, n // 3000)
        a[rng.integers(0, n, k)] = np.frombuffer(b"RYKMSWrynX-*", np.uint8)[rng.integers(0, 12, k)]
    return a


def fnv_tasks(n_cigar, cigar_off, cig):
    """FNV-1a over each task's CIGAR words (what sdfo_extz2_batch returns), all tasks at once."""
    n = len(n_cigar)
    h = np.full(n, 1469598103934665603, np.uint64)
    off, cnt, words = cigar_off.astype(np.int64), n_cigar.astype(np.int64), cig.astype(np.uint64)
    with np.errstate(over="ignore"):
        for j in range(int(cnt.max()) if n else 0):
            live = np.nonzero(cnt > j)[0]
            h[live] = (h[live] ^ words[off[live] + j]) * np.uint64(1099511628211)
    return h


# ---- DP ----------------------------------------------------------------------------------------------------------------------
def strand_tasks(rng, pool_len, n):
    """~n tasks over a pool: gap fills (1..210), 257..8,192 full band, banded at 1,000, a handful of long ones; then the edge
    cases.  Returns (tasks, q_rc, t_rc)."""
    from sedef_amd.extz2 import TASK_DTYPE
    kind = rng.choice(3, n, p=[0.96, 0.01, 0.03])
    ql = np.where(kind == 0, rng.integers(1, 211, n),
                  np.where(kind == 1, np.exp(rng.uniform(np.log(257), np.log(8192), n)).astype(np.int64), 1000))
    tl = np.where(kind == 0, np.clip(ql + rng.integers(-6, 7, n), 1, 210), np.maximum(1, ql + rng.integers(-40, 41, n)))
    w = np.where(kind == 2, rng.choice([64, 128, 512], n), -1)
    # the handful of long ones (Align::MAX_KSW_SEQ_LEN = 60,000): banded, and one full band at 20,000
    long_q = np.array([20000, 60000, 41237, 59999, 33333])
    long_t = np.array([20011, 59990, 41237, 60000, 33200])
    long_w = np.array([-1, 512, 128, 64, 512])
    # edges: lengths around the packing's 16-base words and 32-base groups
    e = np.array([1, 15, 16, 17, 31, 32, 33])
    edge_q, edge_t = np.repeat(e, len(e)), np.tile(e, len(e))
    ql = np.concatenate([ql, long_q, edge_q, edge_q])
    tl = np.concatenate([tl, long_t, edge_t, edge_t])
    w = np.concatenate([w, long_w, np.full(2 * len(edge_q), -1)])
    m = len(ql)
    t = np.zeros(m, TASK_DTYPE)
    t["qlen"], t["tlen"], t["w"], t["zdrop"] = ql, tl, w, -1
    t["q_off"] = (rng.random(m) * (pool_len - ql)).astype(np.int64)
    # targets near their queries, so that the pairs are related sequences
    t["t_off"] = np.clip(t["q_off"] + rng.integers(-3, 4, m), 0, pool_len - tl)
    strand = rng.integers(0, 4, m)
    q_rc, t_rc = (strand & 1).astype(bool), (strand & 2).astype(bool)
    # the second copy of the edge lengths: every range ends at the pool's last byte
    tail = slice(m - len(edge_q), m)
    t["q_off"][tail] = pool_len - t["qlen"][tail]
    t["t_off"][tail] = pool_len - t["tlen"][tail]
    # palindrome checks: both sides name the same range with opposite strands
    pal = np.zeros(40, TASK_DTYPE)
    pal["qlen"] = pal["tlen"] = rng.integers(1, 400, 40)
    pal["q_off"] = pal["t_off"] = (rng.random(40) * (pool_len - 400)).astype(np.int64)
    pal["w"], pal["zdrop"] = -1, -1
    t = np.concatenate([t, pal])
    q_rc = np.concatenate([q_rc, np.arange(40) % 2 == 0])
    t_rc = np.concatenate([t_rc, np.arange(40) % 2 == 1])
    return t, q_rc, t_rc


def forward_equivalent(tab, pool, tasks, q_rc, t_rc):
    """The same tasks without strands on a second pool: every reversed side gets its bytes, rc_inplace'd, behind the pool."""
    t2 = tasks.copy()
    extra, at = [], len(pool)
    for k in np.flatnonzero(q_rc | t_rc):
        for side, flag in (("q", q_rc[k]), ("t", t_rc[k])):
            if flag:
                o, L = int(tasks[side + "_off"][k]), int(tasks[side + "len"][k])
                extra.append(rc_bytes(tab, pool[o:o + L]))
                t2[side + "_off"][k] = at
                at += L
    return np.concatenate([pool] + extra), t2


@pytest.fixture(scope="module")
def dp_case():
    rng = np.random.default_rng(2024)
    tab = rev_table()
    pool = fasta_chars(rng, 3 << 20)
    # make near ranges of opposite strands related: the second half of every 128 kb block is the reverse complement of a
    # mutated copy of its first half, mirrored around the block's middle
    B = 1 << 17
    for b0 in range(0, len(pool), B):
        half = pool[b0:b0 + B // 2].copy()
        sub = rng.random(len(half)) < 0.05
        half[sub] = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, int(sub.sum()))]
        pool[b0 + B // 2:b0 + B] = rc_bytes(tab, half)
    tasks, q_rc, t_rc = strand_tasks(rng, len(pool), 50000)
    # a tenth of the tasks sit astride a block's middle with opposite strands: there rc(t) is a mutated copy of q
    m = len(tasks) - 40
    for k in rng.choice(m - 120, m // 10, replace=False):
        L = int(max(tasks["qlen"][k], tasks["tlen"][k]))
        if L > B // 2:
            continue
        mid = int(rng.integers(0, len(pool) // B)) * B + B // 2
        d = int(rng.integers(0, 2000))
        tasks["q_off"][k] = mid - d - tasks["qlen"][k]
        tasks["t_off"][k] = mid + d + int(rng.integers(0, 3))
        q_rc[k], t_rc[k] = (False, True) if k % 2 else (True, False)
    assert (tasks["q_off"] >= 0).all() and (tasks["t_off"] >= 0).all()
    assert (tasks["q_off"] + tasks["qlen"] <= len(pool)).all() and (tasks["t_off"] + tasks["tlen"] <= len(pool)).all()
    pool2, tasks2 = forward_equivalent(tab, pool, tasks, q_rc, t_rc)
    return tab, pool, tasks, q_rc, t_rc, pool2, tasks2


def _three_calls(eng, tasks, **kw):
    from sedef_amd.extz2 import WANT_ALL
    brief = eng.align_batch_pairs(tasks, **kw)
    full = eng.align_batch_pairs(tasks, want=WANT_ALL, **kw)
    view = eng.align_batch_pairs(tasks, view=True, **kw)
    return brief, full, view


@pytest.mark.parametrize("label,settings", FORCED, ids=[f[0] for f in FORCED])
def test_dp_strand_equals_forward_on_host_rc_bytes(dp_case, label, settings):
    import sedef_amd
    tab, pool, tasks, q_rc, t_rc, pool2, tasks2 = dp_case
    eng = sedef_amd.Extz2Engine(0, config=settings)
    eng.pool_upload(pool2.tobytes())
    exp = _three_calls(eng, tasks2)
    eng.pool_upload(pool.tobytes())
    got = _three_calls(eng, tasks, q_rc=q_rc, t_rc=t_rc)
    for name, (er, ec), (gr, gc) in zip(("pairs", "pairs_full", "pairs_view"), exp, got):
        assert er.tobytes() == gr.tobytes(), (label, name, int(np.flatnonzero(er != gr)[0]))
        assert np.array_equal(ec, gc), (label, name)
    full = got[1][0]
    assert (full["n_cigar"] > 0).all() and (full["matches"][-40:] >= 0).all()
    # the strands matter: the same tasks with the bits dropped align differently
    plain = eng.align_batch_pairs(tasks)
    assert (plain[0]["matches"] != got[0][0]["matches"]).sum() > len(tasks) // 20
    eng.close()


def test_dp_strand_against_the_cpu_oracle(dp_case, oracle):
    """A 2,000-task sample against the scalar oracle on host-coded sequences: not two runs of the same GPU code."""
    import sedef_amd
    from sedef_amd.extz2 import WANT_ALL
    tab, pool, tasks, q_rc, t_rc, _, _ = dp_case
    rng = np.random.default_rng(8)
    cells = tasks["qlen"].astype(np.int64) * tasks["tlen"]
    small = np.flatnonzero((cells <= 400000) | ((tasks["w"] > 0) & (tasks["qlen"] <= 1000)))
    pick = np.sort(rng.choice(small, 1960, replace=False))
    mid = np.flatnonzero((cells > 4000000) & (cells < 40000000) & (tasks["w"] < 0))[:6]  # (and a few of the strips' sizes)
    pick = np.unique(np.concatenate([pick, mid, np.arange(len(tasks) - 40, len(tasks))]))  # (with the palindromes)
    assert len(pick) >= 2000 and len(mid) == 6
    t = tasks[pick]
    codes, q_off, t_off, at = [], np.zeros(len(t), np.int64), np.zeros(len(t), np.int64), 0
    for k in range(len(t)):
        for side, flag, offs in (("q", q_rc[pick[k]], q_off), ("t", t_rc[pick[k]], t_off)):
            o, L = int(t[side + "_off"][k]), int(t[side + "len"][k])
            s = pool[o:o + L]
            codes.append(ALIGN[rc_bytes(tab, s) if flag else s])
            offs[k] = at
            at += L
    codes = np.concatenate(codes)
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(pool.tobytes())
    res, cig = eng.align_batch_pairs(t, want=WANT_ALL, q_rc=q_rc[pick], t_rc=t_rc[pick])
    got_h = fnv_tasks(res["n_cigar"], res["cigar_off"], cig)
    for wv in np.unique(t["w"]):
        sel = np.flatnonzero(t["w"] == wv)
        score, h = oracle.batch(codes, q_off[sel], t["qlen"][sel], t_off[sel], t["tlen"][sel], w=int(wv))
        assert np.array_equal(score, res["score"][sel]), int(wv)
        assert np.array_equal(h, got_h[sel]), int(wv)
    eng.close()


def test_strand_bits_are_unknown_flags_everywhere_else():
    import sedef_amd
    from sedef_amd.extz2 import TASK_DTYPE, TASK_Q_RC, TASK_T_RC, SdfError
    eng = sedef_amd.Extz2Engine(0)
    pool = np.zeros(64, np.uint8)
    # 64 KiB of HBM for the device-resident form, from the HIP runtime the library itself runs on, whichever copy of it this
    # process has loaded: a symbol lookup on the library's own handle goes through the libraries it was resolved against
    hip = eng.lib
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    mem = C.c_void_p()
    assert hip.hipMalloc(C.byref(mem), 1 << 16) == 0
    try:
        for bit in (TASK_Q_RC, TASK_T_RC, 0x400, 0x40000):  # (and two bits that are nobody's)
            t = np.zeros(3, TASK_DTYPE)
            t["qlen"], t["tlen"], t["w"], t["zdrop"] = 20, 20, -1, -1
            t["t_off"] = 20
            t["flag"][1] = bit
            for call in (lambda: eng.align_batch(t, pool), lambda: eng.align_batch_brief(t, pool)):
                with pytest.raises(SdfError, match="rc=-3"):
                    call()
            td = t.copy()
            td["t_off"] = 4
            with pytest.raises(SdfError, match="rc=-3"):
                eng.align_batch_device(td, mem.value, mem.value + 4096, mem.value + 8192, 256)
    finally:
        assert hip.hipFree(mem) == 0
    eng.close()


# ---- anchors -------------------------------------------------------------------------------------------------------------------
def anchor_pairs(rng, tab, n, lo, hi, iupac=True):
    """n pairs with planted repeats and soft-masked stretches.  Returns (desc, r_rc, pool for the strand call, pool with the
    reversed references rc_inplace'd: what a caller of the plain call prepares on the host)."""
    from sedef_amd.extz2 import ANCHOR_PAIR_DTYPE
    desc = np.zeros(n, ANCHOR_PAIR_DTYPE)
    r_rc = np.arange(n) % 2 == 1
    rng.shuffle(r_rc)
    fw, st, off = [], [], 0
    for k in range(n):
        m = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        q = fasta_chars(rng, m, iupac)
        for _ in range(int(rng.integers(0, 4))):  # planted repeats: a unit copied a few (or a thousand) times
            unit = q[:int(rng.integers(8, 60))].copy()
            times = int(rng.choice([3, 8, 30, 1100])) if m > 20000 else int(rng.integers(2, 6))
            rep = np.tile(unit, times)[:m // 4]
            s = int(rng.integers(0, m - len(rep)))
            q[s:s + len(rep)] = rep
        r = q[rng.random(m) > 0.02].copy()
        sub = rng.random(len(r)) < 0.03
        r[sub] = np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, int(sub.sum()))]
        same = int(k % 3 == 0)
        desc[k] = (off, off + len(q), len(q), len(r), same, int(rng.integers(-50, 50)) if same else 0)
        off += len(q) + len(r)
        fw += [q, r]  # r: the sequence the aligner means
        st += [q, rc_bytes(tab, r) if r_rc[k] else r]  # ... and how it lies in the genome
    return desc, r_rc, np.concatenate(st), np.concatenate(fw)


def test_anchors_strand_equals_forward_on_host_rc_bytes():
    import sedef_amd
    rng = np.random.default_rng(77)
    tab = rev_table()
    n = 300
    desc, r_rc, pool_s, pool_f = anchor_pairs(rng, tab, n, 1000, 100000)
    # rc_inplace of the stranded pool's reversed ranges is the forward pool, except where rev_dna is not an involution (IUPAC -> N)
    chk = pool_s.copy()
    for k in np.flatnonzero(r_rc):
        o, L = int(desc["r_off"][k]), int(desc["rlen"][k])
        chk[o:o + L] = rc_bytes(tab, chk[o:o + L])
    pool_f = chk
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(pool_f.tobytes())
    exp, exp_off = eng.anchors_batch_resident(desc, 11)
    h = n // 2
    # (the `more` form does not grow the pinned staging: a view over all pairs sizes it first, as the stage driver's does)
    all_v, all_off = eng.anchors_batch_resident(desc, 11, mode="view")
    assert np.array_equal(all_off, exp_off) and all_v.tobytes() == exp.tobytes()
    exp1, exp_off1 = eng.anchors_batch_resident(desc[:h], 11, mode="view")
    exp2, exp_off2 = eng.anchors_batch_resident(desc[h:], 11, mode="more", keep=len(exp1))
    eng.pool_upload(pool_s.tobytes())
    got, got_off = eng.anchors_batch_resident(desc, 11, r_rc=r_rc)
    assert np.array_equal(exp_off, got_off) and exp.tobytes() == got.tobytes()
    assert len(got) > 10 * n and (got["has_u"] == 0).any() and (got["has_u"] == 1).any()
    rc_has = [k for k in np.flatnonzero(r_rc) if got_off[k + 1] > got_off[k]]
    assert len(rc_has) > n // 3
    # the view and `more` forms (keep > 0), against the same forms forward
    got1, got_off1 = eng.anchors_batch_resident(desc[:h], 11, r_rc=r_rc[:h], mode="view")
    assert len(got1) > 0
    got2, got_off2 = eng.anchors_batch_resident(desc[h:], 11, r_rc=r_rc[h:], mode="more", keep=len(got1))
    assert np.array_equal(exp_off1, got_off1) and exp1.tobytes() == got1.tobytes()
    assert np.array_equal(exp_off2, got_off2) and exp2.tobytes() == got2.tobytes()
    assert np.concatenate([got1, got2]).tobytes() == got.tobytes()
    # forward pairs only, through the strand entry point with an all-zero array: the plain call's answer
    eng.pool_upload(pool_f.tobytes())
    z, z_off = eng.anchors_batch_resident(desc, 11, r_rc=np.zeros(n, bool))
    assert np.array_equal(exp_off, z_off) and exp.tobytes() == z.tobytes()
    # the host-pool form of the strand call (the Python mirror's anchors_batch with r_rc)
    few = [k for k in range(n) if desc["qlen"][k] < 4000][:6]
    pairs_s, pairs_f = [], []
    for k in few:
        qo, ro, ql, rl = (int(desc[f][k]) for f in ("q_off", "r_off", "qlen", "rlen"))
        pairs_s.append((pool_s[qo:qo + ql].tobytes().decode(), pool_s[ro:ro + rl].tobytes().decode(), int(desc["same_chr"][k]),
                        int(desc["delta"][k])))
        pairs_f.append((pairs_s[-1][0], pool_f[ro:ro + rl].tobytes().decode()) + pairs_s[-1][2:])
    assert eng.anchors_batch(pairs_s, 11, r_rc=r_rc[few]) == eng.anchors_batch(pairs_f, 11)
    eng.close()


def test_anchors_strand_against_the_bruteforce_definition():
    import sedef_amd
    from bruteforce import anchors_bruteforce
    rng = np.random.default_rng(5)
    tab = rev_table()
    desc, r_rc, pool_s, pool_f = anchor_pairs(rng, tab, 8, 600, 2500, iupac=False)
    assert r_rc.sum() == 4
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(pool_s.tobytes())
    got, off = eng.anchors_batch_resident(desc, 11, r_rc=r_rc)
    for k in range(len(desc)):
        qo, ro, ql, rl = (int(desc[f][k]) for f in ("q_off", "r_off", "qlen", "rlen"))
        q, r = pool_f[qo:qo + ql].tobytes().decode(), pool_f[ro:ro + rl].tobytes().decode()
        exp = anchors_bruteforce(q, r, 11, same_chr=bool(desc["same_chr"][k]), qstart=0, rstart=int(desc["delta"][k]))
        assert [tuple(int(x) for x in a) for a in got[off[k]:off[k + 1]]] == exp, k
    eng.close()


# ---- FASTA-layout upload ---------------------------------------------------------------------------------------------------------
def _pool_read(eng, off, n):
    buf = np.zeros(max(n, 1), np.uint8)
    eng.lib.sdf_debug_pool_read.restype = C.c_int
    eng.lib.sdf_debug_pool_read.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    assert eng.lib.sdf_debug_pool_read(eng.ctx, off, n, buf.ctypes.data) == 0
    return buf[:n]


def test_pool_append_fasta_against_the_model():
    import sedef_amd
    from sedef_amd.extz2 import SdfError, TASK_DTYPE, WANT_ALL
    from test_resident_strand_cpu import fasta_lines, gather_model, model_records
    rng = np.random.default_rng(1)
    recs = model_records()
    big = fasta_chars(rng, 50_000_000)
    recs.insert(len(recs) // 2, (big.tobytes(), 60, b"\n", True))
    recs.append((fasta_chars(rng, 70_000_001).tobytes(), 61, b"\r\n", False))  # (more than one 64 MiB piece of lines)
    eng = sedef_amd.Extz2Engine(0)
    want, offs = [], []
    for i, (seq, width, eol, last_eol) in enumerate(recs):
        raw = fasta_lines(seq, width, eol, last_eol)
        model = gather_model(raw, len(seq), width, width + len(eol))
        before = eng.pool_bytes()
        off = eng.pool_append_fasta(raw, len(seq), width, width + len(eol), reset=(i == 0))
        assert off == (0 if i == 0 else before) and eng.pool_bytes() == off + len(seq)
        offs.append(off)
        want.append(model)
    want = np.concatenate(want)
    assert eng.pool_bytes() == len(want)
    got = _pool_read(eng, 0, len(want))
    assert got.tobytes() == want.tobytes()
    # a record of one line that comes without a line end at all: line_bytes == line_bases
    one = b"ACGTNacgtn" * 7
    off = eng.pool_append_fasta(one, len(one), len(one), len(one))
    assert off == len(want) and _pool_read(eng, off, len(one)).tobytes() == one
    want = np.concatenate([want, np.frombuffer(one, np.uint8)])
    # invalid geometry: SDF_ERR_INVALID, and the pool is what it was
    raw60 = fasta_lines(b"A" * 150, 60)
    for args in ((raw60, 150, 0, 1), (raw60, 150, 60, 59), (raw60, 150, 60, 60), (raw60, 152, 60, 61), (raw60[:-3], 150, 60, 61),
                 (raw60 + b"\n", 150, 60, 61), (raw60, -1, 60, 61), (raw60, 150, 60, 62)):
        with pytest.raises(SdfError, match="rc=-4"):
            eng.pool_append_fasta(*args)
        assert eng.pool_bytes() == len(want)
    # a record no device has room for: consistent geometry, so that the call gets as far as the capacity check (every check
    # precedes the first read of `bytes`)
    huge = 1 << 50
    dummy = np.zeros(64, np.uint8)
    off = C.c_int64(-7)
    rc = eng.lib.sdf_pool_append_fasta(eng.ctx, dummy.ctypes.data, huge + (huge - 1) // 60 + 1, huge, 60, 61, 0, C.byref(off))
    assert rc == -4 and b"free memory" in eng.lib.sdf_last_error(eng.ctx) and off.value == -7
    assert eng.pool_bytes() == len(want)
    tail = _pool_read(eng, len(want) - 4096, 4096)
    assert tail.tobytes() == want[-4096:].tobytes()
    # ... and through the DP: tasks over known ranges against the same tasks on a plainly uploaded pool
    n = 4000
    t = np.zeros(n, TASK_DTYPE)
    t["qlen"], t["tlen"] = rng.integers(1, 211, n), rng.integers(1, 211, n)
    t["q_off"] = (rng.random(n) * (len(want) - 300)).astype(np.int64)
    t["t_off"] = np.clip(t["q_off"] + rng.integers(-3, 4, n), 0, len(want) - 300)
    t["q_off"][:len(offs)] = offs  # (from each record's base 0)
    t["q_off"] = np.minimum(t["q_off"], len(want) - t["qlen"])
    t["w"], t["zdrop"] = -1, -1
    got_r, got_c = eng.align_batch_pairs(t, want=WANT_ALL, q_rc=np.arange(n) % 2 == 0)
    eng2 = sedef_amd.Extz2Engine(0)
    eng2.pool_upload(want.tobytes())
    exp_r, exp_c = eng2.align_batch_pairs(t, want=WANT_ALL, q_rc=np.arange(n) % 2 == 0)
    assert got_r.tobytes() == exp_r.tobytes() and np.array_equal(got_c, exp_c)
    # sdf_pool_upload keeps replacing the pool
    assert eng.pool_upload(b"ACGT") == 4
    assert eng.pool_append_fasta(b"AC\nGT\n", 4, 2, 3) == 4 and _pool_read(eng, 0, 8).tobytes() == b"ACGTACGT"
    eng.close()
    eng2.close()


def test_pool_append_fasta_from_the_pinned_staging_keeps_what_is_resident():
    """A loader that stages record after record in sdf_pool_host's one pinned buffer, the records in ascending size: every
    staging request is larger than the pool in HBM, and the pool has to grow under the records already resident."""
    import sedef_amd
    from test_resident_strand_cpu import fasta_lines, gather_model
    rng = np.random.default_rng(4)
    eng = sedef_amd.Extz2Engine(0)
    want, offs = [], []
    for i, n in enumerate((500, 16571, 70001, 1200000, 9000000, 40000000)):
        seq = fasta_chars(rng, n).tobytes()
        raw = fasta_lines(seq, 60)
        eng.pool_sync()  # (the upload before has left the staging)
        p = eng.lib.sdf_pool_host(eng.ctx, len(raw))
        assert p
        assert eng.pool_bytes() == sum(len(w) for w in want)
        C.memmove(p, raw, len(raw))
        off = C.c_int64(-1)
        eng._check(eng.lib.sdf_pool_append_fasta(eng.ctx, p, len(raw), n, 60, 61, int(i == 0), C.byref(off)))
        assert off.value == sum(len(w) for w in want)
        offs.append(off.value)
        want.append(gather_model(raw, n, 60, 61))
        # everything resident so far, after every append
        got = _pool_read(eng, 0, eng.pool_bytes())
        assert got.tobytes() == np.concatenate(want).tobytes(), i
    # staging a buffer without appending leaves the pool alone, too
    assert eng.lib.sdf_pool_host(eng.ctx, 200 << 20)
    whole = np.concatenate(want)
    assert eng.pool_bytes() == len(whole) and _pool_read(eng, 0, len(whole)).tobytes() == whole.tobytes()
    eng.close()


# ---- end to end at the interface ---------------------------------------------------------------------------------------------------
def test_chromosome_resident_once_then_base_ranges_and_strands():
    """One chromosome uploaded as the file has it; anchors and a DP round for 64 candidate pairs (half with a reverse-strand
    reference side) named by (base offset, length, strand) -- against the per-pair-slot route: every pair's two sequences cut
    out and reverse-complemented on the host, uploaded as a pool of their own, forward calls."""
    import sedef_amd
    from test_resident_strand_cpu import fasta_lines
    rng = np.random.default_rng(99)
    tab = rev_table()
    chrom = fasta_chars(rng, 6_000_000)
    npairs = 64
    regions = []
    for k in range(npairs):  # planted duplications, half of them reversed
        L = int(rng.integers(1500, 30000))
        a = int(rng.integers(0, 2_900_000 - L))
        b = int(rng.integers(3_000_000, 5_900_000 - L))
        src = chrom[a:a + L][rng.random(L) > 0.02].copy()
        sub = rng.random(len(src)) < 0.04
        src[sub] = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, int(sub.sum()))]
        rcf = k % 2 == 1
        chrom[b:b + len(src)] = rc_bytes(tab, src) if rcf else src
        regions.append((a, L, b, len(src), rcf))
    raw = fasta_lines(chrom.tobytes(), 60)
    eng = sedef_amd.Extz2Engine(0)
    base = eng.pool_append_fasta(raw, len(chrom), 60, 61, reset=True)
    assert base == 0 and eng.pool_bytes() == len(chrom)

    from sedef_amd.extz2 import ANCHOR_PAIR_DTYPE, TASK_DTYPE, WANT_ALL
    desc = np.zeros(npairs, ANCHOR_PAIR_DTYPE)
    slot = np.zeros(npairs, ANCHOR_PAIR_DTYPE)
    parts, at = [], 0
    r_rc = np.array([r[4] for r in regions])
    for k, (a, L, b, L2, rcf) in enumerate(regions):
        desc[k] = (base + a, base + b, L, L2, 0, 0)
        q, r = chrom[a:a + L], chrom[b:b + L2]
        if rcf:
            r = rc_bytes(tab, r)
        slot[k] = (at, at + L, L, L2, 0, 0)
        parts += [q, r]
        at += L + L2
    slots = np.concatenate(parts)
    got_a, got_off = eng.anchors_batch_resident(desc, 11, r_rc=r_rc, mode="view")
    old = sedef_amd.Extz2Engine(0)
    old.pool_upload(slots.tobytes())
    exp_a, exp_off = old.anchors_batch_resident(slot, 11, mode="view")
    assert np.array_equal(got_off, exp_off) and got_a.tobytes() == exp_a.tobytes() and len(got_a) > 20 * npairs

    # a DP round: the gaps between consecutive anchors of each pair (what the stage's first round fills), by base range and strand
    tq, tt, ts = [], [], []
    for k in range(npairs):
        an = got_a[got_off[k]:got_off[k + 1]]
        order = np.argsort(an["q"], kind="stable")
        prev_q = prev_r = 0
        for x in an[order]:
            q0, r0 = int(x["q"]), int(x["r"])
            if q0 >= prev_q and r0 >= prev_r and 0 < max(q0 - prev_q, r0 - prev_r) <= 500 and min(q0 - prev_q, r0 - prev_r) > 0:
                tq.append((k, prev_q, q0 - prev_q))
                tt.append((prev_r, r0 - prev_r))
            if q0 + int(x["l"]) > prev_q and r0 + int(x["l"]) > prev_r:
                prev_q, prev_r = q0 + int(x["l"]), r0 + int(x["l"])
    n = len(tq)
    assert n > 500
    new_t, old_t = np.zeros(n, TASK_DTYPE), np.zeros(n, TASK_DTYPE)
    t_rc = np.zeros(n, bool)
    for i, ((k, qs, ql), (rs, rl)) in enumerate(zip(tq, tt)):
        a, L, b, L2, rcf = regions[k]
        new_t[i]["q_off"], new_t[i]["qlen"] = base + a + qs, ql
        # [rs, rs + rl) of the reverse-complemented reference is bytes [L2 - rs - rl, L2 - rs) of the range, read backwards
        new_t[i]["t_off"], new_t[i]["tlen"] = (base + b + L2 - rs - rl if rcf else base + b + rs), rl
        t_rc[i] = rcf
        old_t[i]["q_off"], old_t[i]["qlen"] = int(slot["q_off"][k]) + qs, ql
        old_t[i]["t_off"], old_t[i]["tlen"] = int(slot["r_off"][k]) + rs, rl
    for t in (new_t, old_t):
        t["w"], t["zdrop"] = -1, -1
    got_r, got_c = eng.align_batch_pairs(new_t, want=WANT_ALL, t_rc=t_rc)
    exp_r, exp_c = old.align_batch_pairs(old_t, want=WANT_ALL)
    assert t_rc.sum() > n // 5 and (~t_rc).sum() > n // 5
    assert got_r.tobytes() == exp_r.tobytes() and np.array_equal(got_c, exp_c)
    gb, gc = eng.align_batch_pairs(new_t, t_rc=t_rc, view=True)
    eb, ec = old.align_batch_pairs(old_t, view=True)
    assert gb.tobytes() == eb.tobytes() and np.array_equal(gc, ec)
    eng.close()
    old.close()

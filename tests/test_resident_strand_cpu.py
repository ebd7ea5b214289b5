"""Resident chromosomes without a GPU (include/sedef_hip.h: SDF_TASK_Q_RC / SDF_TASK_T_RC, sdf_anchors_batch_strand,
sdf_pool_append_fasta): the new symbols and constants, the planner's blindness to the strand bits, and the line-end arithmetic
of the FASTA-layout upload as a numpy model -- the model the GPU gather is compared with (tests/test_gpu_resident_strand.py),
itself compared here with FASTA text written line by line and with sedef_amd.host.fasta_get, which is pinned to the reference's
src/fasta.cc."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["sdf_pool_append_fasta", "sdf_pool_sync", "sdf_anchors_batch_strand", "sdf_anchors_batch_view_strand",
               "sdf_anchors_batch_more_strand"]


# ---- the model of the gather -----------------------------------------------------------------------------------------
def fasta_lines(seq, width, eol=b"\n", last_eol=True):
    """A record's sequence lines as a FASTA writer lays them out: `width` bases a line, the last one short."""
    lines = [seq[i:i + width] for i in range(0, len(seq), width)]
    raw = eol.join(lines)
    if lines and last_eol:
        raw += eol
    return raw


def gather_model(raw, n_bases, line_bases, line_bytes):
    """Base x of a record lies at byte x + (x / line_bases) * (line_bytes - line_bases) of its lines."""
    x = np.arange(n_bases, dtype=np.int64)
    return np.frombuffer(raw, np.uint8)[x + (x // line_bases) * (line_bytes - line_bases)]


def model_records(seed=5):
    """(sequence bytes, width, line end, last line end present) of the records both test files upload."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTacgtNnRY", np.uint8)
    p = np.array([.2, .2, .2, .2, .04, .04, .04, .04, .02, .01, .005, .005])
    recs = []
    for width in (1, 2, 59, 60, 61, 70):
        for eol in (b"\n", b"\r\n"):
            for n in (width * 7 + width // 2 + (width == 1), width * 5, 1, 1000 + width):
                seq = letters[rng.choice(len(letters), n, p=p)].tobytes()
                recs.append((seq, width, eol, bool(rng.integers(0, 2))))
    recs.append((b"", 60, b"\n", True))  # an empty record
    recs.append((b"", 60, b"\n", False))
    return recs


# ---- symbols -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    from sedef_amd.build import build_library
    lib = C.CDLL(build_library())
    src = open(os.path.join(ROOT, "include", "sedef_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdf_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    defs = dict(re.findall(r"#define\s+(SDF_TASK_[A-Z_]+)\s+(0x[0-9a-fA-F]+)", src))
    from sedef_amd import extz2
    assert int(defs["SDF_TASK_Q_RC"], 16) == extz2.TASK_Q_RC and int(defs["SDF_TASK_T_RC"], 16) == extz2.TASK_T_RC
    ksw_bits = 0x01 | 0x02 | 0x04 | 0x08 | 0x10 | 0x20 | 0x40 | 0x80 | 0x100  # extern/ksw2.h:8-16
    assert extz2.TASK_Q_RC & extz2.TASK_T_RC == 0 and (extz2.TASK_Q_RC | extz2.TASK_T_RC) & ksw_bits == 0
    assert hasattr(extz2.Extz2Engine, "pool_append_fasta")


# ---- the planner never sees the strand -----------------------------------------------------------------------------------
def _plan(tasks, want=3, threads=0):
    import sedef_amd
    from sedef_amd import extz2
    lib = sedef_amd.load_library()
    sc = extz2._scoring(extz2.sedef_mat(), 40, 1)
    n = len(tasks)
    per_task = np.zeros((n, 7), np.int64)
    per_chunk = np.zeros((64, 5), np.int64)
    nch = C.c_size_t(0)
    lib.sdf_debug_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = lib.sdf_debug_plan(C.byref(sc), tasks.ctypes.data, n, want, 64 << 30, 160 * 1024, threads, per_task.ctypes.data,
                            per_chunk.ctypes.data, 64, C.byref(nch))
    return rc, per_task, per_chunk[:nch.value]


def mixed_tasks(rng, n):
    """Gap fills, mid-sized full-band tasks, banded ones at 1,000 and a handful of long ones, shuffled."""
    from sedef_amd.extz2 import TASK_DTYPE
    t = np.zeros(n, TASK_DTYPE)
    kind = rng.choice(4, n, p=[0.9, 0.07, 0.0297, 0.0003])
    kind[:3] = 3
    ql = np.where(kind == 0, rng.integers(1, 211, n), np.where(kind == 1, rng.integers(257, 8193, n),
                  np.where(kind == 2, 1000, rng.integers(20000, 60001, n))))
    tl = np.clip(ql + rng.integers(-8, 9, n), 1, 60000)
    t["qlen"], t["tlen"] = ql, tl
    t["w"] = np.where(kind == 2, rng.choice([64, 128, 512], n), -1)
    t["zdrop"] = -1
    rng.shuffle(t)
    return t


@pytest.mark.parametrize("threads", [0, 4])
def test_plan_is_blind_to_strand_bits(threads):
    from sedef_amd.extz2 import TASK_Q_RC, TASK_T_RC
    rng = np.random.default_rng(11)
    t = mixed_tasks(rng, 20000)
    rc0, task0, chunk0 = _plan(t, threads=threads)
    assert rc0 == 0
    s = t.copy()
    s["flag"] |= rng.choice([0, TASK_Q_RC, TASK_T_RC, TASK_Q_RC | TASK_T_RC], len(s)).astype(np.int32)
    assert (s["flag"] != 0).sum() > 10000
    rc1, task1, chunk1 = _plan(s, threads=threads)
    assert rc1 == 0
    assert np.array_equal(task0, task1) and np.array_equal(chunk0, chunk1)
    # a bit that is no strand bit is still an unknown flag to the planner
    u = t.copy()
    u["flag"][7] |= 0x40000
    assert _plan(u, threads=threads)[0] == -3


# ---- the line-end arithmetic ---------------------------------------------------------------------------------------------
def test_gather_model_against_written_lines():
    for seq, width, eol, last_eol in model_records():
        raw = fasta_lines(seq, width, eol, last_eol)
        got = gather_model(raw, len(seq), width, width + len(eol))
        assert got.tobytes() == seq, (width, eol, len(seq))
        # what sdf_pool_append_fasta accepts as "nbytes consistent with n_bases"
        least = len(seq) + ((len(seq) - 1) // width if seq else 0) * len(eol)
        assert least <= len(raw) <= least + len(eol)


def test_gather_model_against_fasta_get(tmp_path):
    """The same arithmetic on a file with an index, against FastaReference::get_sequence (reference: src/fasta.cc:105-142)."""
    from sedef_amd import host
    host.build_host()
    rng = np.random.default_rng(3)
    recs = []
    for k, width in enumerate((1, 2, 59, 60, 61, 70)):
        n = int(rng.integers(3 * width + 1, 40 * width)) if width > 2 else 37 + width
        recs.append(("rec%d" % k, bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), n)), width))
    path = str(tmp_path / "g.fa")
    fai = []
    with open(path, "wb") as f:
        for name, seq, width in recs:
            f.write(b">" + name.encode() + b" test\n")
            fai.append((name, len(seq), f.tell(), width, width + 1))
            f.write(fasta_lines(seq, width))
    with open(path + ".fai", "w") as f:
        for row in fai:
            f.write("%s\t%d\t%d\t%d\t%d\n" % row)
    whole = open(path, "rb").read()
    for (name, seq, width), (_, n, off, lb, lby) in zip(recs, fai):
        nbytes = n + ((n - 1) // lb) * (lby - lb) + (lby - lb)
        model = gather_model(whole[off:off + nbytes], n, lb, lby).tobytes()
        got, _ = host.fasta_get(path, name, 0, None)
        assert got.encode() == model == seq, name
        a, b = n // 3, n - n // 4
        end = b
        part, end2 = host.fasta_get(path, name, a, end)
        assert part.encode() == model[a:b] and end2 == b

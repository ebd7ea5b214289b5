#!/usr/bin/env python3
"""Timing of the resident-sequence paths on one GPU, for two builds of the library side by side.

  resident_probe.py pack [--lib PATH] [--rev] [--calls N]
      sdf_extz2_batch_pairs_view on the stage's round-1 shape (700,000 gap fills of ~25 bases over a 180 MB pool): host-clock
      milliseconds per call (median, min, max).  --rev: every side of every task reversed (SDF_TASK_Q_RC | SDF_TASK_T_RC).
      The pack kernel's own time: run the same command under `rocprofv3 --kernel-trace --stats` (pack_chars_kernel).
  resident_probe.py gather [--lib PATH] [--mb N] [--calls N]
      sdf_pool_append_fasta of one record of N Mb at 60 bases a line from the context's pinned staging: milliseconds per call and
      bytes moved (raw lines over PCIe; the gather reads them and writes the bases: HBM bytes = raw + bases).

--lib: another build of libsedef_hip.so (a parent commit's), through plain ctypes: only calls both builds have."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sedef_amd.build import LIB_PATH  # noqa: E402
from sedef_amd.extz2 import TASK_DTYPE, _scoring, sedef_mat  # noqa: E402


def load(path):
    L = C.CDLL(path)
    L.sdf_create.restype = C.c_void_p
    L.sdf_create.argtypes = [C.c_int, C.c_size_t]
    L.sdf_last_error.restype = C.c_char_p
    L.sdf_last_error.argtypes = [C.c_void_p]
    L.sdf_pool_host.restype = C.c_void_p
    L.sdf_pool_host.argtypes = [C.c_void_p, C.c_size_t]
    L.sdf_pool_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.sdf_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32]
    L.sdf_extz2_batch_pairs_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.sdf_last_ms.restype = C.c_float
    L.sdf_last_ms.argtypes = [C.c_void_p, C.c_int]
    return L


def check(L, ctx, rc):
    if rc != 0:
        raise SystemExit("rc=%d: %s" % (rc, L.sdf_last_error(ctx).decode()))


def stats(ms):
    ms = np.sort(np.array(ms))
    return "median %.2f ms, min %.2f, max %.2f (%d calls)" % (float(np.median(ms)), ms[0], ms[-1], len(ms))


def pack(L, ctx, args):
    rng = np.random.default_rng(1)
    nbytes, n = 180 << 20, 700000
    p = L.sdf_pool_host(ctx, nbytes)
    pool = np.frombuffer((C.c_char * nbytes).from_address(p), np.uint8)
    pool[:] = np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, nbytes)]
    check(L, ctx, L.sdf_pool_upload(ctx, p, nbytes))
    t = np.zeros(n, TASK_DTYPE)
    t["qlen"] = np.clip(rng.normal(25, 12, n), 1, 210).astype(np.int32)
    t["tlen"] = np.clip(t["qlen"] + rng.integers(-4, 5, n), 1, 210)
    t["q_off"] = np.sort((rng.random(n) * (nbytes - 512)).astype(np.int64))  # (a round's tasks follow their pairs through the pool)
    t["t_off"] = t["q_off"] + 256
    t["w"], t["zdrop"] = -1, -1
    if args.rev:
        t["flag"] = 0x30000
    check(L, ctx, L.sdf_reserve(ctx, n, int(t["qlen"].sum() + t["tlen"].sum()), 0, 1))
    sc = _scoring(sedef_mat(), 40, 1)
    pb, pc, used = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    ms, dev = [], []
    for k in range(args.calls + 3):
        t0 = time.perf_counter()
        check(L, ctx, L.sdf_extz2_batch_pairs_view(ctx, C.byref(sc), t.ctypes.data, n, C.byref(pb), C.byref(pc), C.byref(used)))
        if k >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
            dev.append(L.sdf_last_ms(ctx, 3))
    print("pack%s %s: call %s; stream time %s" % (" --rev" if args.rev else "", os.path.basename(os.path.dirname(args.lib)) or args.lib,
                                                 stats(ms), stats(dev)), flush=True)


def gather(L, ctx, args):
    L.sdf_pool_append_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_int32, C.c_int,
                                        C.POINTER(C.c_int64)]
    L.sdf_debug_pool_read.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    n = args.mb * 1000000
    n -= n % 60
    raw_n = n // 60 * 61
    p = L.sdf_pool_host(ctx, raw_n)
    raw = np.frombuffer((C.c_char * raw_n).from_address(p), np.uint8).reshape(-1, 61)
    raw[:, :60] = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(2).integers(0, 4, (n // 60, 60))]
    raw[:, 60] = 10
    off, one = C.c_int64(0), np.zeros(1, np.uint8)
    ms = []
    for k in range(args.calls + 2):
        t0 = time.perf_counter()
        check(L, ctx, L.sdf_pool_append_fasta(ctx, p, raw_n, n, 60, 61, 1, C.byref(off)))
        check(L, ctx, L.sdf_debug_pool_read(ctx, n - 1, 1, one.ctypes.data))  # (drains the stream)
        if k >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    print("gather %d Mb: upload + gather %s; %.1f GB/s of raw lines end to end (kernel alone: rocprofv3, fasta_gather_kernel; "
          "it moves %d + %d bytes)" % (args.mb, stats(ms), raw_n / med / 1e6, raw_n, n), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pack", "gather"])
    ap.add_argument("--lib", default=LIB_PATH)
    ap.add_argument("--rev", action="store_true")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--mb", type=int, default=250)
    a = ap.parse_args()
    lib = load(a.lib)
    c = lib.sdf_create(0, 0)
    if not c:
        raise SystemExit("sdf_create failed: %s" % lib.sdf_last_error(None).decode())
    (pack if a.what == "pack" else gather)(lib, c, a)

"""Pair recall (include/sedef_hip.h: sdf_pair_recall): one function per form of the call, on numpy arrays.

A record is two ends, [start1, end1) of chromosome chr1 and [start2, end2) of chr2; bit 0 of `flags` is the strand of end 1,
bit 1 that of end 2.  Chromosome ids are any numbering the gold and the found records share."""
import ctypes as C

import numpy as np

from .extz2 import SdfError, load_library

IGNORE_STRAND = 1  # SDF_RECALL_IGNORE_STRAND (call flag)
WIDE = 1           # SDF_RECALL_WIDE (result flag)
BAD = 2            # SDF_RECALL_BAD (result flag, device form)
CAP = 1024         # SDF_RECALL_CAP
PAIR_REC_DTYPE = np.dtype([("chr1", "<i4"), ("start1", "<i4"), ("end1", "<i4"), ("chr2", "<i4"), ("start2", "<i4"), ("end2", "<i4"),
                           ("flags", "<u4"), ("reserved", "<u4")])
RECALL_DTYPE = np.dtype([("n_hits", "<u4"), ("cov1", "<i4"), ("cov2", "<i4"), ("flags", "<u4")])

_ARGS = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]


def _lib():
    L = load_library()
    if not getattr(L, "_recall_bound", False):
        L.sdf_pair_recall_host.restype = C.c_int  # gold, n_gold, found, n_found, flags, out
        L.sdf_pair_recall_host.argtypes = _ARGS
        L.sdf_pair_recall.restype = C.c_int  # ctx, then the same
        L.sdf_pair_recall.argtypes = [C.c_void_p] + _ARGS
        L.sdf_pair_recall_device.restype = C.c_int  # ctx, then the same over device pointers, and the two status words
        L.sdf_pair_recall_device.argtypes = [C.c_void_p] + _ARGS + [C.c_void_p]
        L._recall_bound = True
    return L


def pair_recs(rows):
    """(chr1, start1, end1, chr2, start2, end2, flags[, reserved]) rows -> a PAIR_REC_DTYPE array."""
    if isinstance(rows, np.ndarray) and rows.dtype == PAIR_REC_DTYPE:
        return np.ascontiguousarray(rows)
    out = np.zeros(len(rows), PAIR_REC_DTYPE)
    if len(rows):
        a = np.asarray(rows, dtype=np.int64)
        for k, f in enumerate(PAIR_REC_DTYPE.names[:a.shape[1]]):
            out[f] = a[:, k]
    return out


def _call(fn, head, gold, found, flags):
    gold, found = pair_recs(gold), pair_recs(found)
    out = np.zeros(max(len(gold), 1), RECALL_DTYPE)
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    rc = fn(*head, ptr(gold), len(gold), ptr(found), len(found), int(flags), out.ctypes.data)
    return rc, out[:len(gold)].copy()


def pair_recall_host(gold, found, flags=0):
    """sdf_pair_recall_host: no context, no device.  Returns (rc, a RECALL_DTYPE record per gold record)."""
    return _call(_lib().sdf_pair_recall_host, (), gold, found, flags)


def pair_recall(engine, gold, found, flags=0, check=True):
    """sdf_pair_recall on an Extz2Engine: host arrays in and out (check=False: (rc, records))."""
    rc, out = _call(_lib().sdf_pair_recall, (engine.ctx,), gold, found, flags)
    if not check:
        return rc, out
    engine._check(rc)
    return out


def pair_recall_device(engine, d_gold, n_gold, d_found, n_found, flags, d_out, d_status, check=True):
    """sdf_pair_recall_device: device pointers (ints); enqueued on the engine's stream, nothing is read back and nothing waited
    for.  d_status: two uint64 (found records dropped, gold records dropped)."""
    rc = _lib().sdf_pair_recall_device(engine.ctx, d_gold, int(n_gold), d_found, int(n_found), int(flags), d_out, d_status)
    if check and rc != 0:
        raise SdfError("rc=%d: %s" % (rc, engine.lib.sdf_last_error(engine.ctx).decode()))
    return rc

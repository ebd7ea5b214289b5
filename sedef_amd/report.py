"""Line order (include/sedef_hip.h: sdf_line_order): one function per form of the call, on numpy arrays.

A line is a byte string without its newline; `line_records` parses lines into the pool and the 48-byte records the calls take:
eight ascending keys for `sort -k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n` under LC_ALL=C.  order[p] is the index
of the line at place p; flags[p] holds DUP where that line is the one before it (what `uniq` drops) and WIDE."""
import ctypes as C

import numpy as np

from .extz2 import SdfError, load_library

DUP = 1   # SDF_LINE_DUP
WIDE = 2  # SDF_LINE_WIDE
RUN = 64  # SDF_LINE_RUN
LINE_REC_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("reserved", "<u4"), ("key", "<u4", (8,))])

_ARGS = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]  # pool, pool_bytes, lines, n, order, flags


def _lib():
    L = load_library()
    if not getattr(L, "_report_bound", False):
        L.sdf_line_records.restype = C.c_int  # text, text_bytes, pool, pool_cap, pool_bytes, lines, lines_cap, n, plain
        L.sdf_line_records.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p]
        L.sdf_line_order_host.restype = C.c_int
        L.sdf_line_order_host.argtypes = _ARGS + [C.c_void_p]  # ..., n_kept
        L.sdf_line_order.restype = C.c_int
        L.sdf_line_order.argtypes = [C.c_void_p] + _ARGS + [C.c_void_p]
        L.sdf_line_order_device.restype = C.c_int  # ctx, the same over device pointers, the three counts, the stream
        L.sdf_line_order_device.argtypes = [C.c_void_p] + _ARGS + [C.c_void_p, C.c_void_p]
        L._report_bound = True
    return L


def line_records(lines):
    """Lines (bytes, none holding a newline) -> (pool: uint8 array, records: LINE_REC_DTYPE array, plain).  plain is False when
    an `n` field has a sign, a decimal point, more than ten digits or a value of 2^32 or more: the four `n` keys are then ranks,
    and such a call keeps to line_order_host by convention."""
    lines = [bytes(x) for x in lines]
    if any(b"\n" in x for x in lines):
        raise ValueError("a line holds a newline")
    text = np.frombuffer(b"".join(x + b"\n" for x in lines), np.uint8)
    L = _lib()
    need, n, plain = C.c_size_t(0), C.c_size_t(0), C.c_int(1)
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    rc = L.sdf_line_records(ptr(text), len(text), None, 0, C.addressof(need), None, 0, C.addressof(n), None)
    if rc != 0 or n.value != len(lines):
        raise SdfError("sdf_line_records: rc=%d, %d lines of %d" % (rc, n.value, len(lines)))
    pool, recs = np.zeros(max(need.value, 1), np.uint8), np.zeros(max(n.value, 1), LINE_REC_DTYPE)
    rc = L.sdf_line_records(ptr(text), len(text), pool.ctypes.data, need.value, C.addressof(need), recs.ctypes.data, n.value, C.addressof(n),
                            C.addressof(plain))
    if rc != 0:
        raise SdfError("sdf_line_records: rc=%d" % rc)
    return pool[:need.value], recs[:n.value], bool(plain.value)


def _call(fn, head, pool, recs):
    pool, recs = np.ascontiguousarray(pool, np.uint8), np.ascontiguousarray(recs, LINE_REC_DTYPE)
    n = len(recs)
    order, flags, kept = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    rc = fn(*head, ptr(pool), len(pool), ptr(recs), n, order.ctypes.data, flags.ctypes.data, C.addressof(kept))
    return rc, order[:n].copy(), flags[:n].copy(), int(kept.value)


def line_order_host(pool, recs):
    """sdf_line_order_host: no context, no device.  Returns (rc, order, flags, n_kept)."""
    return _call(_lib().sdf_line_order_host, (), pool, recs)


def line_order(engine, pool, recs, check=True):
    """sdf_line_order on an Extz2Engine: host arrays in and out -> (order, flags, n_kept) (check=False: rc in front)."""
    rc, order, flags, kept = _call(_lib().sdf_line_order, (engine.ctx,), pool, recs)
    if not check:
        return rc, order, flags, kept
    engine._check(rc)
    return order, flags, kept


def line_order_device(engine, d_pool, pool_bytes, d_lines, n, d_order, d_flags, d_counts, stream=None, check=True):
    """sdf_line_order_device: device pointers (ints); enqueued on `stream` (None: the engine's), nothing is read back and
    nothing waited for.  d_counts: three uint32 (places without DUP, WIDE runs, lines refused)."""
    rc = _lib().sdf_line_order_device(engine.ctx, d_pool, int(pool_bytes), d_lines, int(n), d_order, d_flags, d_counts, stream)
    if check and rc != 0:
        raise SdfError("rc=%d: %s" % (rc, engine.lib.sdf_last_error(engine.ctx).decode()))
    return rc

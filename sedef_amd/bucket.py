"""`align bucket` on records (include/sedef_hip.h: sdf_bucket_merge): one function per form of the call, on numpy arrays.

Chromosome ids are the caller's numbering in byte-wise lexicographic order of the names; name_tables() makes the ids and the
two tables from names and their groups, as `sedef align bucket` does with SDF_BUCKET_DEVICE=1."""
import ctypes as C

import numpy as np

from .extz2 import SdfError, load_library

SEED_RC = 1  # SDF_SEED_RC
SEED_HIT_DTYPE = np.dtype([("q_chr", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"), ("r_chr", "<i4"), ("r_start", "<i4"), ("r_end", "<i4"),
                           ("flags", "<u4"), ("pad", "<u4")])
BUCKET_HIT_DTYPE = np.dtype([("q_chr", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"), ("r_chr", "<i4"), ("r_start", "<i4"), ("r_end", "<i4"),
                             ("flags", "<u4"), ("bucket", "<i4")])


class BucketParams(C.Structure):  # sdf_bucket_params; the defaults: Globals::Extend (src/globals.cc:32-34)
    _fields_ = [("extend_ratio", C.c_double), ("max_extend", C.c_int32), ("merge_dist", C.c_int32), ("nbins", C.c_int32)]


def bucket_params(nbins, extend_ratio=5.0, max_extend=15000, merge_dist=250):
    return BucketParams(float(extend_ratio), int(max_extend), int(merge_dist), int(nbins))


_TAIL = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(BucketParams), C.c_void_p, C.c_size_t, C.c_void_p]


def _lib():
    L = load_library()
    if not getattr(L, "_bucket_bound", False):
        L.sdf_bucket_merge_host.restype = C.c_int  # hits, n, chr_group, n_chr, group_pair_order, n_groups, params, out, out_cap, n_out
        L.sdf_bucket_merge_host.argtypes = _TAIL
        L.sdf_bucket_merge.restype = C.c_int  # ctx, then the same
        L.sdf_bucket_merge.argtypes = [C.c_void_p] + _TAIL
        L.sdf_bucket_merge_device.restype = C.c_int  # ctx, then the same over device pointers (params: the host's)
        L.sdf_bucket_merge_device.argtypes = [C.c_void_p] + _TAIL
        L._bucket_bound = True
    return L


def seed_hits(rows):
    """(q_chr, q_start, q_end, r_chr, r_start, r_end, rc) rows -> a SEED_HIT_DTYPE array."""
    if isinstance(rows, np.ndarray) and rows.dtype == SEED_HIT_DTYPE:
        return np.ascontiguousarray(rows)
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 7)
    out = np.zeros(len(a), SEED_HIT_DTYPE)
    for k, f in enumerate(("q_chr", "q_start", "q_end", "r_chr", "r_start", "r_end", "flags")):
        out[f] = a[:, k]
    return out


def pair_order(n_groups):
    """group_pair_order for n_groups groups: the rank of "tmp_<gq>_<gr>.tmp" among all such strings."""
    names = sorted(("tmp_%d_%d.tmp" % (a, b), a * n_groups + b) for a in range(n_groups) for b in range(n_groups))
    out = np.zeros(n_groups * n_groups, np.int32)
    for rank, (_, at) in enumerate(names):
        out[at] = rank
    return out


def name_tables(names, group_of, n_groups=None):
    """names: the chromosome names in use; group_of: name -> translation group (a name it does not hold: group 0).
    Returns (sorted names: id = index, chr_group, group_pair_order, n_groups)."""
    names = sorted(set(names), key=lambda s: s.encode())
    chr_group = np.array([group_of.get(nm, 0) for nm in names], np.int32)
    if n_groups is None:
        n_groups = int(max(list(group_of.values()) + [0])) + 1
    return names, chr_group, pair_order(n_groups), n_groups


def _call(fn, head, hits, chr_group, group_pair_order, params, out_cap=None):
    hits = seed_hits(hits)
    chr_group = np.ascontiguousarray(chr_group, dtype=np.int32)
    group_pair_order = np.ascontiguousarray(group_pair_order, dtype=np.int32)
    n_groups = int(round(len(group_pair_order) ** 0.5))
    assert n_groups * n_groups == len(group_pair_order)
    n = len(hits)
    cap = n if out_cap is None else int(out_cap)
    out = np.zeros(max(cap, 1), BUCKET_HIT_DTYPE)
    n_out = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    rc = fn(*head, ptr(hits), n, ptr(chr_group), len(chr_group), ptr(group_pair_order), n_groups, C.byref(params), out.ctypes.data, cap,
            C.addressof(n_out))
    return rc, out[:n_out.value].copy()


def bucket_merge_host(hits, chr_group, group_pair_order, params, out_cap=None):
    """sdf_bucket_merge_host: no context, no device.  Returns (rc, records in deal order)."""
    return _call(_lib().sdf_bucket_merge_host, (), hits, chr_group, group_pair_order, params, out_cap)


def bucket_merge(engine, hits, chr_group, group_pair_order, params, out_cap=None, check=True):
    """sdf_bucket_merge on an Extz2Engine: host arrays in and out.  Returns the records in deal order (check=False: (rc, records))."""
    rc, out = _call(_lib().sdf_bucket_merge, (engine.ctx,), hits, chr_group, group_pair_order, params, out_cap)
    if not check:
        return rc, out
    engine._check(rc)
    return out


def bucket_merge_device(engine, d_hits, n, d_chr_group, n_chr, d_group_pair_order, n_groups, params, d_out, out_cap, d_n_out, check=True):
    """sdf_bucket_merge_device: everything but `params` as device pointers (ints); enqueued on the engine's stream, nothing is
    read back and nothing waited for.  d_n_out: two uint64 (records written, records dropped)."""
    rc = _lib().sdf_bucket_merge_device(engine.ctx, d_hits, int(n), d_chr_group, int(n_chr), d_group_pair_order, int(n_groups),
                                        C.byref(params), d_out, int(out_cap), d_n_out)
    if check and rc != 0:
        raise SdfError("rc=%d: %s" % (rc, engine.lib.sdf_last_error(engine.ctx).decode()))
    return rc

"""Search hits to seed records (include/sedef_hip.h: sdf_seed_records) and `sedef seeds`: one function per form of the call, on
numpy arrays, the chain the command runs (sdf_seeds_bucket_merge), and the command as a child process.

A hit is a record of sdf_search_pairs_indexed; hits[first[j]:first[j + 1]] are job j's; jobs[j] names the chromosomes of job j
(ids in byte-wise lexicographic order of the names, as sedef_amd.bucket numbers them), the reference's length and its strand."""
import ctypes as C
import os
import subprocess

import numpy as np

from .bucket import BUCKET_HIT_DTYPE, SEED_HIT_DTYPE, SEED_RC, BucketParams
from .extz2 import SdfError, load_library

PAIR_HIT_DTYPE = np.dtype([("window", "<i4"), ("query_start", "<i4"), ("query_end", "<i4"), ("ref_start", "<i4"), ("ref_end", "<i4"),
                           ("jaccard", "<i4")])  # sdf_search_pair_hit
SEED_JOB_DTYPE = np.dtype([("q_chr", "<i4"), ("r_chr", "<i4"), ("ref_len", "<i8"), ("flags", "<u4"), ("reserved", "<u4")])  # sdf_seed_job

_HEAD = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]  # hits, n, first, jobs, n_jobs


def _lib():
    L = load_library()
    if not getattr(L, "_seeds_bound", False):
        L.sdf_seed_records_host.restype = C.c_int  # hits, n, first, jobs, n_jobs, out
        L.sdf_seed_records_host.argtypes = _HEAD + [C.c_void_p]
        L.sdf_seed_records.restype = C.c_int  # ctx, then the same
        L.sdf_seed_records.argtypes = [C.c_void_p] + _HEAD + [C.c_void_p]
        L.sdf_seed_records_device.restype = C.c_int  # ctx, then the same over device pointers
        L.sdf_seed_records_device.argtypes = [C.c_void_p] + _HEAD + [C.c_void_p]
        L.sdf_seeds_bucket_merge.restype = C.c_int  # ctx, the same, chr_group, n_chr, group_pair_order, n_groups, params, out, out_cap, n_out, n_dropped
        L.sdf_seeds_bucket_merge.argtypes = [C.c_void_p] + _HEAD + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(BucketParams),
                                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L._seeds_bound = True
    return L


def pair_hits(rows):
    """(query_start, query_end, ref_start, ref_end) rows -> a PAIR_HIT_DTYPE array (window and jaccard 0: the records do not read them)."""
    if isinstance(rows, np.ndarray) and rows.dtype == PAIR_HIT_DTYPE:
        return np.ascontiguousarray(rows)
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(len(a), PAIR_HIT_DTYPE)
    for k, f in enumerate(("query_start", "query_end", "ref_start", "ref_end")):
        out[f] = a[:, k]
    return out


def seed_jobs(rows):
    """(q_chr, r_chr, ref_len, reverse) rows -> a SEED_JOB_DTYPE array."""
    if isinstance(rows, np.ndarray) and rows.dtype == SEED_JOB_DTYPE:
        return np.ascontiguousarray(rows)
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(len(a), SEED_JOB_DTYPE)
    out["q_chr"], out["r_chr"], out["ref_len"], out["flags"] = a[:, 0], a[:, 1], a[:, 2], np.where(a[:, 3] != 0, SEED_RC, 0)
    return out


def _ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def _args(hits, first, jobs, n=None):
    hits = None if hits is None else pair_hits(hits)
    first = None if first is None else np.ascontiguousarray(first, dtype=np.uint64)
    jobs = None if jobs is None else seed_jobs(jobs)
    n = (0 if hits is None else len(hits)) if n is None else int(n)
    return hits, first, jobs, n, (0 if jobs is None else len(jobs))


def seed_records_host(hits, first, jobs, n=None, out=True):
    """sdf_seed_records_host: no context, no device.  Returns (rc, records).  None for an array is a null pointer; n: the count
    the call is told (default: len(hits)); out=False: a null output."""
    hits, first, jobs, n, n_jobs = _args(hits, first, jobs, n)
    rec = np.zeros(max(min(n, 1 << 20), 1), SEED_HIT_DTYPE)
    rc = _lib().sdf_seed_records_host(_ptr(hits), n, _ptr(first), _ptr(jobs), n_jobs, rec.ctypes.data if out else None)
    return rc, rec[:n if rc == 0 else 0].copy()


def seed_records(engine, hits, first, jobs, n=None, out=True, check=True, guard=0):
    """sdf_seed_records on an Extz2Engine: host arrays in and out.  Returns the records (check=False: (rc, records)); guard: that
    many records more behind them, as they were before the call (all bytes 0xEE), are returned too."""
    hits, first, jobs, n, n_jobs = _args(hits, first, jobs, n)
    rec = np.zeros(max(min(n, 1 << 20), 1) + guard, SEED_HIT_DTYPE)
    rec.view(np.uint8)[:] = 0xEE
    rc = _lib().sdf_seed_records(engine.ctx, _ptr(hits), n, _ptr(first), _ptr(jobs), n_jobs, rec.ctypes.data if out else None)
    got = rec[:(n if rc == 0 else 0) + guard].copy()
    if not check:
        return rc, got
    engine._check(rc)
    return got


def seed_records_device(engine, d_hits, n, d_first, d_jobs, n_jobs, d_out, check=True):
    """sdf_seed_records_device: device pointers (ints); enqueued on the engine's stream, nothing is read back and nothing waited
    for."""
    rc = _lib().sdf_seed_records_device(engine.ctx, d_hits, int(n), d_first, d_jobs, int(n_jobs), d_out)
    if check and rc != 0:
        raise SdfError("rc=%d: %s" % (rc, engine.lib.sdf_last_error(engine.ctx).decode()))
    return rc


def seeds_bucket_merge(engine, hits, first, jobs, chr_group, group_pair_order, params, check=True):
    """sdf_seeds_bucket_merge: the records and their merge back to back on the engine's stream.  Returns (merged records in deal
    order, dropped); with dropped != 0 there are no records (check=False: rc in front)."""
    hits, first, jobs, n, n_jobs = _args(hits, first, jobs)
    chr_group = np.ascontiguousarray(chr_group, dtype=np.int32)
    group_pair_order = np.ascontiguousarray(group_pair_order, dtype=np.int32)
    n_groups = int(round(len(group_pair_order) ** 0.5))
    out = np.zeros(max(n, 1), BUCKET_HIT_DTYPE)
    n_out, dropped = C.c_size_t(0), C.c_size_t(0)
    rc = _lib().sdf_seeds_bucket_merge(engine.ctx, _ptr(hits), n, _ptr(first), _ptr(jobs), n_jobs, _ptr(chr_group), len(chr_group),
                                       _ptr(group_pair_order), n_groups, C.byref(params), out.ctypes.data, n, C.addressof(n_out),
                                       C.addressof(dropped))
    if check:
        engine._check(rc)
        return out[:n_out.value].copy(), dropped.value
    return rc, out[:n_out.value].copy(), dropped.value


def seeds_command(genome, buckets_dir, nbins, seeds_dir=None, options=(), env=None, timeout=600):
    """`sedef seeds [options] -n nbins [--seeds-dir seeds_dir] genome buckets_dir` as a child process -> CompletedProcess (the log
    is its stderr)."""
    from . import host
    argv = [host.CLI, "seeds"] + [str(o) for o in options] + ["-n", str(nbins)]
    if seeds_dir is not None:
        argv += ["--seeds-dir", str(seeds_dir)]
    return subprocess.run(argv + [str(genome), str(buckets_dir)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


def seeds_pairs(genome, max_size=100 * 1000 * 1000):
    """The chromosome pairs of a `sedef seeds` run over genome.fa.fai at a group limit, in order ->
    [(query group, reference group, reverse, query, reference, same_genome)]."""
    from . import host
    lib, buf = host.load_host(), host._buffer()
    lib.sdfh_seeds_pairs.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    host._err(lib, lib.sdfh_seeds_pairs(genome.encode(), int(max_size), buf, len(buf)))
    out = []
    for p in buf.value.decode().split("|"):
        if p:
            f = p.split(" ")
            out.append((int(f[0]), int(f[1]), f[2] == "1", f[3], f[4], f[5] == "1"))
    return out


def seeds_args(args):
    """parse_seeds_args over a list of strings -> dict; raises RuntimeError with the refusal."""
    from . import host
    lib, buf = host.load_host(), host._buffer()
    lib.sdfh_seeds_args.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    host._err(lib, lib.sdfh_seeds_args("\n".join(args).encode(), buf, len(buf)))
    f = buf.value.decode().split("|")
    h = f[0].split(" ")
    return dict(k=int(h[0]), w=int(h[1]), u=int(h[2]), nbins=int(h[3]), extend_ratio=float(h[4]), max_extend=int(h[5]), merge_dist=int(h[6]),
                seeds_dir=f[1], pos=f[2:])


def hit_from_bed(line):
    """Hit::from_bed of a seed line as `align bucket` reads it -> (query name, query_start, query_end, reference name, ref_start,
    ref_end, query is_rc, reference is_rc)."""
    from . import host
    lib, buf = host.load_host(), host._buffer()
    out = (C.c_int * 6)()
    lib.sdfh_hit_from_bed.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t]
    host._err(lib, lib.sdfh_hit_from_bed(line.encode(), out, buf, len(buf)))
    qn, rn = buf.value.decode().split("|")
    return (qn, out[0], out[1], rn, out[2], out[3], bool(out[4]), bool(out[5]))

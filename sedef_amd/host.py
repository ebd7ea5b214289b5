"""ctypes access to the host pipeline library (sedef_amd/lib/libsedef_host.so, sources in csrc/host/).

`test_dp` parameters are the library's TEST HOOK: a C function with the oracle's single-task signature that
replaces the GPU provider.  Product code (the `sedef` CLI) never passes one."""
import ctypes as C
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SRC = os.path.join(_HERE, "csrc", "host")
LIB = os.path.join(_HERE, "lib", "libsedef_host.so")
CLI = os.path.join(_HERE, "bin", "sedef")
MULTI = os.path.join(_HERE, "bin", "sdf_multi")
_SOURCES = ["alignment.cc", "hit_fasta.cc", "chain.cc", "host_threads.cc", "stage_settings.cc", "dp_provider.cc", "pair_job.cc",
            "stage_driver.cc", "bucket.cc", "stats.cc", "stats_diff.cc", "stats_recall.cc", "report_cmd.cc", "search_cmd.cc", "seeds_cmd.cc", "host_cabi.cc"]


def build_host(force=False):
    """g++ build of the host library and the `sedef` CLI (needs libsedef_hip.so next to it)."""
    srcs = [os.path.join(HOST_SRC, f) for f in _SOURCES]
    deps = srcs + [os.path.join(HOST_SRC, "sedef_host.h"), os.path.join(HOST_SRC, "stage_internal.h"), os.path.join(HOST_SRC, "search_run.h"),
                   os.path.join(HOST_SRC, "sedef_main.cc"),
                   os.path.join(HOST_SRC, "multi_gpu.cc")]
    multi_ok = os.path.exists(MULTI) or os.path.exists(MULTI + ".skipped")
    built = [LIB, CLI] + ([MULTI] if os.path.exists(MULTI) else [])
    fresh = os.path.exists(LIB) and os.path.exists(CLI) and multi_ok and all(
        os.path.getmtime(d) <= min(os.path.getmtime(b) for b in built) for d in deps)
    if fresh and not force:
        return LIB
    gxx = shutil.which("g++") or "g++"
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    os.makedirs(os.path.dirname(CLI), exist_ok=True)
    libdir = os.path.join(_HERE, "lib")
    subprocess.check_call([gxx, "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-shared", "-o", LIB] + srcs +
                          ["-L" + libdir, "-lsedef_hip", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([gxx, "-O2", "-g", "-rdynamic", "-std=c++17", "-Wall", "-o", CLI, os.path.join(HOST_SRC, "sedef_main.cc"),
                           "-L" + libdir, "-lsedef_host", "-lsedef_hip", "-lpthread", "-Wl,-rpath,$ORIGIN/../lib"])
    # sdf_multi: one batch sharded over the GPUs of a node + RCCL all-gatherv of the results, host C++ above the C ABI.  The
    # file holds no kernels: g++ against the HIP runtime headers; a box without them (CPU-only use of the host library and
    # its test provider) skips the tool instead of failing the build.
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    try:
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-o", MULTI, os.path.join(HOST_SRC, "multi_gpu.cc"),
                               "-L" + libdir, "-lsedef_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lpthread",
                               "-Wl,-rpath,$ORIGIN/../lib", "-Wl,-rpath," + os.path.join(rocm, "lib")])
        if os.path.exists(MULTI + ".skipped"):
            os.remove(MULTI + ".skipped")
    except (subprocess.CalledProcessError, OSError) as e:
        print("sedef_amd.host: sdf_multi not built (%s); the library and the CLI are complete without it" % e)
        if not os.path.exists(MULTI):
            open(MULTI + ".skipped", "w").write(str(e))
    return LIB


_lib = None


def load_host():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError("%s is missing: run __graft_entry__.build()" % LIB)
        _lib = C.CDLL(LIB)
        _lib.sdfh_last_error.restype = C.c_char_p
    return _lib


def _err(lib, rc):
    if rc != 0:
        raise RuntimeError("host pipeline error %d: %s" % (rc, lib.sdfh_last_error().decode()))


def generate(ref_path, bed_path, kmer, out_path, match=5, mismatch=-4, gap_open=-40, gap_extend=-1, test_dp=None,
             device=0):
    """`sedef align generate` (reference: src/align_main.cc:285-337). Returns (lines, hits, dp_tasks, dp_cells, rounds)."""
    lib = load_host()
    stats = (C.c_longlong * 5)()
    rc = lib.sdfh_generate(ref_path.encode(), bed_path.encode(), kmer, out_path.encode(), match, mismatch, gap_open,
                           gap_extend, test_dp, device, stats)
    _err(lib, rc)
    return tuple(int(x) for x in stats)


def generate_many(ref_path, beds, kmer, out_suffix=".aligned.bed", log_dir=None, test_dp=None, device=0):
    """Several buckets through ONE provider (csrc/host/stage_driver.cc: generate_many): bucket b's lines go to b + out_suffix.
    `beds`: bucket files or directories of bucket_???? files.  Returns [(lines, hits)] per bucket."""
    lib = load_host()
    # (two figures per bucket; a directory stands for the bucket_???? files in it)
    nb = sum(len(os.listdir(b)) if os.path.isdir(b) else 1 for b in beds)
    stats = (C.c_longlong * (2 * max(nb, 1) + 2))()
    lib.sdfh_generate_many.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]
    n = lib.sdfh_generate_many(ref_path.encode(), "\n".join(beds).encode(), kmer, out_suffix.encode(),
                               log_dir.encode() if log_dir else None, test_dp, device, stats)
    _err(lib, min(n, 0))
    return [(int(stats[2 * k]), int(stats[2 * k + 1])) for k in range(n)]


def generate_many_resident(ref_path, beds, kmer, out_suffix=".aligned.bed", log_dir=None, test_dp=None, device=0, resident=True):
    """generate_many on chromosomes that stay resident in HBM (sdfh_generate_many_resident; resident=False: generate_many).
    Returns ([(lines, hits)] per bucket, (FASTA records uploaded, characters uploaded to a device pool, super-batches run,
    super-batches that named resident ranges))."""
    lib = load_host()
    nb = sum(len(os.listdir(b)) if os.path.isdir(b) else 1 for b in beds)
    stats = (C.c_longlong * (2 * max(nb, 1) + 4))()
    lib.sdfh_generate_many_resident.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int,
                                                C.c_int, C.c_void_p]
    n = lib.sdfh_generate_many_resident(ref_path.encode(), "\n".join(beds).encode(), kmer, out_suffix.encode(),
                                        log_dir.encode() if log_dir else None, test_dp, device, int(bool(resident)), stats)
    _err(lib, min(n, 0))
    return [(int(stats[2 * k]), int(stats[2 * k + 1])) for k in range(n)], tuple(int(stats[2 * n + i]) for i in range(4))


def dp_chunks(qlen, tlen, step, t_rc=False, t_off=0):
    """Test hook: the DP tasks a request of qlen x tlen bases is cut into, `step` bases at a time (csrc/host/dp_provider.cc:
    for_each_chunk) -> [(first query base, first byte of the target in pool order, query length, target length)]; the target
    starts at pool byte t_off and, with t_rc, is read reversed."""
    lib = load_host()
    lib.sdfh_dp_chunks.restype = C.c_long
    lib.sdfh_dp_chunks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_longlong), C.c_long]
    cap = min(qlen, tlen) // step + 2
    out = (C.c_longlong * (4 * cap))()
    n = lib.sdfh_dp_chunks(qlen, tlen, step, int(bool(t_rc)), t_off, out, cap)
    assert 0 <= n <= cap, n
    return [tuple(int(x) for x in out[4 * k:4 * k + 4]) for k in range(n)]


_buf = None


def _buffer():
    global _buf
    if _buf is None:
        _buf = C.create_string_buffer(4 << 20)
    return _buf


def alignment_pair(fa, fb, test_dp=None, device=0, scoring=None):
    """Alignment(fa, fb) (reference: src/align.cc:76-88) -> (CIGAR string, [matches, mismatches, gaps, gap_bases, span]).
    scoring = (match, mismatch, gap_open, gap_extend) as the CLI overrides (src/align_main.cc:343-352)."""
    lib, buf = load_host(), _buffer()
    cnt = (C.c_int * 5)()
    if scoring is None:
        _err(lib, lib.sdfh_alignment_pair(fa.encode(), fb.encode(), test_dp, device, buf, len(buf), cnt))
    else:
        _err(lib, lib.sdfh_alignment_pair_scored(fa.encode(), fb.encode(), *[int(x) for x in scoring], test_dp, device,
                                                 buf, len(buf), cnt))
    return buf.value.decode(), list(cnt)


def guide_from_chains(q, r, spec, side, test_dp=None, device=0):
    lib, buf = load_host(), _buffer()
    _err(lib, lib.sdfh_guide_from_chains(q.encode(), r.encode(), spec.encode(), side, test_dp, device, buf, len(buf)))
    return buf.value.decode()


def fast_align(query, ref, qname="q", rname="r", q_rc=False, r_rc=False, qstart=0, rstart=0, kmer=11, test_dp=None,
               device=0):
    """fast_align (reference: src/chain.cc:203-268) -> [(qs, qe, rs, re, cigar, matches, mismatches, gaps, gap_bases)]."""
    lib, buf = load_host(), _buffer()
    lib.sdfh_fast_align.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_fast_align(query.encode(), ref.encode(), qname.encode(), rname.encode(), int(q_rc), int(r_rc),
                                  qstart, rstart, kmer, test_dp, device, buf, len(buf)))
    out = []
    for line in buf.value.decode().split("\n"):
        if line:
            f = line.split(" ")
            out.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), f[4]) + tuple(int(x) for x in f[5:9]))
    return out


def chains(q, r, kmer=11):
    lib, buf = load_host(), _buffer()
    lib.sdfh_chains.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_chains(q.encode(), r.encode(), kmer, buf, len(buf)))
    out = []
    for c in buf.value.decode().split("|"):
        if c:
            out.append([tuple(int(x) for x in a.split()) for a in c.split(";") if a])
    return out


def chain_raw(anchors, max_chain_gap=210, match_chain_score=4):
    """chain_anchors on an (m, 4) int32 array of (q, r, l, has_u): returns (path, boundaries)."""
    import numpy as np
    lib = load_host()
    a = np.ascontiguousarray(anchors, dtype=np.int32).reshape(-1, 4)
    m = len(a)
    path = np.zeros(max(m, 1), np.int32)
    bounds = np.zeros(2 * (m + 1), np.int32)
    lib.sdfh_chain_raw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    nb = lib.sdfh_chain_raw(a.ctypes.data, m, max_chain_gap, match_chain_score, path.ctypes.data, bounds.ctypes.data)
    _err(lib, min(nb, 0))
    return path[:m].copy(), bounds[:2 * nb].reshape(-1, 2).copy()


def rangemax_script(pts, ops):
    """Test hook: activate / deactivate / range-maximum calls on the host's priority search tree (chain.cc: RangeMax), in the
    script format of oracle/ref_align_driver.cc: ref_segtree_script.  Returns (out [k, 2], top pointer of every node)."""
    import numpy as np
    lib = load_host()
    pts = np.ascontiguousarray(pts, dtype=np.int32).reshape(-1, 2)
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 5)
    out = np.zeros((max(len(ops), 1), 2), np.int32)
    cap = 4 << max(1, int(len(pts) - 1).bit_length())
    state = np.zeros(cap, np.int32)
    lib.sdfh_rangemax_script.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    size = lib.sdfh_rangemax_script(pts.ctypes.data, len(pts), ops.ctypes.data, len(ops), out.ctypes.data, state.ctypes.data, cap)
    return out[:len(ops)].copy(), state[:size].copy()


def fasta_get(path, name, start, end):
    lib, buf = load_host(), _buffer()
    e = C.c_int(0 if end is None else end)
    _err(lib, lib.sdfh_fasta_get(path.encode(), name.encode(), start, None if end is None else C.byref(e), buf,
                                 len(buf)))
    return buf.value.decode(), (None if end is None else e.value)


def merge(bed_lines, merge_dist=250):
    lib, buf = load_host(), _buffer()
    _err(lib, lib.sdfh_merge("\n".join(bed_lines).encode(), merge_dist, buf, len(buf)))
    return buf.value.decode()


def stats_generate(ref_path, bed_path, out_path, max_ok_gap=-1, min_split=1000, uppercase=100, max_error=0.5,
                   test_cols=None, device=0, resident=False):
    """`sedef stats generate` (reference: src/stats_main.cc:339-389): the table of the final calls.  test_cols: a column
    walker with the oracle's signature (oracle/stats_oracle.c) instead of the device.  resident=True (or SDF_STATS_RESIDENT=1
    in the environment): the chromosomes are uploaded once, as the file has them, and the pieces are counted by base range
    and strand (sdf_stats_columns_pairs); ignored with test_cols.  Returns (lines, hits, pieces, columns)."""
    lib = load_host()
    st = (C.c_longlong * 3)()
    lib.sdfh_stats_generate_resident.restype = C.c_long
    lib.sdfh_stats_generate_resident.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    n = lib.sdfh_stats_generate_resident(ref_path.encode(), bed_path.encode(), out_path.encode(), max_ok_gap, min_split,
                                         uppercase, max_error, test_cols, device, int(bool(resident)), st)
    _err(lib, min(n, 0))
    return (int(n),) + tuple(int(x) for x in st)


# a CPU stand-in for sdf_stats_cuts_pairs on one alignment (csrc/host/sedef_host.h: test_cuts_fn)
CUTS_HOOK = C.CFUNCTYPE(C.c_long, C.POINTER(C.c_char), C.c_int, C.POINTER(C.c_char), C.c_int, C.POINTER(C.c_uint32), C.c_int,
                        C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_long)


def stats_generate_cuts(ref_path, bed_path, out_path, max_ok_gap=-1, min_split=1000, uppercase=100, max_error=0.5,
                        test_cols=None, device=0, resident=True, cuts=True, test_cuts=None):
    """stats_generate with the match counter, the cuts at assembly gaps and the trims on the resident chromosomes too
    (sdfh_stats_generate_cuts; cuts=True or SDF_STATS_CUTS_DEVICE=1, only with resident chromosomes and without max_ok_gap).
    test_cuts: a CUTS_HOOK stand-in for the device call -- the path then runs without a device, with test_cols for the
    columns.  Returns (lines, hits, pieces, columns)."""
    lib = load_host()
    st = (C.c_longlong * 3)()
    lib.sdfh_stats_generate_cuts.restype = C.c_long
    lib.sdfh_stats_generate_cuts.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
    n = lib.sdfh_stats_generate_cuts(ref_path.encode(), bed_path.encode(), out_path.encode(), max_ok_gap, min_split, uppercase,
                                     max_error, test_cols, device, int(bool(resident)), int(bool(cuts)),
                                     C.cast(test_cuts, C.c_void_p) if test_cuts is not None else None, st)
    _err(lib, min(n, 0))
    return (int(n),) + tuple(int(x) for x in st)


def stats_piece_range(start, end, s, e, rc):
    """stats_piece_range (csrc/host/stats.cc): columns [s, e) of a side fetched from [start, end) of its chromosome and, with
    rc, reverse-complemented -> (first base of the range in the chromosome, length)."""
    lib = load_host()
    first = C.c_longlong(0)
    lib.sdfh_stats_piece_range.restype = C.c_int
    lib.sdfh_stats_piece_range.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    n = lib.sdfh_stats_piece_range(int(start), int(end), int(s), int(e), int(bool(rc)), C.byref(first))
    return int(first.value), int(n)


def format_double(x):
    lib, buf = load_host(), _buffer()
    lib.sdfh_format_double.argtypes = [C.c_double, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_format_double(float(x), buf, len(buf)))
    return buf.value.decode()


def stats_recall(bed_path, wgac_path, out_path, host=False, ignore_strand=False, device=0):
    """`sedef stats recall` (csrc/host/stats_recall.cc; reference: scratch/check-overlap.py): which SDs of the WGAC table final.bed
    finds.  The MISS and PART lines go to out_path; returns the four summary lines the command prints on stdout.  host=True:
    sdf_pair_recall_host instead of the device call."""
    lib, buf = load_host(), _buffer()
    lib.sdfh_stats_recall.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_stats_recall(bed_path.encode(), wgac_path.encode(), out_path.encode(), int(bool(host)), int(bool(ignore_strand)),
                                    int(device), buf, len(buf)))
    return buf.value.decode()


def report(ref_path, inputs, out_dir, max_ok_gap=-1, min_split=1000, min_uppercase=100, max_error=0.5, host=False, device=0):
    """`sedef report` (csrc/host/report_cmd.cc; reference: sedef.sh:218-229): the *.aligned.bed files of `inputs` (files or
    directories) ordered and deduplicated to out_dir/aligned.bed, `stats generate` of that file ordered and deduplicated to
    out_dir/final.bed.  Returns the two files' line counts.  host=True: sdf_line_order_host instead of the device call."""
    lib = load_host()
    counts = (C.c_longlong * 2)()
    lib.sdfh_report.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]
    _err(lib, lib.sdfh_report(ref_path.encode(), "\n".join(inputs).encode(), out_dir.encode(), int(max_ok_gap), int(min_split),
                              int(min_uppercase), float(max_error), int(bool(host)), int(device), counts))
    return int(counts[0]), int(counts[1])


def bucket(bed_path, nbins, out_dir, reference):
    lib = load_host()
    _err(lib, lib.sdfh_bucket(bed_path.encode(), nbins, out_dir.encode(), reference.encode()))


def bucket_records(bed_path, nbins, out_dir, reference, form=2, device=0):
    """`sedef align bucket` through the records of include/sedef_hip.h (csrc/host/bucket.cc: bucket_alignments_records) -- form 1:
    one sdf_bucket_merge call on `device` (what SDF_BUCKET_DEVICE=1 selects), form 2: sdf_bucket_merge_host, no device.  True:
    the bucket files are written; False: the seeds keep the host path (one line on stderr, nothing written)."""
    lib = load_host()
    rc = lib.sdfh_bucket_records(bed_path.encode(), int(nbins), out_dir.encode(), reference.encode(), int(form), int(device))
    _err(lib, min(rc, 0))
    return rc == 1


def anchors(q, r, kmer=11, same_chr=False, qstart=0, rstart=0):
    """Host generate_anchors (reference: src/chain.cc:24-101) -> list of (q, r, l, has_u)."""
    lib, buf = load_host(), _buffer()
    lib.sdfh_anchors.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_anchors(q.encode(), r.encode(), kmer, int(same_chr), qstart, rstart, buf, len(buf)))
    return [tuple(int(x) for x in a.split()) for a in buf.value.decode().split(";") if a]


def hit_extend(qs, qe, rs, re_, factor=5.0, max_extend=15000):
    """Hit::extend (reference: src/hit.cc:200-207)."""
    lib = load_host()
    io = (C.c_int * 4)(qs, qe, rs, re_)
    lib.sdfh_hit_extend.argtypes = [C.c_void_p, C.c_double, C.c_int]
    _err(lib, lib.sdfh_hit_extend(io, factor, max_extend))
    return list(io)


def sequence(name, seq, is_rc=False):
    """Sequence ctor (reference: src/hash.cc:104-109) -> (name, seq, is_rc)."""
    lib, buf = load_host(), _buffer()
    _err(lib, lib.sdfh_sequence(name.encode(), seq.encode(), int(is_rc), buf, len(buf)))
    n, s, r = buf.value.decode().split("|")
    return n, s, r == "1"


def search_hit_bed(qname, rname, qs, qe, rs, re_, ref_rc=False, ref_len=0):
    """The BED line `sedef search` prints for a hit (csrc/host/search_cmd.cc: Hit::to_bed() of a search hit, src/hit.cc:134-196);
    rs / re_ as the driver reports them, flipped here under ref_rc by the record's length."""
    lib, buf = load_host(), _buffer()
    lib.sdfh_search_hit_bed.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_char_p,
                                        C.c_size_t]
    _err(lib, lib.sdfh_search_hit_bed(qname.encode(), rname.encode(), int(qs), int(qe), int(rs), int(re_), int(bool(ref_rc)),
                                      int(ref_len), buf, len(buf)))
    return buf.value.decode()


def limit_table(n, kmer=12, max_error=0.30, max_edit_error=0.15, walk=False):
    """limit[0 .. n]: relaxed_jaccard_estimate(s) as `sedef search` computes it (limit[0] = 0); walk=True: by the reference's
    loop as written instead of the bisection."""
    import numpy as np
    lib = load_host()
    out = np.zeros(n + 1, np.int32)
    lib.sdfh_limit_table.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    _err(lib, lib.sdfh_limit_table(int(kmer), float(max_error), float(max_edit_error), int(n), int(bool(walk)), out[1:].ctypes.data))
    return out


def read_limit_table(path, cap=1 << 20):
    """--limit-table parsing (limit[0] = 0 first); raises RuntimeError with the refusal."""
    import numpy as np
    lib = load_host()
    out = np.zeros(cap, np.int32)
    lib.sdfh_read_limit_table.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    n = lib.sdfh_read_limit_table(path.encode(), out.ctypes.data, cap)
    _err(lib, min(n, 0))
    return out[:n].copy()


def translation(ref_path, max_size=100 * 1000 * 1000):
    """generate_translation over genome.fa.fai at a group limit -> [[name, ...], ...]."""
    lib, buf = load_host(), _buffer()
    lib.sdfh_translation.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_translation(ref_path.encode(), int(max_size), buf, len(buf)))
    return [g.split(",") for g in buf.value.decode().split("|") if g]


def search_args(args):
    """parse_search_args over a list of strings -> dict; raises RuntimeError with the refusal."""
    lib, buf = load_host(), _buffer()
    lib.sdfh_search_args.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    _err(lib, lib.sdfh_search_args("\n".join(args).encode(), buf, len(buf)))
    f = buf.value.decode().split("|")
    h = f[0].split(" ")
    return dict(k=int(h[0]), w=int(h[1]), u=int(h[2]), e=float(h[3]), E=float(h[4]), g=float(h[5]), min_read_size=int(h[6]),
                transform=h[7] == "1", reverse=h[8] == "1", limit_table=f[1], pos=f[2:])

"""ctypes mirror of include/sedef_hip.h.

`ksw_extz2()` keeps the argument order and meaning of the reference's ksw_extz2_sse
(reference: extern/ksw2.h:50) so parity tests read like calls to the reference;
`Extz2Engine` exposes the batched entry points.
"""
import ctypes as C
import os

import numpy as np

from .build import LIB_PATH

NEG_INF = -0x40000000
WANT_CIGAR, WANT_SCORE, WANT_EXT, WANT_ALL = 1, 2, 4, 7
# strand bits of a resident task (include/sedef_hip.h: SDF_TASK_Q_RC / SDF_TASK_T_RC; align_batch_pairs only)
TASK_Q_RC, TASK_T_RC = 0x10000, 0x20000

TASK_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"),
                       ("w", "<i4"), ("zdrop", "<i4"), ("flag", "<i4"), ("pad_", "<i4")])
RESULT_DTYPE = np.dtype([("score", "<i4"), ("max", "<i4"), ("max_q", "<i4"), ("max_t", "<i4"),
                         ("mqe", "<i4"), ("mqe_t", "<i4"), ("mte", "<i4"), ("mte_q", "<i4"),
                         ("zdropped", "<i4"), ("n_cigar", "<i4"), ("cigar_off", "<i8"),
                         ("matches", "<i4"), ("mismatches", "<i4"), ("gaps", "<i4"),
                         ("gap_bases", "<i4")])
ANCHOR_PAIR_DTYPE = np.dtype([("q_off", "<i8"), ("r_off", "<i8"), ("qlen", "<i4"), ("rlen", "<i4"),
                              ("same_chr", "<i4"), ("delta", "<i4")])
ANCHOR_DTYPE = np.dtype([("q", "<i4"), ("r", "<i4"), ("l", "<i4"), ("has_u", "<i4")])
BRIEF_DTYPE = np.dtype([("cigar_off", "<i8"), ("n_cigar", "<i4"), ("matches", "<i4")])  # sdf_result_brief
POOL_RANGE_DTYPE = np.dtype([("off", "<i8"), ("len", "<i4"), ("reserved", "<i4")])  # sdf_pool_range
RANGE_CLASSES_DTYPE = np.dtype([(f, "<i4") for f in ("upper_acgt", "lower_acgt", "n_any", "other")])  # sdf_range_classes
# include/sedef_hip.h: sdf_pool_fetch / sdf_pool_fetch_rec (pool_fetch; FETCH_RC in `flags`)
POOL_FETCH_DTYPE = np.dtype([("off", "<i8"), ("len", "<i4"), ("flags", "<i4"), ("dst_off", "<i8")])
POOL_FETCH_REC_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("len", "<i4"), ("rc", "<i4"), ("seg0", "<i8")])
FETCH_RC, FETCH_SEG_BYTES = 0x1, 16384
assert POOL_FETCH_DTYPE.itemsize == 24 and POOL_FETCH_REC_DTYPE.itemsize == 32
# include/sedef_hip.h: sdf_cover_interval / sdf_cover_counts (pool_coverage, pool_coverage_host)
COVER_INTERVAL_DTYPE = np.dtype([(f, "<i4") for f in ("region", "start", "len", "set", "partner", "reserved")])
COVER_COUNTS_DTYPE = np.dtype([(f, "<i8") for f in ("a", "b", "both", "a_only", "b_only", "a_only_upper", "b_only_upper")])
assert COVER_INTERVAL_DTYPE.itemsize == 24 and COVER_COUNTS_DTYPE.itemsize == 56
RESERVE_BRIEF, RESERVE_ANCHORS = 1, 2
assert BRIEF_DTYPE.itemsize == 16
assert TASK_DTYPE.itemsize == 40 and RESULT_DTYPE.itemsize == 64 and ANCHOR_PAIR_DTYPE.itemsize == 32
# include/sedef_hip.h: sdf_stats_task / sdf_stats_cols
STATS_TASK_DTYPE = np.dtype([("a_off", "<u8"), ("b_off", "<u8"), ("a_len", "<u4"), ("b_len", "<u4"),
                             ("cigar_off", "<u8"), ("n_cigar", "<u4"), ("reserved", "<u4")])
STATS_COLS_DTYPE = np.dtype([(f, "<i4") for f in (
    "indel_a", "indel_b", "aln_b", "match_b", "mismatch_b", "transitions_b", "transversions_b", "uppercase_a",
    "uppercase_b", "uppercase_matches", "matches", "mismatches", "gaps", "gap_bases", "span", "flags")])
assert STATS_TASK_DTYPE.itemsize == 40 and STATS_COLS_DTYPE.itemsize == 64
# sdf_stats_piece (sdf_stats_cuts_pairs): a cut piece in the alignment's columns, before and after the trims
STATS_PIECE_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("t_begin", "<i4"), ("t_end", "<i4"), ("matches", "<i4"),
                              ("flags", "<i4"), ("reserved", "<i4", (2,))])
assert STATS_PIECE_DTYPE.itemsize == 32
# include/sedef_hip.h: sdf_minim_range / sdf_minimizer (pool_minimizers, pool_minimizer_index; MINIM_RC in `flags`)
MINIM_RANGE_DTYPE = np.dtype([("off", "<i8"), ("len", "<i4"), ("flags", "<i4")])
MINIMIZER_DTYPE = np.dtype([("hash", "<u4"), ("loc", "<i4"), ("status", "<i4"), ("range", "<i4")])
MINIM_RC, MINIM_MAX_W, MINIM_THRESHOLD_NONE = 0x1, 1000, 1 << 31
assert MINIM_RANGE_DTYPE.itemsize == 16 and MINIMIZER_DTYPE.itemsize == 16
# include/sedef_hip.h: sdf_search_window / sdf_search_interval (search_windows; SEARCH_* in `flags`)
SEARCH_WINDOW_DTYPE = np.dtype([("query_size", "<i4"), ("n_members", "<i4"), ("n_gathered", "<i4"), ("n_candidates", "<i4"),
                                ("flags", "<u4")])
SEARCH_INTERVAL_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4")])
SEARCH_SHORT, SEARCH_NOLIMIT, SEARCH_WIDE = 0x1, 0x2, 0x4
SEARCH_MAX_MEMBERS, SEARCH_MAX_GATHER = 1024, 4096
assert SEARCH_WINDOW_DTYPE.itemsize == 20 and SEARCH_INTERVAL_DTYPE.itemsize == 8
# include/sedef_hip.h: sdf_search_found (search_windows_found, search_overlap; SEARCH_FOUND_WIDE in a window's `flags`)
SEARCH_FOUND_DTYPE = np.dtype([("q_start", "<i4"), ("q_end", "<i4"), ("r_start", "<i4"), ("r_end", "<i4")])
SEARCH_FOUND_WIDE, SEARCH_MAX_FOUND, SEARCH_FOUND_BIN_SHIFT = 0x8, 256, 12
# include/sedef_hip.h: a window search_windows_wide_device finished (WIDE and FOUND_WIDE cleared), and the positions it gathers
SEARCH_WIDE_DONE, SEARCH_WIDE_MAX_GATHER = 0x10, 32768
assert SEARCH_FOUND_DTYPE.itemsize == 16
# include/sedef_hip.h: sdf_search_roll_rec (search_roll; ROLL_* in `flags`)
SEARCH_ROLL_DTYPE = np.dtype([("ref_start", "<i4"), ("ref_end", "<i4"), ("winnow_start", "<i4"), ("winnow_end", "<i4"),
                              ("jaccard", "<i4"), ("flags", "<u4")])
ROLL_WIDE, ROLL_BADWINDOW, ROLL_MAX_SPAN = 0x1, 0x2, 3072
assert SEARCH_ROLL_DTYPE.itemsize == 24
# sdf_filter_task / sdf_filter_rec (the parameters: _FilterParams)
FILTER_TASK_DTYPE = np.dtype([("q_off", "<i8"), ("r_off", "<i8"), ("q_len", "<i4"), ("r_len", "<i4"), ("flags", "<u4"),
                              ("reserved", "<i4")])
FILTER_REC_DTYPE = np.dtype([("q_up", "<i4"), ("r_up", "<i4"), ("dist", "<i4"), ("minqg", "<i4"), ("flags", "<u4")])
assert FILTER_TASK_DTYPE.itemsize == 32 and FILTER_REC_DTYPE.itemsize == 20
# include/sedef_hip.h: sdf_search_hit (search_extend; EXTEND_* in `flags`)
SEARCH_HIT_DTYPE = np.dtype([("query_start", "<i4"), ("query_end", "<i4"), ("ref_start", "<i4"), ("ref_end", "<i4"), ("jaccard", "<i4"),
                             ("q_winnow_start", "<i4"), ("q_winnow_end", "<i4"), ("r_winnow_start", "<i4"), ("r_winnow_end", "<i4"),
                             ("flags", "<u4")])
EXTEND_SKIPPED, EXTEND_WIDE, EXTEND_NOLIMIT, EXTEND_MAX_GROW = 0x1, 0x2, 0x4, 1792
EXTEND_LONG_MAX_GROW = 16384  # SDF_EXTEND_LONG_MAX_GROW: the largest long_grow of search_extend_long_device
assert SEARCH_HIT_DTYPE.itemsize == 40
# include/sedef_hip.h: sdf_search_pair_hit, sdf_search_accept_status, sdf_search_pair_stats (the search driver's section)
SEARCH_PAIR_HIT_DTYPE = np.dtype([("window", "<i4"), ("query_start", "<i4"), ("query_end", "<i4"), ("ref_start", "<i4"),
                                  ("ref_end", "<i4"), ("jaccard", "<i4")])
# sdf_search_index_desc (the resident search index)
SEARCH_INDEX_DESC_DTYPE = np.dtype([("off", "<i8"), ("len", "<i4"), ("flags", "<i4"), ("k", "<i4"), ("w", "<i4"),
                                    ("separate_lowercase", "<i4"), ("threshold", "<u4"), ("n_minimizers", "<u8"), ("n_sorted", "<u8"),
                                    ("n_groups", "<u4"), ("stale", "<u4"), ("device_bytes", "<u8")])
assert SEARCH_INDEX_DESC_DTYPE.itemsize == 64
ACCEPT_STATUS_DTYPE = np.dtype([("frontier", "<u4"), ("flags", "<u4"), ("nf", "<u8"), ("n_out", "<u8"), ("need_found", "<u8"),
                                ("need_out", "<u8"), ("attempted", "<i8"), ("jaccard_failed", "<i8"), ("interval_failed", "<i8")])
PAIR_STATS_DTYPE = np.dtype([(f, "<i8") for f in ("attempted", "jaccard_failed", "interval_failed", "rounds", "windows_run",
                                                  "windows_scheduled", "windows_host")])
ACCEPT_MAX_KEPT, ACCEPT_INCOMPLETE, ACCEPT_OVERFLOW = 512, 0x1, 0x2
# SDF_PAIR_*: the driver's default round, its two starting capacities, the long growths a round finishes on the device
PAIR_ROUND_WINDOWS, PAIR_INTERVALS_START, PAIR_ENTRIES_START, PAIR_LONG_MAX, PAIR_LONG_BATCH = 64, 4096, 4096, 16, 8
assert SEARCH_PAIR_HIT_DTYPE.itemsize == 24 and ACCEPT_STATUS_DTYPE.itemsize == 64 and PAIR_STATS_DTYPE.itemsize == 56
# sdf_search_pair_job (the lanes' section): two handles of search_index_build and same_genome
PAIR_JOB_DTYPE = np.dtype([("q", "<u8"), ("r", "<u8"), ("same_genome", "<i4"), ("reserved", "<i4")])
SEARCH_LANES_MAX = 16  # SDF_SEARCH_LANES_MAX
assert PAIR_JOB_DTYPE.itemsize == 24
FILTER_Q_RC, FILTER_R_RC, FILTER_SKIP = 1, 2, 4
FILTER_UPPER_FAIL, FILTER_QGRAM_FAIL, FILTER_SHORT, FILTER_SKIPPED = 1, 2, 4, 8
FILTER_WAVE_MAX_LEN = 4096
FILTER_DEFAULTS = dict(min_uppercase=12, max_error=0.30, max_edit_error=0.15, gap_frequency=0.005)  # the reference's own
# strand bits of a stats task on the resident pool (include/sedef_hip.h: SDF_STATS_A_RC / SDF_STATS_B_RC; in `reserved`,
# stats_columns_pairs only)
STATS_A_RC, STATS_B_RC = 0x1, 0x2


class SdfError(RuntimeError):
    pass


class _FilterParams(C.Structure):
    _fields_ = [("min_uppercase", C.c_int32), ("reserved", C.c_int32), ("max_error", C.c_double), ("max_edit_error", C.c_double),
                ("gap_frequency", C.c_double)]


def filter_params(min_uppercase=12, max_error=0.30, max_edit_error=0.15, gap_frequency=0.005, reserved=0):
    """sdf_filter_params; the defaults are the reference's (src/globals.cc)."""
    return _FilterParams(int(min_uppercase), int(reserved), float(max_error), float(max_edit_error), float(gap_frequency))


class _ExtendParams(C.Structure):
    _fields_ = [("max_error", C.c_double), ("max_edit_error", C.c_double), ("max_sd_size", C.c_int32), ("same_genome", C.c_int32),
                ("reserved", C.c_int32 * 2)]


def extend_params(max_error=0.30, max_edit_error=0.15, max_sd_size=1 << 20, same_genome=False, reserved=(0, 0)):
    """sdf_extend_params; the defaults are the reference's (src/globals.cc)."""
    return _ExtendParams(float(max_error), float(max_edit_error), int(max_sd_size), int(bool(same_genome)), (C.c_int32 * 2)(*reserved))


class _AcceptRound(C.Structure):
    _fields_ = [("q", C.c_void_p), ("nq", C.c_size_t), ("act", C.c_void_p), ("na", C.c_size_t), ("windows", C.c_void_p),
                ("first", C.c_void_p), ("n_max", C.c_size_t), ("rolls", C.c_void_p), ("overlap", C.c_void_p), ("filter", C.c_void_p),
                ("hits", C.c_void_p), ("hit_filter", C.c_void_p), ("init_len", C.c_int32), ("min_read_size", C.c_int32),
                ("window_base", C.c_int32), ("reserved", C.c_int32)]


def accept_round(q, nq, act, na, windows, first, n_max, rolls, overlap, filt, hits, hit_filter, init_len, min_read_size,
                 window_base=0, reserved=0):
    """sdf_search_accept_round over pointers (ints or None): host memory for search_accept_host / search_accept_raw, device
    memory for search_accept_device."""
    return _AcceptRound(q, int(nq), act, int(na), windows, first, int(n_max), rolls, overlap, filt, hits, hit_filter, int(init_len),
                        int(min_read_size), int(window_base), int(reserved))


class _PairParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("separate_lowercase", C.c_int32), ("uppercase_seeds", C.c_int32),
                ("min_read_size", C.c_int32), ("same_genome", C.c_int32), ("filter", _FilterParams), ("extend", _ExtendParams),
                ("limit", C.c_void_p), ("n_limit", C.c_size_t), ("round_windows", C.c_size_t), ("debug_host_every", C.c_size_t)]


class _MinimRange(C.Structure):
    _fields_ = [("off", C.c_int64), ("len", C.c_int32), ("flags", C.c_int32)]


class _Scoring(C.Structure):
    _fields_ = [("m", C.c_int32), ("mat", C.c_int8 * 25), ("gapo", C.c_int8), ("gape", C.c_int8),
                ("pad_", C.c_int8)]


_lib = None


def library_path():
    return LIB_PATH


def load_library():
    """Loads the HIP library; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdfError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                       % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.sdf_device_count.restype = C.c_int
    L.sdf_create.restype = C.c_void_p
    L.sdf_create.argtypes = [C.c_int, C.c_size_t]
    L.sdf_destroy.argtypes = [C.c_void_p]
    L.sdf_last_error.restype = C.c_char_p
    L.sdf_last_error.argtypes = [C.c_void_p]
    L.sdf_packed_words.restype = C.c_size_t
    L.sdf_packed_words.argtypes = [C.c_int32]
    L.sdf_pack_codes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.sdf_band_cells.restype = C.c_int64
    L.sdf_band_cells.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.sdf_extz2_batch.restype = C.c_int
    L.sdf_extz2_batch.argtypes = [C.c_void_p, C.POINTER(_Scoring), C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_extz2_batch_brief.restype = C.c_int
    L.sdf_extz2_batch_brief.argtypes = [C.c_void_p, C.POINTER(_Scoring), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_pool_host.restype = C.c_void_p
    L.sdf_pool_host.argtypes = [C.c_void_p, C.c_size_t]
    L.sdf_pool_upload.restype = C.c_int
    L.sdf_pool_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.sdf_pool_bytes.restype = C.c_size_t
    L.sdf_pool_bytes.argtypes = [C.c_void_p]
    L.sdf_extz2_batch_pairs.restype = C.c_int
    L.sdf_extz2_batch_pairs.argtypes = [C.c_void_p, C.POINTER(_Scoring), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_extz2_batch_pairs_full.restype = C.c_int
    L.sdf_extz2_batch_pairs_full.argtypes = [C.c_void_p, C.POINTER(_Scoring), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_extz2_batch_pairs_view.restype = C.c_int
    L.sdf_extz2_batch_pairs_view.argtypes = [C.c_void_p, C.POINTER(_Scoring), C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.sdf_pool_append_fasta.restype = C.c_int
    L.sdf_pool_append_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_int32, C.c_int,
                                        C.POINTER(C.c_int64)]
    L.sdf_pool_sync.restype = C.c_int
    L.sdf_pool_sync.argtypes = [C.c_void_p]
    L.sdf_pool_range_classes.restype = C.c_int
    L.sdf_pool_range_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _cover = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sdf_pool_coverage.restype = C.c_int  # ctx, regions, n_regions, iv, n_iv, min_upper, out, iv_upper, iv_painted
    L.sdf_pool_coverage.argtypes = [C.c_void_p] + _cover
    L.sdf_pool_coverage_host.restype = C.c_int  # pool, pool_bytes, then the same
    L.sdf_pool_coverage_host.argtypes = [C.c_char_p, C.c_size_t] + _cover
    L.sdf_pool_fetch_ranges.restype = C.c_int
    L.sdf_pool_fetch_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.sdf_pool_fetch_plan.restype = C.c_int
    L.sdf_pool_fetch_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_int),
                                      C.POINTER(C.c_longlong), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.sdf_pool_fetch_ranges_device.restype = C.c_int
    L.sdf_pool_fetch_ranges_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    L.sdf_pool_share.restype = C.c_int
    L.sdf_pool_share.argtypes = [C.c_void_p, C.c_void_p]
    L.sdf_anchors_batch_strand.restype = C.c_int
    L.sdf_anchors_batch_strand.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
    L.sdf_anchors_batch_view_strand.restype = C.c_int
    L.sdf_anchors_batch_view_strand.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int,
                                                C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_size_t)]
    L.sdf_anchors_batch_more_strand.restype = C.c_int
    L.sdf_anchors_batch_more_strand.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t,
                                                C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_size_t)]
    L.sdf_reserve.restype = C.c_int
    L.sdf_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32]
    L.sdf_device_bytes.restype = C.c_size_t
    L.sdf_device_bytes.argtypes = [C.c_void_p]
    L.sdf_debug_live_device_bytes.restype = C.c_size_t
    L.sdf_debug_live_device_bytes.argtypes = []
    L.sdf_extz2_batch_device.restype = C.c_int
    L.sdf_extz2_batch_device.argtypes = [C.c_void_p, C.POINTER(_Scoring), C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.sdf_anchors_batch.restype = C.c_int
    L.sdf_anchors_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
    L.sdf_chain_batch.restype = C.c_int
    L.sdf_chain_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
    L.sdf_stats_columns_batch.restype = C.c_int
    L.sdf_stats_columns_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
    L.sdf_stats_columns_device.restype = C.c_int
    L.sdf_stats_columns_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    L.sdf_stats_columns_pairs.restype = C.c_int
    L.sdf_stats_columns_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.sdf_stats_cuts_pairs.restype = C.c_int
    L.sdf_stats_cuts_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_stats_cuts_pairs_device.restype = C.c_int
    L.sdf_stats_cuts_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.sdf_stats_columns_pairs_device.restype = C.c_int
    L.sdf_stats_columns_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
    L.sdf_minimizer_block.restype = C.c_int
    L.sdf_minimizer_block.argtypes = []
    L.sdf_pool_minimizers.restype = C.c_int
    L.sdf_pool_minimizers.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_pool_minimizers_device.restype = C.c_int
    L.sdf_pool_minimizers_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.sdf_pool_minimizer_index.restype = C.c_int
    L.sdf_pool_minimizer_index.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]
    _search = [C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_int, C.c_int, C.c_void_p,
               C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sdf_search_windows.restype = C.c_int
    L.sdf_search_windows.argtypes = [C.c_void_p] + _search
    L.sdf_search_windows_device.restype = C.c_int
    L.sdf_search_windows_device.argtypes = [C.c_void_p] + _search + [C.c_void_p]
    L.sdf_search_windows_host.restype = C.c_int
    L.sdf_search_windows_host.argtypes = _search
    _found = [C.c_void_p, C.c_size_t, C.c_void_p]  # found, nf, visible
    _found_dev = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]  # d_found, nf, found_entries_cap, d_found_entries, d_visible
    L.sdf_search_found_entries.restype = C.c_int
    L.sdf_search_found_entries.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.sdf_search_windows_found.restype = C.c_int
    L.sdf_search_windows_found.argtypes = [C.c_void_p] + _search[:11] + _found + _search[11:]
    L.sdf_search_windows_found_device.restype = C.c_int
    L.sdf_search_windows_found_device.argtypes = [C.c_void_p] + _search[:11] + _found_dev + _search[11:] + [C.c_void_p]
    L.sdf_search_windows_wide_device.restype = C.c_int  # ... used, n_wide_max, d_wide_total, stream
    L.sdf_search_windows_wide_device.argtypes = [C.c_void_p] + _search[:11] + _found_dev + _search[11:] + [C.c_size_t, C.c_void_p, C.c_void_p]
    L.sdf_search_windows_found_host.restype = C.c_int
    L.sdf_search_windows_found_host.argtypes = _search[:11] + _found + _search[11:]
    _overlap = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]  # q, nq, first, rolls
    _overlap_tail = [C.c_int32, C.c_int32, C.c_void_p]  # init_len, min_read_size, out
    L.sdf_search_overlap.restype = C.c_int
    L.sdf_search_overlap.argtypes = [C.c_void_p] + _overlap + _found + _overlap_tail
    L.sdf_search_overlap_host.restype = C.c_int
    L.sdf_search_overlap_host.argtypes = _overlap + _found + _overlap_tail
    L.sdf_search_overlap_device.restype = C.c_int
    L.sdf_search_overlap_device.argtypes = [C.c_void_p] + _overlap + [C.c_size_t] + _found_dev + _overlap_tail + [C.c_void_p, C.c_void_p]
    _roll = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]  # q, nq, windows, first, intervals
    _roll_tail = [C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]  # r .. out
    L.sdf_search_roll.restype = C.c_int
    L.sdf_search_roll.argtypes = [C.c_void_p] + _roll + _roll_tail
    L.sdf_search_roll_host.restype = C.c_int
    L.sdf_search_roll_host.argtypes = _roll + _roll_tail
    for fn in (L.sdf_search_roll_device, L.sdf_search_roll_setup_device):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + _roll + [C.c_size_t] + _roll_tail + [C.c_void_p]
    L.sdf_search_filter.restype = C.c_int
    L.sdf_search_filter.argtypes = [C.c_void_p, C.POINTER(_FilterParams), C.c_void_p, C.c_size_t, C.c_void_p]
    L.sdf_search_filter_device.restype = C.c_int
    L.sdf_search_filter_device.argtypes = [C.c_void_p, C.POINTER(_FilterParams), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.sdf_search_filter_phase_device.restype = C.c_int  # (profiles/search_filter.py; not in the header)
    L.sdf_search_filter_phase_device.argtypes = [C.c_void_p, C.POINTER(_FilterParams), C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p]
    L.sdf_search_filter_host.restype = C.c_int
    L.sdf_search_filter_host.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_FilterParams), C.c_void_p, C.c_size_t, C.c_void_p]
    _ftasks = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # q, nq, windows, first, intervals, rolls
    _ftasks_tail = [C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]  # len_q .. out
    L.sdf_search_filter_tasks_host.restype = C.c_int
    L.sdf_search_filter_tasks_host.argtypes = _ftasks + _ftasks_tail
    L.sdf_search_filter_tasks_device.restype = C.c_int
    L.sdf_search_filter_tasks_device.argtypes = [C.c_void_p] + _ftasks + [C.c_size_t] + _ftasks_tail + [C.c_void_p]
    _extend = _roll + [C.c_void_p, C.c_void_p]  # ... rolls, filter
    _extend_tail = [C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(_ExtendParams),
                    C.c_void_p]  # r .. out
    L.sdf_search_extend.restype = C.c_int
    L.sdf_search_extend.argtypes = [C.c_void_p] + _extend + _extend_tail
    L.sdf_search_extend_host.restype = C.c_int
    L.sdf_search_extend_host.argtypes = _extend + _extend_tail
    L.sdf_search_extend_device.restype = C.c_int
    L.sdf_search_extend_device.argtypes = [C.c_void_p] + _extend + [C.c_size_t] + _extend_tail + [C.c_void_p]
    L.sdf_search_extend_long_device.restype = C.c_int  # ... params, long_grow, n_long_max, batch, d_hits, d_left, stream
    L.sdf_search_extend_long_device.argtypes = [C.c_void_p] + _extend + [C.c_size_t] + _extend_tail[:-1] + \
        [C.c_int32, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    _htasks = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p]  # len_q .. out
    L.sdf_search_hit_tasks_host.restype = C.c_int
    L.sdf_search_hit_tasks_host.argtypes = [C.c_void_p, C.c_size_t] + _htasks
    L.sdf_search_hit_tasks_device.restype = C.c_int
    L.sdf_search_hit_tasks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p] + _htasks + [C.c_void_p]
    _accept = [C.POINTER(_AcceptRound), C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.sdf_search_accept.restype = C.c_int  # round, found, nf, found_cap, out, n_out, out_cap, status
    L.sdf_search_accept.argtypes = [C.c_void_p] + _accept
    L.sdf_search_accept_host.restype = C.c_int
    L.sdf_search_accept_host.argtypes = _accept
    L.sdf_search_accept_device.restype = C.c_int
    L.sdf_search_accept_device.argtypes = [C.c_void_p] + _accept + [C.c_void_p]
    L.sdf_search_pair_host.restype = C.c_int  # pool, pool_bytes, q_range, r_range, params, out, cap, used, stats
    L.sdf_search_pair_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_MinimRange), C.POINTER(_MinimRange), C.POINTER(_PairParams),
                                       C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.sdf_search_pair.restype = C.c_int  # ctx, q_range, r_range, params, out, cap, used, stats
    L.sdf_search_pair.argtypes = [C.c_void_p, C.POINTER(_MinimRange), C.POINTER(_MinimRange), C.POINTER(_PairParams), C.c_void_p,
                                  C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.sdf_search_pair_wide.restype = C.c_int  # ... stats, n_wide_max
    L.sdf_search_pair_wide.argtypes = L.sdf_search_pair.argtypes + [C.c_size_t]
    L.sdf_search_index_build.restype = C.c_int  # ctx, range, k, w, separate_lowercase, out
    L.sdf_search_index_build.argtypes = [C.c_void_p, C.POINTER(_MinimRange), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.sdf_search_index_free.restype = C.c_int
    L.sdf_search_index_free.argtypes = [C.c_void_p, C.c_void_p]
    L.sdf_search_index_info.restype = C.c_int
    L.sdf_search_index_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sdf_search_index_builds.restype = C.c_longlong
    L.sdf_search_index_builds.argtypes = [C.c_void_p]
    L.sdf_search_index_live.restype = C.c_size_t
    L.sdf_search_index_live.argtypes = [C.c_void_p]
    L.sdf_search_pair_indexed.restype = C.c_int  # ctx, q, r, params, out, cap, used, stats
    L.sdf_search_pair_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_PairParams), C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.c_void_p]
    L.sdf_search_pair_indexed_wide.restype = C.c_int  # ... stats, n_wide_max
    L.sdf_search_pair_indexed_wide.argtypes = L.sdf_search_pair_indexed.argtypes + [C.c_size_t]
    L.sdf_search_lanes_open.restype = C.c_int  # ctx, n_lanes, out
    L.sdf_search_lanes_open.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.sdf_search_lanes_close.restype = C.c_int
    L.sdf_search_lanes_close.argtypes = [C.c_void_p, C.c_void_p]
    L.sdf_search_pairs_indexed.restype = C.c_int  # ctx, lanes, jobs, n_jobs, params, n_wide_max, out, cap, used, first, stats
    L.sdf_search_pairs_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(_PairParams), C.c_size_t, C.c_void_p,
                                           C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]
    L.sdf_last_ms.restype = C.c_float
    L.sdf_last_ms.argtypes = [C.c_void_p, C.c_int]
    L.sdf_last_launches.restype = C.c_int
    L.sdf_last_launches.argtypes = [C.c_void_p]
    L.sdf_last_paired.restype = C.c_longlong
    L.sdf_last_paired.argtypes = [C.c_void_p]
    L.sdf_last_reran.restype = C.c_longlong
    L.sdf_last_reran.argtypes = [C.c_void_p]
    L.sdf_last_lane_tasks.restype = C.c_longlong
    L.sdf_last_lane_tasks.argtypes = [C.c_void_p]
    L.sdf_last_chain_classes.restype = C.c_int
    L.sdf_last_chain_classes.argtypes = [C.c_void_p, C.c_void_p]
    L.sdf_last_traceback_classes.restype = C.c_int
    L.sdf_last_traceback_classes.argtypes = [C.c_void_p, C.c_void_p]
    _lib = L
    return L


def packed_words(n):
    return int(load_library().sdf_packed_words(int(n)))


def pack_codes(codes):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros(packed_words(len(codes)), np.uint32)
    if len(codes):
        load_library().sdf_pack_codes(codes.ctypes.data, len(codes), out.ctypes.data)
    return out


def live_device_bytes():
    """sdf_debug_live_device_bytes: device bytes the buffers of all contexts of this process hold at this moment."""
    return int(load_library().sdf_debug_live_device_bytes())


def band_cells(qlen, tlen, w):
    return int(load_library().sdf_band_cells(qlen, tlen, w))


def _scoring(mat, gapo, gape, m=5):
    s = _Scoring()
    s.m = m
    mat = np.asarray(mat, dtype=np.int8)
    for i in range(min(25, len(mat))):
        s.mat[i] = int(mat[i])
    s.gapo, s.gape = gapo, gape
    return s


def sedef_mat(match=5, mismatch=-4):
    """The 5x5 matrix align_helper builds (reference: src/align.cc:41-44)."""
    a, b = match, mismatch if mismatch < 0 else -mismatch
    return np.array([a, b, b, b, 0, b, a, b, b, 0, b, b, a, b, 0, b, b, b, a, 0, 0, 0, 0, 0, 0],
                    dtype=np.int8)


class Config:
    """include/sedef_hip.h: sdf_config -- the library's settings as one opaque struct.  Config() holds what sdf_create would
    read from the environment NOW; Config(SDF_NO_PAIR=1, strip_cols=4) sets fields by their environment variable's or
    their own name (a wrong name or a value out of range raises); nothing is written to os.environ."""

    BYTES = 512  # (room for the struct: its first word is its size, checked below)

    def __init__(self, from_env=True, **settings):
        self.lib = load_library()
        self.buf = C.create_string_buffer(self.BYTES)
        err = C.create_string_buffer(512)
        if from_env:
            self.lib.sdf_config_from_env.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
            if self.lib.sdf_config_from_env(self.buf, err, len(err)) != 0:
                raise SdfError("environment: %s" % err.value.decode())
        else:
            self.lib.sdf_config_default.argtypes = [C.c_void_p]
            self.lib.sdf_config_default(self.buf)
        assert 0 < C.cast(self.buf, C.POINTER(C.c_uint32))[0] <= self.BYTES
        self.set(**settings)

    def set(self, **settings):
        err = C.create_string_buffer(512)
        self.lib.sdf_config_set.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
        for k, v in settings.items():
            if isinstance(v, bool):
                v = int(v)
            if self.lib.sdf_config_set(self.buf, k.encode(), str(v).encode(), err, len(err)) != 0:
                raise SdfError(err.value.decode())
        return self

    def dump(self):
        self.lib.sdf_config_dump.restype = C.c_size_t
        self.lib.sdf_config_dump.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        out = C.create_string_buffer(self.lib.sdf_config_dump(self.buf, None, 0))
        self.lib.sdf_config_dump(self.buf, out, len(out))
        return out.value.decode()

    def as_dict(self):
        return {k: float(v.split()[0]) for k, v in (ln.split("=", 1) for ln in self.dump().splitlines() if "=" in ln)}


def describe_config():
    lib = load_library()
    lib.sdf_config_describe.restype = C.c_size_t
    lib.sdf_config_describe.argtypes = [C.c_char_p, C.c_size_t]
    out = C.create_string_buffer(lib.sdf_config_describe(None, 0))
    lib.sdf_config_describe(out, len(out))
    return out.value.decode()


class Extz2Engine:
    """One context = one GPU (include/sedef_hip.h: sdf_create / sdf_create_cfg).  config: a Config, or a dict of settings
    on top of the environment's (Extz2Engine(0, config=dict(SDF_NO_PAIR=1)))."""

    def __init__(self, device=0, workspace_bytes=0, config=None):
        self.lib = load_library()
        if config is None:
            self.ctx = self.lib.sdf_create(device, workspace_bytes)
        else:
            cfg = config if isinstance(config, Config) else Config(**config)
            self.lib.sdf_create_cfg.restype = C.c_void_p
            self.lib.sdf_create_cfg.argtypes = [C.c_int, C.c_size_t, C.c_void_p]
            self.ctx = self.lib.sdf_create_cfg(device, workspace_bytes, cfg.buf)
        if not self.ctx:
            raise SdfError("sdf_create failed: %s" % self.lib.sdf_last_error(None).decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.sdf_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SdfError("rc=%d: %s" % (rc, self.lib.sdf_last_error(self.ctx).decode()))

    def align_pairs(self, pairs, w=-1, zdrop=-1, flag=0, mat=None, gapo=40, gape=1,
                    want=WANT_ALL):
        """pairs: list of (query_codes, target_codes).  w/zdrop/flag: scalar or per-pair list.
        Returns (results structured array, cigar pool)."""
        n = len(pairs)
        tasks = np.zeros(n, TASK_DTYPE)
        chunks, off = [], 0
        for k, (q, t) in enumerate(pairs):
            q = np.ascontiguousarray(q, dtype=np.uint8)
            t = np.ascontiguousarray(t, dtype=np.uint8)
            tasks["q_off"][k], tasks["qlen"][k] = off, len(q)
            off += len(q)
            tasks["t_off"][k], tasks["tlen"][k] = off, len(t)
            off += len(t)
            chunks += [q, t]
        pool = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
        tasks["w"], tasks["zdrop"], tasks["flag"] = w, zdrop, flag
        return self.align_batch(tasks, pool, mat=mat, gapo=gapo, gape=gape, want=want)

    def align_batch(self, tasks, pool, mat=None, gapo=40, gape=1, want=WANT_ALL, cigar_cap=None):
        tasks = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        n = len(tasks)
        sc = _scoring(sedef_mat() if mat is None else mat, gapo, gape)
        out = np.zeros(n, RESULT_DTYPE)
        if cigar_cap is None:
            cigar_cap = int((tasks["qlen"].astype(np.int64) + tasks["tlen"] + 2).sum()) + 1
        cig = np.zeros(cigar_cap, np.uint32)
        used = C.c_size_t(0)
        rc = self.lib.sdf_extz2_batch(self.ctx, C.byref(sc), tasks.ctypes.data, n, pool.ctypes.data,
                                      pool.nbytes, want, out.ctypes.data, cig.ctypes.data,
                                      cigar_cap, C.byref(used))
        self._check(rc)
        return out, cig[:used.value]

    def align_batch_brief(self, tasks, pool, mat=None, gapo=40, gape=1, cigar_cap=None):
        """sdf_extz2_batch_brief: 16-byte records (cigar_off, n_cigar, matches) instead of sdf_result."""
        tasks = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        n = len(tasks)
        sc = _scoring(sedef_mat() if mat is None else mat, gapo, gape)
        out = np.zeros(n, BRIEF_DTYPE)
        if cigar_cap is None:
            cigar_cap = int((tasks["qlen"].astype(np.int64) + tasks["tlen"] + 2).sum()) + 1
        cig = np.zeros(cigar_cap, np.uint32)
        used = C.c_size_t(0)
        self._check(self.lib.sdf_extz2_batch_brief(self.ctx, C.byref(sc), tasks.ctypes.data, n, pool.ctypes.data, pool.nbytes,
                                                   out.ctypes.data, cig.ctypes.data, cigar_cap, C.byref(used)))
        return out, cig[:used.value]

    def pool_upload(self, chars, pinned=True):
        """sdf_pool_host + sdf_pool_upload: raw FASTA characters (bytes) to HBM, where they stay; sdf_extz2_batch_pairs tasks
        name byte ranges of them.  pinned=False: straight from the caller's (pageable) buffer."""
        buf = np.frombuffer(chars, np.uint8)
        if pinned:
            p = self.lib.sdf_pool_host(self.ctx, len(buf))
            if not p:
                raise SdfError(self.lib.sdf_last_error(self.ctx).decode())
            C.memmove(p, buf.ctypes.data, len(buf))
            self._check(self.lib.sdf_pool_upload(self.ctx, p, len(buf)))
        else:
            self._keep = buf  # (unchanged until the next call that returns data)
            self._check(self.lib.sdf_pool_upload(self.ctx, buf.ctypes.data, len(buf)))
        return int(self.lib.sdf_pool_bytes(self.ctx))

    def pool_append_fasta(self, raw, n_bases, line_bases, line_bytes, reset=False):
        """sdf_pool_append_fasta: one FASTA record's sequence lines as the file has them (bytes from the .fai offset: line_bases
        bases, then line_bytes - line_bases line-end bytes, repeated) -> its bases behind the ones resident; the device drops
        the line ends.  Returns the pool offset of the record's base 0."""
        buf = np.frombuffer(raw, np.uint8)
        self._keep = buf  # (unchanged until the next call that returns data)
        off = C.c_int64(-1)
        self._check(self.lib.sdf_pool_append_fasta(self.ctx, buf.ctypes.data if len(buf) else None, len(buf), int(n_bases),
                                                   int(line_bases), int(line_bytes), int(bool(reset)), C.byref(off)))
        return int(off.value)

    def pool_sync(self):
        """sdf_pool_sync: the uploads enqueued so far have left their host buffers."""
        self._check(self.lib.sdf_pool_sync(self.ctx))

    def pool_bytes(self):
        return int(self.lib.sdf_pool_bytes(self.ctx))

    def pool_range_classes(self, ranges, check=True):
        """sdf_pool_range_classes: the character classes of ranges of the resident pool.  ranges: a POOL_RANGE_DTYPE array, or
        (off, len) pairs.  Returns a RANGE_CLASSES_DTYPE array (upper_acgt, lower_acgt, n_any, other), one record per range;
        check=False: (rc, that array, sdf_last_error) instead of raising."""
        if not (isinstance(ranges, np.ndarray) and ranges.dtype == POOL_RANGE_DTYPE):
            pairs = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
            ranges = np.zeros(len(pairs), POOL_RANGE_DTYPE)
            ranges["off"], ranges["len"] = pairs[:, 0], pairs[:, 1]
        ranges = np.ascontiguousarray(ranges)
        n = len(ranges)
        out = np.zeros(n, RANGE_CLASSES_DTYPE)
        rc = self.lib.sdf_pool_range_classes(self.ctx, ranges.ctypes.data if n else None, n, out.ctypes.data if n else None)
        if not check:
            return rc, out, self.lib.sdf_last_error(self.ctx).decode()
        self._check(rc)
        return out

    def pool_coverage(self, regions, intervals, min_upper, check=True):
        """sdf_pool_coverage: how two interval sets cover ranges of the resident pool.  regions: a POOL_RANGE_DTYPE array, or
        (off, len) pairs; intervals: a COVER_INTERVAL_DTYPE array, or (region, start, len, set, partner) rows.  Returns (counts,
        upper, painted): a COVER_COUNTS_DTYPE record per region, the uppercase bytes of every interval (int32) and whether it was
        painted (uint8); check=False: (rc, that tuple, sdf_last_error) instead of raising."""
        rc, out = pool_coverage_call(self.lib.sdf_pool_coverage, (self.ctx,), regions, intervals, min_upper)
        if not check:
            return rc, out, self.lib.sdf_last_error(self.ctx).decode()
        self._check(rc)
        return out

    def pool_fetch_raw(self, ranges, rc=None):
        """sdf_pool_fetch_ranges: the characters of ranges of the resident pool, reverse-complemented where asked, packed back
        to back.  ranges: (off, len) pairs, rc: one truth value for all or one per range -- or a POOL_FETCH_DTYPE array, whose
        flags and dst_off are used as they are (rc must be None).  Returns (bytes as one numpy.uint8 array, offsets): range i
        is out[offsets[i]:offsets[i + 1]] for pairs; for a POOL_FETCH_DTYPE array `offsets` is its dst_off and the array is as
        long as the furthest destination."""
        if isinstance(ranges, np.ndarray) and ranges.dtype == POOL_FETCH_DTYPE:
            assert rc is None
            recs = np.ascontiguousarray(ranges)
            offsets = recs["dst_off"].astype(np.int64)
            size = int((offsets + recs["len"]).max()) if len(recs) else 0
        else:
            pairs = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
            recs = np.zeros(len(pairs), POOL_FETCH_DTYPE)
            recs["off"], recs["len"] = pairs[:, 0], pairs[:, 1]
            if rc is not None:
                recs["flags"] = np.where(np.broadcast_to(np.asarray(rc, dtype=bool), len(pairs)), FETCH_RC, 0)
            offsets = np.zeros(len(pairs) + 1, np.int64)
            np.cumsum(np.maximum(pairs[:, 1], 0), out=offsets[1:])
            recs["dst_off"] = offsets[:-1]
            size = int(offsets[-1])
        out = np.zeros(size, np.uint8)
        n = len(recs)
        self._check(self.lib.sdf_pool_fetch_ranges(self.ctx, recs.ctypes.data if n else None, n, out.ctypes.data if size else None,
                                                   size))
        return out, offsets

    def pool_fetch(self, ranges, rc=None):
        """The same as a list of bytes objects, one per (off, len) range."""
        out, offsets = self.pool_fetch_raw(np.asarray(ranges, dtype=np.int64).reshape(-1, 2), rc)
        return [out[int(a):int(b)].tobytes() for a, b in zip(offsets[:-1], offsets[1:])]

    def pool_fetch_plan(self, ranges, pool_bytes=None, dst_bytes=None):
        """sdf_pool_fetch_plan: the device form's records of a POOL_FETCH_DTYPE array.  Returns (rc, POOL_FETCH_REC_DTYPE array,
        any_rc, n_seg, bytes, index of the first offending range); pool_bytes / dst_bytes default to the resident pool's size
        and to no bound."""
        recs = np.ascontiguousarray(ranges, dtype=POOL_FETCH_DTYPE)
        n = len(recs)
        out = np.zeros(n, POOL_FETCH_REC_DTYPE)
        any_rc, n_seg, nbytes, bad = C.c_int(0), C.c_longlong(0), C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.sdf_pool_fetch_plan(recs.ctypes.data if n else None, n, self.pool_bytes() if pool_bytes is None else pool_bytes,
                                          (1 << 62) if dst_bytes is None else dst_bytes, out.ctypes.data if n else None,
                                          C.byref(any_rc), C.byref(n_seg), C.byref(nbytes), C.byref(bad))
        return rc, out, int(any_rc.value), int(n_seg.value), int(nbytes.value), int(bad.value)

    def pool_fetch_device(self, d_recs, n, any_rc, n_seg, d_dst, stream=None):
        """sdf_pool_fetch_ranges_device: records (POOL_FETCH_REC_DTYPE, as pool_fetch_plan makes them) and destination in HBM,
        given as device pointers."""
        self._check(self.lib.sdf_pool_fetch_ranges_device(self.ctx, d_recs, n, int(bool(any_rc)), n_seg, d_dst, stream))

    def pool_share(self, owner):
        """sdf_pool_share: this context reads `owner`'s resident pool from now on (a view: no memory of its own).  The owner
        outlives the view and leaves its pool alone meanwhile."""
        self._check(self.lib.sdf_pool_share(self.ctx, owner.ctx))
        return self.pool_bytes()

    def align_batch_pairs(self, tasks, mat=None, gapo=40, gape=1, want=None, cigar_cap=None, q_rc=None, t_rc=None, view=False):
        """sdf_extz2_batch_pairs (want=None: 16-byte records) / sdf_extz2_batch_pairs_full: q_off / t_off of the tasks are byte
        offsets into the resident character pool; align_dna and the packing happen on the device.  q_rc / t_rc: per task (or
        one for all), that side is the reverse complement of its range (TASK_Q_RC / TASK_T_RC are or-ed into the flags).
        view=True: sdf_extz2_batch_pairs_view, results copied out of the context's staging."""
        tasks = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        if q_rc is not None or t_rc is not None:
            tasks = tasks.copy()
            for side, bit in ((q_rc, TASK_Q_RC), (t_rc, TASK_T_RC)):
                if side is not None:
                    tasks["flag"] |= np.where(np.broadcast_to(np.asarray(side, bool), tasks.shape), bit, 0).astype(np.int32)
        n = len(tasks)
        sc = _scoring(sedef_mat() if mat is None else mat, gapo, gape)
        if view:
            pb, pc, used = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
            self._check(self.lib.sdf_extz2_batch_pairs_view(self.ctx, C.byref(sc), tasks.ctypes.data, n, C.byref(pb), C.byref(pc),
                                                            C.byref(used)))
            out = np.frombuffer((C.c_char * (n * BRIEF_DTYPE.itemsize)).from_address(pb.value), BRIEF_DTYPE).copy() if n else \
                np.zeros(0, BRIEF_DTYPE)
            cig = np.frombuffer((C.c_char * (used.value * 4)).from_address(pc.value), np.uint32).copy() if used.value else \
                np.zeros(0, np.uint32)
            return out, cig
        if cigar_cap is None:
            cigar_cap = int((tasks["qlen"].astype(np.int64) + tasks["tlen"] + 2).sum()) + 1
        cig = np.zeros(cigar_cap, np.uint32)
        used = C.c_size_t(0)
        if want is None:
            out = np.zeros(n, BRIEF_DTYPE)
            self._check(self.lib.sdf_extz2_batch_pairs(self.ctx, C.byref(sc), tasks.ctypes.data, n, out.ctypes.data,
                                                       cig.ctypes.data, cigar_cap, C.byref(used)))
        else:
            out = np.zeros(n, RESULT_DTYPE)
            self._check(self.lib.sdf_extz2_batch_pairs_full(self.ctx, C.byref(sc), tasks.ctypes.data, n, want, out.ctypes.data,
                                                            cig.ctypes.data, cigar_cap, C.byref(used)))
        return out, cig[:used.value]

    def batch_call(self, form, tasks, pool=None, want=WANT_ALL, cigar_cap=0, guard=0, sentinel=0, fill=0, null_cigar=False,
                   mat=None, gapo=40, gape=1):
        """One host-form batch call that reports instead of raising.  form: "batch" / "brief" (the tasks name bytes of `pool`)
        or "pairs" / "pairs_full" (bytes of the resident pool); `want` is read by "batch" and "pairs_full".  Every byte of the
        records starts out as `fill`; the CIGAR pool handed over is cigar_cap words long and has `guard` more words behind
        it, all of them `sentinel` (null_cigar: no pool at all).  Returns (rc, cigar_used, records, the pool's words with the
        guard, sdf_last_error) -- a caller that sizes its pool by an estimate reads rc == -5 and the need from these."""
        tasks = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        n = len(tasks)
        sc = _scoring(sedef_mat() if mat is None else mat, gapo, gape)
        out = np.zeros(n, BRIEF_DTYPE if form in ("brief", "pairs") else RESULT_DTYPE)
        out.view(np.uint8)[:] = fill
        cig = np.full(cigar_cap + guard, sentinel, np.uint32)
        cig_p = None if null_cigar else cig.ctypes.data
        used = C.c_size_t(0)
        if form in ("batch", "brief"):
            pool = np.ascontiguousarray(pool, dtype=np.uint8)
            head = (self.ctx, C.byref(sc), tasks.ctypes.data, n, pool.ctypes.data, pool.nbytes)
            if form == "batch":
                rc = self.lib.sdf_extz2_batch(*head, want, out.ctypes.data, cig_p, cigar_cap, C.byref(used))
            else:
                rc = self.lib.sdf_extz2_batch_brief(*head, out.ctypes.data, cig_p, cigar_cap, C.byref(used))
        elif form == "pairs":
            rc = self.lib.sdf_extz2_batch_pairs(self.ctx, C.byref(sc), tasks.ctypes.data, n, out.ctypes.data, cig_p, cigar_cap,
                                                C.byref(used))
        elif form == "pairs_full":
            rc = self.lib.sdf_extz2_batch_pairs_full(self.ctx, C.byref(sc), tasks.ctypes.data, n, want, out.ctypes.data, cig_p,
                                                     cigar_cap, C.byref(used))
        else:
            raise ValueError("batch_call: unknown form %r" % (form,))
        return rc, int(used.value), out, cig, self.lib.sdf_last_error(self.ctx).decode()

    def reserve(self, max_tasks, max_bases, workspace_bytes=0, flags=0):
        """sdf_reserve: buffers, pinned staging and pipeline streams sized once (flags: RESERVE_BRIEF | RESERVE_ANCHORS)."""
        self._check(self.lib.sdf_reserve(self.ctx, int(max_tasks), int(max_bases), int(workspace_bytes), int(flags)))

    def device_bytes(self):
        return int(self.lib.sdf_device_bytes(self.ctx))

    def align_batch_device(self, tasks, d_pool, d_out, d_cig, cigar_cap, mat=None, gapo=40, gape=1,
                           want=WANT_ALL, stream=None, check=True):
        """Device-resident form: d_pool/d_out/d_cig are raw HBM addresses (ints; d_cig None: no CIGAR pool).  check=False:
        returns (rc, cigar_used, sdf_last_error) instead of raising -- with rc == -5 cigar_used is the need."""
        tasks = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        sc = _scoring(sedef_mat() if mat is None else mat, gapo, gape)
        used = C.c_size_t(0)
        rc = self.lib.sdf_extz2_batch_device(self.ctx, C.byref(sc), tasks.ctypes.data, len(tasks),
                                             d_pool, want, d_out, d_cig, cigar_cap, C.byref(used),
                                             stream)
        if not check:
            return rc, int(used.value), self.lib.sdf_last_error(self.ctx).decode()
        self._check(rc)
        return used.value

    def anchors_batch_resident(self, desc, kmer=11, r_rc=None, pool_bytes=None, mode="copy", keep=0):
        """sdf_anchors_batch_strand / _view_strand / _more_strand (mode "copy" / "view" / "more") on the resident pool.  desc: an
        ANCHOR_PAIR_DTYPE array whose offsets are pool bytes; r_rc: per pair, the reference range is read reverse-complemented
        (None: all forward).  Returns (anchors, out_off) as arrays; `more` writes behind the first `keep` anchors of the staging."""
        desc = np.ascontiguousarray(desc, dtype=ANCHOR_PAIR_DTYPE)
        n = len(desc)
        rc_arr = None if r_rc is None else np.ascontiguousarray(np.asarray(r_rc) != 0, dtype=np.uint8)
        rc_p = None if rc_arr is None else rc_arr.ctypes.data
        if pool_bytes is None:
            pool_bytes = self.pool_bytes()
        offs = np.zeros(n + 1, np.int64)
        used = C.c_size_t(0)
        if mode == "copy":
            cap = 1 << 16
            while True:
                out = np.zeros(cap, ANCHOR_DTYPE)
                rc = self.lib.sdf_anchors_batch_strand(self.ctx, desc.ctypes.data, rc_p, n, None, pool_bytes, kmer, out.ctypes.data,
                                                       cap, offs.ctypes.data, C.byref(used))
                if rc == -5:
                    cap = used.value
                    continue
                self._check(rc)
                return out[:used.value], offs
        p = C.c_void_p()
        if mode == "view":
            self._check(self.lib.sdf_anchors_batch_view_strand(self.ctx, desc.ctypes.data, rc_p, n, None, pool_bytes, kmer,
                                                               C.byref(p), offs.ctypes.data, C.byref(used)))
        else:
            self._check(self.lib.sdf_anchors_batch_more_strand(self.ctx, desc.ctypes.data, rc_p, n, pool_bytes, kmer, int(keep),
                                                               C.byref(p), offs.ctypes.data, C.byref(used)))
        out = np.frombuffer((C.c_char * (used.value * 16)).from_address(p.value), ANCHOR_DTYPE).copy() if used.value else \
            np.zeros(0, ANCHOR_DTYPE)
        return out, offs

    def anchors_batch(self, pairs, kmer=11, r_rc=None):
        """GPU generate_anchors.  pairs: list of (query str, ref str, same_chr, delta).  Returns one list of
        (q, r, l, has_u) per pair (include/sedef_hip.h: sdf_anchors_batch).  r_rc: per pair, the anchors are those of the
        reverse complement of `ref str` (sdf_anchors_batch_strand)."""
        n = len(pairs)
        desc = np.zeros(n, ANCHOR_PAIR_DTYPE)
        chunks, off = [], 0
        for k, (q, r, same, delta) in enumerate(pairs):
            qb, rb = q.encode(), r.encode()
            desc[k] = (off, off + len(qb), len(qb), len(rb), int(same), int(delta))
            off += len(qb) + len(rb)
            chunks += [qb, rb]
        pool = b"".join(chunks)
        cap = max(1024, off)
        while True:
            out = np.zeros(cap, ANCHOR_DTYPE)
            offs = np.zeros(n + 1, np.int64)
            used = C.c_size_t(0)
            if r_rc is None:
                rc = self.lib.sdf_anchors_batch(self.ctx, desc.ctypes.data, n, pool, len(pool), kmer, out.ctypes.data, cap,
                                                offs.ctypes.data, C.byref(used))
            else:
                strand = np.ascontiguousarray(np.asarray(r_rc) != 0, dtype=np.uint8)
                assert len(strand) == n
                rc = self.lib.sdf_anchors_batch_strand(self.ctx, desc.ctypes.data, strand.ctypes.data, n, pool, len(pool), kmer,
                                                       out.ctypes.data, cap, offs.ctypes.data, C.byref(used))
            if rc == -5:
                cap = used.value
                continue
            self._check(rc)
            break
        return [[tuple(int(x) for x in a) for a in out[offs[k]:offs[k + 1]]] for k in range(n)]

    def chain_batch(self, anchor_lists, max_chain_gap=210, match_chain_score=4):
        """GPU chain_anchors.  anchor_lists: one (m, 4) int32 array of (q, r, l, has_u) per pair.  Returns one
        (path, boundaries) per pair like the reference's chain_anchors (include/sedef_hip.h: sdf_chain_batch)."""
        n = len(anchor_lists)
        arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 4) for a in anchor_lists]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        total = int(off[n])
        flat = np.concatenate(arrs) if total else np.zeros((0, 4), np.int32)
        path = np.zeros(max(total, 1), np.int32)
        bounds = np.zeros(2 * (total + n) + 2, np.int32)
        nb = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.sdf_chain_batch(self.ctx, flat.ctypes.data, off.ctypes.data, n, max_chain_gap,
                                             match_chain_score, path.ctypes.data, bounds.ctypes.data, nb.ctypes.data))
        out = []
        for i in range(n):
            b0 = 2 * (int(off[i]) + i)
            out.append((path[off[i]:off[i + 1]].copy(), bounds[b0:b0 + 2 * int(nb[i])].reshape(-1, 2).copy()))
        return out

    def stats_columns_batch(self, alignments):
        """Per-alignment columns of `stats generate`.  alignments: list of (a, b, cigar) with a, b the FASTA characters
        (str / bytes) and cigar uint32 runs len << 4 | op (0 'M', 1 'D', 2 'I').  Returns a STATS_COLS_DTYPE array
        (include/sedef_hip.h: sdf_stats_columns_batch)."""
        n = len(alignments)
        tasks = np.zeros(n, STATS_TASK_DTYPE)
        chunks, cigs, off, coff = [], [], 0, 0
        for k, (a, b, cg) in enumerate(alignments):
            a = a.encode() if isinstance(a, str) else bytes(a)
            b = b.encode() if isinstance(b, str) else bytes(b)
            cg = np.ascontiguousarray(cg, dtype=np.uint32)
            tasks[k] = (off, off + len(a), len(a), len(b), coff, len(cg), 0)
            off += len(a) + len(b)
            coff += len(cg)
            chunks += [a, b]
            cigs.append(cg)
        pool = b"".join(chunks)
        cig = np.concatenate(cigs) if cigs else np.zeros(0, np.uint32)
        out = np.zeros(n, STATS_COLS_DTYPE)
        self._check(self.lib.sdf_stats_columns_batch(self.ctx, tasks.ctypes.data, n, pool, len(pool), cig.ctypes.data,
                                                     len(cig), out.ctypes.data))
        return out

    def stats_columns_device(self, d_tasks, n, d_pool, d_cigar, d_out, stream=None):
        """The same over device pointers (ints); asynchronous on `stream` when one is given."""
        self._check(self.lib.sdf_stats_columns_device(self.ctx, d_tasks, n, d_pool, d_cigar, d_out, stream))

    def stats_columns_pairs(self, tasks, cigar, a_rc=None, b_rc=None, out=None):
        """sdf_stats_columns_pairs: a_off / b_off of the tasks (STATS_TASK_DTYPE) are byte offsets into the resident character
        pool (pool_upload / pool_append_fasta), cigar the uint32 runs the tasks' cigar_off / n_cigar name.  a_rc / b_rc: per
        task (or one for all), that side is the reverse complement of its range (STATS_A_RC / STATS_B_RC are or-ed into
        `reserved`).  out: a STATS_COLS_DTYPE array to fill (it holds the records also when the call raises for a CIGAR
        that does not fit).  Returns the STATS_COLS_DTYPE array."""
        tasks = np.ascontiguousarray(tasks, dtype=STATS_TASK_DTYPE)
        if a_rc is not None or b_rc is not None:
            tasks = tasks.copy()
            for side, bit in ((a_rc, STATS_A_RC), (b_rc, STATS_B_RC)):
                if side is not None:
                    tasks["reserved"] |= np.where(np.broadcast_to(np.asarray(side, bool), tasks.shape), bit, 0).astype(np.uint32)
        cig = np.ascontiguousarray(cigar, dtype=np.uint32)
        n = len(tasks)
        if out is None:
            out = np.zeros(n, STATS_COLS_DTYPE)
        assert out.dtype == STATS_COLS_DTYPE and len(out) == n and out.flags.c_contiguous
        self._check(self.lib.sdf_stats_columns_pairs(self.ctx, tasks.ctypes.data if n else None, n,
                                                     cig.ctypes.data if len(cig) else None, len(cig),
                                                     out.ctypes.data if n else None))
        return out

    def stats_columns_pairs_device(self, d_tasks, n, any_rc, d_cigar, d_out, stream=None):
        """The same over device pointers (ints) of tasks, runs and records; asynchronous on `stream` when one is given
        (pool_sync() first: the pool's uploads run on the context's stream).  any_rc: some task may carry a strand bit."""
        self._check(self.lib.sdf_stats_columns_pairs_device(self.ctx, d_tasks, n, int(bool(any_rc)), d_cigar, d_out, stream))

    def stats_cuts_pairs_raw(self, tasks, cigar, scores=(5, -4, -40, -1), cap=None, pieces=None):
        """sdf_stats_cuts_pairs as it is: returns (rc, first, pieces, used).  tasks as stats_columns_pairs takes them (strand
        bits in `reserved`), scores (match, mismatch, gap_open, gap_extend) of the trims, cap: capacity in pieces (default:
        len(pieces), or what the batch needs, found by a first call), pieces: a STATS_PIECE_DTYPE array to fill."""
        tasks = np.ascontiguousarray(tasks, dtype=STATS_TASK_DTYPE)
        cig = np.ascontiguousarray(cigar, dtype=np.uint32)
        n = len(tasks)
        first = np.zeros(n + 1, np.uint64)
        used = C.c_size_t(0)

        def call(buf, c):
            return self.lib.sdf_stats_cuts_pairs(self.ctx, tasks.ctypes.data if n else None, n, cig.ctypes.data if len(cig) else None,
                                                 len(cig), *[int(x) for x in scores], first.ctypes.data,
                                                 buf.ctypes.data if len(buf) else None, c, C.byref(used))
        if pieces is None:
            if cap is None:
                rc = call(np.zeros(0, STATS_PIECE_DTYPE), 0)
                if rc not in (0, -5):  # (SDF_ERR_CIGAR_OVERFLOW: *pieces_used holds the need)
                    return rc, first, np.zeros(0, STATS_PIECE_DTYPE), int(used.value)
                cap = int(used.value)
            pieces = np.zeros(cap, STATS_PIECE_DTYPE)
        assert pieces.dtype == STATS_PIECE_DTYPE and pieces.flags.c_contiguous
        rc = call(pieces, len(pieces) if cap is None else cap)
        return rc, first, pieces, int(used.value)

    def stats_cuts_pairs(self, tasks, cigar, a_rc=None, b_rc=None, scores=(5, -4, -40, -1)):
        """sdf_stats_cuts_pairs: per alignment of the resident pool (tasks, cigar, a_rc / b_rc as stats_columns_pairs takes
        them) the pieces `stats generate` cuts at assembly gaps, before and after trim_back / trim_front, and the matches
        inside.  Returns (first, pieces): pieces[first[i]:first[i + 1]] (STATS_PIECE_DTYPE) are alignment i's, in column order."""
        tasks = np.ascontiguousarray(tasks, dtype=STATS_TASK_DTYPE)
        if a_rc is not None or b_rc is not None:
            tasks = tasks.copy()
            for side, bit in ((a_rc, STATS_A_RC), (b_rc, STATS_B_RC)):
                if side is not None:
                    tasks["reserved"] |= np.where(np.broadcast_to(np.asarray(side, bool), tasks.shape), bit, 0).astype(np.uint32)
        rc, first, pieces, used = self.stats_cuts_pairs_raw(tasks, cigar, scores)
        self._check(rc)
        return first.astype(np.int64), pieces[:used]

    def stats_cuts_pairs_device(self, d_tasks, n, any_rc, d_cigar, d_first, d_pieces, cap, scores=(5, -4, -40, -1), stream=None):
        """The same over device pointers (ints) of tasks, runs, first (n + 1 uint64) and records; asynchronous on `stream` when
        one is given (pool_sync() first), else returns the pieces the batch needs (raises when they exceed cap)."""
        used = C.c_size_t(0)
        self._check(self.lib.sdf_stats_cuts_pairs_device(self.ctx, d_tasks, n, int(bool(any_rc)), d_cigar, *[int(x) for x in scores],
                                                         d_first, d_pieces, cap, C.byref(used), stream))
        return int(used.value)

    @staticmethod
    def minim_ranges(ranges, rc=None):
        """A MINIM_RANGE_DTYPE array from (off, len) pairs; rc: one truth value for all or one per range (MINIM_RC in
        `flags`).  An array of that dtype passes through (rc must be None)."""
        if isinstance(ranges, np.ndarray) and ranges.dtype == MINIM_RANGE_DTYPE:
            assert rc is None
            return np.ascontiguousarray(ranges)
        pairs = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        recs = np.zeros(len(pairs), MINIM_RANGE_DTYPE)
        recs["off"], recs["len"] = pairs[:, 0], pairs[:, 1]
        if rc is not None:
            recs["flags"] = np.where(np.broadcast_to(np.asarray(rc, dtype=bool), len(pairs)), MINIM_RC, 0)
        return recs

    def pool_minimizers_raw(self, ranges, k=12, w=16, separate_lowercase=True, cap=None, out=None, index=False):
        """sdf_pool_minimizers (index=True: sdf_pool_minimizer_index) as it is.  ranges: a MINIM_RANGE_DTYPE array; cap:
        capacity in records (default: len(out), or what the ranges need, found by a first call); out: a MINIMIZER_DTYPE array
        to fill.  Returns (rc, first, records, used), and (n_groups, threshold) behind them for the index."""
        recs = np.ascontiguousarray(ranges, dtype=MINIM_RANGE_DTYPE)
        n = len(recs)
        first = np.zeros(n + 1, np.uint64)
        n_groups, threshold = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        used = C.c_size_t(0)

        def call(buf, c):
            head = (self.ctx, recs.ctypes.data if n else None, n, int(k), int(w), int(bool(separate_lowercase)), first.ctypes.data,
                    buf.ctypes.data if len(buf) else None, c, C.byref(used))
            if index:
                return self.lib.sdf_pool_minimizer_index(*head, n_groups.ctypes.data, threshold.ctypes.data)
            return self.lib.sdf_pool_minimizers(*head)
        if out is None:
            if cap is None:
                rc = call(np.zeros(0, MINIMIZER_DTYPE), 0)
                if rc not in (0, -5):  # (SDF_ERR_CIGAR_OVERFLOW: *used holds the need)
                    return (rc, first, np.zeros(0, MINIMIZER_DTYPE), int(used.value)) + ((n_groups, threshold) if index else ())
                cap = int(used.value)
            out = np.zeros(cap, MINIMIZER_DTYPE)
        assert out.dtype == MINIMIZER_DTYPE and out.flags.c_contiguous
        rc = call(out, len(out) if cap is None else cap)
        return (rc, first, out, int(used.value)) + ((n_groups, threshold) if index else ())

    def pool_minimizers(self, ranges, k=12, w=16, separate_lowercase=True, rc=None):
        """sdf_pool_minimizers: the winnowed minimizers (the reference's get_minimizers) of ranges of the resident pool --
        (off, len) pairs with rc as minim_ranges takes it, or a MINIM_RANGE_DTYPE array.  Returns (first, records): a
        MINIMIZER_DTYPE array (hash, loc, status, range), records[first[i]:first[i + 1]] range i's in ascending loc; loc counts
        in the reverse complement for a reversed range."""
        code, first, out, used = self.pool_minimizers_raw(self.minim_ranges(ranges, rc), k, w, separate_lowercase)
        self._check(code)
        return first.astype(np.int64), out[:used]

    def pool_minimizers_device(self, d_ranges, n, any_rc, d_first, d_out, cap, k=12, w=16, separate_lowercase=True, stream=None):
        """The same over device pointers (ints) of ranges, first (n + 1 uint64) and records; on `stream` when one is given
        (pool_sync() first), else returns the records the ranges have (raises when they exceed cap)."""
        used = C.c_size_t(0)
        self._check(self.lib.sdf_pool_minimizers_device(self.ctx, d_ranges, n, int(bool(any_rc)), int(k), int(w),
                                                        int(bool(separate_lowercase)), d_first, d_out, cap, C.byref(used), stream))
        return int(used.value)

    def pool_minimizer_index(self, ranges, k=12, w=16, separate_lowercase=True, rc=None):
        """sdf_pool_minimizer_index: the reference's Index of every range.  Returns (first, sorted, n_groups, threshold):
        sorted[first[i]:first[i + 1]] are range i's minimizers in ascending (status, hash, loc) order -- a group is a run of equal
        (status, hash) --, n_groups[i] its groups and threshold[i] the reference's cutoff (MINIM_THRESHOLD_NONE where none)."""
        code, first, out, used, n_groups, threshold = self.pool_minimizers_raw(self.minim_ranges(ranges, rc), k, w,
                                                                              separate_lowercase, index=True)
        self._check(code)
        return first.astype(np.int64), out[:used], n_groups, threshold

    def search_windows_raw(self, q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, cap=None,
                           out=None):
        """sdf_search_windows as it is.  q: the query's minimizers in loc order, r_sorted: the reference's in index order
        (MINIMIZER_DTYPE arrays); limit: the table of relaxed_jaccard_estimate by query_size; cap: capacity in intervals
        (default: len(out), or what the windows need, found by a first call); out: a SEARCH_INTERVAL_DTYPE array to fill.
        Returns (rc, first, windows, intervals, used)."""
        return search_windows_call(self.lib.sdf_search_windows, (self.ctx,), q, r_sorted, r_threshold, len_q, init_len, same_genome,
                                   uppercase_seeds, limit, cap, out)

    def search_windows_device(self, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome, uppercase_seeds, d_limit,
                              n_limit, d_first, d_windows, d_out, cap, stream=None):
        """The same over device pointers (ints) of the records, the table, first (nq + 1 uint64), windows and intervals; on
        `stream` when one is given, else returns the intervals the windows have (raises when they exceed cap).  A WIDE window
        is flagged and has no interval."""
        used = C.c_size_t(0)
        self._check(self.lib.sdf_search_windows_device(self.ctx, d_q, nq, int(len_q), d_r_sorted, nr, int(r_threshold), int(init_len),
                                                       int(bool(same_genome)), int(bool(uppercase_seeds)), d_limit, n_limit, d_first,
                                                       d_windows, d_out, cap, C.byref(used), stream))
        return int(used.value)

    def search_windows(self, q_range, r_range, k=12, w=16, separate_lowercase=True, init_len=700, same_genome=False,
                       uppercase_seeds=True, limit=(), r_threshold=None):
        """The reference intervals of every query window (the front half of the reference's search(), empty tree): q_range and
        r_range are (off, len) or (off, len, rc) ranges of the resident pool; the query's minimizers come from pool_minimizers,
        the reference's index and threshold from pool_minimizer_index (r_threshold: another threshold).  Returns (first,
        windows, intervals): SEARCH_WINDOW_DTYPE and SEARCH_INTERVAL_DTYPE arrays, intervals[first[i]:first[i + 1]] those of
        query minimizer i."""
        def one(rng):
            return self.minim_ranges([rng[:2]], rc=bool(rng[2]) if len(rng) > 2 else None)
        _, q = self.pool_minimizers(one(q_range), k, w, separate_lowercase)
        _, r_sorted, _, threshold = self.pool_minimizer_index(one(r_range), k, w, separate_lowercase)
        threshold = int(threshold[0]) if r_threshold is None else int(r_threshold)
        code, first, windows, out, used = self.search_windows_raw(q, r_sorted, threshold, int(q_range[1]), init_len, same_genome,
                                                                  uppercase_seeds, limit)
        self._check(code)
        return first.astype(np.int64), windows, out[:used]

    def search_windows_found_raw(self, q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, found, visible,
                                 cap=None, out=None):
        """sdf_search_windows_found as it is: search_windows_raw with the exclusions of the found records.  found: a
        SEARCH_FOUND_DTYPE array in the order the hits were added; visible: per query minimizer the length of the prefix of
        `found` its window sees.  Returns (rc, first, windows, intervals, used)."""
        return search_windows_call(self.lib.sdf_search_windows_found, (self.ctx,), q, r_sorted, r_threshold, len_q, init_len,
                                   same_genome, uppercase_seeds, limit, cap, out, found=found, visible=visible)

    def search_windows_found_device(self, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome, uppercase_seeds, d_limit,
                                    n_limit, d_found, nf, found_entries_cap, d_found_entries, d_visible, d_first, d_windows, d_out, cap,
                                    stream=None):
        """The same over device pointers (ints); found_entries_cap: the bin entries the index may hold (found_entries counts
        them), d_found_entries: eight bytes that receive the need, or None.  On `stream` when one is given, else returns the
        intervals the windows have (raises when they exceed cap, or the entries found_entries_cap).  A WIDE or FOUND_WIDE
        window is flagged and has no interval."""
        used = C.c_size_t(0)
        self._check(self.lib.sdf_search_windows_found_device(
            self.ctx, d_q, nq, int(len_q), d_r_sorted, nr, int(r_threshold), int(init_len), int(bool(same_genome)),
            int(bool(uppercase_seeds)), d_limit, n_limit, d_found, nf, found_entries_cap, d_found_entries, d_visible, d_first, d_windows,
            d_out, cap, C.byref(used), stream))
        return int(used.value)

    def search_windows_wide_device(self, d_q, nq, len_q, d_r_sorted, nr, r_threshold, init_len, same_genome, uppercase_seeds, d_limit,
                                   n_limit, d_found, nf, found_entries_cap, d_found_entries, d_visible, d_first, d_windows, d_out, cap,
                                   n_wide_max, d_wide_total=None, stream=None):
        """sdf_search_windows_wide_device: search_windows_found_device, and the lowest n_wide_max windows it flags WIDE or
        FOUND_WIDE and that fit the wide kernel (at most SEARCH_MAX_MEMBERS members and SEARCH_WIDE_MAX_GATHER gathered
        positions, no NOLIMIT) finished on the device: SEARCH_WIDE_DONE instead of the two flags, the counts and intervals of
        the host form.  d_wide_total: eight bytes that receive the number of such windows, or None."""
        used = C.c_size_t(0)
        self._check(self.lib.sdf_search_windows_wide_device(
            self.ctx, d_q, nq, int(len_q), d_r_sorted, nr, int(r_threshold), int(init_len), int(bool(same_genome)),
            int(bool(uppercase_seeds)), d_limit, n_limit, d_found, nf, found_entries_cap, d_found_entries, d_visible, d_first, d_windows,
            d_out, cap, C.byref(used), int(n_wide_max), d_wide_total, stream))
        return int(used.value)

    def search_windows_wide(self, q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, found=None,
                            visible=None, n_wide_max=64):
        """search_windows_wide_device on numpy arrays: uploads them, runs the call on the context's stream (a second time when
        the first found the intervals' room short) and brings the answer back.  Returns (first, windows, intervals, wide_total):
        wide_total the windows the wide kernel could take, of which the lowest n_wide_max are SEARCH_WIDE_DONE."""
        import torch
        q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
        r_sorted = np.ascontiguousarray(r_sorted, dtype=MINIMIZER_DTYPE)
        limit = np.ascontiguousarray(limit, dtype=np.int32)
        found = np.zeros(0, SEARCH_FOUND_DTYPE) if found is None else np.ascontiguousarray(found, dtype=SEARCH_FOUND_DTYPE)
        visible = np.zeros(len(q), np.uint32) if visible is None else np.ascontiguousarray(visible, dtype=np.uint32)
        assert len(visible) == len(q)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

        def ptr(t):
            return t.data_ptr() if t.numel() else None
        d_q, d_r, d_limit, d_found, d_vis = up(q), up(r_sorted), up(limit), up(found), up(visible)
        d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        d_win = torch.zeros(len(q) * SEARCH_WINDOW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        cap = 4096
        while True:
            d_out = torch.zeros(cap * SEARCH_INTERVAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
            used = C.c_size_t(0)
            rc = self.lib.sdf_search_windows_wide_device(
                self.ctx, ptr(d_q), len(q), int(len_q), ptr(d_r), len(r_sorted), int(r_threshold), int(init_len), int(bool(same_genome)),
                int(bool(uppercase_seeds)), ptr(d_limit), len(limit), ptr(d_found), len(found), found_entries(found), None, ptr(d_vis),
                d_first.data_ptr(), ptr(d_win), d_out.data_ptr(), cap, C.byref(used), int(n_wide_max), d_total.data_ptr(), None)
            if rc != -5 or int(used.value) <= cap:
                break
            cap = int(used.value)
        self._check(rc)
        n = int(used.value)
        return (d_first.cpu().numpy(), np.frombuffer(d_win.cpu().numpy().tobytes(), SEARCH_WINDOW_DTYPE),
                np.frombuffer(d_out.cpu().numpy().tobytes()[:n * SEARCH_INTERVAL_DTYPE.itemsize], SEARCH_INTERVAL_DTYPE),
                int(d_total.cpu()[0]) if len(q) and n_wide_max else 0)

    def search_overlap_raw(self, q, first, rolls, found, visible_iv, init_len, min_read_size):
        """sdf_search_overlap as it is: the reference's is_overlap for every rolled interval.  q, first: as search_windows_raw
        takes and returns them; rolls: search_roll_raw's records; found: a SEARCH_FOUND_DTYPE array; visible_iv: per interval
        the length of the prefix of `found` it sees; min_read_size: the reference's MIN_READ_SIZE.  Returns (rc, verdicts):
        uint32, 1 or 0."""
        return search_overlap_call(self.lib.sdf_search_overlap, (self.ctx,), q, first, rolls, found, visible_iv, init_len, min_read_size)

    def search_overlap_device(self, d_q, nq, d_first, d_rolls, n_max, d_found, nf, found_entries_cap, d_found_entries, d_visible_iv,
                              init_len, min_read_size, d_out, d_filter_tasks=None, stream=None):
        """The same over device pointers (ints), behind search_filter_tasks_device on one stream: n_max lanes, d_out and
        d_visible_iv hold n_max entries.  d_filter_tasks: the tasks search_filter_tasks_device wrote, or None; where the verdict
        is 1 the task becomes the skip task, so that the filter and the extension skip the interval."""
        self._check(self.lib.sdf_search_overlap_device(self.ctx, d_q, nq, d_first, d_rolls, n_max, d_found, nf, found_entries_cap,
                                                       d_found_entries, d_visible_iv, int(init_len), int(min_read_size), d_out,
                                                       d_filter_tasks, stream))

    def search_pair(self, q_range, r_range, **kw):
        """sdf_search_pair: the SDs of two ranges of the resident pool as `sedef search` reports them, the stages and the
        acceptance step run in rounds on the device.  Arguments and result as search_pair_host's, and round_windows (0: the
        default) and debug_host_every (every n-th scheduled window on the host)."""
        return search_pair_call(self.lib.sdf_search_pair, (self.ctx,), q_range, r_range, **kw)

    def search_pair_wide(self, q_range, r_range, n_wide_max=64, **kw):
        """sdf_search_pair_wide: search_pair whose rounds finish up to n_wide_max WIDE / FOUND_WIDE windows of the seeding on
        the device (search_windows_wide_device) where search_pair hands them to the host."""
        return search_pair_call(self.lib.sdf_search_pair_wide, (self.ctx,), q_range, r_range, tail=(int(n_wide_max),), **kw)

    def search_index_build(self, rng, k=12, w=16, separate_lowercase=True):
        """sdf_search_index_build: the minimizers and the index of one range (off, len) or (off, len, flags) of the resident
        pool, computed once and kept in HBM.  Returns (rc, handle): an int for search_pair_indexed / search_index_info /
        search_index_free, None after a refusal.  A handle dies with its engine (close) at the latest."""
        r = _MinimRange(int(rng[0]), int(rng[1]), int(rng[2]) if len(rng) > 2 else 0)
        h = C.c_void_p(0)
        rc = self.lib.sdf_search_index_build(self.ctx, C.byref(r), int(k), int(w), int(bool(separate_lowercase)), C.byref(h))
        return rc, (h.value if rc == 0 else None)

    def search_index_free(self, handle):
        """sdf_search_index_free -> rc (None is SDF_OK; a handle that is not live in this engine is -4)."""
        return self.lib.sdf_search_index_free(self.ctx, handle)

    def search_index_info(self, handle):
        """sdf_search_index_info -> a SEARCH_INDEX_DESC_DTYPE record."""
        d = np.zeros(1, SEARCH_INDEX_DESC_DTYPE)
        self._check(self.lib.sdf_search_index_info(self.ctx, handle, d.ctypes.data))
        return d[0]

    def search_index_builds(self):
        """(handles built since the engine was made, handles live now)"""
        return int(self.lib.sdf_search_index_builds(self.ctx)), int(self.lib.sdf_search_index_live(self.ctx))

    def search_pair_indexed(self, q_index, r_index, **kw):
        """sdf_search_pair_indexed: search_pair on two handles of search_index_build (same_genome: one handle as both).
        Keywords and result as search_pair's."""
        return search_pair_call(self.lib.sdf_search_pair_indexed, (self.ctx,), q_index, r_index, **kw)

    def search_pair_indexed_wide(self, q_index, r_index, n_wide_max=64, **kw):
        """sdf_search_pair_indexed_wide: search_pair_wide on two handles of search_index_build."""
        return search_pair_call(self.lib.sdf_search_pair_indexed_wide, (self.ctx,), q_index, r_index, tail=(int(n_wide_max),), **kw)

    def search_lanes_open(self, n):
        """sdf_search_lanes_open: n (1 .. 16) lanes for search_pairs_indexed -- child contexts that view this engine's pool, so
        the pool cannot grow or be replaced until they are closed.  Returns (rc, lanes): an int for search_pairs_indexed and
        search_lanes_close, None after a refusal.  Lanes die with their engine (close) at the latest."""
        h = C.c_void_p(0)
        rc = self.lib.sdf_search_lanes_open(self.ctx, int(n), C.byref(h))
        return rc, (h.value if rc == 0 else None)

    def search_lanes_close(self, lanes):
        """sdf_search_lanes_close -> rc (None is SDF_OK; lanes that are not live in this engine are -4)."""
        return self.lib.sdf_search_lanes_close(self.ctx, lanes)

    def search_pairs_indexed(self, lanes, jobs, n_wide_max=0, cap=None, **kw):
        """sdf_search_pairs_indexed: every job (q_handle, r_handle, same_genome) as search_pair_indexed_wide(q, r, n_wide_max,
        same_genome=..., **kw), several in flight on the lanes.  Keywords as search_pair's (same_genome and extend's own come
        from the job); cap: the hits `out` holds (None: retried with the need).  Returns (rc, hits, first, stats): job j's hits
        are hits[first[j]:first[j + 1]], stats[j] its PAIR_STATS_DTYPE record; after -5 hits is empty and first[-1] the need."""
        J = np.zeros(len(jobs), PAIR_JOB_DTYPE)
        for j, (q, r, same) in enumerate(jobs):
            J[j] = (q or 0, r or 0, int(bool(same)), 0)
        P, keep = pair_params(**kw)
        first = np.zeros(len(jobs) + 1, np.uint64)
        stats = np.zeros(len(jobs), PAIR_STATS_DTYPE)
        used = C.c_size_t(0)
        room = 0 if cap is None else int(cap)
        while True:
            out = np.zeros(room, SEARCH_PAIR_HIT_DTYPE)
            rc = self.lib.sdf_search_pairs_indexed(self.ctx, lanes, J.ctypes.data if len(jobs) else None, len(jobs), C.byref(P),
                                                   int(n_wide_max), out.ctypes.data if room else None, room, C.byref(used),
                                                   first.ctypes.data, stats.ctypes.data if len(jobs) else None)
            if rc != -5 or cap is not None:
                break
            room = int(used.value)
        del keep
        return rc, out[:int(used.value)] if rc == 0 else out[:0], first, stats

    def search_accept_raw(self, *args, **kw):
        """sdf_search_accept as it is: one round of the search driver's acceptance step on numpy arrays, run by the device
        form on copies.  Arguments and result as search_accept_call's."""
        return search_accept_call(self.lib.sdf_search_accept, (self.ctx,), *args, **kw)

    def search_accept_device(self, d_round, d_found, nf, found_cap, d_out, n_out, out_cap, d_status, stream=None):
        """The same over device pointers (ints), behind the second filter on one stream without a host read: d_round is what
        accept_round makes of the round's device arrays; the status record (ACCEPT_STATUS_DTYPE) goes to d_status.  Three
        launches, whatever the data."""
        self._check(self.lib.sdf_search_accept_device(self.ctx, C.byref(d_round), d_found, int(nf), int(found_cap), d_out, int(n_out),
                                                      int(out_cap), d_status, stream))

    def search_roll_raw(self, q, windows, first, intervals, r, len_r, init_len, limit):
        """sdf_search_roll as it is.  q, windows, first, intervals: as search_windows_raw takes and returns them; r: the
        reference's minimizers in loc order (MINIMIZER_DTYPE); limit: the same table.  Returns (rc, rolls): a
        SEARCH_ROLL_DTYPE record per interval."""
        return search_roll_call(self.lib.sdf_search_roll, (self.ctx,), q, windows, first, intervals, r, len_r, init_len, limit)

    def search_roll_device(self, d_q, nq, d_windows, d_first, d_intervals, n_max, d_r, nr, len_r, init_len, d_limit, n_limit, d_out,
                           stream=None):
        """The same over device pointers (ints), behind search_windows_device on one stream without a host read: n_max
        wavefronts, d_out holds n_max records.  A WIDE interval is flagged and the rest of its record is zero."""
        self._check(self.lib.sdf_search_roll_device(self.ctx, d_q, nq, d_windows, d_first, d_intervals, n_max, d_r, nr, int(len_r),
                                                    int(init_len), d_limit, n_limit, d_out, stream))

    def _search_roll(self, q_range, r_range, k, w, separate_lowercase, init_len, same_genome, uppercase_seeds, limit, r_threshold):
        """search_roll with the query's minimizers in front: (q, first, windows, intervals, rolls)."""
        def one(rng):
            return self.minim_ranges([rng[:2]], rc=bool(rng[2]) if len(rng) > 2 else None)
        _, q = self.pool_minimizers(one(q_range), k, w, separate_lowercase)
        _, r = self.pool_minimizers(one(r_range), k, w, separate_lowercase)
        _, r_sorted, _, threshold = self.pool_minimizer_index(one(r_range), k, w, separate_lowercase)
        threshold = int(threshold[0]) if r_threshold is None else int(r_threshold)
        code, first, windows, out, used = self.search_windows_raw(q, r_sorted, threshold, int(q_range[1]), init_len, same_genome,
                                                                  uppercase_seeds, limit)
        self._check(code)
        code, rolls = self.search_roll_raw(q, windows, first, out[:used], r, int(r_range[1]), init_len, limit)
        self._check(code)
        return q, first.astype(np.int64), windows, out[:used], rolls

    def search_roll(self, q_range, r_range, k=12, w=16, separate_lowercase=True, init_len=700, same_genome=False,
                    uppercase_seeds=True, limit=(), r_threshold=None):
        """search_windows, and every interval rolled to its best initial match (the first loop of the reference's
        search_in_reference_interval).  Returns (first, windows, intervals, rolls): rolls[t] is the SEARCH_ROLL_DTYPE record
        of intervals[t]."""
        return self._search_roll(q_range, r_range, k, w, separate_lowercase, init_len, same_genome, uppercase_seeds, limit, r_threshold)[1:]

    def search_filter_raw(self, tasks, params=None, out=None):
        """sdf_search_filter as it is.  tasks: a FILTER_TASK_DTYPE array of pairs of ranges of the resident pool; params: what
        filter_params makes (default: the reference's defaults); out: a FILTER_REC_DTYPE array to fill.  Returns (rc, records)."""
        tasks = np.ascontiguousarray(tasks, dtype=FILTER_TASK_DTYPE)
        if out is None:
            out = np.zeros(len(tasks), FILTER_REC_DTYPE)
        assert out.dtype == FILTER_REC_DTYPE and out.flags.c_contiguous and len(out) >= len(tasks)
        params = filter_params() if params is None else params
        rc = self.lib.sdf_search_filter(self.ctx, C.byref(params), tasks.ctypes.data if len(tasks) else None, len(tasks),
                                        out.ctypes.data if len(out) else None)
        return rc, out

    def search_filter_device(self, d_tasks, n, any_rc, d_out, params=None, stream=None):
        """The same over device pointers (ints) of n tasks and n records; on `stream` when one is given.  A task that does not
        lie in the pool or carries an unknown flag answers a zero record with FILTER_SKIPPED."""
        params = filter_params() if params is None else params
        self._check(self.lib.sdf_search_filter_device(self.ctx, C.byref(params), d_tasks, n, int(bool(any_rc)), d_out, stream))

    def search_filter_tasks_device(self, d_q, nq, d_windows, d_first, d_intervals, d_rolls, n_max, len_q, len_r, init_len, q_off, q_rc,
                                   r_off, r_rc, allow_extend, d_out, stream=None):
        """sdf_search_filter_tasks_device: a FILTER_TASK_DTYPE record per interval behind search_roll_device on one stream, n_max
        of them; those at or beyond d_first[nq] carry FILTER_SKIP."""
        self._check(self.lib.sdf_search_filter_tasks_device(self.ctx, d_q, nq, d_windows, d_first, d_intervals, d_rolls, n_max, int(len_q),
                                                            int(len_r), int(init_len), int(q_off), int(bool(q_rc)), int(r_off),
                                                            int(bool(r_rc)), int(bool(allow_extend)), d_out, stream))

    def search_filter(self, q_range, r_range, k=12, w=16, separate_lowercase=True, init_len=700, same_genome=False,
                      uppercase_seeds=True, limit=(), r_threshold=None, params=None, allow_extend=True):
        """search_roll, and the filter's verdict on every rolled interval whose jaccard is at least 0 (the reference's filter()
        as search_in_reference_interval calls it in front of extend, or with allow_extend=False in its place).  Returns
        (first, windows, intervals, rolls, records): records[t] is the FILTER_REC_DTYPE record of intervals[t], FILTER_SKIPPED
        where the reference does not filter."""
        q, first, windows, intervals, rolls = self._search_roll(q_range, r_range, k, w, separate_lowercase, init_len, same_genome,
                                                                uppercase_seeds, limit, r_threshold)
        code, tasks = search_filter_tasks_host(q, windows, first, intervals, rolls, int(q_range[1]), int(r_range[1]), init_len,
                                               int(q_range[0]), len(q_range) > 2 and bool(q_range[2]), int(r_range[0]),
                                               len(r_range) > 2 and bool(r_range[2]), allow_extend)
        self._check(code)
        code, recs = self.search_filter_raw(tasks, params)
        self._check(code)
        return first, windows, intervals, rolls, recs

    def search_extend_raw(self, q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit, params=None):
        """sdf_search_extend as it is.  q .. limit: as search_roll_raw takes them; rolls: as it returns them; filt: the first
        filter's FILTER_REC_DTYPE records or None; params: what extend_params makes (default: the reference's defaults).
        Returns (rc, hits): a SEARCH_HIT_DTYPE record per interval, the WIDE ones completed on the host."""
        return search_extend_call(self.lib.sdf_search_extend, (self.ctx,), q, windows, first, intervals, rolls, filt, r, len_q, len_r,
                                  init_len, limit, params)

    def search_extend_device(self, d_q, nq, d_windows, d_first, d_intervals, d_rolls, d_filter, n_max, d_r, nr, len_q, len_r, init_len,
                             d_limit, n_limit, d_out, params=None, stream=None):
        """The same over device pointers (ints; d_filter may be None), behind search_filter_device on one stream without a host
        read: n_max wavefronts, d_out holds n_max records.  A WIDE interval is flagged and the rest of its record is zero."""
        params = extend_params() if params is None else params
        self._check(self.lib.sdf_search_extend_device(self.ctx, d_q, nq, d_windows, d_first, d_intervals, d_rolls, d_filter, n_max, d_r,
                                                      nr, int(len_q), int(len_r), int(init_len), d_limit, n_limit, C.byref(params),
                                                      d_out, stream))

    def search_extend_long_device(self, d_q, nq, d_windows, d_first, d_intervals, d_rolls, d_filter, n_max, d_r, nr, len_q, len_r,
                                  init_len, d_limit, n_limit, d_hits, long_grow=EXTEND_LONG_MAX_GROW, n_long_max=None, batch=0,
                                  d_left=None, params=None, stream=None, check=True):
        """sdf_search_extend_long_device, behind search_extend_device on one stream: the first n_long_max (default: n_max)
        records of d_hits that are WIDE for their growth are completed in place, up to long_grow records an end; d_left (a
        device pointer to eight bytes, or None) receives how many were not.  Returns the code; check: raise on a refusal."""
        params = extend_params() if params is None else params
        rc = self.lib.sdf_search_extend_long_device(self.ctx, d_q, nq, d_windows, d_first, d_intervals, d_rolls, d_filter, n_max, d_r, nr,
                                                    int(len_q), int(len_r), int(init_len), d_limit, n_limit, C.byref(params),
                                                    int(long_grow), n_max if n_long_max is None else n_long_max, batch, d_hits, d_left,
                                                    stream)
        if check:
            self._check(rc)
        return rc

    def search_hit_tasks_device(self, d_hits, n, d_count, len_q, len_r, q_off, q_rc, r_off, r_rc, d_out, stream=None):
        """sdf_search_hit_tasks_device: the FILTER_TASK_DTYPE record of n hits, those at or beyond *d_count (None: none) SKIP."""
        self._check(self.lib.sdf_search_hit_tasks_device(self.ctx, d_hits, n, d_count, int(len_q), int(len_r), int(q_off),
                                                         int(bool(q_rc)), int(r_off), int(bool(r_rc)), d_out, stream))

    def search_extend(self, q_range, r_range, k=12, w=16, separate_lowercase=True, init_len=700, same_genome=False,
                      uppercase_seeds=True, limit=(), r_threshold=None, params=None, extend=None):
        """The reference's search() on two pool ranges with an empty tree, to its end: search_filter (allow_extend), every
        interval that passed grown to its hit, and the filter's verdict on every hit.  extend: what extend_params makes
        (default: the reference's defaults with this same_genome).  Returns (first, windows, intervals, rolls, records, hits,
        hit_records): hits[t] is the SEARCH_HIT_DTYPE record of intervals[t], hit_records[t] its FILTER_REC_DTYPE record."""
        q, first, windows, intervals, rolls = self._search_roll(q_range, r_range, k, w, separate_lowercase, init_len, same_genome,
                                                                uppercase_seeds, limit, r_threshold)
        _, r = self.pool_minimizers(self.minim_ranges([r_range[:2]], rc=bool(r_range[2]) if len(r_range) > 2 else None), k, w,
                                    separate_lowercase)
        len_q, len_r = int(q_range[1]), int(r_range[1])
        strands = (int(q_range[0]), len(q_range) > 2 and bool(q_range[2]), int(r_range[0]), len(r_range) > 2 and bool(r_range[2]))
        code, tasks = search_filter_tasks_host(q, windows, first, intervals, rolls, len_q, len_r, init_len, *strands, True)
        self._check(code)
        code, recs = self.search_filter_raw(tasks, params)
        self._check(code)
        extend = extend_params(same_genome=same_genome) if extend is None else extend
        code, hits = self.search_extend_raw(q, windows, first, intervals, rolls, recs, r, len_q, len_r, init_len, limit, extend)
        self._check(code)
        code, tasks = search_hit_tasks_host(hits, len_q, len_r, *strands)
        self._check(code)
        code, hit_recs = self.search_filter_raw(tasks, params)
        self._check(code)
        return first, windows, intervals, rolls, recs, hits, hit_recs

    def last_ms(self, which):
        return float(self.lib.sdf_last_ms(self.ctx, which))

    def last_launches(self):
        return int(self.lib.sdf_last_launches(self.ctx))

    def last_paired(self):
        """Tasks of the last batch that ran two per wavefront (same-geometry pairs)."""
        return int(self.lib.sdf_last_paired(self.ctx))

    def last_lane_tasks(self):
        """Tasks of the last batch that ran one per lane (extz2_lane.hip: small full-band tasks of a large batch)."""
        return int(self.lib.sdf_last_lane_tasks(self.ctx))

    def last_chain_classes(self):
        """Pairs of the last chain_batch per launch class: [0..5] the LDS classes of the wavefront kernel, [6] the
        thread-per-pair kernel; [7] the LDS cap of class 5 in bytes (include/sedef_hip.h: sdf_last_chain_classes)."""
        out = np.zeros(8, np.int64)
        self._check(self.lib.sdf_last_chain_classes(self.ctx, out.ctypes.data))
        return [int(x) for x in out]

    def last_traceback_classes(self):
        """Traceback launches of the last batch call per instantiation: [2 * layout + (G == 16)] for the direction-flag
        layouts 0..6 and groups of G = 64 or 16 lanes (include/sedef_hip.h: sdf_last_traceback_classes)."""
        out = np.zeros(14, np.int64)
        self._check(self.lib.sdf_last_traceback_classes(self.ctx, out.ctypes.data))
        return [int(x) for x in out]

    def last_reran(self):
        """Tasks of the last batch that a stripe kernel gave up and the call ran again on another kernel."""
        return int(self.lib.sdf_last_reran(self.ctx))


def pool_coverage_call(fn, head, regions, intervals, min_upper):
    """sdf_pool_coverage (head: its context) or sdf_pool_coverage_host (head: the characters and their number) on numpy arrays.
    Returns (rc, (counts, upper, painted))."""
    if not (isinstance(regions, np.ndarray) and regions.dtype == POOL_RANGE_DTYPE):
        pairs = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
        regions = np.zeros(len(pairs), POOL_RANGE_DTYPE)
        regions["off"], regions["len"] = pairs[:, 0], pairs[:, 1]
    if not (isinstance(intervals, np.ndarray) and intervals.dtype == COVER_INTERVAL_DTYPE):
        rows = np.asarray(intervals, dtype=np.int64).reshape(-1, 5)
        intervals = np.zeros(len(rows), COVER_INTERVAL_DTYPE)
        for k, f in enumerate(("region", "start", "len", "set", "partner")):
            intervals[f] = rows[:, k]
    regions, intervals = np.ascontiguousarray(regions), np.ascontiguousarray(intervals)
    nr, ni = len(regions), len(intervals)
    counts, upper, painted = np.zeros(nr, COVER_COUNTS_DTYPE), np.zeros(ni, np.int32), np.zeros(ni, np.uint8)
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    rc = fn(*head, ptr(regions), nr, ptr(intervals), ni, int(min_upper), ptr(counts), ptr(upper), ptr(painted))
    return rc, (counts, upper, painted)


def pool_coverage_host(pool, regions, intervals, min_upper, pool_bytes=None):
    """sdf_pool_coverage_host: Extz2Engine.pool_coverage without a context or a GPU, over the characters `pool` (bytes or a
    uint8 array).  Returns (rc, (counts, upper, painted))."""
    pool = bytes(pool) if not isinstance(pool, bytes) else pool
    return pool_coverage_call(load_library().sdf_pool_coverage_host, (pool, len(pool) if pool_bytes is None else int(pool_bytes)),
                              regions, intervals, min_upper)


def search_windows_call(fn, head, q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, cap=None, out=None,
                        found=None, visible=None):
    """sdf_search_windows (head: its context) or sdf_search_windows_host (head: nothing) on numpy arrays; the overflow protocol
    as Extz2Engine.pool_minimizers_raw has it.  found and visible: for the _found forms of the two (a SEARCH_FOUND_DTYPE array,
    a prefix length per query minimizer).  Returns (rc, first, windows, intervals, used)."""
    q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
    r_sorted = np.ascontiguousarray(r_sorted, dtype=MINIMIZER_DTYPE)
    limit = np.ascontiguousarray(limit, dtype=np.int32)
    first, windows = np.zeros(len(q) + 1, np.uint64), np.zeros(len(q), SEARCH_WINDOW_DTYPE)
    used = C.c_size_t(0)

    def ptr(a):
        return a.ctypes.data if len(a) else None

    mid = ()
    if found is not None:
        found = np.ascontiguousarray(found, dtype=SEARCH_FOUND_DTYPE)
        visible = np.ascontiguousarray(visible, dtype=np.uint32)
        assert len(visible) == len(q)
        mid = (ptr(found), len(found), ptr(visible))

    def call(buf, c):
        return fn(*head, ptr(q), len(q), int(len_q), ptr(r_sorted), len(r_sorted), int(r_threshold), int(init_len),
                  int(bool(same_genome)), int(bool(uppercase_seeds)), ptr(limit), len(limit), *mid, first.ctypes.data, ptr(windows),
                  ptr(buf), c, C.byref(used))
    if out is None:
        if cap is None:
            rc = call(np.zeros(0, SEARCH_INTERVAL_DTYPE), 0)
            if rc not in (0, -5):  # (SDF_ERR_CIGAR_OVERFLOW: *used holds the need)
                return rc, first, windows, np.zeros(0, SEARCH_INTERVAL_DTYPE), int(used.value)
            cap = int(used.value)
        out = np.zeros(cap, SEARCH_INTERVAL_DTYPE)
    assert out.dtype == SEARCH_INTERVAL_DTYPE and out.flags.c_contiguous
    rc = call(out, len(out) if cap is None else cap)
    return rc, first, windows, out, int(used.value)


def search_windows_host(q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, cap=None, out=None):
    """sdf_search_windows_host: search_windows_raw without a context or a GPU, in plain C++ on one thread."""
    return search_windows_call(load_library().sdf_search_windows_host, (), q, r_sorted, r_threshold, len_q, init_len, same_genome,
                               uppercase_seeds, limit, cap, out)


def search_windows_found_host(q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, found, visible, cap=None,
                              out=None):
    """sdf_search_windows_found_host: search_windows_found_raw without a context or a GPU, in plain C++ on one thread."""
    return search_windows_call(load_library().sdf_search_windows_found_host, (), q, r_sorted, r_threshold, len_q, init_len, same_genome,
                               uppercase_seeds, limit, cap, out, found=found, visible=visible)


def found_entries(found):
    """sdf_search_found_entries: the bin entries of a list of found records -- what found_entries_cap of the device forms must
    grant."""
    found = np.ascontiguousarray(found, dtype=SEARCH_FOUND_DTYPE)
    n = C.c_uint64(0)
    rc = load_library().sdf_search_found_entries(found.ctypes.data if len(found) else None, len(found), C.byref(n))
    assert rc == 0
    return int(n.value)


def search_overlap_call(fn, head, q, first, rolls, found, visible_iv, init_len, min_read_size):
    """sdf_search_overlap (head: its context) or sdf_search_overlap_host (head: nothing) on numpy arrays.  Returns
    (rc, verdicts)."""
    q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    rolls = np.ascontiguousarray(rolls, dtype=SEARCH_ROLL_DTYPE)
    found = np.ascontiguousarray(found, dtype=SEARCH_FOUND_DTYPE)
    visible_iv = np.ascontiguousarray(visible_iv, dtype=np.uint32)
    n = int(first[-1])
    assert len(first) == len(q) + 1 and len(rolls) >= n and len(visible_iv) >= n
    out = np.zeros(n, np.uint32)

    def ptr(a):
        return a.ctypes.data if len(a) else None
    rc = fn(*head, ptr(q), len(q), first.ctypes.data, ptr(rolls), ptr(found), len(found), ptr(visible_iv), int(init_len),
            int(min_read_size), ptr(out))
    return rc, out


def search_overlap_host(q, first, rolls, found, visible_iv, init_len, min_read_size):
    """sdf_search_overlap_host: search_overlap_raw without a context or a GPU, in plain C++ on one thread."""
    return search_overlap_call(load_library().sdf_search_overlap_host, (), q, first, rolls, found, visible_iv, init_len, min_read_size)


def search_roll_call(fn, head, q, windows, first, intervals, r, len_r, init_len, limit):
    """sdf_search_roll (head: its context) or sdf_search_roll_host (head: nothing) on numpy arrays.  Returns (rc, rolls)."""
    q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
    r = np.ascontiguousarray(r, dtype=MINIMIZER_DTYPE)
    windows = np.ascontiguousarray(windows, dtype=SEARCH_WINDOW_DTYPE)
    intervals = np.ascontiguousarray(intervals, dtype=SEARCH_INTERVAL_DTYPE)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    limit = np.ascontiguousarray(limit, dtype=np.int32)
    assert len(first) == len(q) + 1 and len(windows) == len(q) and len(intervals) >= int(first[-1])
    out = np.zeros(int(first[-1]), SEARCH_ROLL_DTYPE)

    def ptr(a):
        return a.ctypes.data if len(a) else None
    rc = fn(*head, ptr(q), len(q), ptr(windows), first.ctypes.data, ptr(intervals), ptr(r), len(r), int(len_r), int(init_len),
            ptr(limit), len(limit), ptr(out))
    return rc, out


def search_roll_host(q, windows, first, intervals, r, len_r, init_len, limit):
    """sdf_search_roll_host: search_roll_raw without a context or a GPU, in plain C++ on one thread."""
    return search_roll_call(load_library().sdf_search_roll_host, (), q, windows, first, intervals, r, len_r, init_len, limit)


def search_filter_host(pool, tasks, params=None, out=None, pool_bytes=None):
    """sdf_search_filter_host: search_filter_raw without a context or a GPU, over the characters `pool` (bytes)."""
    tasks = np.ascontiguousarray(tasks, dtype=FILTER_TASK_DTYPE)
    if out is None:
        out = np.zeros(len(tasks), FILTER_REC_DTYPE)
    assert out.dtype == FILTER_REC_DTYPE and out.flags.c_contiguous and len(out) >= len(tasks)
    params = filter_params() if params is None else params
    pool = bytes(pool)
    rc = load_library().sdf_search_filter_host(pool, len(pool) if pool_bytes is None else pool_bytes, C.byref(params),
                                               tasks.ctypes.data if len(tasks) else None, len(tasks),
                                               out.ctypes.data if len(out) else None)
    return rc, out


def search_filter_tasks_host(q, windows, first, intervals, rolls, len_q, len_r, init_len, q_off, q_rc, r_off, r_rc, allow_extend,
                             out=None):
    """sdf_search_filter_tasks_host: the FILTER_TASK_DTYPE record of every rolled interval.  Returns (rc, tasks)."""
    q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
    windows = np.ascontiguousarray(windows, dtype=SEARCH_WINDOW_DTYPE)
    intervals = np.ascontiguousarray(intervals, dtype=SEARCH_INTERVAL_DTYPE)
    rolls = np.ascontiguousarray(rolls, dtype=SEARCH_ROLL_DTYPE)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    assert len(first) == len(q) + 1 and len(windows) == len(q)
    if out is None:
        out = np.zeros(int(first[-1]) if len(q) else 0, FILTER_TASK_DTYPE)

    def ptr(a):
        return a.ctypes.data if len(a) else None
    rc = load_library().sdf_search_filter_tasks_host(ptr(q), len(q), ptr(windows), first.ctypes.data, ptr(intervals), ptr(rolls),
                                                     int(len_q), int(len_r), int(init_len), int(q_off), int(bool(q_rc)), int(r_off),
                                                     int(bool(r_rc)), int(bool(allow_extend)), ptr(out))
    return rc, out


def search_extend_call(fn, head, q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit, params=None):
    """sdf_search_extend (head: its context) or sdf_search_extend_host (head: nothing) on numpy arrays.  Returns (rc, hits)."""
    q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
    r = np.ascontiguousarray(r, dtype=MINIMIZER_DTYPE)
    windows = np.ascontiguousarray(windows, dtype=SEARCH_WINDOW_DTYPE)
    intervals = np.ascontiguousarray(intervals, dtype=SEARCH_INTERVAL_DTYPE)
    rolls = np.ascontiguousarray(rolls, dtype=SEARCH_ROLL_DTYPE)
    filt = None if filt is None else np.ascontiguousarray(filt, dtype=FILTER_REC_DTYPE)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    limit = np.ascontiguousarray(limit, dtype=np.int32)
    n = int(first[-1])
    assert len(first) == len(q) + 1 and len(windows) == len(q) and len(intervals) >= n and len(rolls) >= n
    assert filt is None or len(filt) >= n
    out = np.zeros(n, SEARCH_HIT_DTYPE)
    params = extend_params() if params is None else params

    def ptr(a):
        return a.ctypes.data if a is not None and len(a) else None
    rc = fn(*head, ptr(q), len(q), ptr(windows), first.ctypes.data, ptr(intervals), ptr(rolls), ptr(filt), ptr(r), len(r), int(len_q),
            int(len_r), int(init_len), ptr(limit), len(limit), C.byref(params), ptr(out))
    return rc, out


def search_extend_host(q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit, params=None):
    """sdf_search_extend_host: search_extend_raw without a context or a GPU, in plain C++ on one thread."""
    return search_extend_call(load_library().sdf_search_extend_host, (), q, windows, first, intervals, rolls, filt, r, len_q, len_r,
                              init_len, limit, params)


def search_hit_tasks_host(hits, len_q, len_r, q_off, q_rc, r_off, r_rc, out=None):
    """sdf_search_hit_tasks_host: the FILTER_TASK_DTYPE record of every hit.  Returns (rc, tasks)."""
    hits = np.ascontiguousarray(hits, dtype=SEARCH_HIT_DTYPE)
    if out is None:
        out = np.zeros(len(hits), FILTER_TASK_DTYPE)
    rc = load_library().sdf_search_hit_tasks_host(hits.ctypes.data if len(hits) else None, len(hits), int(len_q), int(len_r), int(q_off),
                                                  int(bool(q_rc)), int(r_off), int(bool(r_rc)), out.ctypes.data if len(out) else None)
    return rc, out


ACCEPT_CANARY = 4  # records behind a capacity that search_accept_call leaves filled with 0xEE


def search_accept_call(fn, head, q, act, windows, first, rolls, overlap, filt, hits, hit_filter, init_len, min_read_size, found, out,
                       found_cap=None, out_cap=None, window_base=0, n_max=None, reserved=0):
    """sdf_search_accept (head: its context) or sdf_search_accept_host (head: nothing) on numpy arrays: one round of the
    acceptance step.  act: the ascending window indices that ran; windows, first, rolls, overlap (the is_overlap verdicts against
    the list as it stood), filt, hits, hit_filter: what the stages wrote; found, out: the records so far (SEARCH_FOUND_DTYPE,
    SEARCH_PAIR_HIT_DTYPE); found_cap, out_cap: the capacities (None: just enough for everything the round could add).
    Returns (rc, status, found_buf, out_buf): the ACCEPT_STATUS_DTYPE record and the two lists in buffers of their capacity plus
    ACCEPT_CANARY records that were 0xEE before the call."""
    q = np.ascontiguousarray(q, dtype=MINIMIZER_DTYPE)
    act = np.ascontiguousarray(act, dtype=np.uint32)
    windows = np.ascontiguousarray(windows, dtype=SEARCH_WINDOW_DTYPE)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    rolls = np.ascontiguousarray(rolls, dtype=SEARCH_ROLL_DTYPE)
    overlap = np.ascontiguousarray(overlap, dtype=np.uint32)
    filt = np.ascontiguousarray(filt, dtype=FILTER_REC_DTYPE)
    hits = np.ascontiguousarray(hits, dtype=SEARCH_HIT_DTYPE)
    hit_filter = np.ascontiguousarray(hit_filter, dtype=FILTER_REC_DTYPE)
    found = np.ascontiguousarray(found, dtype=SEARCH_FOUND_DTYPE)
    out = np.ascontiguousarray(out, dtype=SEARCH_PAIR_HIT_DTYPE)
    n = len(rolls) if n_max is None else int(n_max)
    assert min(len(rolls), len(overlap), len(filt), len(hits), len(hit_filter)) >= n
    found_cap = len(found) + n if found_cap is None else int(found_cap)
    out_cap = len(out) + n if out_cap is None else int(out_cap)
    found_buf = np.frombuffer(bytearray(b"\xEE" * (16 * (found_cap + ACCEPT_CANARY))), SEARCH_FOUND_DTYPE)
    out_buf = np.frombuffer(bytearray(b"\xEE" * (24 * (out_cap + ACCEPT_CANARY))), SEARCH_PAIR_HIT_DTYPE)
    found_buf[:min(len(found), found_cap)] = found[:found_cap]
    out_buf[:min(len(out), out_cap)] = out[:out_cap]
    status = np.zeros(1, ACCEPT_STATUS_DTYPE)

    def ptr(a):
        return a.ctypes.data if len(a) else None
    R = accept_round(ptr(q), len(q), ptr(act), len(act), ptr(windows), first.ctypes.data if len(first) else None, n, ptr(rolls),
                     ptr(overlap), ptr(filt), ptr(hits), ptr(hit_filter), init_len, min_read_size, window_base, reserved)
    rc = fn(*head, C.byref(R), found_buf.ctypes.data, len(found), found_cap, out_buf.ctypes.data, len(out), out_cap, status.ctypes.data)
    return rc, status[0], found_buf, out_buf


def search_accept_host(*args, **kw):
    """sdf_search_accept_host: search_accept_raw without a context or a GPU, the same rules in plain C++."""
    return search_accept_call(load_library().sdf_search_accept_host, (), *args, **kw)


def pair_params(k=12, w=16, separate_lowercase=True, uppercase_seeds=True, min_read_size=700, same_genome=False, limit=(), filter=None,
                extend=None, round_windows=0, debug_host_every=0):
    """sdf_search_pair_params from keywords -> (the struct, the limit table it points into: keep it until the call has returned)."""
    limit = np.ascontiguousarray(limit, dtype=np.int32)
    P = _PairParams(int(k), int(w), int(bool(separate_lowercase)), int(bool(uppercase_seeds)), int(min_read_size), int(bool(same_genome)),
                    filter_params() if filter is None else filter,
                    extend_params(same_genome=bool(same_genome)) if extend is None else extend,
                    limit.ctypes.data if len(limit) else None, len(limit), int(round_windows), int(debug_host_every))
    return P, limit


def search_pair_call(fn, head, q_range, r_range, cap=None, tail=(), **kw):
    """sdf_search_pair (head: its context) or sdf_search_pair_host (head: the characters and their number); tail: what a form
    takes behind stats (the _wide forms' n_wide_max); the other keywords: pair_params'.  Returns (rc, hits, used, stats)."""
    P, limit = pair_params(**kw)
    if isinstance(q_range, (tuple, list, np.ndarray)):
        ranges = [C.byref(_MinimRange(int(r[0]), int(r[1]), int(r[2]) if len(r) > 2 else 0)) for r in (q_range, r_range)]
    else:  # two handles of search_index_build (ints, or None)
        ranges = [q_range, r_range]
    stats = np.zeros(1, PAIR_STATS_DTYPE)
    used = C.c_size_t(0)
    room = 0 if cap is None else int(cap)
    while True:
        out = np.zeros(room, SEARCH_PAIR_HIT_DTYPE)
        rc = fn(*head, ranges[0], ranges[1], C.byref(P), out.ctypes.data if room else None, room, C.byref(used),
                stats.ctypes.data, *tail)
        if rc != -5 or cap is not None:
            break
        room = int(used.value)
    return rc, out[:int(used.value)] if rc == 0 else out[:0], int(used.value), stats[0]


def search_pair_host(pool, q_range, r_range, pool_bytes=None, **kw):
    """sdf_search_pair_host: initial_search window by window in plain C++ over the characters `pool` (bytes), no context and no
    GPU.  q_range, r_range: (off, len) or (off, len, flags) with MINIM_RC.  limit: the table of
    relaxed_jaccard_estimate(query_size).  cap: the hits `out` holds (None: retried with the need).  Returns (rc, hits, used,
    stats): SEARCH_PAIR_HIT_DTYPE records, the need, a PAIR_STATS_DTYPE record."""
    pool = bytes(pool)
    return search_pair_call(load_library().sdf_search_pair_host, (pool, len(pool) if pool_bytes is None else int(pool_bytes)), q_range, r_range,
                            **kw)


_default_engine = None


def ksw_extz2(query, target, m=5, mat=None, q=40, e=1, w=-1, zdrop=-1, flag=0, engine=None):
    """Mirror of ksw_extz2_sse(km, qlen, query, tlen, target, m, mat, q, e, w, zdrop, flag, &ez)
    (reference: extern/ksw2.h:50).  Returns the ksw_extz_t fields as a dict + 'cigar' words."""
    global _default_engine
    if engine is None:
        if _default_engine is None:
            _default_engine = Extz2Engine()
        engine = _default_engine
    if m != 5:
        raise SdfError("GPU path implements m=5 only")
    want = WANT_ALL & ~WANT_CIGAR if flag & 1 else WANT_ALL
    res, cig = engine.align_pairs([(query, target)], w=w, zdrop=zdrop, flag=flag, mat=mat, gapo=q,
                                  gape=e, want=want)
    r = res[0]
    d = {k: int(r[k]) for k in ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q",
                                "score")}
    d["cigar"] = cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].copy()
    d["counts"] = {k: int(r[k]) for k in ("matches", "mismatches", "gaps", "gap_bases")}
    return d

/*
 * sedef_hip.h -- C ABI of the MI355X-native `sedef align` DP hot path.
 *
 * This is the drop-in boundary.  The reference has exactly one native interface on this path:
 *
 *     void ksw_extz2_sse(void *km, int qlen, const uint8_t *query, int tlen,
 *                        const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e,
 *                        int w, int zdrop, int flag, ksw_extz_t *ez);
 *                                              (reference: extern/ksw2.h:50, result ksw2.h:22-30)
 *
 * called once per DP task from align_helper (reference: src/align.cc:39-68).  A GPU needs the
 * tasks in batches, so the boundary is exported twice:
 *
 *   sdf_ksw_extz2()         same signature and result struct as ksw_extz2_sse -> 1-task drop-in;
 *   sdf_extz2_batch()       n tasks over a shared code pool; host buffers in, host buffers out;
 *   sdf_extz2_batch_device()  the same with inputs/outputs resident in HBM (no PCIe in the call).
 *
 * All entry points are plain C: pointers and sizes only.  Buffers are owned by the caller.
 * Every function that can fail returns 0 on success or a negative SDF_ERR_* code; the message
 * is available from sdf_last_error().  There is no CPU fallback: without a usable HIP device
 * sdf_create() fails.
 */
#ifndef SEDEF_HIP_H
#define SEDEF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDF_NEG_INF (-0x40000000) /* KSW_NEG_INF, reference extern/ksw2.h:6 */

/* task flag bits: numerically the reference's KSW_EZ_* (extern/ksw2.h:8-16) */
#define SDF_FLAG_SCORE_ONLY 0x01 /* no direction matrix, no CIGAR */
#define SDF_FLAG_RIGHT 0x02      /* right-align gaps */
#define SDF_FLAG_GENERIC_SC 0x04 /* scores from the whole m x m matrix (general kernel; SEDEF never sets it) */
#define SDF_FLAG_APPROX_MAX 0x08 /* approximate max: score only along one followed path (general kernel) */
#define SDF_FLAG_APPROX_DROP 0x10 /* with APPROX_MAX: z-drop test on the followed value */
#define SDF_FLAG_EXTZ_ONLY 0x40  /* traceback from the best extension cell */
#define SDF_FLAG_REV_CIGAR 0x80  /* leave the CIGAR reversed */
/* strand bits of a RESIDENT task, outside the KSW_EZ_* range: valid in sdf_extz2_batch_pairs, _pairs_full and _pairs_view only
 * (an unknown flag, SDF_ERR_UNSUPPORTED, everywhere else).  That side of the task is the reverse complement of its range:
 * base i = rev_dna(pool[off + len - 1 - i]) (reference: src/common.h:72-77,93 -- what rc() applies, src/align_main.cc:305-306);
 * q_off / t_off keep naming the first byte of the range in pool order.
 * Since these bits exist, every batch entry point answers SDF_ERR_UNSUPPORTED ("unknown task flag") to ANY flag bit beyond
 * 0xff; before, only 0x100 / 0x200 (KSW_EZ_SPLICE_FOR / _REV) were refused and higher bits were ignored. */
#define SDF_TASK_Q_RC 0x10000
#define SDF_TASK_T_RC 0x20000

/* error codes */
#define SDF_OK 0
#define SDF_ERR_NO_DEVICE (-1)
#define SDF_ERR_HIP (-2)
#define SDF_ERR_UNSUPPORTED (-3) /* alphabet (m != 5) or flag bits the GPU path does not implement */
#define SDF_ERR_INVALID (-4)
#define SDF_ERR_CIGAR_OVERFLOW (-5) /* cigar_cap too small; *cigar_used holds the need */
#define SDF_ERR_NOMEM (-6)

/* what to compute for a batch (bit mask) */
#define SDF_WANT_CIGAR 0x1  /* CIGAR + n_cigar + column counts */
#define SDF_WANT_SCORE 0x2  /* score, mte, mte_q, zdropped (always produced) */
#define SDF_WANT_EXT 0x4    /* also max, max_q, max_t, mqe, mqe_t: every ksw_extz_t field.  Needed
                               for zdrop >= 0 and SDF_FLAG_EXTZ_ONLY; SEDEF reads none of them
                               (reference: src/align.cc:49-66 uses ez.cigar / ez.n_cigar only). */
#define SDF_WANT_ALL 0x7

typedef struct sdf_ctx sdf_ctx;

/* Scoring, as passed to ksw_extz2_sse: alphabet size m (must be 5: ACGT + wildcard), the m*m
 * matrix of which the non-generic kernel uses mat[0] (match), mat[1] (mismatch) and the
 * min over all entries (reference: extern/ksw2_extz2_sse.cc:66-67,77-81), gap open q, extend e. */
typedef struct {
  int32_t m;
  int8_t mat[25];
  int8_t gapo, gape;
  int8_t pad_;
} sdf_scoring;

/* One DP task.  q_off/t_off index the sequence pool: bytes for sdf_extz2_batch (one code 0..4
 * per byte, exactly what ksw_extz2_sse takes), 32-bit words of the packed pool for
 * sdf_extz2_batch_device (see sdf_pack_codes). */
typedef struct {
  int64_t q_off, t_off;
  int32_t qlen, tlen;
  int32_t w;     /* band width, <0 = full (reference default, src/align.cc:86) */
  int32_t zdrop; /* <0 = off */
  int32_t flag;
  int32_t pad_;
} sdf_task;

/* Per-task result record (64 B).  First nine fields mirror ksw_extz_t (extern/ksw2.h:22-30). */
typedef struct {
  int32_t score;
  int32_t max, max_q, max_t;
  int32_t mqe, mqe_t;
  int32_t mte, mte_q;
  int32_t zdropped;
  int32_t n_cigar;    /* number of CIGAR words */
  int64_t cigar_off;  /* first word in the CIGAR pool; words are len<<4|op, op 0=M 1=I 2=D */
  /* alignment column statistics over the CIGAR (the counters of populate_nice_alignment,
   * reference: src/align.cc:274-315, for ACGTN input): */
  int32_t matches, mismatches, gaps, gap_bases;
} sdf_result;

/* ksw_extz_t, field-for-field (reference: extern/ksw2.h:22-30) */
typedef struct {
  uint32_t max : 31, zdropped : 1;
  int max_q, max_t;
  int mqe, mqe_t;
  int mte, mte_q;
  int score;
  uint32_t *cigar; /* malloc'd by the callee, caller free()s (reference: src/align.cc:65) */
  int64_t m_cigar, n_cigar;
} sdf_ksw_extz_t;

/* ---- context ---------------------------------------------------------------------------- */
int sdf_device_count(void);
/* device: HIP ordinal.  workspace_bytes: HBM budget for direction matrices per internal
 * batch (0 = half of the memory free when the context is made; any figure is clamped to that).  The
 * workspace is allocated by need, up to the budget: a batch that needs more runs in chunks.
 * Returns NULL on failure (sdf_last_error(NULL) has the reason). */
sdf_ctx *sdf_create(int device, size_t workspace_bytes);
void sdf_destroy(sdf_ctx *ctx);

/* ---- configuration -------------------------------------------------------------------------------------------------
 * Every tunable and test switch of the library in ONE struct.  sdf_create() fills it from the SDF_* environment variables,
 * once, when the context is made (an unknown value or one out of range makes sdf_create fail with the reason);
 * sdf_create_cfg() takes it from the caller instead -- tests force a kernel through sdf_config_set(&cfg, "SDF_NO_PAIR",
 * "1", ...) and never touch the environment.  A context's settings do not change after it is made; the contexts it
 * creates for itself (the first part of a split batch, the re-run of tasks a stripe kernel gave up) inherit them.
 * Fields are int64_t (0 / 1 for switches) except workspace_gib; sdf_config_describe() lists name, environment
 * variable, default and meaning of each, sdf_config_dump() the values of one struct (SDF_DEBUG_PLAN=1 prints that for
 * every context made). */
typedef struct sdf_config {
  uint32_t size; /* sizeof(sdf_config), set by sdf_config_default / sdf_config_from_env */
  uint32_t reserved;
  /* which kernel serves a task */
  int64_t force_general, no_pair, no_mixed, mixed_min, self_pair_max;
  int64_t no_stripe, stripe_min, stripe_nreg, stripe_claim, stripe_spin_cap;
  int64_t bstripe_min_rows, bstripe_nreg, bstripe_all;
  int64_t no_strip, strip_always, strip_cols, chain_min;
  int64_t no_lane, lane_min, lane_plan_sort, lane_prio;
  /* how a batch is cut and planned */
  int64_t pipeline, cut_chunks, heavy_bytes, early_heavy, split_min, split_div;
  int64_t plan_threads, plan_pool_from, scan_pool_from, pool_spin_us;
  int64_t pin_register;
  double workspace_gib;
  /* other entry points */
  int64_t chain_threads_only, stats_items, stats_group_max, fetch_stage_bytes;
  /* diagnostics on stderr */
  int64_t debug_plan, debug_timing, debug_classes, debug_plan_early;
} sdf_config;
void sdf_config_default(sdf_config *cfg);
/* defaults, then every SDF_* variable that is set; SDF_ERR_INVALID + message for a value that is not a number or out of range */
int sdf_config_from_env(sdf_config *cfg, char *err, size_t errcap);
/* one setting by its environment variable's or its field's name */
int sdf_config_set(sdf_config *cfg, const char *name, const char *value, char *err, size_t errcap);
size_t sdf_config_dump(const sdf_config *cfg, char *buf, size_t cap); /* "NAME=value" lines; returns the bytes needed */
size_t sdf_config_describe(char *buf, size_t cap);                    /* every setting: variable, field, default, meaning */
/* sdf_create with the caller's settings (cfg == NULL: sdf_config_from_env, which is what sdf_create does) */
sdf_ctx *sdf_create_cfg(int device, size_t workspace_bytes, const sdf_config *cfg);
const sdf_config *sdf_get_config(const sdf_ctx *ctx);
/* Sizes the context's buffers ONCE for host-buffer batch calls of up to max_tasks tasks whose sequences add up to
 * max_bases bases: the pinned staging (task plan, launch order, packed sequences, results), the device copies of
 * those, the CIGAR staging and the streams of the call's pipeline -- no call within the bounds allocates, pins or sets
 * up a hardware queue afterwards (pinning runs at ~4 MB per
 * millisecond: a first call of 700,000 tasks spends 40-50 ms on it) -- and workspace_bytes of the direction-flag
 * workspace (clamped to the context's budget; 0: left to the first call that needs it).  Larger calls still grow the
 * buffers.  Call it where a context is set up: pinning takes the process's memory-map lock, and a pageable upload that
 * runs meanwhile (sdf_anchors_batch) waits for it -- measured: 46-78 ms for a 34-54 MB upload next to a reserve on another
 * thread, 4 ms without.  It must have returned before the context's first batch call.  (The stage driver: once per lane,
 * with the lane's context, host/dp_provider.cc.) */
#define SDF_RESERVE_BRIEF 1u /* the caller reads results through sdf_extz2_batch_brief: 16 bytes of result staging per task */
#define SDF_RESERVE_ANCHORS 2u /* the caller will use sdf_anchors_batch: one tiny call now, so that the first real one does not
                                  pay for the first launch of its kernels and of the library sort behind it */
#define SDF_RESERVE_FEW_STREAMS 4u /* this context is one of several that share the device (the lanes of the stage driver): it
                                       never creates the four extra pipeline streams -- a stream costs 7-15 ms to set up, and the
                                       other contexts' work fills the device where the extra streams would */
int sdf_reserve(sdf_ctx *ctx, size_t max_tasks, size_t max_bases, size_t workspace_bytes, uint32_t flags);
/* Debug: out[4096] receives the wavefronts the chained-strip launches started per (XCD, shader engine, CU, SIMD) since the
 * last call (index xcd << 9 | se << 6 | cu << 2 | simd) and the counters are cleared; the first call (out may be NULL) switches
 * the counting on for the process. */
int sdf_debug_placement(sdf_ctx *ctx, uint32_t *out);
/* Device bytes the context holds at this moment: every device buffer of it and of the contexts it owns (buffers in use,
 * outgrown ones not yet freed). */
size_t sdf_device_bytes(const sdf_ctx *ctx);
/* Debug: device bytes all contexts of the process hold in their buffers at this moment -- what their allocations obtained
 * minus what they gave back.  The sum of sdf_device_bytes over the live contexts; what it was before, once they are gone. */
size_t sdf_debug_live_device_bytes(void);
const char *sdf_last_error(const sdf_ctx *ctx);

/* ---- packed sequence format --------------------------------------------------------------
 * A sequence of len codes occupies sdf_packed_words(len) 32-bit words:
 *   ceil(len/16) words of 2-bit codes (base b in bits 2*(b%16) of word b/16; N stored as 0)
 *   ceil(len/32) words of N mask      (bit b%32 of word b/32 set <=> code >= 4). */
size_t sdf_packed_words(int32_t len);
void sdf_pack_codes(const uint8_t *codes, int32_t len, uint32_t *out);
/* Packs both sequences of n tasks (byte offsets into `codes`, as sdf_extz2_batch takes them) back to back into `out`
 * and writes each task's word offsets, as sdf_extz2_batch_device takes them.  `out` holds
 * sum(sdf_packed_words(qlen) + sdf_packed_words(tlen)) words.  Returns that number. */
size_t sdf_pack_tasks(const uint8_t *codes, const int64_t *q_off, const int32_t *qlen, const int64_t *t_off,
                      const int32_t *tlen, size_t n, uint32_t *out, int64_t *q_word, int64_t *t_word);

/* ---- batched DP ---------------------------------------------------------------------------
 * Host-buffer form.  seq_pool holds byte codes; out[n]; cigar_pool[cigar_cap] words receives
 * all CIGARs back to back in task order (out[i].cigar_off, out[i].n_cigar); *cigar_used gets
 * the number of words written (or needed, with SDF_ERR_CIGAR_OVERFLOW). */
int sdf_extz2_batch(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                    const uint8_t *seq_pool, size_t pool_bytes, uint32_t want, sdf_result *out,
                    uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used);

/* The same call with 16-byte result records: what a caller that only stitches CIGARs reads (the stage driver:
 * src/align.cc:129-175 keeps the CIGAR of every piece and nothing else of ksw_extz_t) -- a quarter of the bytes
 * of sdf_result across PCIe and through the caller's caches.  Always computes CIGARs. */
typedef struct {
  int64_t cigar_off; /* first word of the task's CIGAR in cigar_pool */
  int32_t n_cigar;
  int32_t matches;   /* 'M' columns with equal bases (what src/align.cc:274-311 counts as error.matches) */
} sdf_result_brief;
int sdf_extz2_batch_brief(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                          const uint8_t *seq_pool, size_t pool_bytes, sdf_result_brief *out,
                          uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used);


/* ---- resident sequences: DP tasks that name ranges of characters already in HBM ------------------------------------
 * The reference's align_helper reads the bases of every DP call in place: the caller hands it two substrings of the pair's
 * sequences, mapped through align_dna (reference: src/align.cc:39-57,80-84; src/common.h:60-70,91).  The stage driver has
 * each super-batch's FASTA characters in HBM already -- sdf_anchors_batch uploaded them for the seed anchors -- and its DP
 * rounds (hundreds of thousands of gap fills of ~25 bases) used to cut the same bases out again on the host, code them,
 * pack them and upload them, round after round.  Here a task's q_off / t_off are BYTE offsets into that resident pool of raw
 * FASTA characters; the device does align_dna (ACGT of either case -> 0..3, anything else -> the wildcard 4) and the
 * packing (seq_pack.hip).  Results as sdf_extz2_batch_brief / sdf_extz2_batch return them.
 *
 *   sdf_pool_host(ctx, bytes)       a pinned host buffer of at least `bytes` owned by the context (NULL on failure): filled
 *                                   there, a pool crosses PCIe as one asynchronous DMA instead of a staged pageable copy
 *                                   (182 MB: 26 ms pageable).  Valid until the next sdf_pool_host call or sdf_destroy.
 *   sdf_pool_upload(ctx, p, bytes)  copies `bytes` characters to HBM, enqueued on the context's stream (any host memory;
 *                                   the buffer must stay unchanged until the next call on this context that returns data).
 *                                   The pool replaces the one before.
 *   sdf_anchors_batch(..., seq_pool = NULL, pool_bytes, ...)   the seed anchors of pairs whose offsets point into the
 *                                   resident pool; with a host seq_pool the call uploads it and leaves it resident.
 *   sdf_extz2_batch_pairs           the DP batch on ranges of the resident pool, 16-byte results;
 *   sdf_extz2_batch_pairs_full      the same with sdf_result records and a `want` mask.
 *   sdf_extz2_batch_pairs_view / sdf_anchors_batch_view   the same calls for a caller that reads the results where the device's
 *                                   copies land -- the context's pinned staging -- instead of receiving a second copy in
 *                                   arrays of its own (the stage driver: 17 MB of records and CIGAR words per round, 34 MB of
 *                                   anchors per super-batch).  *out / *cigar_pool are valid until the context's next call of
 *                                   the same kind.
 *
 * Resident chromosomes: a caller that serves many batches of one genome uploads each FASTA record once, as the file has
 * it, with sdf_pool_append_fasta, and names (base offset, length, strand) afterwards: SDF_TASK_Q_RC / SDF_TASK_T_RC on the
 * DP tasks, r_rc on the anchor pairs (sdf_anchors_batch_strand), SDF_STATS_A_RC / SDF_STATS_B_RC on the alignments whose
 * statistics are taken (sdf_stats_columns_pairs).  A forward and a reverse-strand pair on one region share the one
 * resident copy. */
char *sdf_pool_host(sdf_ctx *ctx, size_t bytes);
int sdf_pool_upload(sdf_ctx *ctx, const char *chars, size_t bytes);
size_t sdf_pool_bytes(const sdf_ctx *ctx); /* characters resident at this moment */
/* Appends the bases of one FASTA record to the resident pool.  `bytes` are the record's sequence lines as they lie in
 * the file (nbytes of them, starting at the .fai offset): line_bases bases, then line_bytes - line_bases line-end
 * bytes, repeated; the last line may be short, and its line end may be missing.  The device drops the line ends (characters
 * stay as they are: case, N); *base_off receives the pool offset of the record's base 0, so base x of the record is pool byte
 * *base_off + x, and sdf_pool_bytes() grows by n_bases.  reset != 0: the pool is emptied first.  SDF_ERR_INVALID, with the
 * pool as it was: a geometry that is none (line_bases < 1, line_bytes < line_bases, line_bytes == line_bases in a record of
 * more than one line), nbytes that does not fit n_bases, a record that does not fit the device's free memory (a pool that
 * grows moves: the old and the new buffer exist side by side for the copy).  SDF_ERR_NOMEM, with the pool EMPTY
 * (sdf_pool_bytes() == 0): the allocation failed although the free memory sufficed.  Enqueued on the context's stream like
 * sdf_pool_upload, from any host memory (sdf_pool_host's pinned buffer: one asynchronous DMA per 64 MiB piece); `bytes`
 * must stay unchanged until the next call on this context that returns data, or until sdf_pool_sync() has returned -- a
 * loader that stages record after record in the one buffer of sdf_pool_host calls sdf_pool_sync before it overwrites the
 * buffer.  While bases are resident, sdf_pool_host only sizes the staging and leaves the pool in HBM alone. */
int sdf_pool_append_fasta(sdf_ctx *ctx, const char *bytes, size_t nbytes, int64_t n_bases, int32_t line_bases,
                          int32_t line_bytes, int reset, int64_t *base_off);
/* Waits until everything enqueued on the context's stream has run: the uploads of sdf_pool_upload / sdf_pool_append_fasta
 * have left their host buffers. */
int sdf_pool_sync(sdf_ctx *ctx);
int sdf_extz2_batch_pairs(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, sdf_result_brief *out,
                          uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used);
int sdf_extz2_batch_pairs_full(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n, uint32_t want,
                               sdf_result *out, uint32_t *cigar_pool, size_t cigar_cap, size_t *cigar_used);
int sdf_extz2_batch_pairs_view(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                               const sdf_result_brief **out, const uint32_t **cigar_pool, size_t *cigar_used);

/* ---- character classes of ranges of the resident pool ----------------------------------------------------------------
 * How many bytes of pool[off, off + len), as they lie in HBM, are ACGT, acgt, 'N' or 'n', and anything else; the four counts
 * add up to len.  The class of a byte is decided on the WHOLE byte: one of 128 or more is `other` (the stage driver's own
 * scan, PairJob in host/pair_job.cc, indexes its table by the unsigned char -- unlike rev_dna and align_dna, which look at
 * c & 127).  The counts are strand-free: rev_dna maps every class onto itself or onto 'N' (A <-> T and C <-> G keep their
 * case, N and n become N, everything else becomes N), so `other == 0` holds for a range exactly when it holds for its
 * reverse complement, and a pair of the stage driver is "plain" -- nothing but ACGTNacgtn -- exactly when other == 0 on both
 * of its ranges.
 * SDF_ERR_INVALID, before any launch: a range outside sdf_pool_bytes() (an empty pool holds no non-empty range), len < 0,
 * n != 0 without ranges or out.  SDF_ERR_UNSUPPORTED: reserved != 0.  len == 0 is legal (all counts zero), and so is
 * n == 0 with NULL pointers.  Enqueued on the context's stream, behind the pool's uploads; returns with out[0, n) filled. */
typedef struct { int64_t off; int32_t len; int32_t reserved; /* must be 0 */ } sdf_pool_range;
typedef struct { int32_t upper_acgt, lower_acgt, n_any /* 'N' or 'n' */, other; } sdf_range_classes;
int sdf_pool_range_classes(sdf_ctx *ctx, const sdf_pool_range *ranges, size_t n, sdf_range_classes *out);

/* ---- reading ranges of the resident pool back, by strand ---------------------------------------------------------------
 * The characters of pool[off, off + len) as they lie in HBM, or their reverse complement (SDF_FETCH_RC), written to
 * dst[dst_off, dst_off + len):
 *   forward    dst[dst_off + j] = pool[off + j]                          byte for byte, bytes of 128 and above included
 *   reversed   dst[dst_off + j] = rev_dna(pool[off + len - 1 - j])      the reference's table, indexed c & 127
 *              (src/common.h:72-87,93: what rc() applies): A <-> T and C <-> G keep their case, every other byte becomes 'N'.
 * No byte of dst outside the ranges' destinations is written; source ranges may overlap and repeat.  Destination ranges that
 * overlap one another are the caller's error: they are NOT checked, and which range's bytes such a place ends up with is
 * unspecified.  (seq_pack.hip: pool_fetch_kernel.)
 *
 * Host form.  dst is any host memory of dst_bytes bytes.  Everything is validated before any launch; a refused call leaves
 * dst untouched and sdf_last_error() names the first offending range ("range <index>: ...").
 *   SDF_ERR_INVALID      off < 0, len < 0, off + len > sdf_pool_bytes(ctx) (an empty pool holds no non-empty range), dst_off < 0,
 *                        dst_off + len > dst_bytes, r == NULL with n > 0, dst == NULL with a byte to write
 *   SDF_ERR_UNSUPPORTED  a flags bit other than SDF_FETCH_RC
 * n == 0, or lengths that are all 0, is SDF_OK without a launch.  The bytes cross PCIe through a pinned staging buffer of the
 * context, in pieces of at most sdf_config.fetch_stage_bytes when there are more; the call is enqueued on the context's stream,
 * behind the pool's uploads (on a view made by sdf_pool_share: behind the owner's, as for every reader of a view), and returns
 * when dst is complete.
 *
 * Device form.  Records and destination in HBM, nothing copied to the host: enqueued on `stream` (NULL: the context's own, and
 * the call then returns after it has drained; a caller's stream is not waited for -- after sdf_pool_sync() when the pool was
 * uploaded on the context's stream, as for sdf_stats_columns_pairs_device).  The kernel cuts ranges into segments of
 * SDF_FETCH_SEG_BYTES destination bytes, a group of sixteen lanes each, and finds a segment's range by its record's seg0 -- the
 * segments of the records before it.  sdf_pool_fetch_plan() makes those records from ranges, on the host, without a context:
 * recs[i] describes r[i] (recs may be NULL: validation and counts only), *any_rc is whether a range carries SDF_FETCH_RC,
 * *n_seg the segments of all of them, *bytes the sum of the lengths; the checks and codes are the host form's (pool_bytes /
 * dst_bytes: the bounds to check against), and *bad receives the index of the first offending range.  The device form
 * checks what it can see -- a resident pool, its alignment, n, n_seg -- and trusts the records: any_rc == 0 with a record
 * whose rc is set copies that range forward. */
#define SDF_FETCH_RC 0x1
#define SDF_FETCH_SEG_BYTES 16384
typedef struct { int64_t off; int32_t len; int32_t flags; int64_t dst_off; } sdf_pool_fetch;
typedef struct {
  int64_t src_off; /* first byte of the range in the pool, in pool order, whatever the strand */
  int64_t dst_off;
  int32_t len;
  int32_t rc;      /* != 0: reversed */
  int64_t seg0;    /* sum of ceil(len / SDF_FETCH_SEG_BYTES) over the records before this one */
} sdf_pool_fetch_rec;
int sdf_pool_fetch_ranges(sdf_ctx *ctx, const sdf_pool_fetch *r, size_t n, char *dst, size_t dst_bytes);
int sdf_pool_fetch_plan(const sdf_pool_fetch *r, size_t n, size_t pool_bytes, size_t dst_bytes, sdf_pool_fetch_rec *recs,
                        int *any_rc, long long *n_seg, size_t *bytes, size_t *bad);
int sdf_pool_fetch_ranges_device(sdf_ctx *ctx, const sdf_pool_fetch_rec *d_recs /* HBM */, size_t n, int any_rc, long long n_seg,
                                 char *d_dst, void *stream);

/* ---- coverage of ranges of the resident pool ------------------------------------------------------------------------------
 * How two sets of intervals cover ranges of the pool: `stats diff` (the reference's get_differences, src/stats_main.cc:397-509)
 * with a chromosome per region, the SDs found as set 0 and the gold standard as set 1.  (pool_cover.hip.)
 *
 * A REGION is a range of the pool.  An INTERVAL is bases [start, start + len) of region `region` -- start counts from the
 * region's first byte -- in set 0 or 1, with a `partner`: another interval's index, or -1.  Two predicates on a pool byte c, both
 * decided on the WHOLE byte as it lies in HBM:
 *   upper(c)     'A' <= c <= 'Z'                the reference's isupper() in the C locale: N and the IUPAC letters count, n and
 *                                               every byte of 128 and above do not
 *   upper_base(c) 'A' <= c <= 'Z' && c != 'N'   the reference's isupper(c) && toupper(c) != 'N': R counts, N and n do not
 * Neither depends on strand: both count bytes of a range, whatever order they are read in, and no interval carries a strand.
 *   1. iv_upper[i] = the bytes of interval i with upper(c).
 *   2. Interval i is PAINTED when partner < 0, or when iv_upper[i] >= min_upper and iv_upper[partner] >= min_upper (the
 *      reference's `qa < 100 || qb < 100` on the two sides of a hit; a partner need not name i back, and may lie in another
 *      region or set).  A painted interval sets its bases in its set's bitmap of its region; iv_painted[i] = 1, else 0.
 *   3. Per region, over its bases x with A / B = x is set in the bitmap of set 0 / 1:  a = |A|, b = |B|, both = |A & B|,
 *      a_only = |A & ~B|, b_only = |B & ~A|, a_only_upper / b_only_upper = the bases of a_only / b_only with upper_base(c).
 * Regions may overlap or repeat: each has bitmaps of its own, one bit a base, in a buffer of the context that
 * sdf_device_bytes() counts (2 bits a base of all regions, zeroed on the stream in front of every call).
 * Before any launch, with the context usable afterwards:
 *   SDF_ERR_INVALID      a region outside sdf_pool_bytes(ctx) or with len < 0, an interval whose region is not in [0, n_regions),
 *                        with len < 0 or not inside [0, region.len), a partner that is neither -1 nor in [0, n_iv), set not 0 or
 *                        1, regions / out == NULL with n_regions > 0, iv == NULL with n_iv > 0, bitmaps that do not fit the
 *                        device's free memory
 *   SDF_ERR_UNSUPPORTED  reserved != 0 (region or interval), more than 2^31 - 1 regions or intervals
 * Legal: intervals and regions with len == 0, n_iv == 0 (all counts zero), n_regions == 0 (with n_iv == 0: nothing is done).
 * iv_upper and iv_painted may be NULL.  Three launches on the context's stream, behind the pool's uploads, with no host wait
 * between them; the call returns with its outputs filled.
 * sdf_pool_coverage_host: the same checks, codes and results in plain C++ over the characters pool[0, pool_bytes), without a
 * context or a device (it has no error text; "free memory" is not asked). */
typedef struct { int32_t region; int32_t start; int32_t len; int32_t set; int32_t partner; int32_t reserved; /* must be 0 */ } sdf_cover_interval;
typedef struct { int64_t a, b, both, a_only, b_only, a_only_upper, b_only_upper; } sdf_cover_counts;
int sdf_pool_coverage(sdf_ctx *ctx, const sdf_pool_range *regions, size_t n_regions, const sdf_cover_interval *iv, size_t n_iv,
                      int32_t min_upper, sdf_cover_counts *out /* n_regions */, int32_t *iv_upper /* n_iv, may be NULL */,
                      uint8_t *iv_painted /* n_iv, may be NULL */);
int sdf_pool_coverage_host(const char *pool, size_t pool_bytes, const sdf_pool_range *regions, size_t n_regions,
                           const sdf_cover_interval *iv, size_t n_iv, int32_t min_upper, sdf_cover_counts *out, int32_t *iv_upper,
                           uint8_t *iv_painted);

/* ---- one resident pool read by several contexts of a device ---------------------------------------------------------
 * dst reads src's resident pool: dst's pool is replaced by a VIEW of src's (same device; SDF_ERR_INVALID otherwise, or when
 * src == dst, or when src is itself a view, or when dst's own pool has views).  sdf_pool_bytes(dst) == sdf_pool_bytes(src) at
 * the time of the call.  The view holds no memory: sdf_device_bytes(dst) does not count it and sdf_destroy(dst) does not free
 * it.  Before the call returns, dst's streams wait for everything src has enqueued on its own: the uploads.
 *   on dst   sdf_pool_upload, sdf_pool_append_fasta(reset != 0) and an anchors call with a host seq_pool drop the view and give
 *            dst a pool of its own again; sdf_pool_append_fasta(reset == 0) answers SDF_ERR_INVALID while dst holds a view.
 *   on src   the owner must not grow or replace its pool while views exist -- a pool that grows moves: sdf_pool_upload,
 *            sdf_pool_append_fasta and an anchors call with a host seq_pool answer SDF_ERR_INVALID ("pool is shared") with the
 *            pool as it was, until every view has been destroyed or has a pool of its own; sdf_pool_host leaves the pool alone.
 * The owner must outlive its views.  sdf_destroy(owner) with live views is the caller's error: the views are left with an
 * EMPTY pool, so their later calls that name a range answer SDF_ERR_INVALID instead of reading freed memory.
 * Not thread-safe against calls in flight on either context: share where the contexts are set up. */
int sdf_pool_share(sdf_ctx *dst, const sdf_ctx *src);

/* Device-resident form: d_packed_pool, d_out and d_cigar_pool are HBM pointers on ctx's device;
 * tasks (host) carry word offsets into d_packed_pool.  Work is enqueued on `stream`
 * (a hipStream_t, NULL = the context's own stream) and the call returns after the stream has
 * drained (it needs *cigar_used).  */
int sdf_extz2_batch_device(sdf_ctx *ctx, const sdf_scoring *sc, const sdf_task *tasks, size_t n,
                           const uint32_t *d_packed_pool, uint32_t want, sdf_result *d_out,
                           uint32_t *d_cigar_pool, size_t cigar_cap, size_t *cigar_used,
                           void *stream);

/* In-band DP cells of a task: the unit of the Gcell/s metric
 * (sum over anti-diagonals of en0-st0+1, reference: extern/ksw2_extz2_sse.cc:101-114). */
int64_t sdf_band_cells(int32_t qlen, int32_t tlen, int32_t w);

/* Timing of the last batch call, from HIP events recorded on the launch streams:
 * which = 0 DP kernels, 1 traceback, 2 CIGAR compaction, 3 whole call (stream time);
 * 4 host-side planning before the first launch, 5 whole call on the host clock.
 * Large batches run as a pipeline of chunks (planning of chunk i+1, DP of chunk i+1 and traceback of chunk i
 * overlap); 0 and 1 are then the time during which at least one DP / traceback kernel was in flight and
 * 6 is the sum of the chunks' DP intervals.  SDF_PIPELINE=0 in the environment of sdf_create() keeps a batch
 * in one chunk on one stream. */
float sdf_last_ms(const sdf_ctx *ctx, int which);
/* Number of DP kernel launches in the last batch call and algorithmic bytes they moved (sdf_stats_cuts_pairs adds its own). */
int sdf_last_launches(const sdf_ctx *ctx);
/* Number of tasks of the last batch call that ran two per wavefront: tasks with the same (qlen, tlen, w, flag)
 * share the reference's band schedule (extern/ksw2_extz2_sse.cc:101-115) and are packed side by side. */
long long sdf_last_paired(const sdf_ctx *ctx);
/* Number of tasks of the last batch call that were run a second time, inside the call, on the one-wavefront / one-workgroup
 * kernels because a stripe kernel's wavefront gave up waiting for its neighbour (SDF_STRIPE_SPIN_CAP polls; the stripe
 * protocol's forward progress rests on the dispatch order).  0 in normal operation. */
long long sdf_last_reran(const sdf_ctx *ctx);
/* Number of tasks of the last batch call that ran one per LANE (extz2_lane.hip): small full-band tasks -- both sequences of
 * at most 256 bases, at most 16,384 cells; SEDEF's gap fills (reference: src/align.cc:235) -- of a batch that holds at
 * least 8,192 of them, under a scoring with match + 2 (gap open + gap extend) <= 127.  They are sorted and planned on the
 * device; the host only marks them. */
long long sdf_last_lane_tasks(const sdf_ctx *ctx);
/* Pairs of the context's last sdf_chain_batch per launch class: out[0..5] the LDS classes of the wavefront kernel
 * (smallest first), out[6] the thread-per-pair kernel, out[7] the LDS cap in bytes of class 5 on this device. */
int sdf_last_chain_classes(const sdf_ctx *ctx, int64_t out[8]);
/* Traceback launches of the context's last batch call per instantiation: out[2 * layout + (G == 16)] counts the launches of
 * the walk over direction-flag layout `layout` (0 general kernel, 1 wave, 2 pair, 3 full-band stripes, 4 banded stripes,
 * 5 lane, 6 strips and chained strips) with groups of G = 64 (one task per wavefront) or G = 16 lanes (four tasks per
 * wavefront).  Counted on the host where the kernels are launched, the parts of a split call and a re-run of abandoned
 * stripe tasks included; all zero after a call that asked for no CIGAR. */
int sdf_last_traceback_classes(const sdf_ctx *ctx, int64_t out[14]);

/* ---- seed anchors on the GPU (next row of the scope table) -----------------------------------
 * Replaces generate_anchors (reference: src/chain.cc:24-101) for a batch of candidate pairs: maximal exact
 * k-mer matches, in the reference's order (query position, then reference position).  Sequences are the raw
 * FASTA characters (case = soft-masking, N = unknown).  kmer <= 15 and sequences shorter than 2 Gb (SDF_ERR_UNSUPPORTED
 * otherwise); any number of pairs per call (the call runs them in ranges that fit its 64-bit sort key).  seq_pool = NULL: the
 * offsets point into the pool sdf_pool_upload left in HBM (pool_bytes: how much of it the pairs may name). */
typedef struct {
  int64_t q_off, r_off; /* byte offsets of query / reference characters in seq_pool */
  int32_t qlen, rlen;
  int32_t same_chr;     /* 1: same chromosome and strand -> k-mers within `kmer` of the main diagonal are skipped */
  int32_t delta;        /* ref_start - query_start of the pair (src/chain.cc:67-69) */
} sdf_anchor_pair;

typedef struct {
  int32_t q, r, l, has_u; /* reference: struct Anchor, src/align.h:25-28 */
} sdf_anchor;

/* out[out_off[i] .. out_off[i+1]) are the anchors of pair i (out_off has n+1 entries).  *out_used receives the
 * total; with SDF_ERR_CIGAR_OVERFLOW it holds the capacity needed. */
int sdf_anchors_batch(sdf_ctx *ctx, const sdf_anchor_pair *pairs, size_t n, const char *seq_pool, size_t pool_bytes,
                      int kmer, sdf_anchor *out, size_t out_cap, int64_t *out_off, size_t *out_used);
/* ... with the anchors left in the context's pinned staging (*out: valid until the context's next anchors call) */
int sdf_anchors_batch_view(sdf_ctx *ctx, const sdf_anchor_pair *pairs, size_t n, const char *seq_pool, size_t pool_bytes,
                           int kmer, const sdf_anchor **out, int64_t *out_off, size_t *out_used);
/* ... of more pairs of the resident pool, written BEHIND the first `keep` anchors of that staging, which stay valid (the stage
 * driver chains one half of a super-batch while the device finds the anchors of the other).  out_off counts from *out.  The
 * staging does not grow here: SDF_ERR_CIGAR_OVERFLOW when it has no room (*out_used: the anchors there would be). */
int sdf_anchors_batch_more(sdf_ctx *ctx, const sdf_anchor_pair *pairs, size_t n, size_t pool_bytes, int kmer, size_t keep,
                           const sdf_anchor **out, int64_t *out_off, size_t *out_used);

/* The three calls with a strand per pair: r_rc[i] != 0 (r_rc: n bytes, or NULL = all forward) reads pair i's REFERENCE
 * range reverse-complemented, rev_dna(pool[r_off + rlen - 1 - x]) as base x (reference: fb = rc(fb), src/align_main.cc:305-306).
 * The anchors are exactly those, in that order, of the plain call on a pool that holds the reverse-complemented bytes of
 * the range; their r are positions in the reverse-complemented sequence.  r_off names the first byte of the range in pool
 * order; same_chr and delta mean what they mean above.  The plain calls are these with r_rc = NULL. */
int sdf_anchors_batch_strand(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, const char *seq_pool,
                             size_t pool_bytes, int kmer, sdf_anchor *out, size_t out_cap, int64_t *out_off, size_t *out_used);
int sdf_anchors_batch_view_strand(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, const char *seq_pool,
                                  size_t pool_bytes, int kmer, const sdf_anchor **out, int64_t *out_off, size_t *out_used);
int sdf_anchors_batch_more_strand(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, size_t pool_bytes,
                                  int kmer, size_t keep, const sdf_anchor **out, int64_t *out_off, size_t *out_used);

/* ---- anchor chaining on the GPU ---------------------------------------------------------------
 * Replaces chain_anchors (reference: src/chain.cc:103-199) for a batch of pairs whose anchors are laid out as
 * sdf_anchors_batch returns them: anchors[off[i] .. off[i+1]).  The reference returns, per pair, `path` (anchor
 * indices, best chain first, each chain from its last anchor backwards) and `boundaries` ({end position in path,
 * any-uppercase flag}, starting with {0, 0}):
 *   path[off[i] + k]                    k-th path element of pair i (index within the pair), k < off[i+1]-off[i]
 *   bounds[2 * (off[i] + i + b) + 0/1]  b-th boundary of pair i, b < nbound[i]
 * path holds off[n] entries, bounds 2 * (off[n] + n), nbound n.  max_chain_gap / match_chain_score are the
 * reference's MAX_CHAIN_GAP / MATCH_CHAIN_SCORE (src/common.h).  Coordinates and scores are `int` and are ordered as
 * `int`, as in the reference: negative ones sort before the others, whichever kernel takes the pair. */
int sdf_chain_batch(sdf_ctx *ctx, const sdf_anchor *anchors, const int64_t *off, size_t n, int max_chain_gap,
                    int match_chain_score, int32_t *path, int32_t *bounds, int32_t *nbound);

/* ---- per-alignment columns of `stats generate` on the GPU (scope row f4) -------------------------
 * Replaces the column walk of process() (reference: src/stats_main.cc:228-270) and the AlignmentError counters of
 * populate_nice_alignment (src/align.cc:300-314) for a batch of finished alignments.  An alignment is the two
 * sequences as FASTA characters (case = soft-masking) and its CIGAR as runs `len << 4 | op` with op 0 = 'M',
 * 1 = 'D' (consumes a only), 2 = 'I' (consumes b only) -- the reference's letters (src/align.cc:59-63), numerically
 * the words sdf_extz2_batch returns.  Nothing is expanded into column strings.  Sequences up to 16 Mb
 * (SDF_ERR_UNSUPPORTED beyond); a CIGAR that consumes more than its sequences, where the reference would read past
 * its strings, sets `flags` to 1 and makes the host-buffer call return SDF_ERR_INVALID. */
typedef struct {
  uint64_t a_off, b_off;   /* byte offsets of the two sequences in seq_pool */
  uint32_t a_len, b_len;
  uint64_t cigar_off;      /* first run of the alignment in cigar_pool (in words) */
  uint32_t n_cigar, reserved; /* sdf_stats_columns_pairs: SDF_STATS_A_RC | SDF_STATS_B_RC; the other calls ignore it */
} sdf_stats_task;

typedef struct {
  /* src/stats_main.cc:231-270, in the order of the output columns 15-21 and 27-29 */
  int32_t indel_a, indel_b, aln_b, match_b, mismatch_b, transitions_b, transversions_b;
  int32_t uppercase_a, uppercase_b, uppercase_matches;
  /* Alignment::matches() / mismatches() / gaps() / gap_bases() / span() (src/align.h:79-83) */
  int32_t matches, mismatches, gaps, gap_bases, span;
  int32_t flags;           /* 1: the CIGAR does not fit the sequences (counters undefined) */
} sdf_stats_cols;

int sdf_stats_columns_batch(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, const char *seq_pool, size_t pool_bytes,
                            const uint32_t *cigar_pool, size_t cigar_words, sdf_stats_cols *out);
/* The same with tasks, pools and results resident in HBM; asynchronous on `stream` (a hipStream_t; NULL = the
 * context's own stream, synchronised before returning).  Offsets are not checked against the pools here.  One
 * wavefront takes one alignment; an alignment of more than 1,024 runs is cut into segments of 512 runs on the device, which
 * wavefronts of a second launch count side by side (a list of 2^18 segments in the context: calls on one context do not
 * overlap). */
int sdf_stats_columns_device(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, const char *d_seq_pool,
                             const uint32_t *d_cigar_pool, sdf_stats_cols *d_out, void *stream);

/* Alignments on the RESIDENT pool, by range and strand: a_off / b_off are byte offsets into the characters sdf_pool_upload or
 * sdf_pool_append_fasta left in HBM (after sdf_pool_append_fasta: *base_off + x), and no character crosses PCIe.  The strand
 * bits travel in sdf_stats_task::reserved and follow the rule of SDF_TASK_Q_RC / SDF_TASK_T_RC: base i of a reversed side is
 * rev_dna(pool[off + len - 1 - i]) -- rev_dna: the reference's table (src/common.h:72-87,93), indexed c & 127 as the host does:
 * the case is kept, everything that is not ACGTacgt becomes upper-case 'N' -- and `off` keeps naming the first byte of the range
 * in pool order.  The counters are those of sdf_stats_columns_batch on a pool that holds the reverse-complemented bytes.
 * Only these two calls read `reserved`; sdf_stats_columns_batch / sdf_stats_columns_device never do. */
#define SDF_STATS_A_RC 0x1 /* side a is the reverse complement of its range */
#define SDF_STATS_B_RC 0x2 /* side b likewise */
/* Host form: tasks, runs and results in host memory.  SDF_ERR_INVALID: a sequence range outside sdf_pool_bytes() (an empty
 * pool holds no non-empty range), a CIGAR range outside cigar_words, or -- after the launch, out[] filled, flags == 1 on the
 * record -- a CIGAR that does not fit its sequences.  SDF_ERR_UNSUPPORTED: a bit of `reserved` beyond the two above
 * ("unknown stats task flag"), a side of more than 16 Mb.  All checks but the last precede the first launch.  A call
 * without a reversed side runs the kernels of sdf_stats_columns_device. */
int sdf_stats_columns_pairs(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, const uint32_t *cigar_pool, size_t cigar_words,
                            sdf_stats_cols *out);
/* Device form: tasks, runs and results in HBM, asynchronous on `stream` like sdf_stats_columns_device (NULL: the context's
 * own stream, synchronised before returning).  Offsets are not checked.  any_rc != 0: some task may carry a strand bit;
 * any_rc == 0: the bits are not looked at.  The pool's uploads are enqueued on the context's stream: a caller with a
 * stream of its own calls sdf_pool_sync() between the last upload and this call. */
int sdf_stats_columns_pairs_device(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, int any_rc,
                                   const uint32_t *d_cigar_pool, sdf_stats_cols *d_out, void *stream);

/* ---- the cuts of `stats generate` on the RESIDENT pool: match counter, assembly-gap cuts, trims ----------------------
 * What the host does to every input alignment before the column counters (reference: Alignment(fa, fb, cigar),
 * src/align.cc:90-105; split_alignment, src/stats_main.cc:163-211; subhit with trim_back / trim_front, src/stats_main.cc:33-84,
 * src/align.cc:343-456), for the tasks sdf_stats_columns_pairs takes: ranges of the resident pool, strand bits in `reserved`,
 * runs `len << 4 | op`.  All in COLUMN space: column i of side a is '-' inside an I run, of side b inside a D run.
 *   matches   Two characters match when they are equal ignoring case and are not N (sdf_stats_cols::matches).
 *   events    A column is N for a side when toupper(c) == 'N': on a forward side the bytes 'N' and 'n'; on a reversed side the
 *             character is rev_dna(pool byte), so every byte that is not ACGTacgt (indexed c & 127) is N; '-' is not N.  A
 *             maximal N run [s, e) of one side is an event at e when e - s >= 100 and a non-N column follows it (e < span; a
 *             run that reaches the last column is no event).  Events are ordered by e; at equal e, side a's comes first.
 *   pieces    With begin = 0 before the first event, every event emits the piece [begin, s) if s > begin, then sets begin = e;
 *             after the last event the final piece is [begin, span).  An alignment without an event is ONE piece [0, span),
 *             and that piece is NOT trimmed.
 *   trims     Every piece of an alignment that has an event goes through trim_back, then trim_front on the result.  A pair
 *             column scores `match` or `mismatch`; a gap column `gap_extend`, plus `gap_open` when it is the first column of
 *             the scan or its neighbour towards the scan's origin is not a gap in the same sequence (a piece that starts
 *             inside a gap run pays gap_open at its first column).  trim_back keeps the best prefix: score >= best, from
 *             best = 0, ties to the longer prefix; no prefix reaches 0: the piece becomes empty.  trim_front keeps the best
 *             suffix of what trim_back kept, ties to the longer suffix.  The reference's "nothing found" marker there is the
 *             number of a-bases of the piece, not its column count: a best suffix that starts at that column of the piece
 *             empties the piece, and so it does here.
 * Per piece one record: the untrimmed columns [begin, end), the trimmed columns [t_begin, t_end) (t_begin == t_end: emptied)
 * and the matches inside the trimmed range.  Everything else (bases before and inside a range, run slices, gaps, gap bases,
 * mismatches) follows from the CIGAR.  pieces[first[i] .. first[i + 1]) are alignment i's, in column order; first has n + 1
 * entries, in TASK order.  Scores: |match|, |mismatch| <= 63 and |gap_open| + |gap_extend| <= 63 (sums in 32 bits over 2^25
 * columns; SDF_ERR_UNSUPPORTED beyond).  One wavefront per alignment, whatever its number of runs. */
typedef struct {
  int32_t begin, end;     /* the piece as it was cut, in the alignment's columns */
  int32_t t_begin, t_end; /* ... after the trims */
  int32_t matches;        /* match columns of [t_begin, t_end) */
  int32_t flags;          /* 1: the CIGAR does not fit the sequences (the alignment's ONE record; ranges 0) */
  int32_t reserved[2];
} sdf_stats_piece;
/* Host form.  pieces_cap: capacity of `pieces` in records.  SDF_ERR_CIGAR_OVERFLOW when the batch needs more: *pieces_used
 * holds the need, first[] is filled, and nothing is written to `pieces`; else *pieces_used = first[n].  SDF_ERR_INVALID: a
 * sequence range outside sdf_pool_bytes(), a CIGAR range outside cigar_words, or -- after the launches, everything filled,
 * flags == 1 on the alignment's record -- a CIGAR that does not fit its sequences.  SDF_ERR_UNSUPPORTED: a bit of `reserved`
 * beyond SDF_STATS_A_RC | SDF_STATS_B_RC, a side of more than 16 Mb, scores out of range.  All checks but the CIGAR misfit
 * precede the first launch; n == 0 is SDF_OK without one (first[0] = 0).  sdf_last_launches() grows by the call's launches
 * (two for the count, one more for the records), and not at all for a call that is refused. */
int sdf_stats_cuts_pairs(sdf_ctx *ctx, const sdf_stats_task *tasks, size_t n, const uint32_t *cigar_pool, size_t cigar_words,
                         int match, int mismatch, int gap_open, int gap_extend, uint64_t *first, sdf_stats_piece *pieces,
                         size_t pieces_cap, size_t *pieces_used);
/* Device form: tasks, runs, d_first (n + 1 entries) and d_pieces in HBM, asynchronous on `stream` (NULL: the context's own
 * stream, synchronised before returning -- then *pieces_used, if given, holds d_first[n] and the call answers
 * SDF_ERR_CIGAR_OVERFLOW when that exceeds pieces_cap).  An alignment whose pieces do not all lie below pieces_cap writes
 * none, so no record is written past the capacity; with a stream of its own the caller compares d_first[n] with pieces_cap
 * itself.  Offsets are not checked; any_rc and the pool's uploads as for sdf_stats_columns_pairs_device.  The counts of the
 * call live in the context: calls on one context do not overlap. */
int sdf_stats_cuts_pairs_device(sdf_ctx *ctx, const sdf_stats_task *d_tasks, size_t n, int any_rc, const uint32_t *d_cigar_pool,
                                int match, int mismatch, int gap_open, int gap_extend, uint64_t *d_first,
                                sdf_stats_piece *d_pieces, size_t pieces_cap, size_t *pieces_used, void *stream);

/* ---- winnowed minimizers of ranges of the resident pool, and the index over them (minimizers.hip) --------------------------
 * What `sedef search -k 12 -w 16` rests on: get_minimizers and Index::Index of the reference (src/hash.cc:53-141), for many
 * ranges in one call.  The sequence s of a range is pool[off, off + len) as it lies, or -- SDF_MINIM_RC -- its reverse complement
 * by rev_dna (s[i] = rev_dna(pool[off + len - 1 - i]): every byte that is not ACGTacgt becomes 'N'; loc counts in s, as for the
 * reference's Sequence(..., is_rc)).  Characters are taken & 127 on either strand.  With k-mer starts j = 0 .. len - k:
 *   hash     the 2-bit codes of s[j, j + k), first character most significant: A/a 0, C/c 1, G/g 2, T/t 3, anything else 0
 *   status   2 when one of the k characters is N or n, else 0 when one is an uppercase letter, else 1 -- or 0 with
 *            separate_lowercase == 0
 *   root     start j is a root when no y in [max(0, j - w), j) has (status, hash)(y) < (status, hash)(j); equal keys do not
 *            suppress each other, start 0 is always one
 *   records  the largest root <= w, then every root > w, in ascending loc; none when the range has w starts or fewer.
 * That is the reference's deque loop, whose second loop tests the back and pops the front, in closed form
 * (tests/minim_model.py holds the loop as written).  out[first[i], first[i + 1]) are range i's records, `range` = i.
 * Limits: k 1..15 (the reference's mask is undefined at 16), w 1..SDF_MINIM_MAX_W (a wavefront keeps the keys of a block of
 * SDF_MINIM_BLOCK starts and of the w before them in LDS, and looks back w deep per start).
 *
 * Host form.  Every check precedes the first launch, and a refused call launches nothing (sdf_last_launches() as it was):
 *   SDF_ERR_INVALID      off < 0, len < 0, off + len > sdf_pool_bytes(ctx), w < 1, r / first / used == NULL with n > 0,
 *                        out == NULL with cap > 0
 *   SDF_ERR_UNSUPPORTED  k outside 1..15, w > SDF_MINIM_MAX_W, a flags bit other than SDF_MINIM_RC
 * n == 0 is SDF_OK without a launch.  SDF_ERR_CIGAR_OVERFLOW when the ranges have more than cap records: *used holds the need,
 * first[] is filled and nothing is written to out; else *used = first[n].  Six launches: blocks per range and their scan, records
 * per block and their scan, first[], the records (five when cap is short).  Works on a view (sdf_pool_share) like every reader
 * of the pool; enqueued on the context's stream behind the pool's uploads, returns with everything filled. */
#define SDF_MINIM_RC 0x1
#define SDF_MINIM_BLOCK 1024  /* k-mer starts of one range that one wavefront takes (sdf_minimizer_block()) */
#define SDF_MINIM_MAX_W 1000
typedef struct { int64_t off; int32_t len; int32_t flags; } sdf_minim_range;
typedef struct { uint32_t hash; int32_t loc; int32_t status; int32_t range; } sdf_minimizer; /* 16 bytes */
int sdf_minimizer_block(void); /* SDF_MINIM_BLOCK as the library was built */
int sdf_pool_minimizers(sdf_ctx *ctx, const sdf_minim_range *r, size_t n, int k, int w, int separate_lowercase,
                        uint64_t *first /* n + 1 */, sdf_minimizer *out, size_t cap, size_t *used);
/* Device form: ranges, d_first (n + 1 entries) and d_out in HBM.  k, w and n are checked as above; the ranges are not, but a
 * range that does not lie in the pool or carries an unknown flag has no records instead of being read.  any_rc == 0 with a range
 * that carries SDF_MINIM_RC reads that range forward.  The call waits ONCE on the host, for the ranges' block count (eight
 * bytes), before it enqueues the other launches on `stream` (NULL: the context's own, synchronised before returning -- then
 * *used, if given, holds d_first[n] and the call answers SDF_ERR_CIGAR_OVERFLOW when that exceeds cap).  No record is written
 * at or behind d_out[cap]; with a stream of its own the caller compares d_first[n] with cap itself.  The pool's uploads as for
 * sdf_stats_columns_pairs_device (sdf_pool_sync() first).  The counts of the call live in the context: calls on one context
 * do not overlap. */
int sdf_pool_minimizers_device(sdf_ctx *ctx, const sdf_minim_range *d_ranges, size_t n, int any_rc, int k, int w,
                               int separate_lowercase, uint64_t *d_first, sdf_minimizer *d_out, size_t cap, size_t *used,
                               void *stream);
/* The index of every range (Index::Index): the range's records grouped by (status, hash) -- sorted[first[i], first[i + 1]) are
 * range i's in ascending (status, hash, loc) order, so a group is a run of equal (status, hash) with ascending locs --,
 * n_groups[i] the number of groups and threshold[i] the reference's cutoff: with ignore = int(records * 0.001 / 100.0) (the
 * reference's doubles), the distinct group sizes are walked from the largest down, the groups of each size added up, and while
 * the sum is <= ignore the threshold becomes that size; it starts at 2147483648 and stays there for fewer than 100,000 records.
 * Checks, overflow protocol (cap, *used) and first[] as for sdf_pool_minimizers; n_groups and threshold (n entries each) must
 * be given.  At most 2^31 - 1 records in one call (SDF_ERR_UNSUPPORTED beyond).  One radix sort of range | status | hash
 * keys (stable: the records come in loc order), one more of the group sizes.  There is NO device form of the index: the call
 * reads the number of records and of groups back to size its sorts. */
int sdf_pool_minimizer_index(sdf_ctx *ctx, const sdf_minim_range *r, size_t n, int k, int w, int separate_lowercase,
                             uint64_t *first /* n + 1 */, sdf_minimizer *sorted, size_t cap, size_t *used,
                             uint32_t *n_groups /* n */, uint32_t *threshold /* n */);

/* ---- search seeding: the reference intervals of every query window (search_seeds.hip) -----------------------------------------
 * The front half of the reference's search() (src/search.cc:395-452) for EVERY query minimizer in one call, with an EMPTY
 * tree: the exclusions of the SDs already found (pf->second.find(pos)) are sdf_search_windows_found's, in the section behind
 * this one.  Inputs: q[0, nq), the query range's minimizers in ascending loc as sdf_pool_minimizers writes
 * them; r_sorted[0, nr), the reference range's records in ascending (status, hash, loc) as sdf_pool_minimizer_index writes them
 * for ONE range (status 0..2, compared unsigned; `range` is not read); r_threshold, that range's threshold; len_q, the query
 * sequence's length; limit[0, n_limit), the caller's table of relaxed_jaccard_estimate(query_size) (src/util.cc:85 -- the library
 * never computes it).  For window i, with qs = q[i].loc:
 *   1. qs + init_len > len_q: SDF_SEARCH_SHORT, every count 0, no intervals.
 *   2. members: j = i, i + 1, ... while q[j].loc - qs <= init_len (inclusive); n_members of them.
 *   3. query_size: the distinct (status, hash) among the members, whatever their status.
 *   4. a member seeds when uppercase_seeds == 0 or its status is 0.  Its group is the run of r_sorted with its (status, hash);
 *      absent, or of r_threshold records and more: skipped.  n_gathered: the sizes of the other groups added up, one term per
 *      seeding member (two members with one key count their group twice), before any filter; 2^31 - 1 when the sum is larger.
 *      Candidates: the locs of those groups, with same_genome only those >= qs + init_len, as a SET: ascending, distinct;
 *      n_candidates of them.
 *   5. query_size >= n_limit: SDF_SEARCH_NOLIMIT, no intervals (the counts stay).  Else L = limit[query_size].
 *   6. for a = 0 .. n_candidates - L, b = a + L - 1: when c[b] - c[a] <= init_len, x = max(0, c[b] - init_len + 1) and
 *      y = c[a] + 1; if there is a last interval and x < last.end (strictly) then last.end = max(last.end, y), else (x, y) is
 *      pushed.
 *   7. same_genome: start = max(start, qs + init_len), and an interval with start > end is dropped.
 * out[first[i], first[i + 1]) are window i's intervals, in ascending order.
 *
 * SDF_SEARCH_WIDE: n_members > SDF_SEARCH_MAX_MEMBERS or n_gathered > SDF_SEARCH_MAX_GATHER -- both read off the inputs, so the
 * flag does not depend on who computes.  The device form flags such a window, fills its counts except n_candidates (0) and
 * writes no interval for it; sdf_search_windows completes it on the host (sdf_search_windows_host's code on the arrays it was
 * given), into the same first[] / out layout, and keeps the flag: its answer is complete for every input.
 * sdf_search_windows_wide_device (behind the found records' section) finishes such a window on the device up to
 * SDF_SEARCH_WIDE_MAX_GATHER gathered positions, and marks it SDF_SEARCH_WIDE_DONE in place of the flag.
 *
 * Overflow as for sdf_pool_minimizers: SDF_ERR_CIGAR_OVERFLOW when the windows have more than cap intervals -- *used holds the
 * need, first[] and windows[] are filled, nothing is written to out; no record is ever written at or behind out[cap].
 *   SDF_ERR_INVALID      a null pointer with nq > 0 (out may be null with cap == 0; r_sorted with nr == 0), init_len < 1
 *   SDF_ERR_UNSUPPORTED  limit[s] < 1 for some s >= 1 (the reference indexes candidates[-1] there; the device form reads such
 *                        an entry as 1 instead of checking), init_len > 2^30, nq > 2^30 - 1, nr or n_limit > 2^31 - 1
 * Every check precedes the first launch.  nq == 0 is SDF_OK without a launch (*used = 0; the host forms set first[0] = 0, the
 * device form leaves d_first as it is).  The call reads no
 * pool; it uses the context's stream and buffers: calls on one context do not overlap. */
#define SDF_SEARCH_SHORT 0x1
#define SDF_SEARCH_NOLIMIT 0x2
#define SDF_SEARCH_WIDE 0x4
#define SDF_SEARCH_MAX_MEMBERS 1024
#define SDF_SEARCH_MAX_GATHER 4096
typedef struct { int32_t query_size, n_members, n_gathered, n_candidates; uint32_t flags; } sdf_search_window; /* 20 bytes */
typedef struct { int32_t start, end; } sdf_search_interval;
int sdf_search_windows(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                       uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *limit,
                       size_t n_limit, uint64_t *first /* nq + 1 */, sdf_search_window *windows /* nq */,
                       sdf_search_interval *out, size_t cap, size_t *used);
/* Device form: every array in HBM, nothing checked beyond the scalars, no host wait: the launches are enqueued on `stream` (NULL:
 * the context's own, synchronised before returning -- then *used, if given, holds d_first[nq] and the call answers
 * SDF_ERR_CIGAR_OVERFLOW when that exceeds cap).  WIDE windows as said above.  The intervals that lie below d_out[cap] are
 * written whatever the need, none at or behind it; with a stream of its own the caller compares d_first[nq] with cap itself. */
int sdf_search_windows_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted,
                              size_t nr, uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                              const int32_t *d_limit, size_t n_limit, uint64_t *d_first, sdf_search_window *d_windows,
                              sdf_search_interval *d_out, size_t cap, size_t *used, void *stream);
/* No context, no GPU: steps 1 to 7 in plain C++, every window (WIDE ones flagged and completed).  Same checks and codes. */
int sdf_search_windows_host(const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                            uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *limit,
                            size_t n_limit, uint64_t *first /* nq + 1 */, sdf_search_window *windows /* nq */,
                            sdf_search_interval *out, size_t cap, size_t *used);

/* ---- search against the SDs already found: the tree's two queries (search_found.hip) --------------------------------------------
 * The reference's Tree (src/search.h: Boost.ICL interval maps that aggregate by set union) is read in two places: search()
 * drops a gathered position `pos` of the member at `loc` when the tree's segment at loc covers pos (src/search.cc:420-434), and
 * search_in_reference_interval asks is_overlap (src/search.cc:35-71, called at :335) before it filters and extends.  Both are
 * answered here for every window and every rolled interval of a call at once, against an explicit list found[0, nf) of records
 * {q_start, q_end, r_start, r_end} in the order the hits were added: a hit is added as a = [query_start, query_end) and
 * b = [ref_start, ref_end), both right-open.  The tree only grows as far as a later query can see -- the reference's
 * tree -= Interval(0, query_start - MIN_READ_SIZE) removes only points below every loc a later window asks for --, so what a
 * query sees is a PREFIX found[0, v) of the list:
 *   tree.find(loc)->second.find(pos) != end()   exactly when a visible record has q_start <= loc < q_end and
 *                                               r_start <= pos < r_end;
 *   is_overlap iterates                         exactly the visible records with q_start <= pf_pos < q_end and
 *                                               r_start <= pfp_pos < r_end;
 *   a record with q_start >= q_end or r_start >= r_end is never visible (ICL adds nothing for an empty interval and absorbs an
 *   empty Subtree).
 * The prefix is per WINDOW for the exclusions (the tree is read before the window's intervals are walked) and per INTERVAL for
 * is_overlap (a hit of a window's first interval is in the tree when its second is tested).  tests/found_model.py holds the
 * record-list statement and a point-level model of the ICL tree that ties it to the reference's text.  parse_hits,
 * next_to_attain and the acceptance step of a round-based driver stand in the search driver's section, behind the extension.
 *
 * sdf_search_windows_found*: sdf_search_windows* with found, nf and visible[0, nq) -- window i sees found[0, visible[i]).  Steps
 * 1 to 7 as written there, with one addition in step 4: a gathered position pos of the member at loc is dropped when a visible
 * record has q_start <= loc < q_end && r_start <= pos < r_end.  The exclusion is per (member, position): a position dropped for
 * one member stays a candidate when another member gathers it and no record excludes it there.  n_gathered is unchanged (it is
 * counted before any filter), n_candidates counts what is left.  With nf == 0, or every visible[i] == 0, the output equals
 * sdf_search_windows* byte for byte.
 *
 * SDF_SEARCH_FOUND_WIDE: more than SDF_SEARCH_MAX_FOUND distinct visible, non-empty records have q_start <= qs + init_len and
 * q_end > qs -- the records that can contain a member's loc.  Read off the inputs, so the flag does not depend on who computes;
 * a SHORT window carries SHORT alone.  The device form flags such a window, fills its counts except n_candidates (0) and writes
 * no interval for it, as for WIDE (a window may carry both); sdf_search_windows_found completes it on the host and keeps the
 * flag.
 *
 * The device keeps a bin index over the query axis, rebuilt by every call: the bin of a base is base >>
 * SDF_SEARCH_FOUND_BIN_SHIFT (a base below 0 counts as 0), and a non-empty record is entered in every bin that
 * [q_start, q_end) touches.  The forms that take host arrays size the index themselves; the device forms take
 * found_entries_cap, the entries the caller grants (sdf_search_found_entries counts them for a host list), and write the need to
 * *d_found_entries (device memory, or NULL).  When the need exceeds the grant the index is incomplete and the outputs of the
 * call are NOT the answer -- no entry is written at or behind the grant, and none is read --; with the context's own stream the
 * call then answers SDF_ERR_CIGAR_OVERFLOW (the need in sdf_last_error's text and in *d_found_entries), with a stream of its
 * own the caller compares *d_found_entries with the grant itself.
 *   SDF_ERR_INVALID      as for sdf_search_windows; found == NULL with nf > 0, visible == NULL; checked forms: visible[i] > nf
 *                        (the device form reads such a prefix as nf)
 *   SDF_ERR_UNSUPPORTED  as for sdf_search_windows; nf > 2^31 - 1, more than 2^31 - 1 bin entries (found_entries_cap beyond it)
 * Every check precedes the first launch.  The device form enqueues on the caller's stream without a host wait: three launches
 * for the index, then those of sdf_search_windows_device. */
typedef struct { int32_t q_start, q_end, r_start, r_end; } sdf_search_found; /* 16 bytes */
#define SDF_SEARCH_FOUND_WIDE 0x8   /* window flag, next to SHORT / NOLIMIT / WIDE */
#define SDF_SEARCH_MAX_FOUND 256
#define SDF_SEARCH_FOUND_BIN_SHIFT 12
/* the bin entries of a list: what found_entries_cap must grant */
int sdf_search_found_entries(const sdf_search_found *found, size_t nf, uint64_t *entries);
int sdf_search_windows_found(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                             uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *limit,
                             size_t n_limit, const sdf_search_found *found, size_t nf, const uint32_t *visible /* nq */,
                             uint64_t *first /* nq + 1 */, sdf_search_window *windows /* nq */, sdf_search_interval *out, size_t cap,
                             size_t *used);
int sdf_search_windows_found_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted,
                                    size_t nr, uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                    const int32_t *d_limit, size_t n_limit, const sdf_search_found *d_found, size_t nf,
                                    size_t found_entries_cap, uint64_t *d_found_entries /* or NULL */, const uint32_t *d_visible,
                                    uint64_t *d_first, sdf_search_window *d_windows, sdf_search_interval *d_out, size_t cap,
                                    size_t *used, void *stream);
int sdf_search_windows_found_host(const sdf_minimizer *q, size_t nq, int64_t len_q, const sdf_minimizer *r_sorted, size_t nr,
                                  uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds, const int32_t *limit,
                                  size_t n_limit, const sdf_search_found *found, size_t nf, const uint32_t *visible /* nq */,
                                  uint64_t *first /* nq + 1 */, sdf_search_window *windows /* nq */, sdf_search_interval *out,
                                  size_t cap, size_t *used);
/* sdf_search_windows_wide_device: sdf_search_windows_found_device, and the windows it flags WIDE or FOUND_WIDE finished on the
 * device by a second kernel (search_seeds_wide.hip: one workgroup of 256 lanes per window, 32-bit keys of
 * SDF_SEARCH_WIDE_MAX_GATHER positions in LDS, the found records walked out of the bins in chunks of 256 -- any number of them).
 *   eligible   a window of the existing device form with WIDE and/or FOUND_WIDE, without NOLIMIT, with n_members <=
 *              SDF_SEARCH_MAX_MEMBERS and n_gathered <= SDF_SEARCH_WIDE_MAX_GATHER.  All read off the inputs.
 *   listed     the LOWEST n_wide_max eligible window indices, in ascending order (an ordered compaction: which windows stay
 *              behind does not depend on how the device ran).  *d_wide_total (HBM, or NULL) receives the number of eligible
 *              windows, so a caller sees that the list was short.
 *   completed  a listed window's record has WIDE and FOUND_WIDE CLEARED and SDF_SEARCH_WIDE_DONE set; every other field,
 *              first[] and its intervals are byte for byte what sdf_search_windows_found_host / sdf_search_windows_found write
 *              for it (those forms keep the WIDE bits, and stay as they are).  With the old bits cleared the acceptance step,
 *              the roll and everything behind them take the window like any other.
 *   the rest   a window that is not eligible, or not among the first n_wide_max, keeps exactly the record the existing device
 *              form writes, and has no interval.
 * Launches, on one stream without a host wait: the existing count pass, the list, the wide count, the scan of the counts, the
 * existing emit pass (which writes nothing for a window it finds WIDE or FOUND_WIDE), the wide emit: the listed windows' intervals
 * at first[i], nothing at or behind d_out[cap].  nf == 0 with d_visible == NULL runs the plain instantiations without an index.
 * n_wide_max == 0 is sdf_search_windows_found_device byte for byte (*d_wide_total is not written).  Refusals are that form's,
 * before the first launch, and SDF_ERR_UNSUPPORTED for n_wide_max > 2^20. */
#define SDF_SEARCH_WIDE_DONE 0x10   /* window flag: finished by sdf_search_windows_wide_device */
#define SDF_SEARCH_WIDE_MAX_GATHER 32768
int sdf_search_windows_wide_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, int64_t len_q, const sdf_minimizer *d_r_sorted,
                                   size_t nr, uint32_t r_threshold, int32_t init_len, int same_genome, int uppercase_seeds,
                                   const int32_t *d_limit, size_t n_limit, const sdf_search_found *d_found, size_t nf,
                                   size_t found_entries_cap, uint64_t *d_found_entries /* or NULL */, const uint32_t *d_visible,
                                   uint64_t *d_first, sdf_search_window *d_windows, sdf_search_interval *d_out, size_t cap,
                                   size_t *used, size_t n_wide_max, uint64_t *d_wide_total /* or NULL */, void *stream);
/* (sdf_search_overlap*, the tree's second query, stand behind the filter's section: they take its tasks) */

/* ---- search roll: every reference interval rolled to its best initial match (search_roll.hip) ----------------------------------
 * The first loop of the reference's search_in_reference_interval (src/search.cc:274-314, "Roll until we find best inital
 * match") for EVERY interval of sdf_search_windows in one call.  It reads no tree; filter and extend follow it in their own
 * sections, is_overlap in its own behind them; the tree update is the caller's list.  Inputs: q[0, nq), windows[0, nq), first[0, nq + 1] and
 * intervals[0, first[nq]) as sdf_search_windows takes and writes them; r[0, nr), the reference range's minimizers in ASCENDING
 * LOC (sdf_pool_minimizers' list, not the sorted index); len_r, the reference sequence's length; init_len; limit[0, n_limit),
 * the same table.
 *
 * Interval t belongs to window i, first[i] <= t < first[i + 1]; its members are q[i .. i + windows[i].n_members) and
 * L = limit[windows[i].query_size].  A key is (status, hash), compared as status << 32 | hash, unsigned.  The state is the
 * reference's SlidingMap as it behaves, not a clean pair of sets: bits[key] in {0, 1, 2, 3} (1: query, 2: reference; a key is
 * STORED while bits != 0), a boundary key B and a counter I.  At the start bits = 1 for every distinct member key, whatever
 * its status, B is the largest member key and I = 0.
 *   add(record)     nothing for status 2.  Else, k its key: bits[k] & 2: nothing.  bits[k] == 1: bits[k] = 3, and I += 1 when
 *                   k < B -- strictly: an add that lands on B itself is never counted (quirk 1).  bits[k] == 0: bits[k] = 2,
 *                   and when k < B: I -= (bits[B] == 3), then B becomes the largest stored key below B (that may be k).
 *   remove(record)  nothing for status 2, or when bits[k] & 2 == 0 (the key came twice and an earlier remove cleared the bit:
 *                   two adds set one bit and one remove clears it -- quirk 2, the count depends on the path).  Else, when
 *                   k <= B: I -= (bits[k] == 3), and when bits[k] == 2, B becomes the smallest stored key above B and
 *                   I += (bits[B] == 3).  Then bits[k] &= ~2.
 *   J = I >= L ? I : I - L.  I may go negative; J is defined all the same.
 *   walk   1. s = start, e = min(start + init_len, len_r).
 *          2. ws = the first index with r[ws].loc >= s (nr: none); we = ws.
 *          3. while we < nr and r[we].loc < e: add(r[we++]).
 *          4. best = (s, e, ws, we, J).
 *          5. while s < end and e < len_r:  if ws < nr and r[ws].loc <= s: remove(r[ws++]);  if we < nr and r[we].loc == e:
 *             add(r[we++]);  if J > best.J (strictly): best = (s, e, ws, we, J);  s++, e++.
 * out[t] = best as {ref_start, ref_end, winnow_start, winnow_end, jaccard, flags}.
 *
 * The device keeps a key in 32 bits, status << 30 | hash: hash < 2^30 is the contract (k <= 15, as sdf_pool_minimizers writes
 * them), and status is 0, 1 or 2.  The host form compares whole keys.
 *
 * SDF_ROLL_WIDE: windows[i].n_members > SDF_SEARCH_MAX_MEMBERS, or more than SDF_ROLL_MAX_SPAN records of r have
 * start <= loc <= end + init_len -- both read off the inputs, so the flag does not depend on who computes.  The device form
 * flags such an interval and writes the rest of its record as zero; sdf_search_roll completes it on the host
 * (sdf_search_roll_host's code) and keeps the flag.  SDF_ROLL_BADWINDOW (device form only, which checks no array): the
 * window's query_size is outside the table or its n_members outside 1 .. nq - i; the rest of the record is zero.
 *   SDF_ERR_INVALID      a null array with nq > 0 (intervals and out may be null when first[nq] == 0), init_len < 1, len_r < 0,
 *                        nr == 0 with any interval; host forms: first[] not ascending from 0, an interval with start > end or
 *                        start < 0, and on a window that has intervals query_size outside [0, n_limit) or n_members outside
 *                        1 .. nq - i
 *   SDF_ERR_UNSUPPORTED  init_len > 2^30, nq > 2^30 - 1, nr, n_limit, len_r or the number of intervals > 2^31 - 1
 * Every check precedes the first launch.  nq == 0 or no interval is SDF_OK without a launch. */
#define SDF_ROLL_WIDE 0x1
#define SDF_ROLL_BADWINDOW 0x2
#define SDF_ROLL_MAX_SPAN 3072
typedef struct { int32_t ref_start, ref_end, winnow_start, winnow_end, jaccard; uint32_t flags; } sdf_search_roll_rec; /* 24 bytes */
int sdf_search_roll(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                    const sdf_search_interval *intervals, const sdf_minimizer *r, size_t nr, int64_t len_r, int32_t init_len,
                    const int32_t *limit, size_t n_limit, sdf_search_roll_rec *out /* first[nq] */);
/* Device form: every array in HBM, nothing checked beyond the scalars, no host wait, so that it follows
 * sdf_search_windows_device on one stream: n_max wavefronts are enqueued on `stream` (NULL: the context's own, synchronised
 * before returning), those at or beyond d_first[nq] leave at once.  d_out has n_max records; nothing is written at or behind
 * d_out[n_max], and an interval at or behind n_max has no record.  n_max == 0 is SDF_OK without a launch. */
int sdf_search_roll_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                           const uint64_t *d_first, const sdf_search_interval *d_intervals, size_t n_max, const sdf_minimizer *d_r,
                           size_t nr, int64_t len_r, int32_t init_len, const int32_t *d_limit, size_t n_limit,
                           sdf_search_roll_rec *d_out, void *stream);
/* No context, no GPU: the same in plain C++, every interval (WIDE ones flagged and completed).  Same checks and codes. */
int sdf_search_roll_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                         const sdf_search_interval *intervals, const sdf_minimizer *r, size_t nr, int64_t len_r, int32_t init_len,
                         const int32_t *limit, size_t n_limit, sdf_search_roll_rec *out /* first[nq] */);

/* ---- search filter: uppercase and q-gram verdicts per pair of pool ranges (search_filter.hip) -----------------------------------
 * The reference's filter() (src/filter.cc; called at src/search.cc:337, 356 and 374: once per rolled interval whose jaccard is
 * at least 0, once per hit after extend) for many pairs in one call.  It reads nothing but the resident pool.  is_overlap
 * stands behind this section.
 *
 * The sequence s of a side is pool[off, off + len) as it lies, or -- SDF_FILTER_Q_RC / SDF_FILTER_R_RC -- its reverse
 * complement by rev_dna: s[i] = rev_dna(pool[off + len - 1 - i]).  off is the first byte of the range in pool order whatever the
 * strand, as for sdf_pool_fetch_ranges.  Characters are taken & 127 on either strand.
 *   up      the number of i with 'A' <= s[i] <= 'Z'.  rev_dna turns n and every unknown byte into 'N', so on the reverse strand
 *           up counts every byte that is not acgt -- a forward 'n' is not uppercase, a reversed one is: the one place where the
 *           strand changes a count.
 *   dist    with h(c) = 0, 1, 2, 3 for Aa, Cc, Gg, Tt and 0 for anything else, the q-gram at i >= 4 is h(s[i - 4]) .. h(s[i]),
 *           first character most significant, 10 bits; dist = the sum over the 1,024 grams of min(count in q, count in r).  A side
 *           shorter than 5 has no grams.
 *   minqg   with l = max(q_len, r_len):
 *             (int)(l * (1 - (max_error - max_edit_error) - 5 * max_edit_error) - (gap_frequency * l + 1) * 4)
 *           in double, in exactly this association, no fused multiply-add, truncated toward zero (beyond the int32 range -- which
 *           the reference's parameters never reach -- it takes the nearest end).
 *   flags   SDF_FILTER_UPPER_FAIL when q_up < min_uppercase or r_up < min_uppercase; else SDF_FILTER_QGRAM_FAIL when
 *           dist < minqg.  SDF_FILTER_SHORT when minqg < 10, where the reference asserts: the verdict is that of its NDEBUG build.
 * q_up, r_up, dist and minqg are filled whatever the verdict, so a record does not depend on who computed it.  A task that
 * carries SDF_FILTER_SKIP is not read: its record is zero with SDF_FILTER_SKIPPED.
 *
 * A task is of one of two classes, read off its lengths alone: both sides up to SDF_FILTER_WAVE_MAX_LEN characters -- one
 * wavefront, 16-bit counts --, or longer -- a workgroup of four wavefronts, 32-bit counts.  The answer does not depend on it.
 *
 * Host form.  Every check precedes the first launch, and a refused call launches nothing (sdf_last_launches() as it was) and
 * writes nothing:
 *   SDF_ERR_INVALID      a range outside sdf_pool_bytes(ctx), a negative len, params / tasks / out == NULL with n > 0, a
 *                        parameter that is not finite
 *   SDF_ERR_UNSUPPORTED  a flags bit other than the three above, reserved != 0 (task or parameters), n > 2^31 - 1
 * n == 0 is SDF_OK without a launch.  One launch, two when a task is of the long class, per 2^22 tasks (a grid has fewer than
 * 2^32 lanes: the call cuts a larger n into pieces itself).  Works on a view (sdf_pool_share) like
 * every reader of the pool; enqueued on the context's stream behind the pool's uploads, returns with everything filled. */
#define SDF_FILTER_Q_RC 0x1
#define SDF_FILTER_R_RC 0x2
#define SDF_FILTER_SKIP 0x4          /* task flag: answer a zero record that carries SKIPPED */
#define SDF_FILTER_WAVE_MAX_LEN 4096 /* a task with a longer side goes to a workgroup of four wavefronts */
typedef struct { int64_t q_off, r_off; int32_t q_len, r_len; uint32_t flags; int32_t reserved; /* 0 */ } sdf_filter_task; /* 32 bytes */
typedef struct { int32_t min_uppercase, reserved; double max_error, max_edit_error, gap_frequency; } sdf_filter_params;
#define SDF_FILTER_UPPER_FAIL 0x1    /* what the reference reports: "upper (q_up, r_up) < min" */
#define SDF_FILTER_QGRAM_FAIL 0x2    /* "q-grams dist < minqg"; set only when UPPER_FAIL is not */
#define SDF_FILTER_SHORT      0x4    /* minqg < 10: the reference's assert; verdict as with NDEBUG */
#define SDF_FILTER_SKIPPED    0x8
typedef struct { int32_t q_up, r_up, dist, minqg; uint32_t flags; } sdf_filter_rec; /* 20 bytes */
int sdf_search_filter(sdf_ctx *ctx, const sdf_filter_params *params, const sdf_filter_task *tasks, size_t n, sdf_filter_rec *out);
/* Device form: tasks and d_out (n records) in HBM, asynchronous on `stream` (NULL: the context's own, synchronised before
 * returning).  The parameters and n are checked as above; the tasks are not, but a task that does not lie in the pool, has a
 * negative length, carries an unknown flag or reserved != 0 answers a zero record with SDF_FILTER_SKIPPED and is not read.
 * any_rc == 0 with a task that carries a strand flag reads that side forward.  Two launches per 2^22 tasks, the second for the
 * long class (its workgroups leave at once on a task of the other: profiles/search_filter.txt has what that costs).  The pool's uploads as for sdf_stats_columns_pairs_device
 * (sdf_pool_sync() first). */
int sdf_search_filter_device(sdf_ctx *ctx, const sdf_filter_params *params, const sdf_filter_task *d_tasks, size_t n, int any_rc,
                             sdf_filter_rec *d_out, void *stream);
/* No context, no GPU: the same over pool[0, pool_bytes) in plain C++ on one thread.  Same checks and codes. */
int sdf_search_filter_host(const char *pool, size_t pool_bytes, const sdf_filter_params *params, const sdf_filter_task *tasks,
                           size_t n, sdf_filter_rec *out);
/* The tasks of the rolled intervals: out[t] for interval t of sdf_search_roll, t < first[nq] -- no compaction, out[t] stays
 * aligned with rolls[t].  q, windows, first and intervals as sdf_search_roll takes them, rolls as it writes them; the query
 * sequence is pool[q_off, q_off + len_q), the reference sequence pool[r_off, r_off + len_r), each read reverse-complemented when
 * its q_rc / r_rc is not 0 (the task then carries the strand flag).  Interval t of window i:
 *   query side      positions [q[i].loc, q[i].loc + init_len) of the query sequence
 *   reference side  allow_extend == 0: the roll's best, [ref_start, ref_end) (src/search.cc:374).  allow_extend != 0: where the
 *                   walk ENDED, not its best -- src/search.cc:337-338 passes ref_start and ref_end, and the quirk is kept --:
 *                   with e0 = min(start + init_len, len_r) and steps = max(0, min(end - start, len_r - e0)) of the interval,
 *                   [start + steps, e0 + steps).
 * Positions [a, b) of a sequence map to pool order as off = base + a, or on the reverse strand off = base + len_seq - b.
 * The task carries SDF_FILTER_SKIP (every other field zero) when the roll has jaccard < 0, SDF_ROLL_BADWINDOW, or SDF_ROLL_WIDE
 * on a record nobody completed (ref_end == 0), when the window is SHORT or NOLIMIT, or when a side does not lie inside its
 * sequence.
 *   SDF_ERR_INVALID      a null array with nq > 0 (intervals, rolls and out may be null when first[nq] == 0), init_len < 1,
 *                        len_q or len_r < 0, q_off or r_off < 0, first[] not ascending from 0
 *   SDF_ERR_UNSUPPORTED  init_len > 2^30, len_q or len_r or the number of intervals > 2^31 - 1 */
int sdf_search_filter_tasks_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                                 const sdf_search_interval *intervals, const sdf_search_roll_rec *rolls, int64_t len_q,
                                 int64_t len_r, int32_t init_len, int64_t q_off, int q_rc, int64_t r_off, int r_rc,
                                 int allow_extend, sdf_filter_task *out /* first[nq] */);
/* Device form: every array in HBM, the scalars checked, no host wait -- one lane per interval, behind sdf_search_roll_device on
 * one stream and in front of sdf_search_filter_device.  n_max as for sdf_search_roll_device, but the lanes at or beyond
 * d_first[nq] write a SKIP task (no roll record is read there), so that sdf_search_filter_device may take all n_max; nothing is
 * written at or behind d_out[n_max].  nq == 0 or n_max == 0 is SDF_OK without a launch. */
int sdf_search_filter_tasks_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                   const uint64_t *d_first, const sdf_search_interval *d_intervals,
                                   const sdf_search_roll_rec *d_rolls, size_t n_max, int64_t len_q, int64_t len_r, int32_t init_len,
                                   int64_t q_off, int q_rc, int64_t r_off, int r_rc, int allow_extend, sdf_filter_task *d_out,
                                   void *stream);

/* ---- search against the SDs already found, second query: is_overlap for every rolled interval (search_found.hip) ----------------
 * The found records, their prefixes and the bin index as stated behind the search seeding.  out[t] = 1 or 0 for interval t of sdf_search_roll, first[i] <= t < first[i + 1] for its
 * window i; interval t sees found[0, visible_iv[t]).  min_read_size is the reference's Globals::Search::MIN_READ_SIZE -- a
 * separate argument: initial_search passes the same number as init_len, but is_overlap reads the global.  With
 * pf_pos = q[i].loc, pf_end = pf_pos + init_len, pfp_pos = rolls[t].ref_start and pfp_end = rolls[t].ref_end:
 *   1. every visible, non-empty record with q_start <= pf_pos < q_end and r_start <= pfp_pos < r_end is looked at; sA, eA, sB,
 *      eB are its four fields;
 *   2. pf_pos >= sA && pf_end <= eA && pfp_pos >= sB && pfp_end <= eB: the answer is 1;
 *   3. else min(eA - sA, eB - sB) < min_read_size * 1.5 (in double, as the reference's): the next record;
 *   4. else eA - pf_pos >= min_read_size && eB - pfp_pos >= min_read_size: the answer is 1;
 *   5. no record answered 1: the answer is 0.
 * The verdict is computed from the roll record as given, whatever its flags; no field beyond those four is read.
 *   SDF_ERR_INVALID      a null array with nq > 0 (rolls, visible_iv and out may be null when first[nq] == 0; found with
 *                        nf == 0), init_len < 1, min_read_size < 0; checked forms: first[] not ascending from 0,
 *                        visible_iv[t] > nf
 *   SDF_ERR_UNSUPPORTED  init_len > 2^30, nq > 2^30 - 1, nf or the number of intervals > 2^31 - 1, more than 2^31 - 1 bin
 *                        entries
 * nq == 0 or no interval is SDF_OK without a launch. */
int sdf_search_overlap(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, const uint64_t *first, const sdf_search_roll_rec *rolls,
                       const sdf_search_found *found, size_t nf, const uint32_t *visible_iv /* first[nq] */, int32_t init_len,
                       int32_t min_read_size, uint32_t *out /* first[nq] */);
/* Device form: every array in HBM, the scalars checked, no host wait -- three launches for the index and one lane per interval,
 * behind sdf_search_filter_tasks_device on one stream and in front of sdf_search_filter_device.  n_max as for
 * sdf_search_roll_device: d_out and d_visible_iv have n_max entries, the lanes at or beyond d_first[nq] write 0 and read
 * neither a roll record nor a prefix; nothing is written at or behind d_out[n_max].  d_filter_tasks (or NULL): the n_max tasks
 * sdf_search_filter_tasks_device wrote; where the verdict is 1 the interval's task is replaced by the skip task
 * {0, 0, 0, 0, SDF_FILTER_SKIP, 0}, so that sdf_search_filter_device answers SDF_FILTER_SKIPPED and sdf_search_extend_device
 * SDF_EXTEND_SKIPPED for it -- the reference's INTERVAL_FAILED branch; no other task is touched.  found_entries_cap and
 * d_found_entries as above. */
int sdf_search_overlap_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const uint64_t *d_first,
                              const sdf_search_roll_rec *d_rolls, size_t n_max, const sdf_search_found *d_found, size_t nf,
                              size_t found_entries_cap, uint64_t *d_found_entries /* or NULL */, const uint32_t *d_visible_iv,
                              int32_t init_len, int32_t min_read_size, uint32_t *d_out, sdf_filter_task *d_filter_tasks /* or NULL */,
                              void *stream);
/* No context, no GPU: the same in plain C++, a linear pass over found[0, visible).  Same checks and codes. */
int sdf_search_overlap_host(const sdf_minimizer *q, size_t nq, const uint64_t *first, const sdf_search_roll_rec *rolls,
                            const sdf_search_found *found, size_t nf, const uint32_t *visible_iv /* first[nq] */, int32_t init_len,
                            int32_t min_read_size, uint32_t *out /* first[nq] */);

/* ---- search extend: every rolled interval grown to its hit (search_extend.hip) ---------------------------------------------------
 * The reference's extend() (src/search.cc:95-259) for EVERY interval of sdf_search_roll in one call, as the reference calls it
 * with an EMPTY tree (sdf_search_overlap_device turns an overlapped interval's task into a skip).  Inputs: q, windows, first, intervals, r (ascending loc), nr,
 * len_r, init_len, limit, n_limit as sdf_search_roll takes them; rolls[t] as it writes them; len_q; filter[t], the first
 * filter's verdicts (sdf_search_filter on the tasks with allow_extend != 0), or NULL; the parameters (the reference's defaults:
 * 0.30, 0.15, 1,048,576).
 *
 * Interval t of window i RUNS when rolls[t].jaccard >= 0, the record carries no SDF_ROLL_BADWINDOW and no SDF_ROLL_WIDE with
 * ref_end == 0, lo <= winnow_start <= winnow_end <= nr (lo: the first index with r[lo].loc >= start), and filter is NULL or
 * filter[t].flags has none of UPPER_FAIL | QGRAM_FAIL | SKIPPED.  Every other interval gets a zero record with
 * SDF_EXTEND_SKIPPED.
 *
 * Entry state: the roll's best_winnow, which its record does not carry -- the state is path-dependent (the roll's quirk 2).  It
 * is the state of the roll's walk (steps 1-5 there) at the FIRST evaluation of J, step 4 or a round of step 5, at which
 * ws >= rolls[t].winnow_start and we >= rolls[t].winnow_end (the walk's end when there is none): for a record the roll wrote,
 * the evaluation that last assigned `best` (ref_start alone does not tell step 4 from the round at s = start).  bits, B and I
 * stand as they are there;  query_size = windows[i].query_size, L = limit[query_size];  qws = i, qwe = i + n_members,
 * rws = rolls[t].winnow_start, rwe = rolls[t].winnow_end.
 *
 * The map, in the roll section's terms, B now a key or NONE.  below(B) / above(B): the largest stored key < B / the smallest
 * stored key > B.  Every comparison with B is false while B is NONE or query_size == 0.
 *   add(k, BIT)      bits[k] & BIT: false, nothing changes.  Else was = bits[k], bits[k] |= BIT; when k < B: I += (bits[k] == 3),
 *                    and when was == 0: I -= (bits[B] == 3), B = below(B).  True.
 *   remove(k, BIT)   bits[k] & BIT == 0: false.  Else, when k <= B: I -= (bits[k] == 3), and when bits[k] == BIT and above(B)
 *                    exists: B = above(B), I += (bits[B] == 3).  Then bits[k] &= ~BIT.  True.
 *   add_to_reference / remove_from_reference (record): nothing for status 2, else add / remove(k, 2) -- the roll's.
 *   add_to_query(record): its status does NOT matter.  add(k, 1) false: nothing more -- query_size, L and B stay.  Else
 *                    query_size += 1, L = limit[query_size];  B = the smallest stored key when B is NONE, else above(B) when
 *                    that exists;  I += (bits[B] == 3).
 *   remove_from_query(record): remove(k, 1) false: nothing more.  Else query_size -= 1 (not below 0), L = limit[query_size];  when B is not
 *                    NONE: I -= (bits[B] == 3), B = below(B), NONE when there is none.
 * bits[B] of a key that is not stored counts as 0.  Where above(B) does not exist the reference steps its boundary past the
 * last key (and reads it at once, or in the next call), and a remove of a key above every stored one reads lower_bound() ==
 * end(): the rules above make each a no-op at that point.  tests/golden/make_golden_search_extend.py guards the same spots and
 * keeps no case that reached one.
 *
 * The extension (src/search.cc:201-258).  With nq, nr the record counts:
 *   query_start = qws ? q[qws - 1].loc + 1 : 0,  query_end = qwe < nq ? q[qwe].loc : len_q;  ref_start, ref_end likewise.
 *   loop:  G = max_error - max_edit_error, all in double, this association, no fused multiply-add, correctly rounded division:
 *     max_match = same_genome ? min(max_sd_size, (int)((1.0 / G + .5) * |query_start - ref_start|)) : max_sd_size  (the
 *                 conversion takes the nearest int32 end beyond the range);
 *     aln_len = max(query_end - query_start, ref_end - ref_start), seq_len = their min;
 *     stop when aln_len > max_match;  stop when 100.0 * seq_len / aln_len < 100 * (1 - 2 * G);
 *     same_genome: overlap = query_end - ref_start; stop when overlap > 0 and
 *                 100.0 * overlap / (ref_end - ref_start) > 100 * max_error;
 *     try both_both, both_right, both_left in this order; the first that passes its precheck and leaves J >= 0 is kept and the
 *     loop goes on; one that leaves J < 0 is undone; stop when none is kept.
 *   prechecks    left: qws != 0 and rws != 0;  right: rwe < nr and qwe < nq;  both_both: both.
 *   do           left:  add_to_query(q[--qws]), query_start = qws ? q[qws - 1].loc + 1 : 0;  add_to_reference(r[--rws]),
 *                       ref_start likewise.   right: add_to_query(q[qwe++]), query_end = qwe < nq ? q[qwe].loc : len_q;
 *                       add_to_reference(r[rwe++]), ref_end likewise.   both_both: left, then right.
 *   undo         right: remove_from_reference(r[--rwe]), ref_end = r[rwe].loc;  remove_from_query(q[--qwe]),
 *                       query_end = q[qwe].loc.   left: ref_start = r[rws].loc + 1, remove_from_reference(r[rws++]);
 *                       query_start = q[qws].loc + 1, remove_from_query(q[qws++]).   both_both: right, then left.
 * THE UNDO IS THESE REMOVES, NOT A RESTORE OF A SAVED STATE: they are not the inverse of the do steps.  An add_to_query that
 * returned false is still undone by a remove_from_query that clears the bit and lowers query_size; a form that snapshots and
 * restores gives other hits.
 * out[t] = {query_start, query_end, ref_start, ref_end, J, qws, qwe, rws, rwe, flags}, aligned with rolls[t].
 *
 * SDF_EXTEND_MAX_GROW: the records by which either end of either side's winnow range may grow beyond its entry value in a
 * wavefront's LDS.  1,792 records are some 15 kb of a k = 12, w = 16 sequence (two records in 17 bases) per end, and
 * 1,024 + 3,072 + 4 * 1,792 keys of seven bytes are 77 KB: two wavefronts share a CU's 160 KB.  SDF_EXTEND_WIDE: a do step,
 * kept or undone, would take a range beyond that growth; or the replay does not fit: the roll record carries SDF_ROLL_WIDE,
 * n_members > SDF_SEARCH_MAX_MEMBERS, or winnow_end - lo > SDF_ROLL_MAX_SPAN.  The flag follows from the inputs and the walk
 * alone.  The device form flags such an interval and writes the rest of its record as zero; sdf_search_extend completes it with
 * the host form and keeps the flag.  SDF_EXTEND_NOLIMIT: an add_to_query needs limit[s] with s >= n_limit; the rest of the
 * record is zero, in every form.  The two together: the cap is looked at for every side of a step (both sides of both_both)
 * before the step's first add, and the device form ends there, so it writes WIDE alone whenever the growth comes first; the
 * host form walks on, and when a later add then needs the table beyond its end the completed record is zero with
 * WIDE | NOLIMIT.  WIDE is set by the same walk in every form; NOLIMIT without WIDE is the same in every form.  The device keeps a key in 32 bits as the roll does (hash < 2^30).
 * Refusals as for sdf_search_roll, and SDF_ERR_INVALID for len_q < 0, rolls or params == NULL with an interval, a parameter
 * that is not finite, max_error - max_edit_error <= 0;  SDF_ERR_UNSUPPORTED for len_q > 2^31 - 1, reserved != 0.  Every check
 * precedes the first launch.  nq == 0 or no interval is SDF_OK without a launch. */
#define SDF_EXTEND_SKIPPED 0x1
#define SDF_EXTEND_WIDE 0x2
#define SDF_EXTEND_NOLIMIT 0x4
#define SDF_EXTEND_MAX_GROW 1792
typedef struct { double max_error, max_edit_error; int32_t max_sd_size, same_genome; int32_t reserved[2]; /* 0 */ } sdf_extend_params;
typedef struct { int32_t query_start, query_end, ref_start, ref_end, jaccard; int32_t q_winnow_start, q_winnow_end, r_winnow_start,
                 r_winnow_end; uint32_t flags; } sdf_search_hit; /* 40 bytes */
int sdf_search_extend(sdf_ctx *ctx, const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                      const sdf_search_interval *intervals, const sdf_search_roll_rec *rolls, const sdf_filter_rec *filter /* or NULL */,
                      const sdf_minimizer *r, size_t nr, int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *limit,
                      size_t n_limit, const sdf_extend_params *params, sdf_search_hit *out /* first[nq] */);
/* Device form: every array in HBM, nothing checked beyond the scalars, no host wait, behind sdf_search_filter_device on one
 * stream: n_max wavefronts on `stream` (NULL: the context's own, synchronised before returning), those at or beyond
 * d_first[nq] leave at once.  Nothing is written at or behind d_out[n_max].  A window whose query_size is outside the table or
 * whose n_members is outside 1 .. nq - i answers SDF_EXTEND_SKIPPED.  n_max == 0 is SDF_OK without a launch. */
int sdf_search_extend_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                             const uint64_t *d_first, const sdf_search_interval *d_intervals, const sdf_search_roll_rec *d_rolls,
                             const sdf_filter_rec *d_filter /* or NULL */, size_t n_max, const sdf_minimizer *d_r, size_t nr,
                             int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *d_limit, size_t n_limit,
                             const sdf_extend_params *params, sdf_search_hit *d_out, void *stream);
/* No context, no GPU: the same in plain C++ with a std::map, every interval (WIDE ones flagged and completed). */
int sdf_search_extend_host(const sdf_minimizer *q, size_t nq, const sdf_search_window *windows, const uint64_t *first,
                           const sdf_search_interval *intervals, const sdf_search_roll_rec *rolls, const sdf_filter_rec *filter,
                           const sdf_minimizer *r, size_t nr, int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *limit,
                           size_t n_limit, const sdf_extend_params *params, sdf_search_hit *out /* first[nq] */);
/* The long form of the device form: it completes, in place in d_hits and on the same stream without a host wait, intervals that
 * sdf_search_extend_device flagged SDF_EXTEND_WIDE for their GROWTH.  Inputs as for sdf_search_extend_device; d_hits: what that
 * call wrote (n_max records).  Record t < min(d_first[nq], n_max) is a CANDIDATE when its flags are exactly SDF_EXTEND_WIDE, its
 * query_end is 0 (nobody completed it) and its replay fits a wavefront: the roll record carries no SDF_ROLL_WIDE, n_members <=
 * SDF_SEARCH_MAX_MEMBERS and winnow_end - lo <= SDF_ROLL_MAX_SPAN.  No byte of any other record changes -- SKIPPED, NOLIMIT,
 * completed ones, and those that are WIDE because of the replay.  The first n_long_max candidates in ascending t are TAKEN
 * (not in the order wavefronts arrive: which ones are taken follows from the inputs).  A taken candidate is walked exactly as
 * the section above states, with long_grow records per end where the short form allows SDF_EXTEND_MAX_GROW:
 *   the walk ends inside long_grow           the hit, flags = SDF_EXTEND_WIDE (the 1,792 rule set the flag; every form keeps it)
 *   an add_to_query needs limit[s], s >= n_limit   a zero record with SDF_EXTEND_WIDE | SDF_EXTEND_NOLIMIT
 *   a do step would pass long_grow (looked at for every side of a step before its first add)   unchanged: zero, WIDE
 * Every record is what sdf_search_extend_host writes for it, or untouched.  *d_left (device memory, or NULL) receives the
 * number of candidates that were not taken or not finished.
 * SDF_EXTEND_LONG_MAX_GROW: bits[] of a wavefront is one byte per key in LDS, 1,024 + 3,072 + 4 * 16,384 = 69,632 bytes, so that
 * two wavefronts share a CU's 160 KB as they do in the short form; 16,384 records are some 139 kb per end at k = 12, w = 16.
 * The keys' sort and the slots lie in a workspace of the context's, `batch` intervals at a time (0: 128), 32 bytes per entry
 * of a batch slot's 1,024 + 3,072 + 4 * long_grow plus the sort's scratch: batch is taken down to n_long_max, and up to 4,096.
 * The number of launches -- 3, and 6 per batch -- and the workspace follow from n_max, n_long_max, long_grow and batch, never
 * from the data.
 * Refusals as for sdf_search_extend_device (d_hits for d_out), and SDF_ERR_INVALID for long_grow <= SDF_EXTEND_MAX_GROW or
 * > SDF_EXTEND_LONG_MAX_GROW;  SDF_ERR_NOMEM when the workspace is more than the context's workspace budget or cannot be
 * allocated.  Every check precedes the first launch.  nq == 0, n_max == 0 or n_long_max == 0 is SDF_OK without a launch, and
 * *d_left is not written then.
 * sdf_search_extend runs this form (long_grow = SDF_EXTEND_LONG_MAX_GROW, n_long_max = its candidates) on the arrays it has
 * uploaded when the short form left candidates, and completes on the host only what is still WIDE with query_end == 0
 * afterwards; without a candidate it launches what it launched before. */
#define SDF_EXTEND_LONG_MAX_GROW 16384
int sdf_search_extend_long_device(sdf_ctx *ctx, const sdf_minimizer *d_q, size_t nq, const sdf_search_window *d_windows,
                                  const uint64_t *d_first, const sdf_search_interval *d_intervals, const sdf_search_roll_rec *d_rolls,
                                  const sdf_filter_rec *d_filter /* or NULL */, size_t n_max, const sdf_minimizer *d_r, size_t nr,
                                  int64_t len_q, int64_t len_r, int32_t init_len, const int32_t *d_limit, size_t n_limit,
                                  const sdf_extend_params *params, int32_t long_grow, size_t n_long_max, size_t batch /* 0: default */,
                                  sdf_search_hit *d_hits /* in and out */, uint64_t *d_left /* or NULL */, void *stream);
/* The filter task of every hit, for the reference's second filter() (src/search.cc:356): out[t] for hits[t], n of them.  The
 * query side is positions [query_start, query_end) of the query sequence, the reference side [ref_start, ref_end) of the
 * reference's; sequences, strands and pool offsets as for sdf_search_filter_tasks_*.  SDF_FILTER_SKIP (every other field zero)
 * for a hit that carries SKIPPED or NOLIMIT, or WIDE on a record nobody completed (query_end == 0), or whose sides do not lie
 * inside their sequences.  SDF_ERR_INVALID: hits or out == NULL with n > 0, a negative length or offset;
 * SDF_ERR_UNSUPPORTED: n, len_q or len_r > 2^31 - 1.  The device form: one lane per hit on `stream`, no host wait; d_count
 * (or NULL) points at the number of hits that were written -- d_first + nq behind sdf_search_extend_device --, and the lanes at
 * or beyond it write a SKIP task without reading a hit, so that sdf_search_filter_device may take all n. */
int sdf_search_hit_tasks_host(const sdf_search_hit *hits, size_t n, int64_t len_q, int64_t len_r, int64_t q_off, int q_rc,
                              int64_t r_off, int r_rc, sdf_filter_task *out);
int sdf_search_hit_tasks_device(sdf_ctx *ctx, const sdf_search_hit *d_hits, size_t n, const uint64_t *d_count, int64_t len_q,
                                int64_t len_r, int64_t q_off, int q_rc, int64_t r_off, int r_rc, sdf_filter_task *d_out, void *stream);

/* ---- search driver: a pair's hits in the reference's order (search_accept.hip, sdf_driver_api.hip) -------------------------------
 * initial_search (src/search_main.cc:41-82) over the stages above.  Three facts of the reference's text carry the design:
 *   1. The windows that run do not depend on the hits.  initial_search calls search() with init_len = MIN_READ_SIZE and
 *      allow_extend; every reported hit comes out of extend(), which first snaps the query range outward to minimizer boundaries
 *      and whose undo only restores them, so query_end - query_start >= init_len for every hit, min_len >= MIN_READ_SIZE, and
 *      next_to_attain = (int)(loc + (MIN_READ_SIZE * MAX_ERROR) / 2) after every window that is not skipped: the schedule is a
 *      greedy walk over q[].loc and q[].status.
 *   2. Only the tree couples windows, and it is read in the two places the found-record sections answer.  A record can change
 *      window j, at qs_j = q[j].loc, only if its q_end > qs_j: both queries need a visible record whose query interval contains a
 *      position in [qs_j, qs_j + init_len], and every record of an earlier window has q_start <= qs_j.
 *   3. Inside one window the tree enters only through is_overlap: intervals and rolls are fixed once the window's exclusions
 *      are known, filter and extend read no tree.  The order-dependent part is a replay of is_overlap against the hits of the
 *      window's own earlier intervals.
 * So many windows may run speculatively against the found list as it stood, and the ACCEPTANCE STEP below takes, in order,
 * every window that no newly kept record reaches.
 *
 * sdf_search_pair_host: the reference-order statement in plain C++, no context, no GPU.  The query sequence is
 * pool[q_range.off, + len), the reference's pool[r_range.off, + len), each reverse-complemented under SDF_MINIM_RC; minimizers
 * and index as the minimizer section states them (k, w, separate_lowercase), init_len = is_overlap's min_read_size =
 * params->min_read_size, MAX_ERROR = params->filter.max_error.  For window i over q[0, nq) in order, next = 0 at the start:
 *   skip       q[i].loc < next, or uppercase_seeds and q[i].status != 0.
 *   window     sdf_search_windows_found's window i with the whole found list visible; SHORT or NOLIMIT: no intervals, no hits.
 *   intervals  in order, attempted += 1, then: the roll's jaccard < 0: jaccard_failed += 1.  Else is_overlap (rules 1 to 5 of
 *              the sdf_search_overlap section) against the whole current list, the records of this window's earlier intervals
 *              included: interval_failed += 1.  Else the first filter (the task of sdf_search_filter_tasks_* with
 *              allow_extend != 0) fails: nothing.  Else extend; SDF_EXTEND_SKIPPED or SDF_EXTEND_NOLIMIT is no hit, a WIDE record
 *              is completed and is one.  Else the second filter (sdf_search_hit_tasks_*) fails: nothing.  Else the hit joins the
 *              window's list and {query_start, query_end, ref_start, ref_end} is appended to the found list.
 *   parse_hits hit h of the window's list is dropped when some OTHER hit p of it has h.ref_start >= p.ref_start, h.ref_end <=
 *              p.ref_end, h.query_start >= p.query_start and h.query_end <= p.query_end; two identical hits drop each other.
 *              The survivors are reported in list order.  A dropped hit stays in the found list.
 *   next       min_len = the minimum of len_q and the reported hits' query lengths; next = min_len >= min_read_size ?
 *              (int)(q[i].loc + (min_read_size * max_error) / 2) : q[i].loc, in double, this association, truncated.
 * out[0, *used) are the reported hits, `window` the index i; stats the three counters (rounds 0, the three window counts the
 * windows that were not skipped).  More than cap hits: SDF_ERR_CIGAR_OVERFLOW, *used the need, nothing written.
 *   SDF_ERR_INVALID      a null pointer (out may be null with cap == 0), a range with off < 0, len < 0 or outside the pool,
 *                        min_read_size < 1, same_genome with different ranges or a strand flag, a parameter that is not finite,
 *                        max_error - max_edit_error <= 0
 *   SDF_ERR_UNSUPPORTED  k outside 1..15, w outside 1..SDF_MINIM_MAX_W, a range flag other than SDF_MINIM_RC, limit[s] < 1 for
 *                        some s >= 1, n_limit > 2^31 - 1, min_read_size > 2^30, reserved != 0
 *
 * The acceptance step, sdf_search_accept*: ONE ROUND -- the ascending window indices act[0, na) that ran, and what the chain
 * wrote for them: windows, first, rolls, the is_overlap verdicts against the found list as it stood (`overlap`), the first
 * filter's records, the hits and the second filter's records, all indexed as the stages write them (n_max: the records the
 * per-interval arrays hold) -- against found[0, nf) and out[0, n_out).
 *   per window, in interval order   attempted += 1.  jaccard < 0: jaccard_failed += 1.  Else verdict != 0: interval_failed += 1.
 *              Else is_overlap with pf_pos = q[i].loc and the roll's range answers 1 against the records KEPT so far in this
 *              window: interval_failed += 1.  Else the interval is a candidate -- its first filter has none of UPPER_FAIL |
 *              QGRAM_FAIL | SKIPPED, its hit neither SKIPPED nor NOLIMIT, its second filter passed likewise --: it is kept.
 *              parse_hits over the kept hits as above.
 *   incomplete the device left a record for the host: window flags WIDE or FOUND_WIDE; a roll with SDF_ROLL_WIDE and
 *              ref_end == 0, or BADWINDOW; a hit with SDF_EXTEND_WIDE and query_end == 0; more than SDF_ACCEPT_MAX_KEPT kept
 *              hits; first[i + 1] > n_max (device form: act[j] >= nq or first[] descending too).
 *   frontier   reach_j: the maximum q_end over the records kept by the round's windows before act[j] (0: none).  The frontier
 *              is the first j with reach_j > q[act[j]].loc -- strictly: q_end == qs_j does not reach -- or act[j] incomplete; na
 *              when there is none.  The windows before it are ACCEPTED.
 *   append     in window order, then interval order: the kept records of accepted windows to found[nf ..], their survivors to
 *              out[n_out ..] as {window_base + i, query_start, query_end, ref_start, ref_end, jaccard}; the counters of accepted
 *              windows added up.  Nothing of a window at or behind the frontier is written anywhere.
 *   status     {frontier, flags, nf, n_out, need_found, need_out, attempted, jaccard_failed, interval_failed}: the new counts
 *              (need_* equal them), SDF_ACCEPT_INCOMPLETE when the frontier window is incomplete.  A capacity is short
 *              (need_found > found_cap or need_out > out_cap): SDF_ACCEPT_OVERFLOW alone, the needs, frontier 0, nf and n_out as
 *              given, the counters 0, and nothing is written: the round is not accepted.
 * SDF_ACCEPT_MAX_KEPT: a wavefront keeps a window's kept records in LDS, 16 bytes of coordinates, the interval's index and a
 * byte: 512 of them are 10.5 KB, so fifteen wavefronts share a CU's 160 KB and LDS does not bound the occupancy before the
 * wavefront slots do at one wavefront per workgroup.
 * The device form: every array of the round in HBM (the struct itself on the host), nothing checked beyond the scalars, no host
 * wait, on `stream` (NULL: the context's own, synchronised before returning): one wavefront per round window, one workgroup for
 * the frontier (prefix maximum, first-true, exclusive sums), one wavefront per round window for the append -- three launches, one
 * when na == 0.  Nothing is written at or behind d_found[found_cap] or d_out[out_cap].  sdf_search_accept takes host arrays,
 * runs the device form on copies and brings found[nf, status->nf), out[n_out, status->n_out) and the status back.  The host form
 * is the same rules in plain C++; the three agree byte for byte, the status included.
 *   SDF_ERR_INVALID      a null pointer where a count is not 0, init_len < 1, min_read_size < 0, nf > found_cap,
 *                        n_out > out_cap; checked forms: act[] not strictly ascending or >= nq, first[] not ascending from 0
 *   SDF_ERR_UNSUPPORTED  init_len > 2^30, nq > 2^30 - 1, na, n_max, found_cap or out_cap > 2^31 - 1, reserved != 0
 *
 * sdf_search_pair: the driver, over two ranges of the resident pool; out, *used and the three counters of stats equal what
 * sdf_search_pair_host writes for the same characters, byte for byte, for every round_windows.  Set-up: sdf_pool_minimizers of
 * both ranges and sdf_pool_minimizer_index of the reference's (host copies serve the schedule and the host step; the device
 * copies stay in HBM for every round), and the schedule by fact 1, one pass over q.  A round takes the next round_windows
 * scheduled windows (0: 64, not measured) and enqueues on the context's stream: sdf_search_windows_found_device on the slice of q
 * from the round's first window to the last member of its last one, every window seeing the whole list (the tail of first[]
 * behind the slice is filled, so that every later call takes all of q and the windows outside the slice have no intervals),
 * roll, filter tasks, overlap with the skip-task rewrite, filter, extend, extend-long (16 candidates a round, batches of 8),
 * hit tasks, the second filter, sdf_search_accept_device with act = the scheduled windows -- the windows of the slice that are
 * not scheduled run but are not in act and contribute nothing.  Then ONE wait for 80 bytes: the status, the bin entries the
 * index needed and the intervals the slice had; when the round added records, they are copied to the host's mirrors of found
 * and out behind a second wait.  After it the next round starts at the frontier.  SDF_ACCEPT_INCOMPLETE: the host runs the
 * frontier window by the per-window step of sdf_search_pair_host on characters fetched from the pool once, uploads its
 * records and goes on behind it; with debug_host_every = d it does the same for every d-th scheduled window.  A capacity that
 * was short -- bin entries, intervals (4,096 at the start) -- is doubled beyond the need and the round repeated (a round whose
 * first windows had their records is taken as far as they go); found and the round's out are sized for the round beforehand.
 * A round that accepts nothing, hands nothing to the host and raised no capacity is SDF_ERR_HIP, "internal error".  stats:
 * rounds, windows_run (round windows, repeats counted, and host windows), windows_scheduled, windows_host -- these alone may
 * differ between forms and round sizes.  Refusals as for sdf_search_pair_host, ranges against sdf_pool_bytes(ctx); every check
 * precedes the first launch.  Overflow of out as for sdf_pool_minimizers.  The host form scans the whole found list per
 * interval and keeps a window record per query minimizer: a statement to compare with, not to time at chromosome size.
 * The command line above it (FASTA reading, BED text, the -r coordinate flip of to_bed, -t translation) is `sedef search`,
 * host/search_cmd.cc; it calls the indexed form below.
 * The driver's own sizes: SDF_PAIR_ROUND_WINDOWS, the round of round_windows == 0; SDF_PAIR_INTERVALS_START and
 * SDF_PAIR_ENTRIES_START, the intervals a round's arrays and the bin entries its index hold at a call's start (a short one is
 * raised to twice the need); SDF_PAIR_LONG_MAX and SDF_PAIR_LONG_BATCH, the n_long_max and batch a round gives
 * sdf_search_extend_long_device -- a round's further long growths leave their windows to the host. */
#define SDF_PAIR_ROUND_WINDOWS 64
#define SDF_PAIR_INTERVALS_START 4096
#define SDF_PAIR_ENTRIES_START 4096
#define SDF_PAIR_LONG_MAX 16
#define SDF_PAIR_LONG_BATCH 8
#define SDF_ACCEPT_MAX_KEPT 512
#define SDF_ACCEPT_INCOMPLETE 0x1
#define SDF_ACCEPT_OVERFLOW 0x2
typedef struct { int32_t window, query_start, query_end, ref_start, ref_end, jaccard; } sdf_search_pair_hit; /* 24 bytes */
typedef struct {
  uint32_t frontier, flags;
  uint64_t nf, n_out, need_found, need_out;
  int64_t attempted, jaccard_failed, interval_failed;
} sdf_search_accept_status; /* 64 bytes */
typedef struct {
  const sdf_minimizer *q;
  size_t nq;
  const uint32_t *act;
  size_t na;
  const sdf_search_window *windows; /* nq */
  const uint64_t *first;            /* nq + 1 */
  size_t n_max;
  const sdf_search_roll_rec *rolls; /* n_max, as the four behind it */
  const uint32_t *overlap;
  const sdf_filter_rec *filter;
  const sdf_search_hit *hits;
  const sdf_filter_rec *hit_filter;
  int32_t init_len, min_read_size, window_base, reserved; /* 0 */
} sdf_search_accept_round;
int sdf_search_accept(sdf_ctx *ctx, const sdf_search_accept_round *round, sdf_search_found *found, size_t nf, size_t found_cap,
                      sdf_search_pair_hit *out, size_t n_out, size_t out_cap, sdf_search_accept_status *status);
int sdf_search_accept_device(sdf_ctx *ctx, const sdf_search_accept_round *round /* its arrays in HBM */, sdf_search_found *d_found,
                             size_t nf, size_t found_cap, sdf_search_pair_hit *d_out, size_t n_out, size_t out_cap,
                             sdf_search_accept_status *d_status, void *stream);
int sdf_search_accept_host(const sdf_search_accept_round *round, sdf_search_found *found, size_t nf, size_t found_cap,
                           sdf_search_pair_hit *out, size_t n_out, size_t out_cap, sdf_search_accept_status *status);
typedef struct {
  int32_t k, w, separate_lowercase, uppercase_seeds, min_read_size, same_genome;
  sdf_filter_params filter;
  sdf_extend_params extend;
  const int32_t *limit;
  size_t n_limit;
  size_t round_windows;    /* the driver's: 0 means a default */
  size_t debug_host_every; /* the driver's: 0 means off */
} sdf_search_pair_params;
typedef struct {
  int64_t attempted, jaccard_failed, interval_failed;
  int64_t rounds, windows_run, windows_scheduled, windows_host;
} sdf_search_pair_stats; /* 56 bytes */
int sdf_search_pair(sdf_ctx *ctx, const sdf_minim_range *q_range, const sdf_minim_range *r_range, const sdf_search_pair_params *params,
                    sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats);
int sdf_search_pair_host(const char *pool, size_t pool_bytes, const sdf_minim_range *q_range, const sdf_minim_range *r_range,
                         const sdf_search_pair_params *params, sdf_search_pair_hit *out, size_t cap, size_t *used,
                         sdf_search_pair_stats *stats);
/* sdf_search_pair_wide (and sdf_search_pair_indexed_wide, below): sdf_search_pair whose rounds seed with
 * sdf_search_windows_wide_device(n_wide_max) -- a window that is WIDE or FOUND_WIDE for the seeding kernel alone is finished on
 * the device and no longer ends the round for the host.  out, *used and the three counters equal sdf_search_pair_host's byte
 * for byte for every round_windows; rounds, windows_run and windows_host may differ, as between any two forms.  n_wide_max == 0
 * is sdf_search_pair itself; n_wide_max > 2^20: SDF_ERR_UNSUPPORTED before the first launch. */
int sdf_search_pair_wide(sdf_ctx *ctx, const sdf_minim_range *q_range, const sdf_minim_range *r_range,
                         const sdf_search_pair_params *params, sdf_search_pair_hit *out, size_t cap, size_t *used,
                         sdf_search_pair_stats *stats, size_t n_wide_max);

/* ---- the resident search index: a range's minimizers and index ONCE, for every pair that names the range ------------------
 * The reference's search_single builds one Index per (chromosome, strand) and reuses it for every pair
 * (src/search_main.cc:155-168); sdf_search_pair computes both ranges' minimizers and the reference's index in every call.
 * A handle holds, for one range of the resident pool (SDF_MINIM_RC honoured) and one (k, w, separate_lowercase): the
 * records of sdf_pool_minimizers in ascending loc and those of sdf_pool_minimizer_index with n_groups and threshold, each
 * computed once by those two calls as they are; their device copies in HBM buffers of the handle's own (not the context's
 * per-call dr_q / dr_r / dr_rs), and the host copies the driver's schedule and host step read.
 *   sdf_search_index_build   checks and refusals are those of the two calls it makes, before the first launch; *out is NULL
 *                            after a failure.  Returns after the copies have reached HBM.
 *   sdf_search_index_free    frees the device and host copies.  NULL is SDF_OK.  Handles are recognised by ADDRESS, in the
 *                            context's list of live ones: a pointer that is not in that list (another context's handle, one
 *                            already freed) is SDF_ERR_INVALID and is not read -- in every call that takes a handle.  That is
 *                            all an address can tell: once a later sdf_search_index_build has returned the same address, a
 *                            stale copy of the freed pointer names the NEW handle.  Using a handle after freeing it is the
 *                            caller's error, as with any freed pointer; the check catches it only until the address is reused.
 *   LIFETIME, the one rule   a handle belongs to the context that built it.  sdf_destroy(ctx) frees every handle of ctx that
 *                            is still live; after it those pointers are dead like ctx itself and must not be passed to any call,
 *                            sdf_search_index_free included.  Nothing leaks, and nothing is freed twice by a caller that frees
 *                            each handle at most once before the context goes.  sdf_device_bytes(ctx) counts the handles' buffers.
 *   the pool                 a handle names bases by pool offset.  Appending to the pool (sdf_pool_append_fasta, reset == 0)
 *                            keeps every handle valid, although the pool may move.  Replacing it -- sdf_pool_upload,
 *                            sdf_pool_append_fasta(reset != 0), an anchors call with a host seq_pool, sdf_pool_share on this
 *                            context, a view dropped -- makes the context's handles STALE: sdf_search_pair_indexed refuses them,
 *                            sdf_search_index_info reports stale = 1, and all that remains is to free them.  A context that views
 *                            another's pool builds handles of its own; the owner's are not its.
 *   sdf_search_index_info    the range, k, w, separate_lowercase, the threshold, the records of both lists, n_groups, stale, and
 *                            the device bytes the handle holds.  sdf_search_index_builds: the handles this context has built since
 *                            it was made; sdf_search_index_live: those not yet freed.
 * sdf_search_pair_indexed: the driver of sdf_search_pair on two handles; out, *used and the three counters equal what
 * sdf_search_pair writes for (q's range, r's range, params), byte for byte, for every round_windows.  The query side reads q's
 * loc-ordered list; the reference side r's loc-ordered list, r's index and r's threshold.  One handle may be the query of one
 * call and the reference of the next, and both sides of one call; a call writes nothing into a handle's arrays -- first[] and
 * the window records of a call (search_accept_tail_kernel, sdf_search_windows_found_device) lie in the context's per-call
 * buffers.  Before the first launch:
 *   SDF_ERR_INVALID      a null pointer (out may be null with cap == 0); q or r not a live handle of ctx; a stale handle;
 *                        params->k, w or separate_lowercase (as 0 / not 0) different from a handle's; same_genome with q != r
 *                        (same_genome names ONE handle, on the forward strand); then every refusal of sdf_search_pair on the
 *                        handles' ranges, with its code.
 * Calls on one context do not overlap, as for sdf_search_pair. */
typedef struct sdf_search_index sdf_search_index;
typedef struct {
  sdf_minim_range range;
  int32_t k, w, separate_lowercase;
  uint32_t threshold;
  uint64_t n_minimizers, n_sorted;
  uint32_t n_groups, stale;
  uint64_t device_bytes;
} sdf_search_index_desc; /* 64 bytes */
int sdf_search_index_build(sdf_ctx *ctx, const sdf_minim_range *range, int k, int w, int separate_lowercase, sdf_search_index **out);
int sdf_search_index_free(sdf_ctx *ctx, sdf_search_index *index);
int sdf_search_index_info(const sdf_ctx *ctx, const sdf_search_index *index, sdf_search_index_desc *info);
long long sdf_search_index_builds(const sdf_ctx *ctx);
size_t sdf_search_index_live(const sdf_ctx *ctx);
int sdf_search_pair_indexed(sdf_ctx *ctx, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                            sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats);
/* (sdf_search_pair_wide on two handles) */
int sdf_search_pair_indexed_wide(sdf_ctx *ctx, const sdf_search_index *q, const sdf_search_index *r, const sdf_search_pair_params *params,
                                 sdf_search_pair_hit *out, size_t cap, size_t *used, sdf_search_pair_stats *stats, size_t n_wide_max);

/* ---- several pairs in flight: lanes ------------------------------------------------------------------------------------------
 * The rounds of ONE pair cannot overlap -- each needs the found list the round before it left --, and a round is a few dozen
 * wavefronts behind about twenty launches and one wait.  The rounds of DIFFERENT pairs are independent (the reference makes a
 * fresh Tree per initial_search call and keeps one Index per chromosome and strand for all of them, src/search.cc), so a run
 * over many pairs keeps several of them in flight.
 *   sdf_search_lanes_open   n_lanes (1 .. SDF_SEARCH_LANES_MAX, else SDF_ERR_INVALID) child contexts of ctx on ctx's device, with
 *                           ctx's sdf_config.  A lane holds a VIEW of ctx's pool (sdf_pool_share), a stream of its own and its
 *                           own per-call buffers, reserved by need: it costs what its rounds reserve.  While lanes are open ctx's
 *                           pool is shared, and the rule of sdf_pool_share holds unchanged: ctx cannot grow or replace its pool
 *                           (SDF_ERR_INVALID, "pool is shared").  sdf_device_bytes(ctx) counts the lanes' buffers.  A lanes
 *                           object is recognised by ADDRESS in a list ctx keeps, as handles are.
 *   sdf_search_lanes_close  destroys the lanes and drops their views: appending to the pool works again, and ctx's handles stay
 *                           valid, as after any append.  NULL is SDF_OK; lanes that are not live lanes of ctx: SDF_ERR_INVALID.
 *                           sdf_destroy(ctx) closes the lanes that are still open.
 *   sdf_search_pairs_indexed  job j is sdf_search_pair_indexed_wide(jobs[j].q, jobs[j].r, params with same_genome and
 *                           extend.same_genome taken from jobs[j].same_genome, n_wide_max).  Its hits are out[first[j],
 *                           first[j + 1]), in job order, first[0] == 0 and *used == first[n_jobs]; stats[j] is that call's stats.
 *                           The hits and the counters attempted, jaccard_failed, interval_failed and windows_scheduled equal the
 *                           single-pair call's byte for byte, for every n_lanes, every round_windows and whatever order the lanes
 *                           took the jobs in.  The handles are ctx's: a lane reads them (their liveness and pool_epoch are
 *                           checked against ctx) and never builds, frees or writes one, so the same (q, r) may appear in several
 *                           jobs and one handle may serve several lanes at once.  One host thread per lane lives inside the
 *                           call and is joined before it returns; the jobs come off one shared queue, those with the most query
 *                           minimizers first; with n_jobs < n_lanes the spare lanes stay idle.  n_jobs == 0: SDF_OK, first[0] = 0.
 * Before the first launch, for ALL jobs -- nothing is written, the context stays usable --: SDF_ERR_INVALID for a null pointer (out
 * may be null with cap == 0; jobs and stats with n_jobs == 0), lanes that are not live lanes of ctx, a job with a null, freed,
 * foreign or stale handle, k, w or separate_lowercase different from a handle's, same_genome with q != r; then the refusals of
 * sdf_search_pair_indexed_wide on each job's ranges and on n_wide_max, with their codes.  sdf_last_error names the job.
 * SDF_ERR_CIGAR_OVERFLOW: the jobs' hits exceed cap; *used and all of first[] are right, out is unspecified, and a second call
 * with cap >= *used succeeds.  A job that fails in flight: jobs not yet started are not started (after a HIP error nothing more
 * is started on the device in the call), those running finish; the call returns the code of the failed job with the lowest
 * index, *used = 0, and sdf_last_error gives that lane's message behind the job's index.
 * Calls on one context do not overlap; a lanes object serves one call at a time. */
#define SDF_SEARCH_LANES_MAX 16
typedef struct sdf_search_lanes sdf_search_lanes;
typedef struct { const sdf_search_index *q, *r; int32_t same_genome, reserved; } sdf_search_pair_job; /* 24 bytes */
int sdf_search_lanes_open(sdf_ctx *ctx, int n_lanes, sdf_search_lanes **out);
int sdf_search_lanes_close(sdf_ctx *ctx, sdf_search_lanes *lanes);
int sdf_search_pairs_indexed(sdf_ctx *ctx, sdf_search_lanes *lanes, const sdf_search_pair_job *jobs, size_t n_jobs,
                             const sdf_search_pair_params *params, size_t n_wide_max, sdf_search_pair_hit *out, size_t cap,
                             size_t *used, uint64_t *first /* n_jobs + 1 */, sdf_search_pair_stats *stats /* n_jobs */);

/* ---- multi-GPU: the one exchange step of the path.  DP tasks are independent (the reference runs one
 * single-threaded process per bucket file and concatenates their output files, sedef.sh:187-190,218-221), so a batch is
 * sharded over the GPUs of a node with no data-path collective; after the DP an RCCL all-gatherv over xGMI gives every GPU
 * every shard's result records and CIGAR words.  One communicator per (process, device): either
 *   rank 0: sdf_comm_unique_id(id, 128) -> id handed to the other processes out of band -> every rank:
 *   sdf_comm_create(device, world, rank, id)                                   (one process per GPU), or
 *   sdf_comm_create_all(devices, n, comms)                                      (one process, a thread per GPU).
 * RCCL is dlopen'ed by the first of these calls. */
typedef struct sdf_comm sdf_comm;
int sdf_comm_unique_id(void *id, size_t bytes /* >= 128 */);
sdf_comm *sdf_comm_create(int device, int world, int rank, const void *id);
int sdf_comm_create_all(const int *devices, int n, sdf_comm **out);
void sdf_comm_destroy(sdf_comm *c);
int sdf_comm_world(const sdf_comm *c);
int sdf_comm_rank(const sdf_comm *c);
const char *sdf_comm_last_error(const sdf_comm *c);
/* All-gatherv of one batch's results: d_out[n_tasks] and d_cig[cig_used] are this rank's (HBM, what
 * sdf_extz2_batch_device left), d_all_out / d_all_cig receive every rank's back to back in rank order -- exactly
 * counts[2 r] records and counts[2 r + 1] CIGAR words from rank r (counts: host, 2 * world entries; cigar_off of a record
 * stays relative to its rank's words).  Two collectives whatever the world size: an all-gather of the counts and one
 * group of point-to-point transfers on the exact sizes.  Enqueued on `stream` (NULL: the communicator's own, synchronised
 * before returning); with a stream the call returns once the counts are on the host and the transfers are enqueued.
 * SDF_ERR_CIGAR_OVERFLOW: a capacity is too small ON ANY RANK (counts holds the sizes): the capacities travel with the
 * counts, so every rank returns this together and none is left waiting in a receive. */
int sdf_allgatherv_results(sdf_comm *c, const sdf_result *d_out, size_t n_tasks, const uint32_t *d_cig, size_t cig_used,
                           sdf_result *d_all_out, size_t all_out_cap, uint32_t *d_all_cig, size_t all_cig_cap,
                           uint64_t *counts, void *stream);

/* ---- `align bucket`: seed hits extended, sorted, merged and dealt into buckets (bucket_merge.hip) -------------------------------
 * What bucket_alignments_extern does between `sedef search` and `sedef align generate` (src/align_main.cc:38-198, merge() of
 * src/merge.cc:35-109), on records: a SEED HIT is a query range and a reference range of two chromosomes, both [start, end),
 * with the strand of its reference side in bit 0 of `flags` (the query side of a seed is always forward).  Chromosome ids are
 * the caller's numbering IN BYTE-WISE LEXICOGRAPHIC ORDER OF THE NAMES ("chr10" < "chr2"), so that every name comparison of
 * the reference is an integer comparison here.  Two small tables come with them:
 *   chr_group[n_chr]                       the translation group of each chromosome (`sedef translate`), in [0, n_groups)
 *   group_pair_order[n_groups * n_groups]  entry gq * n_groups + gr: the rank of the string "tmp_<gq>_<gr>.tmp" among all such
 *                                          strings -- the order the reference reads its temporary files in ("tmp_10_2" sorts
 *                                          before "tmp_2_1"); a permutation of [0, n_groups^2)
 * The steps, in the reference's arithmetic:
 *   1. Hit::extend (src/hit.cc:200-207): w = max(q_end - q_start, r_end - r_start); w = min(max_extend, (int)(extend_ratio * w))
 *      in fp64; starts = max(0, start - w), ends += w.
 *   2. The sides are ordered: when (q_chr, q_start, q_end) > (r_chr, r_start, r_end) ids and coordinates change sides; the
 *      strand bit stays where it is.  A hit is SELF when ids, starts and ends of its sides agree and the strand bit is clear;
 *      self hits are dropped.
 *   3. The hits are sorted by (group_pair_order of the two chromosomes' groups, strand, q_chr, r_chr, q_start, r_start) and swept
 *      in that order: a hit opens a new RUN when one of the first four changes or when the largest q_end of the run so far +
 *      merge_dist < its q_start; else it swallows every surviving hit W of its run that is not APART from it --
 *      W.q_end + merge_dist < q_start, W.r_end < r_start - merge_dist or W.r_start > r_end + merge_dist --, grows to the union
 *      and looks again until nothing more is swallowed.  A run's survivors leave in the order of (r_end, position in the sort).
 *   4. The deal: cls = (int)sqrt((double)(q_end - q_start) * (double)(r_end - r_start)) / 1000; every class goes round the nbins
 *      buckets on its own, starting where the class below it stopped (src/align_main.cc:147-175).
 * out[0 .. *n_out) holds the merged hits in the order the reference deals them, each with its bucket: bucket file b is the
 * hits with bucket == b in this order.  On seeds as `sedef search` prints them (no name, forward query) the result does not
 * depend on how hits of equal sort key are ordered, which is what lets the device sort them stably.
 * Before anything else, the same in all three forms (sdf_bucket_merge_device: what the host can see -- the first two, the last
 * five and the pointers; a record or table entry that fails the rest there is dropped and counted in d_n_out[1]):
 *   SDF_ERR_INVALID      n_chr > 2^19 or n_groups > 4096 or either < 1 with n > 0; an id or a group outside its range, a
 *                        group_pair_order entry outside [0, n_groups^2); start < 0 or start > end; a coordinate above
 *                        2^31 - 1 - max_extend - merge_dist (no int sum of the reference wraps); extend_ratio that is negative,
 *                        not a number, or with extend_ratio * max(len) >= 2^31; max_extend < 0; nbins < 1; merge_dist < 0;
 *                        out_cap < n; a null pointer with n > 0; a flags bit other than SDF_SEED_RC or pad != 0
 *   SDF_ERR_UNSUPPORTED  n > 2^30
 * n == 0 is SDF_OK with *n_out = 0 and no launch.
 *   sdf_bucket_merge_host    plain C++ with the reference's containers: no context, no device, no error text
 *   sdf_bucket_merge         host arrays in and out: uploads, the launches below, one wait
 *   sdf_bucket_merge_device  everything in HBM (the tables too) on the context's stream, no host wait inside and nothing read
 *                            back: d_n_out[0] = the number of records, d_n_out[1] = the records and table entries dropped as
 *                            said above (0 for a call the other forms would accept); d_out holds out_cap >= n records
 * The launches: bucket_prepare_kernel (steps 1-2 and the sort keys, a lane a seed), two stable radix sorts, a segmented
 * max-scan and a sum for the runs, bucket_sweep_kernel (a wavefront per run of two or more hits), one radix sort by
 * (run, r_end) for the order of step 3, one by class for step 4.  Buffers of the context that sdf_device_bytes() counts:
 * about 150 bytes a seed. */
#define SDF_SEED_RC 1u /* sdf_seed_hit::flags, sdf_bucket_hit::flags: the reference side is the reverse strand */
typedef struct { int32_t q_chr, q_start, q_end, r_chr, r_start, r_end; uint32_t flags; uint32_t pad; /* must be 0 */ } sdf_seed_hit;
typedef struct { int32_t q_chr, q_start, q_end, r_chr, r_start, r_end; uint32_t flags; int32_t bucket; } sdf_bucket_hit;
typedef struct { double extend_ratio; int32_t max_extend, merge_dist, nbins; } sdf_bucket_params;
int sdf_bucket_merge_host(const sdf_seed_hit *hits, size_t n, const int32_t *chr_group, size_t n_chr, const int32_t *group_pair_order,
                          size_t n_groups, const sdf_bucket_params *params, sdf_bucket_hit *out, size_t out_cap, size_t *n_out);
int sdf_bucket_merge(sdf_ctx *ctx, const sdf_seed_hit *hits, size_t n, const int32_t *chr_group, size_t n_chr,
                     const int32_t *group_pair_order, size_t n_groups, const sdf_bucket_params *params, sdf_bucket_hit *out,
                     size_t out_cap, size_t *n_out);
int sdf_bucket_merge_device(sdf_ctx *ctx, const sdf_seed_hit *d_hits /* HBM */, size_t n, const int32_t *d_chr_group, size_t n_chr,
                            const int32_t *d_group_pair_order, size_t n_groups, const sdf_bucket_params *params /* host */,
                            sdf_bucket_hit *d_out, size_t out_cap, uint64_t *d_n_out /* two words */);

/* ---- search hits to seed records (seed_records.hip): the seam between `sedef search` and `align bucket` --------------------------
 * The hits of sdf_search_pairs_indexed -- hits[first[j], first[j + 1]) are job j's -- become the sdf_seed_hit records that their
 * BED lines would give `align bucket` (Hit::from_bed of search_hit_bed, csrc/host/search_cmd.cc), without the text.  jobs[j] says
 * what the hits of job j do not: the ids of the query and the reference chromosome (the numbering of sdf_bucket_merge: byte order
 * of the names), the reference's length and, in bit 0 of `flags` (SDF_SEED_RC), whether the reference was searched on the reverse
 * strand.  Record t, of job j = the last job with first[j] <= t (jobs without hits repeat a value of first[] and are stepped over):
 *   q_chr = jobs[j].q_chr, q_start = query_start, q_end = query_end, r_chr = jobs[j].r_chr, pad = 0
 *   forward:  r_start = ref_start, r_end = ref_end, flags = 0
 *   reverse:  r_start = (int)(ref_len - ref_end + 1), r_end = (int)(ref_len - ref_start + 1), flags = SDF_SEED_RC
 *             (the low 32 bits of the difference, as the BED text has them: a flip may come out negative, and sdf_bucket_merge
 *             then refuses the record)
 * window and jaccard of a hit are not read.  Before anything else, the same in all three forms (sdf_seed_records_device: what
 * the host can see -- n, n_jobs and the pointers; a first[] or a job it cannot read is the caller's to have checked):
 *   SDF_ERR_UNSUPPORTED  n > 2^30; a job with reserved != 0 or a flags bit other than SDF_SEED_RC
 *   SDF_ERR_INVALID      a null pointer with n > 0; first[0] != 0, first[] decreasing somewhere, first[n_jobs] != n (so n > 0 with
 *                        n_jobs == 0)
 * n == 0 is SDF_OK with no launch (first and jobs are still checked where they are given).
 *   sdf_seed_records_host    plain C++: no context, no device, no error text
 *   sdf_seed_records         host arrays in and out: uploads, the launch, one wait
 *   sdf_seed_records_device  everything in HBM on the context's stream, no host wait inside and nothing read back, so that
 *                            sdf_bucket_merge_device can follow on the same stream with d_out as its d_hits
 * One launch, seed_records_kernel: a lane a hit, its job by a binary search of first[]. */
typedef struct { int32_t q_chr, r_chr; int64_t ref_len; uint32_t flags /* SDF_SEED_RC */, reserved /* must be 0 */; } sdf_seed_job; /* 24 bytes */
int sdf_seed_records_host(const sdf_search_pair_hit *hits, size_t n, const uint64_t *first /* n_jobs + 1 */, const sdf_seed_job *jobs,
                          size_t n_jobs, sdf_seed_hit *out /* n */);
int sdf_seed_records(sdf_ctx *ctx, const sdf_search_pair_hit *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs,
                     size_t n_jobs, sdf_seed_hit *out);
int sdf_seed_records_device(sdf_ctx *ctx, const sdf_search_pair_hit *d_hits /* HBM */, size_t n, const uint64_t *d_first,
                            const sdf_seed_job *d_jobs, size_t n_jobs, sdf_seed_hit *d_out);
/* The chain `sedef seeds` runs, from host arrays: hits, first[] and the job table go up in one piece with the two tables of the
 * merge, sdf_seed_records_device and sdf_bucket_merge_device follow each other on the context's stream, then the two words of
 * d_n_out come back and, behind them, the merged records.  Refusals: those of sdf_seed_records, then those sdf_bucket_merge_device
 * makes; a null n_dropped is SDF_ERR_INVALID.  *n_dropped = d_n_out[1]: when it is not 0 -- a flipped coordinate below 0 or beyond
 * what the merge takes, a table entry out of range -- the call is SDF_OK with *n_out = 0 and nothing in out, and the caller
 * buckets these hits another way.  Buffers of the context that sdf_device_bytes() counts. */
int sdf_seeds_bucket_merge(sdf_ctx *ctx, const sdf_search_pair_hit *hits, size_t n, const uint64_t *first, const sdf_seed_job *jobs,
                           size_t n_jobs, const int32_t *chr_group, size_t n_chr, const int32_t *group_pair_order, size_t n_groups,
                           const sdf_bucket_params *params, sdf_bucket_hit *out, size_t out_cap, size_t *n_out, size_t *n_dropped);

/* ---- pair recall: which records of a gold standard a set of found pairs hits, and how much of them (pair_recall.hip) ----------
 * The per-pair comparison `sedef stats recall` prints (the reference's scratch/check-overlap.py over `bedtools pairtopair -type
 * both`; bedtools is no part of this build, so THIS is the project's statement of that join).  A RECORD of either set is two ENDS,
 * bases [start1, end1) of chromosome chr1 and [start2, end2) of chr2; bit 0 of `flags` is the strand of end 1, bit 1 that of
 * end 2 (set: reverse).  Chromosome ids are any numbering the two sets share.
 *   Two ends MEET when they lie on the same chromosome id, min(end) - max(start) >= 1 (ends that touch do not meet, an empty
 *   end meets nothing) and their strand bits are equal; the call flag SDF_RECALL_IGNORE_STRAND drops the last clause.
 *   A found record f HITS a gold record g DIRECTLY when g.1 meets f.1 and g.2 meets f.2, CROSSWISE when g.1 meets f.2 and g.2
 *   meets f.1; a record that does both is one hit.
 * Per gold record g, out[g] holds
 *   n_hits       the found records that hit g, each once
 *   cov1, cov2   the bases of g's end 1 / end 2 inside the union of the hitting records' matching ends, clipped to that end of
 *                g: a direct hit gives f.1 to end 1 and f.2 to end 2, a crosswise hit f.2 to end 1 and f.1 to end 2, a record
 *                that hits both ways gives both
 *   flags        SDF_RECALL_WIDE: the direct and crosswise hits of g together are more than SDF_RECALL_CAP (a property of the
 *                inputs, the same in every form).  sdf_pair_recall_host and sdf_pair_recall answer such a record in full;
 *                sdf_pair_recall_device answers its n_hits, leaves cov1 = cov2 = 0 and leaves the rest to its caller.
 * Before anything else, in sdf_pair_recall_host and sdf_pair_recall, the first failing record's refusal (gold first):
 *   SDF_ERR_INVALID      start > end, a start below 0, a chromosome id below 0, reserved != 0, a flags bit above bit 1; a null
 *                        pointer with a count above 0
 *   SDF_ERR_UNSUPPORTED  a call flag other than SDF_RECALL_IGNORE_STRAND; more than 2^30 gold or 2^29 found records
 * sdf_pair_recall_device makes the refusals the host can see (pointers, counts, call flags); a FOUND record that fails the rest
 * there hits nothing and is counted in d_status[0], a GOLD record that fails it is answered {0, 0, 0, SDF_RECALL_BAD} and counted
 * in d_status[1]; both words are 0 for a call the other forms accept.  With n_gold == 0 nothing is launched and both are 0.
 *   sdf_pair_recall_host    plain C++: no context, no device, no error text
 *   sdf_pair_recall         host arrays in and out: uploads, the launches, one wait, the WIDE records completed on the host
 *   sdf_pair_recall_device  everything in HBM on the context's stream; nothing is read back and nothing waited for
 * The launches: recall_entries_kernel (a lane a found record: a sort key (chromosome, start) per end, the longest end), one
 * radix sort, recall_kernel (a wavefront a gold record).  Buffers of the context that sdf_device_bytes() counts: 48 bytes a
 * found record and the sort's scratch. */
#define SDF_RECALL_IGNORE_STRAND 1u /* call flag */
#define SDF_RECALL_WIDE 1u          /* sdf_pair_recall_rec::flags */
#define SDF_RECALL_BAD 2u           /* sdf_pair_recall_rec::flags, sdf_pair_recall_device only */
#define SDF_RECALL_CAP 1024         /* clipped intervals per end that recall_kernel keeps in LDS */
typedef struct { int32_t chr1, start1, end1, chr2, start2, end2; uint32_t flags; uint32_t reserved; /* must be 0 */ } sdf_pair_rec;
typedef struct { uint32_t n_hits; int32_t cov1, cov2; uint32_t flags; } sdf_pair_recall_rec;
int sdf_pair_recall_host(const sdf_pair_rec *gold, size_t n_gold, const sdf_pair_rec *found, size_t n_found, uint32_t flags,
                         sdf_pair_recall_rec *out /* n_gold */);
int sdf_pair_recall(sdf_ctx *ctx, const sdf_pair_rec *gold, size_t n_gold, const sdf_pair_rec *found, size_t n_found, uint32_t flags,
                    sdf_pair_recall_rec *out /* n_gold */);
int sdf_pair_recall_device(sdf_ctx *ctx, const sdf_pair_rec *d_gold /* HBM */, size_t n_gold, const sdf_pair_rec *d_found, size_t n_found,
                           uint32_t flags, sdf_pair_recall_rec *d_out /* n_gold */, uint64_t *d_status /* two words */);

/* ---- line order: text lines by eight keys and, inside equal keys, by their bytes; duplicates flagged (line_order.hip) ---------
 * What `sort -k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n | uniq` (LC_ALL=C; sedef.sh:218-229) does with lines the
 * caller has parsed: `sedef report` is the command over it.  The LINES lie in one byte pool, line i in [off, off + len) -- without
 * its newline, len 0 is a line --, `off` a multiple of 16 (what lies between a line's end and the next line's start is never
 * compared, and nothing behind pool_bytes is read).  key[0 .. 7] are eight ASCENDING unsigned keys, most significant first: the
 * caller has turned the eight sort fields, in the order k1 k9 k10 k4 k2 k3 k5 k6, into ranks or values such that a smaller key
 * sorts in front (the reversed fields' ranks already reversed).
 *   The order: by key[0], then key[1], ... key[7]; lines whose eight keys are equal (a RUN) by memcmp over the shorter length,
 *   the shorter line first when one is a prefix of the other; identical lines in the order of their indices.
 * order[p] is the index of the line at place p.  flags[p] holds
 *   SDF_LINE_DUP   the line at place p is byte for byte the line at place p - 1 (what `uniq` drops)
 *   SDF_LINE_WIDE  place p lies in a run of more than SDF_LINE_RUN lines (a property of the inputs, the same in every form).
 *                  sdf_line_order_host and sdf_line_order answer such a run in full; sdf_line_order_device leaves its places in
 *                  index order without SDF_LINE_DUP and leaves the rest to its caller.
 * *n_kept counts the places without SDF_LINE_DUP.
 * Refusals of sdf_line_order_host and sdf_line_order, before anything else:
 *   SDF_ERR_INVALID      a line whose off is no multiple of 16, whose reserved is not 0 or whose range runs past pool_bytes (the
 *                        first such line's); a null pointer with a count above 0; n_kept missing
 *   SDF_ERR_UNSUPPORTED  more than 2^30 lines or a pool of 2^40 bytes or more
 * sdf_line_order_device makes the refusals the host can see (pointers, counts); a line that fails the rest there is ordered by
 * its keys as a line of no bytes and counted in d_counts[2], which is 0 for a call the other forms accept.  d_counts: three
 * words -- [0] the places without SDF_LINE_DUP (every place of a WIDE run counts), [1] the WIDE runs, [2] the lines refused.
 * With n == 0 nothing is launched but the clearing of d_counts.
 *   sdf_line_order_host    plain C++: no context, no device, no error text
 *   sdf_line_order         host arrays in and out: uploads, the launches, one wait, the WIDE runs completed on the host
 *   sdf_line_order_device  everything in HBM on `stream` (NULL: the context's stream); nothing is read back, nothing waited for
 * The launches: four times line_keys_kernel and a radix sort (least significant pair of keys first, stable), line_heads_kernel
 * (where a run starts, the runs of two lines and more listed), line_tie_kernel (a wavefront a listed run).  Buffers of the
 * context that sdf_device_bytes() counts: about 27 bytes a line and the sort's scratch, and in sdf_line_order the pool and records. */
#define SDF_LINE_DUP 1u  /* flags[p] */
#define SDF_LINE_WIDE 2u /* flags[p] */
#define SDF_LINE_RUN 64  /* lines of equal keys that line_tie_kernel orders */
typedef struct { uint64_t off; uint32_t len; uint32_t reserved; /* must be 0 */ uint32_t key[8]; } sdf_line_rec; /* 48 bytes */
int sdf_line_order_host(const uint8_t *pool, size_t pool_bytes, const sdf_line_rec *lines, size_t n, uint32_t *order /* n */,
                        uint32_t *flags /* n */, size_t *n_kept);
int sdf_line_order(sdf_ctx *ctx, const uint8_t *pool, size_t pool_bytes, const sdf_line_rec *lines, size_t n, uint32_t *order,
                   uint32_t *flags, size_t *n_kept);
/* The parse in front of it, on the host: `text` holds lines that end in '\n' (a last line without one counts, an empty text has
 * none).  Line i goes to pool[lines[i].off ...), each start a multiple of 16, and lines[i].key[] become the eight keys of
 *   sort -k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n     under LC_ALL=C, GNU sort's rules taken literally:
 *   fields    no -t: a field ends where a non-blank (not ' ', '\t') is followed by a blank, and KEEPS its leading blanks; so two
 *             tabs in a row do not make an empty field -- a line of `align generate` whose name column is empty has one field
 *             fewer, and its "field 9" is the second strand.  A field the line does not have is empty.
 *   V (1, 4)  version order (this file's restatement of the coreutils manual's "version sort": runs of non-digits by the order
 *             '~' < end < letters < everything else by byte value, runs of digits by value, a file suffix
 *             (\.[A-Za-z~][A-Za-z0-9~]*)*$ set aside unless the rest is equal, a leading '.' first, equal strings by strcmp):
 *             key = the rank among the call's distinct values
 *   r (9, 10) byte strings, the shorter first when one is a prefix: key = the REVERSED rank among the distinct values
 *   n         the number in front after blanks -- [-]digits[.digits], anything else counts as 0 --: key = its value
 * *plain = 0 when some n field has a sign or a decimal point in front, more than ten digits or a value of 2^32 or more: the
 * four n keys are then ranks among the distinct values by numeric comparison, which orders the same on every form, and the
 * caller keeps to the host form by convention (`sedef report` says so on stderr).  pool == NULL or lines == NULL: only
 * *pool_bytes and *n, the sizes a second call needs.  SDF_ERR_INVALID: a capacity too small, text missing with text_bytes > 0,
 * a size pointer missing; SDF_ERR_UNSUPPORTED: more than 2^30 lines, a line of 2^32 bytes or more. */
int sdf_line_records(const uint8_t *text, size_t text_bytes, uint8_t *pool, size_t pool_cap, size_t *pool_bytes, sdf_line_rec *lines,
                     size_t lines_cap, size_t *n, int *plain);
int sdf_line_order_device(sdf_ctx *ctx, const uint8_t *d_pool /* HBM */, size_t pool_bytes, const sdf_line_rec *d_lines, size_t n,
                          uint32_t *d_order /* n */, uint32_t *d_flags /* n */, uint32_t *d_counts /* three words */, void *stream /* a hipStream_t */);

/* ---- one-task drop-in: same contract as ksw_extz2_sse (extern/ksw2.h:50).  `km` is ignored
 * like in the reference build (no HAVE_KALLOC).  Uses a process-wide context on device 0 (or
 * the device named by SDF_DEVICE).  On a fatal error prints to stderr and exits with 120, the
 * reference's own failure mode (extern/ksw2.h:106). */
void sdf_ksw_extz2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target,
                   int8_t m, const int8_t *mat, int8_t q, int8_t e, int w, int zdrop, int flag,
                   sdf_ksw_extz_t *ez);

#ifdef __cplusplus
}
#endif
#endif

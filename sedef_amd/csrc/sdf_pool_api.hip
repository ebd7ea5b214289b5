// The C ABI, resident sequences (include/sedef_hip.h; seq_pack.hip): the pool itself and what reads ranges of it back.
#include <hip/hip_runtime.h>

#include "sdf_entry.h"
#include "stripe_sync.h"

using namespace sdf;

extern "C" char *sdf_pool_host(sdf_ctx *ctx, size_t bytes) {
  if (!ctx) return nullptr;
  ctx->err.clear();
  const auto t0 = std::chrono::steady_clock::now();
  const size_t had = ctx->host_chars.cap;
  const bool plain = ctx->cfg.pin_register < 2;  // (sdf_config: the pool crosses PCIe every super-batch -- see pin_register)
  if (hipSetDevice(ctx->device) != hipSuccess ||
      (plain ? ctx->host_chars.reserve_exact(std::max<size_t>(bytes, 64)) : ctx->host_chars.reserve_huge(std::max<size_t>(bytes, 64))) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "cannot pin the character pool's staging";
    return nullptr;
  }
  // (its place in HBM with it: a first upload of 180 MB waited 8 ms for this -- but only while nothing is resident: a grown
  // buffer starts empty, and the records sdf_pool_append_fasta left must stay where they are)
  // (... and a pool that is shared, either way, is not touched at all: sdf_pool_share)
  if (!ctx->pool_bytes && !ctx->an_pool.borrowed && ctx->views.empty()) (void)ctx->an_pool.reserve(bytes + 64);
  if (ctx->cfg.debug_timing && ctx->host_chars.cap != had)
    fprintf(stderr, "[sdf_pool_host %zu MiB %s in %.1f ms]\n", ctx->host_chars.cap >> 20, ctx->host_chars.registered ? "registered huge pages" : "hipHostMalloc",
            ms_since(t0));
  return (char *)ctx->host_chars.p;
}

extern "C" int sdf_pool_upload(sdf_ctx *ctx, const char *chars, size_t bytes) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!chars && bytes) {  // (before anything changes: a view stays a view)
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  if (pool_writable(ctx) != SDF_OK) return SDF_ERR_INVALID;  // (an owner with views keeps its pool as it is)
  ctx->pool_bytes = 0;
  ctx->pool_epoch += 1;
  SDF_HIP(hipSetDevice(ctx->device));
  ctx->an_pool.new_call();
  SDF_HIP(ctx->an_pool.reserve(bytes + 64));
  if (bytes) SDF_HIP(hipMemcpyAsync(ctx->an_pool.p, chars, bytes, hipMemcpyHostToDevice, ctx->stream));
  ctx->pool_bytes = bytes;
  return SDF_OK;
}

extern "C" size_t sdf_pool_bytes(const sdf_ctx *ctx) { return ctx ? ctx->pool_bytes : 0; }

// The context's stream drained: every upload enqueued so far has left its host buffer (include/sedef_hip.h)
extern "C" int sdf_pool_sync(sdf_ctx *ctx) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  SDF_HIP(hipSetDevice(ctx->device));
  SDF_HIP(hipStreamSynchronize(ctx->stream));
  return SDF_OK;
}

// A FASTA record's sequence lines -> its bases behind the ones resident (include/sedef_hip.h; seq_pack.hip: fasta_gather_kernel).
// The lines cross PCIe as they are, in pieces of whole lines through one scratch buffer (everything is enqueued on the context's
// stream, so a piece's upload waits for the gather of the piece before it), and the device drops the line ends.
extern "C" int sdf_pool_append_fasta(sdf_ctx *ctx, const char *bytes, size_t nbytes, int64_t n_bases, int32_t line_bases,
                                     int32_t line_bytes, int reset, int64_t *base_off) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  auto invalid = [&](const char *why) {
    ctx->err = std::string("sdf_pool_append_fasta: ") + why;
    return SDF_ERR_INVALID;
  };
  if (!base_off || n_bases < 0 || (!bytes && nbytes)) return invalid("invalid arguments");
  // line_bases bases, then line_bytes - line_bases line-end bytes; a record of one line may come without a line end at all
  if (line_bases < 1 || line_bytes < line_bases) return invalid("a line holds at least one base and line_bytes >= line_bases");
  const size_t gap = (size_t)(line_bytes - line_bases);
  if (gap == 0 && n_bases > line_bases) return invalid("lines without line ends (line_bytes == line_bases) in a record of several lines");
  // n_bases bases and the line ends between them, with or without the last line's own
  const size_t least = (size_t)n_bases + (n_bases ? (size_t)((n_bases - 1) / line_bases) * gap : 0);
  if (nbytes < least || nbytes > least + gap) return invalid("nbytes does not fit n_bases bases in lines of this geometry");
  if (pool_writable(ctx, /*keep_view=*/reset == 0) != SDF_OK) return SDF_ERR_INVALID;
  const size_t at = reset ? 0 : ctx->pool_bytes, need = at + (size_t)n_bases;
  if (reset) ctx->pool_epoch += 1;
  SDF_HIP(hipSetDevice(ctx->device));
  // pieces of whole lines, 64 MiB or so each (the gather's indices within a piece are 32-bit)
  const size_t piece_lines = std::max<size_t>(1, ((size_t)64 << 20) / (size_t)line_bytes);
  const size_t piece_raw = std::min(nbytes, piece_lines * (size_t)line_bytes);
  // Growth has to fit beside what is resident (the pool moves: old and new buffer live side by side for the copy).  With room
  // to spare the pool grows with DevBuf's headroom, so that a genome's records do not move it once each; without, to the byte.
  const bool grow_pool = need + 64 > ctx->an_pool.cap, grow_raw = piece_raw + 64 > ctx->fa_raw.cap;
  bool headroom = false;
  if (grow_pool || grow_raw) {
    size_t free_b = 0, total_b = 0;
    SDF_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t exact = (grow_pool ? need + 64 : 0) + (grow_raw ? piece_raw + 64 : 0);
    // (exact < need: the sum wrapped -- only where the pool itself grows; a record that fits the pool's headroom but needs a
    // larger scratch buffer asks for piece_raw + 64 bytes, which may well be fewer than `need`)
    if (exact > free_b || (grow_pool && exact < need)) return invalid("the record does not fit the device's free memory beside the resident pool");
    headroom = grow_pool && exact + std::min<size_t>((need + 64) / 2, (size_t)8 << 30) + ((size_t)64 << 20) <= free_b;
  }
  for_each_device_buffer(ctx, [](DevBuf &b) { b.new_call(); }, BufGroup::Pool);
  if (grow_pool) {  // (the bases resident move to the larger buffer; the outgrown one is retired, not freed: DevBuf)
    const void *old = ctx->an_pool.p;
    ctx->pool_bytes = 0;  // (nothing is resident until the move has been enqueued: a failure below leaves an empty pool)
    const hipError_t e = headroom ? ctx->an_pool.reserve(need + 64) : ctx->an_pool.reserve_exact(need + 64);
    if (e != hipSuccess || (at && std::find(ctx->an_pool.retired.begin(), ctx->an_pool.retired.end(), old) == ctx->an_pool.retired.end())) {
      (void)hipGetLastError();
      ctx->err = "sdf_pool_append_fasta: out of device memory while growing the pool (the pool is empty now)";
      ctx->pool_epoch += 1;
      return SDF_ERR_NOMEM;
    }
    if (at) SDF_HIP(hipMemcpyAsync(ctx->an_pool.p, old, at, hipMemcpyDeviceToDevice, ctx->stream));
  }
  ctx->pool_bytes = at;
  SDF_HIP(ctx->fa_raw.reserve_exact(piece_raw + 64));
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t b0 = 0, x0 = 0; x0 < (size_t)n_bases; b0 += piece_raw, x0 += piece_lines * (size_t)line_bases) {
    const size_t nb = std::min(piece_raw, nbytes - b0), nx = std::min(piece_lines * (size_t)line_bases, (size_t)n_bases - x0);
    SDF_HIP(hipMemcpyAsync(ctx->fa_raw.p, bytes + b0, nb, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sdf::fasta_gather_kernel, dim3((unsigned)((nx / 16 + 2 + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const char *)ctx->fa_raw.p, (char *)ctx->an_pool.p + at + x0, (uint32_t)nx, (uint32_t)line_bases, (uint32_t)gap);
  }
  SDF_HIP(hipGetLastError());
  if (ctx->cfg.debug_timing) {
    SDF_HIP(hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "[sdf_pool_append_fasta %zu bytes -> %lld bases at %zu] %.2f ms\n", nbytes, (long long)n_bases, at, ms_since(t0));
  }
  ctx->pool_bytes = need;
  *base_off = (int64_t)at;
  return SDF_OK;
}

// Character classes of ranges of the resident pool (include/sedef_hip.h; seq_pack.hip: pool_classes_kernel)
extern "C" int sdf_pool_range_classes(sdf_ctx *ctx, const sdf_pool_range *ranges, size_t n, sdf_range_classes *out) {
  using sdf::ClassRange;
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) return SDF_OK;
  if (!ranges || !out || n > 0x3fffffffu) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  SDF_HIP(hipSetDevice(ctx->device));
  // the device's records in the pinned staging, the counts behind them
  SDF_HIP(ctx->host_cls.reserve(n * (sizeof(ClassRange) + sizeof(sdf_range_classes))));
  ClassRange *recs = (ClassRange *)ctx->host_cls.p;
  sdf_range_classes *back = (sdf_range_classes *)(recs + n);
  const size_t pool_bytes = ctx->pool_bytes;
  long long n_seg = 0;
  for (size_t i = 0; i < n; ++i) {
    const sdf_pool_range &r = ranges[i];
    if (r.reserved != 0) return refuse(ctx, SDF_ERR_UNSUPPORTED, "sdf_pool_range_classes: reserved must be 0");
    if (!in_range(r.off, r.len, pool_bytes)) return refuse(ctx, SDF_ERR_INVALID, "sdf_pool_range_classes: range outside the resident pool");
    recs[i] = ClassRange{r.off, r.len, (int32_t)n_seg};
    n_seg += (r.len + sdf::kClassSegBytes - 1) / sdf::kClassSegBytes;
    if (n_seg > 0x7fffff00ll) {
      ctx->err = "sdf_pool_range_classes: more than 2^31 segments in one call";
      return SDF_ERR_UNSUPPORTED;
    }
  }
  if (n_seg == 0) {
    memset(out, 0, n * sizeof(sdf_range_classes));
    return SDF_OK;
  }
  // (the kernel reads aligned slots: those of the first range start at the base)
  if (!pool_base_aligned(ctx)) return refuse(ctx, SDF_ERR_INVALID, "sdf_pool_range_classes: the pool's base is not 16-byte aligned");
  for_each_device_buffer(ctx, [](DevBuf &b) { b.new_call(); }, BufGroup::Pairs);
  SDF_HIP(ctx->cl_ranges.reserve(n * sizeof(ClassRange)));
  SDF_HIP(ctx->cl_out.reserve(n * sizeof(sdf_range_classes)));
  SDF_HIP(hipMemcpyAsync(ctx->cl_ranges.p, recs, n * sizeof(ClassRange), hipMemcpyHostToDevice, ctx->stream));
  SDF_HIP(hipMemsetAsync(ctx->cl_out.p, 0, n * sizeof(sdf_range_classes), ctx->stream));
  hipLaunchKernelGGL(sdf::pool_classes_kernel, dim3((unsigned)((n_seg + 15) / 16)), dim3(256), 0, ctx->stream,
                     (const ClassRange *)ctx->cl_ranges.p, (int)n, n_seg, (const char *)ctx->an_pool.p,
                     (sdf_range_classes *)ctx->cl_out.p);
  SDF_HIP(hipGetLastError());
  SDF_HIP(hipMemcpyAsync(back, ctx->cl_out.p, n * sizeof(sdf_range_classes), hipMemcpyDeviceToHost, ctx->stream));
  SDF_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(out, back, n * sizeof(sdf_range_classes));
  return SDF_OK;
}

// ---- ranges of the resident pool read back, by strand (include/sedef_hip.h; seq_pack.hip: pool_fetch_kernel) ----
// The checks of one range, and its record.  `why` gets the reason of a refusal.
static int fetch_check(const sdf_pool_fetch &r, size_t pool_bytes, size_t dst_bytes, const char **why) {
  if (r.flags & ~SDF_FETCH_RC) {
    *why = "unknown flag";
    return SDF_ERR_UNSUPPORTED;
  }
  if (!in_range(r.off, r.len, pool_bytes)) {
    *why = "outside the resident pool";
    return SDF_ERR_INVALID;
  }
  if (!in_range(r.dst_off, r.len, dst_bytes)) {
    *why = "destination outside dst";
    return SDF_ERR_INVALID;
  }
  return SDF_OK;
}

extern "C" int sdf_pool_fetch_plan(const sdf_pool_fetch *r, size_t n, size_t pool_bytes, size_t dst_bytes, sdf_pool_fetch_rec *recs,
                                   int *any_rc, long long *n_seg, size_t *bytes, size_t *bad) {
  int rc_any = 0;
  long long seg = 0;
  size_t sum = 0;
  int ret = SDF_OK;
  if (bad) *bad = 0;
  if ((!r && n) || n > 0x3fffffffu) ret = SDF_ERR_INVALID;
  for (size_t i = 0; i < n && ret == SDF_OK; ++i) {
    const char *why = nullptr;
    ret = fetch_check(r[i], pool_bytes, dst_bytes, &why);
    if (ret == SDF_OK && seg + (r[i].len + sdf::kFetchSegBytes - 1) / sdf::kFetchSegBytes > 0x7fffff00ll) ret = SDF_ERR_UNSUPPORTED;
    if (ret != SDF_OK) {
      if (bad) *bad = i;
      break;
    }
    if (recs) recs[i] = sdf_pool_fetch_rec{r[i].off, r[i].dst_off, r[i].len, (r[i].flags & SDF_FETCH_RC) ? 1 : 0, (int64_t)seg};
    seg += (r[i].len + sdf::kFetchSegBytes - 1) / sdf::kFetchSegBytes;
    sum += (size_t)r[i].len;
    rc_any |= r[i].flags & SDF_FETCH_RC;
  }
  if (any_rc) *any_rc = ret == SDF_OK && rc_any;
  if (n_seg) *n_seg = ret == SDF_OK ? seg : 0;
  if (bytes) *bytes = ret == SDF_OK ? sum : 0;
  return ret;
}

// what both forms ask of the pool before the kernel may read aligned slots of it
static int fetch_pool_ok(sdf_ctx *ctx, const char *who) {
  if (ctx->pool_bytes == 0 || !ctx->an_pool.p) return refuse(ctx, SDF_ERR_INVALID, std::string(who) + ": no resident pool");
  // (the slots of the first range start at the base; those of the last end inside the 64 bytes behind every pool allocation)
  if (!pool_base_aligned(ctx) || ctx->an_pool.cap < ctx->pool_bytes + 16)
    return refuse(ctx, SDF_ERR_INVALID, std::string(who) + ": the pool's base is not 16-byte aligned, or nothing is allocated behind its last character");
  return SDF_OK;
}

static void fetch_launch(const sdf::FetchRec *d_recs, int n, long long n_seg, bool rev, const char *d_pool, char *d_dst, hipStream_t st) {
  hipLaunchKernelGGL(rev ? sdf::pool_fetch_kernel<true> : sdf::pool_fetch_kernel<false>, dim3((unsigned)((n_seg + 15) / 16)), dim3(256),
                     0, st, d_recs, n, n_seg, d_pool, d_dst);
}

extern "C" int sdf_pool_fetch_ranges_device(sdf_ctx *ctx, const sdf_pool_fetch_rec *d_recs, size_t n, int any_rc, long long n_seg,
                                            char *d_dst, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0 || n_seg == 0) return SDF_OK;
  if (!d_recs || !d_dst || n > 0x3fffffffu || n_seg < 0 || n_seg > 0x7fffff00ll) {
    ctx->err = "sdf_pool_fetch_ranges_device: invalid arguments";
    return SDF_ERR_INVALID;
  }
  if (int rc = fetch_pool_ok(ctx, "sdf_pool_fetch_ranges_device")) return rc;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  fetch_launch(d_recs, (int)n, n_seg, any_rc != 0, (const char *)ctx->an_pool.p, d_dst, st);
  SDF_HIP(hipGetLastError());
  if (!stream) SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

// The host form: the output crosses PCIe through the context's pinned staging, a piece of at most fetch_stage_bytes at a time.
// A piece's device buffer mirrors the caller's dst modulo 16: ranges whose destinations follow one another without a gap lie
// back to back in it (the stage driver's slots: one copy out of the staging per piece), any other range begins at the next
// place that is congruent to its dst_off -- so the kernel's stores are aligned where the caller's destination is.  A range
// that does not fit the rest of a piece is cut: the sub-range [a, a + take) of a reversed range's output reads the source
// bytes [off + len - a - take, off + len - a).
extern "C" int sdf_pool_fetch_ranges(sdf_ctx *ctx, const sdf_pool_fetch *r, size_t n, char *dst, size_t dst_bytes) {
  using sdf::FetchRec;
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (n == 0) return SDF_OK;
  if (!r || n > 0x3fffffffu) {
    ctx->err = "sdf_pool_fetch_ranges: invalid arguments";
    return SDF_ERR_INVALID;
  }
  const size_t pool_bytes = ctx->pool_bytes;
  size_t total = 0, first_byte = 0;  // (first_byte: the first range that has one)
  bool any_rc = false;
  for (size_t i = 0; i < n; ++i) {
    const char *why = nullptr;
    if (int rc = fetch_check(r[i], pool_bytes, dst_bytes, &why)) {
      ctx->err = "sdf_pool_fetch_ranges: range " + std::to_string(i) + ": " + why;
      return rc;
    }
    if (total == 0) first_byte = i;
    total += (size_t)r[i].len;
    any_rc |= (r[i].flags & SDF_FETCH_RC) != 0;
  }
  if (total == 0) return SDF_OK;
  if (!dst) {
    ctx->err = "sdf_pool_fetch_ranges: range " + std::to_string(first_byte) + ": a byte to write and no dst";
    return SDF_ERR_INVALID;
  }
  if (int rc = fetch_pool_ok(ctx, "sdf_pool_fetch_ranges")) return rc;
  SDF_HIP(hipSetDevice(ctx->device));
  // (a range costs its bytes and up to 30 of padding; records: one per range of a piece and one per cut)
  const size_t cap = std::min<size_t>((size_t)ctx->cfg.fetch_stage_bytes, total + 32 * n + 4095) & ~(size_t)4095;
  const size_t max_recs = std::min<size_t>(n + 1, (size_t)1 << 18);
  SDF_HIP(ctx->host_fetch.reserve_exact(cap + max_recs * sizeof(FetchRec)));
  SDF_HIP(ctx->pf_out.reserve_exact(cap + 64));
  SDF_HIP(ctx->pf_recs.reserve_exact(max_recs * sizeof(FetchRec)));
  char *back = (char *)ctx->host_fetch.p;
  FetchRec *recs = (FetchRec *)(back + cap);
  struct Run { size_t dst_off, at, len; };
  std::vector<Run> runs;
  size_t i = 0, a = 0;  // the next byte to fetch: byte a of range i's output
  while (i < n) {
    size_t p = 0, nrec = 0;
    long long n_seg = 0;
    runs.clear();
    while (i < n && nrec < max_recs) {
      const size_t len = (size_t)r[i].len;
      if (a >= len) {
        ++i, a = 0;
        continue;
      }
      const size_t d = (size_t)r[i].dst_off + a;
      const bool follows = !runs.empty() && runs.back().dst_off + runs.back().len == d;
      const size_t at = follows ? p : ((p + 15) & ~(size_t)15) + (d & 15);
      if (at >= cap) break;
      const size_t take = std::min(len - a, cap - at);
      if (take < len - a && take < 4096 && nrec) break;  // (no slivers at the end of a piece)
      const bool rc = (r[i].flags & SDF_FETCH_RC) != 0;
      recs[nrec++] = FetchRec{r[i].off + (int64_t)(rc ? len - a - take : a), (int64_t)at, (int32_t)take, rc ? 1 : 0, (int64_t)n_seg};
      n_seg += (long long)((take + sdf::kFetchSegBytes - 1) / sdf::kFetchSegBytes);
      if (follows) runs.back().len += take;
      else runs.push_back(Run{d, at, take});
      p = at + take;
      a += take;
    }
    if (nrec == 0) continue;  // (only empty ranges were left)
    SDF_HIP(hipMemcpyAsync(ctx->pf_recs.p, recs, nrec * sizeof(FetchRec), hipMemcpyHostToDevice, ctx->stream));
    fetch_launch((const FetchRec *)ctx->pf_recs.p, (int)nrec, n_seg, any_rc, (const char *)ctx->an_pool.p, (char *)ctx->pf_out.p, ctx->stream);
    SDF_HIP(hipGetLastError());
    SDF_HIP(hipMemcpyAsync(back, ctx->pf_out.p, p, hipMemcpyDeviceToHost, ctx->stream));
    SDF_HIP(hipStreamSynchronize(ctx->stream));
    for (const Run &q : runs) memcpy(dst + q.dst_off, back + q.at, q.len);
  }
  return SDF_OK;
}

// Debug: wavefronts started per (XCD, shader engine, CU, SIMD) since the last call, 4096 counters indexed
// xcd << 9 | se << 6 | cu << 2 | simd (the chained strips note theirs: how evenly the dispatcher spreads a launch).
extern "C" int sdf_debug_placement(sdf_ctx *ctx, uint32_t *out) {
  if (!ctx) return SDF_ERR_INVALID;
  SDF_HIP(hipSetDevice(ctx->device));
  static unsigned *buf = nullptr;
  if (!buf) {
    SDF_HIP(hipMalloc(&buf, 4096 * sizeof(unsigned)));
    SDF_HIP(hipMemset(buf, 0, 4096 * sizeof(unsigned)));
    SDF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(sdf::g_place), &buf, sizeof(buf)));
  }
  SDF_HIP(hipDeviceSynchronize());
  if (out) {
    SDF_HIP(hipMemcpy(out, buf, 4096 * sizeof(unsigned), hipMemcpyDeviceToHost));
    SDF_HIP(hipMemset(buf, 0, 4096 * sizeof(unsigned)));
  }
  return SDF_OK;
}

// ---- debugging aid (not part of the public header): the resident pool's characters [off, off + bytes) as they lie in HBM ----
extern "C" int sdf_debug_pool_read(sdf_ctx *ctx, size_t off, size_t bytes, char *host) {
  if (!ctx || !host || !in_range(off, bytes, ctx->pool_bytes)) return SDF_ERR_INVALID;
  if (!bytes) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  SDF_HIP(hipStreamSynchronize(ctx->stream));
  return hipMemcpy(host, (const char *)ctx->an_pool.p + off, bytes, hipMemcpyDeviceToHost) == hipSuccess ? SDF_OK : SDF_ERR_HIP;
}

// Search filter: the reference's filter() (src/filter.cc) for many pairs of ranges of the resident pool -- uppercase counts and
// the q-gram (q = 5) histogram min-sum of both sides; include/sedef_hip.h states up, dist, minqg and the verdict.
//   class     a task whose sides both hold at most FILTER_WAVE_MAX_LEN characters takes ONE wavefront and counts in 16 bits,
//             two bins a word: 2 x 2 KB of LDS.  A longer one takes a workgroup of FILTER_LONG_WAVES wavefronts on one pair of
//             histograms with 32-bit counts (a side may hold 2^31 - 1 characters): 2 x 4 KB.  One launch per class over all
//             tasks; a workgroup whose task is of the other class leaves at once, so the class is read off the task alone;
//   pass      every lane takes a contiguous run of ceil(len / lanes) characters and reads the four before it as well to fill its
//             rolling 10-bit gram: eight bytes a load (stats_fetch8: no load leaves the range, the reverse strand is the same
//             load turned round).  Uppercase is counted in the same pass, over the lane's own run only;
//   adds      a lane keeps its gram and a run length and adds to LDS only when the gram changes: a homopolymer run -- where
//             every lane would add to one bin once per character, and the LDS would take those adds one after the other -- costs
//             one add a lane.  Repeats of a longer period are not aggregated;
//   min-sum   the bins are dealt round the lanes (sixteen a lane for the wavefront class), summed by stats_wave_sum and, for the
//             long class, over the wavefronts through LDS.
// MINSUM false (profiles/search_filter.py): the workgroup leaves behind the histogram pass, so that its time against the whole
// launch's is the pass's share.
// No scratch, no global atomics.  A task that carries SDF_FILTER_SKIP, or that the device form may not read (filter_task_bad),
// gets a zero record with SDF_FILTER_SKIPPED from the wavefront-class launch.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "stats_dev.h"

namespace sdf {

// One side: its grams into hist (PACKED: bin g is the 16-bit half g & 1 of word g >> 1), returns this lane's uppercase count.
template <int NT, bool PACKED, bool REV>
__device__ __forceinline__ int filter_side(const char *s, const int len, const bool rc, uint32_t *hist, const int tid) {
  if (len <= 0) return 0;
  const int run = (len - 1) / NT + 1;
  const long long b64 = (long long)tid * run;
  const int b = b64 < len ? (int)b64 : len, e = len - b < run ? len : b + run;
  const int p0 = b >= 4 ? b - 4 : 0;
  const bool wide = len >= 8;  // wave-uniform
  uint32_t g = 0, cur = 0;
  int up = 0, cnt = 0;
  const auto flush = [&]() {
    if (cnt) atomicAdd(&hist[PACKED ? cur >> 1 : cur], PACKED ? (uint32_t)cnt << (16 * (cur & 1)) : (uint32_t)cnt);
  };
  int pos = b < e ? p0 : e;  // (a lane behind the last run reads nothing)
  while (pos < e) {
    uint64_t v = stats_fetch8<REV>(s, pos, len, wide, rc);
    if (!(REV && rc)) v &= 0x7F7F7F7F7F7F7F7FULL;  // (stats_revcomp4 has done so on the reverse strand)
    const int m = e - pos < 8 ? e - pos : 8;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (j < m) {
        const uint32_t c = (uint32_t)(v >> (8 * j)) & 0xFFu, u = c & 0xDFu;
        const uint32_t code = (u == 'C' || u == 'G' || u == 'T') ? ((c >> 1) ^ (c >> 2)) & 3u : 0u;
        g = ((g << 2) | code) & (FILTER_GRAMS - 1);
        const int i = pos + j;
        if (i >= b) {
          up += c - 'A' < 26u ? 1 : 0;
          if (i >= 4) {
            if (cnt && g == cur) {
              ++cnt;
            } else {
              flush();
              cur = g, cnt = 1;
            }
          }
        }
      }
    }
    if (e - pos <= 8) break;
    pos += 8;
  }
  flush();
  return up;
}

template <int WAVES, bool REV, bool MINSUM>
__global__ __launch_bounds__(64 * WAVES) void search_filter_kernel(const sdf_filter_task *__restrict__ tasks, int n, const char *__restrict__ pool,
                                                                   long long pool_bytes, sdf_filter_params P, sdf_filter_rec *__restrict__ out) {
  constexpr int NT = 64 * WAVES;
  constexpr bool PACKED = WAVES == 1;
  constexpr int WORDS = PACKED ? FILTER_GRAMS / 2 : FILTER_GRAMS;
  __shared__ uint32_t hist[2][WORDS];
  __shared__ int part[3][WAVES];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  if (t >= n) return;
  const sdf_filter_task T = tasks[t];
  if ((T.flags & SDF_FILTER_SKIP) || filter_task_bad(T, pool_bytes)) {
    if (PACKED && tid == 0) out[t] = sdf_filter_rec{0, 0, 0, 0, SDF_FILTER_SKIPPED};
    return;
  }
  if ((T.q_len > FILTER_WAVE_MAX_LEN || T.r_len > FILTER_WAVE_MAX_LEN) == PACKED) return;
  for (int w = tid; w < WORDS; w += NT) hist[0][w] = 0, hist[1][w] = 0;
  __syncthreads();
  int q_up = filter_side<NT, PACKED, REV>(pool + T.q_off, T.q_len, REV && (T.flags & SDF_FILTER_Q_RC), hist[0], tid);
  int r_up = filter_side<NT, PACKED, REV>(pool + T.r_off, T.r_len, REV && (T.flags & SDF_FILTER_R_RC), hist[1], tid);
  __syncthreads();
  int dist = 0;
  if (!MINSUM) {  // (profiles/search_filter.py: the histogram pass alone; the record is NOT the pair's)
    if (tid == 0) out[t] = sdf_filter_rec{q_up, r_up, (int32_t)(hist[0][0] + hist[1][0]), 0, 0u};
    return;
  }
  for (int w = tid; w < WORDS; w += NT) {
    const uint32_t a = hist[0][w], b = hist[1][w];
    if (PACKED) {
      const uint32_t al = a & 0xFFFFu, bl = b & 0xFFFFu, ah = a >> 16, bh = b >> 16;
      dist += (int)((al < bl ? al : bl) + (ah < bh ? ah : bh));
    } else {
      dist += (int)(a < b ? a : b);
    }
  }
  q_up = stats_wave_sum(q_up), r_up = stats_wave_sum(r_up), dist = stats_wave_sum(dist);
  if (WAVES > 1) {
    if ((tid & 63) == 0) part[0][tid >> 6] = q_up, part[1][tid >> 6] = r_up, part[2][tid >> 6] = dist;
    __syncthreads();
    q_up = r_up = dist = 0;
    for (int w = 0; w < WAVES; w++) q_up += part[0][w], r_up += part[1][w], dist += part[2][w];
  }
  if (tid == 0) out[t] = filter_verdict(q_up, r_up, dist, T.q_len > T.r_len ? T.q_len : T.r_len, P);
}

#define SDF_FILTER_INSTANCE(WAVES, REV, MINSUM)                                                                                       \
  template __global__ void search_filter_kernel<WAVES, REV, MINSUM>(const sdf_filter_task *, int, const char *, long long, sdf_filter_params, \
                                                                    sdf_filter_rec *);
SDF_FILTER_INSTANCE(1, false, true)
SDF_FILTER_INSTANCE(1, true, true)
SDF_FILTER_INSTANCE(FILTER_LONG_WAVES, false, true)
SDF_FILTER_INSTANCE(FILTER_LONG_WAVES, true, true)
SDF_FILTER_INSTANCE(1, false, false)
SDF_FILTER_INSTANCE(1, true, false)
#undef SDF_FILTER_INSTANCE

// One lane per interval: the interval's window by a binary search in first[], its task by filter_task_of.
__global__ __launch_bounds__(256) void search_filter_tasks_kernel(const sdf_minimizer *__restrict__ q, int nq, const sdf_search_window *__restrict__ windows,
                                                                  const uint64_t *__restrict__ first, const sdf_search_interval *__restrict__ intervals,
                                                                  const sdf_search_roll_rec *__restrict__ rolls, int n_max, FilterTaskArgs A,
                                                                  sdf_filter_task *__restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_max) return;
  if ((uint64_t)t >= first[nq]) {
    out[t] = sdf_filter_task{0, 0, 0, 0, SDF_FILTER_SKIP, 0};
    return;
  }
  int lo = 0, hi = nq;  // the last i in [0, nq) with first[i] <= t
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (first[mid] <= (uint64_t)t) lo = mid;
    else hi = mid;
  }
  out[t] = filter_task_of(A, q[lo].loc, windows[lo], intervals[t], rolls[t]);
}

}  // namespace sdf

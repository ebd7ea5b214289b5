// The acceptance step of the search driver: which windows of a round that ran speculatively against the found list as it stood
// are the reference's own, and their records appended; include/sedef_hip.h states the rules.
//   search_accept_window_kernel    one wavefront per round window: the classes of its intervals 64 at a time, the serial replay
//                                  of is_overlap over them with the lanes testing the kept records in LDS, parse_hits over the
//                                  kept hits; an AcceptWin record, and the kept entries -- the interval's index, kAcceptDropped
//                                  -- at kept[first[i] ..] (a window keeps no more records than it has intervals).
//   search_accept_frontier_kernel  one workgroup: the exclusive prefix maximum of reach and the first window it reaches or that
//                                  is incomplete, then the exclusive sums of the accepted windows' records and survivors, the
//                                  counters, the status record, and *go: the windows the append may write (0 on overflow).
//   search_accept_append_kernel    one wavefront per round window below *go: its kept records to found, its survivors to out.
//   search_accept_tail_kernel      (the driver's) the tail of first[] behind a round's slice.
// Every store is a vector store from C++; nothing is written at or behind a capacity.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

__global__ __launch_bounds__(64) void search_accept_window_kernel(const AcceptRound A, AcceptWin *__restrict__ win, uint32_t *__restrict__ kept) {
  __shared__ sdf_search_found recs[ACCEPT_MAX_KEPT];
  __shared__ uint32_t kept_t[ACCEPT_MAX_KEPT];
  __shared__ uint8_t drop[ACCEPT_MAX_KEPT];
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= A.na) return;
  const uint32_t i = A.act[j];
  AcceptWin W{0, 0, 0, 1, 0, 0, 0, 0};
  if (i >= (uint32_t)A.nq) {
    if (lane == 0) win[j] = W;
    return;
  }
  W.qs = A.q[i].loc;
  const uint64_t t0 = A.first[i], t1 = A.first[i + 1];
  if (t1 < t0 || t1 > (uint64_t)A.n_max) {
    if (lane == 0) win[j] = W;
    return;
  }
  bool incomplete = (A.windows[i].flags & (SDF_SEARCH_WIDE | SDF_SEARCH_FOUND_WIDE)) != 0;
  const long long pf_pos = W.qs, pf_end = pf_pos + A.init_len;
  int nk = 0;  // the kept hits, those beyond the cap counted too
  for (uint64_t base = t0; base < t1; base += 64) {
    const uint64_t t = base + lane;
    const bool live = t < t1;
    sdf_search_roll_rec R{0, 0, 0, 0, 0, 0};
    sdf_search_hit H{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cls = -1;
    if (live) {
      R = A.rolls[t], H = A.hits[t];
      cls = accept_class(R, A.overlap[t], A.filter[t], H, A.hit_filter[t]);
    }
    incomplete |= __ballot(live && accept_unfinished(R, H)) != 0;
    W.attempted += __popcll(__ballot(live));
    W.jaccard_failed += __popcll(__ballot(cls == 0));
    W.interval_failed += __popcll(__ballot(cls == 1));
    unsigned long long todo = __ballot(cls >= 2);
    while (todo) {  // (wave-uniform: the replay, in interval order)
      const int s = __builtin_ctzll(todo);
      todo &= todo - 1;
      const long long pfp_pos = __shfl(R.ref_start, s), pfp_end = __shfl(R.ref_end, s);
      const sdf_search_found mine{__shfl(H.query_start, s), __shfl(H.query_end, s), __shfl(H.ref_start, s), __shfl(H.ref_end, s)};
      const int cls_s = __shfl(cls, s);
      const int have = nk < ACCEPT_MAX_KEPT ? nk : ACCEPT_MAX_KEPT;
      bool hit = false;
      for (int k0 = 0; k0 < have && !hit; k0 += 64) {
        const int k = k0 + lane;
        bool h = false;
        if (k < have) {
          const sdf_search_found P = recs[k];
          h = !found_empty(P) && found_covers(P, pf_pos, pfp_pos) && found_overlaps(P, pf_pos, pf_end, pfp_pos, pfp_end, A.min_read_size);
        }
        hit = __ballot(h) != 0;
      }
      if (hit) {
        W.interval_failed += 1;
      } else if (cls_s == 3) {
        if (nk < ACCEPT_MAX_KEPT && lane == 0) recs[nk] = mine, kept_t[nk] = (uint32_t)(base + s);
        W.reach = mine.q_end > W.reach ? mine.q_end : W.reach;
        nk += 1;
        __syncthreads();  // (one wavefront per workgroup: this only orders lane 0's LDS stores before the next test's reads)
      }
    }
  }
  incomplete |= nk > ACCEPT_MAX_KEPT;
  const int have = nk < ACCEPT_MAX_KEPT ? nk : ACCEPT_MAX_KEPT;
  __syncthreads();
  // parse_hits: a kept hit is dropped when another kept hit contains it
  int n_out = 0;
  for (int k0 = 0; k0 < have; k0 += 64) {
    const int k = k0 + lane;
    bool dropped = false;
    if (k < have) {
      const sdf_search_found h = recs[k];
      for (int p = 0; p < have && !dropped; p++) dropped = p != k && accept_contains(recs[p], h);
      drop[k] = dropped ? 1 : 0;
    }
    n_out += __popcll(__ballot(k < have && !dropped));
  }
  __syncthreads();
  // (have <= the window's intervals, so t0 + k < t1 <= n_max)
  for (int k = lane; k < have; k += 64) kept[t0 + k] = kept_t[k] | (drop[k] ? kAcceptDropped : 0u);
  W.n_kept = have, W.n_out = n_out, W.incomplete = incomplete ? 1 : 0;
  if (lane == 0) win[j] = W;
}

// inclusive scans over a wavefront's lanes
__device__ __forceinline__ int accept_wave_max(int v, const int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off);
    v = lane >= off && o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned accept_wave_sum(unsigned v, const int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(v, off);
    v += lane >= off ? o : 0u;
  }
  return v;
}

__global__ __launch_bounds__(1024) void search_accept_frontier_kernel(const AcceptWin *__restrict__ win, const int na, const unsigned long long nf,
                                                                      const unsigned long long found_cap, const unsigned long long n_out,
                                                                      const unsigned long long out_cap, AcceptOff *__restrict__ off,
                                                                      sdf_search_accept_status *__restrict__ status, uint32_t *__restrict__ go) {
  __shared__ int tot_max[16];
  __shared__ unsigned tot_f[16], tot_o[16];
  __shared__ int s_front;
  __shared__ unsigned long long s_count[3];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  if (tid == 0) s_front = na, s_count[0] = s_count[1] = s_count[2] = 0;
  __syncthreads();
  // the frontier: the first window that an earlier window's kept record reaches, or that is incomplete
  int carry = 0;
  for (int base = 0; base < na; base += 1024) {  // (uniform trip count)
    const int j = base + tid;
    AcceptWin W{0, 0, 0, 0, 0, 0, 0, 0};
    if (j < na) W = win[j];
    const int incl = accept_wave_max(W.reach, lane);
    const int left = __shfl_up(incl, 1);
    if (lane == 63) tot_max[wv] = incl;
    __syncthreads();
    int before = carry, all = carry;
#pragma unroll
    for (int k = 0; k < 16; k++) before = k < wv && tot_max[k] > before ? tot_max[k] : before, all = tot_max[k] > all ? tot_max[k] : all;
    const int reach = lane && left > before ? left : before;
    if (j < na && (reach > W.qs || W.incomplete)) atomicMin(&s_front, j);
    carry = all;
    __syncthreads();
  }
  const int frontier = s_front;
  // where the accepted windows' records go, and their counters
  unsigned long long carry_f = 0, carry_o = 0, c0 = 0, c1 = 0, c2 = 0;
  for (int base = 0; base < na; base += 1024) {
    const int j = base + tid;
    AcceptWin W{0, 0, 0, 0, 0, 0, 0, 0};
    if (j < frontier) W = win[j];
    const unsigned vf = (unsigned)W.n_kept, vo = (unsigned)W.n_out;
    const unsigned in_f = accept_wave_sum(vf, lane), in_o = accept_wave_sum(vo, lane);
    if (lane == 63) tot_f[wv] = in_f, tot_o[wv] = in_o;
    __syncthreads();
    unsigned long long bf = 0, bo = 0, af = 0, ao = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) bf += k < wv ? tot_f[k] : 0u, bo += k < wv ? tot_o[k] : 0u, af += tot_f[k], ao += tot_o[k];
    if (j < na) off[j] = AcceptOff{(uint32_t)(carry_f + bf + in_f - vf), (uint32_t)(carry_o + bo + in_o - vo)};
    carry_f += af, carry_o += ao;
    c0 += (unsigned long long)W.attempted, c1 += (unsigned long long)W.jaccard_failed, c2 += (unsigned long long)W.interval_failed;
    __syncthreads();
  }
  atomicAdd(&s_count[0], c0), atomicAdd(&s_count[1], c1), atomicAdd(&s_count[2], c2);
  __syncthreads();
  if (tid == 0) {
    sdf_search_accept_status S;
    S.need_found = nf + carry_f, S.need_out = n_out + carry_o;
    const bool over = S.need_found > found_cap || S.need_out > out_cap;
    S.frontier = over ? 0u : (uint32_t)frontier;
    S.flags = over ? SDF_ACCEPT_OVERFLOW : frontier < na && win[frontier].incomplete ? SDF_ACCEPT_INCOMPLETE : 0u;
    S.nf = over ? nf : S.need_found, S.n_out = over ? n_out : S.need_out;
    S.attempted = over ? 0 : (int64_t)s_count[0], S.jaccard_failed = over ? 0 : (int64_t)s_count[1];
    S.interval_failed = over ? 0 : (int64_t)s_count[2];
    *status = S;
    *go = S.frontier;
  }
}

__global__ __launch_bounds__(64) void search_accept_append_kernel(const AcceptRound A, const AcceptWin *__restrict__ win,
                                                                  const uint32_t *__restrict__ kept, const AcceptOff *__restrict__ off,
                                                                  const uint32_t *__restrict__ go, sdf_search_found *__restrict__ found,
                                                                  const unsigned long long nf, const unsigned long long found_cap,
                                                                  sdf_search_pair_hit *__restrict__ out, const unsigned long long n_out,
                                                                  const unsigned long long out_cap) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= A.na || (uint32_t)j >= *go) return;
  const AcceptWin W = win[j];  // (accepted: complete, so act[j] and first[] passed the first launch's tests)
  const uint32_t i = A.act[j];
  const uint64_t t0 = A.first[i];
  const unsigned long long at_f = nf + off[j].found, at_o = n_out + off[j].out;
  int written = 0;
  for (int k0 = 0; k0 < W.n_kept; k0 += 64) {
    const int k = k0 + lane;
    const bool live = k < W.n_kept;
    const uint32_t e = live ? kept[t0 + k] : kAcceptDropped;
    const uint32_t t = e & ~kAcceptDropped;
    sdf_search_hit H{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live && t < (uint64_t)A.n_max) H = A.hits[t];
    if (live && at_f + k < found_cap) found[at_f + k] = sdf_search_found{H.query_start, H.query_end, H.ref_start, H.ref_end};
    const bool survives = live && !(e & kAcceptDropped);
    const unsigned long long m = __ballot(survives);
    const unsigned long long at = at_o + written + __popcll(m & ((1ull << lane) - 1ull));
    if (survives && at < out_cap)
      out[at] = sdf_search_pair_hit{(int32_t)(A.window_base + (int)i), H.query_start, H.query_end, H.ref_start, H.ref_end, H.jaccard};
    written += __popcll(m);
  }
}

// For the driver's rounds, which run the windows call on a slice q[i0, e) but every later call on all of q: first[e + 1 .. n]
// take first[e], the slice's total, so that the windows behind the slice have no intervals.
__global__ __launch_bounds__(256) void search_accept_tail_kernel(uint64_t *__restrict__ first, const int e, const int n) {
  const long long j = (long long)e + 1 + (long long)blockIdx.x * 256 + threadIdx.x;
  if (j <= n) first[j] = first[e];
}

}  // namespace sdf

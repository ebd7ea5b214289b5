// Search roll: every reference interval of sdf_search_windows rolled to its best initial match -- the first loop of the
// reference's search_in_reference_interval (src/search.cc:274-314) with its SlidingMap as it behaves; include/sedef_hip.h
// states add, remove, J and the walk.  One wavefront per interval, LDS only: a literal transcription with an array in place
// of the map.
//   window    interval t belongs to the last window i with first[i] <= t: a 64-way search in first[] (search_wave_bound);
//   span      the records of r the walk can meet, start <= loc <= end + init_len: two 64-way searches over the locs.  No
//             record beyond the span causes an event (a remove needs loc <= s < end, an add loc == e <= end - 1 + init_len),
//             so the walk counts its records from the span's first and the span's size stands for nr;
//   keys      a key is status << 30 | hash (hash < 2^30: the header's contract).  The members' keys and the span's go into
//             LDS -- a status-2 record, which no add or remove looks at, stands there as the first member's key --, are sorted
//             (search_sort_u32) and compacted (search_compact_u32): a slot per distinct key, in ascending key order;
//   slots     every record finds its slot by a binary search, in parallel; bits[slot] = 1 for the members, B = the members'
//             largest slot.  Then the span's locs take the keys' place;
//   walk      serial by nature -- I depends on the path -- and wave-uniform: every lane carries s, e, ws, we, B and I and
//             makes every write to bits[] itself, so a lane reads back only what it wrote and the walk needs no barrier.
//             It jumps from event to event (a step without one cannot change J).  The boundary's predecessor and
//             successor are the one place the lanes share work: 64 neighbouring slots a round, a ballot over bits != 0.
// The wavefronts at or beyond first[nq] leave at once.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "search_dev.h"

namespace sdf {

template <bool WALK>
__global__ __launch_bounds__(64) void search_roll_kernel(const sdf_minimizer *__restrict__ q, int nq, const sdf_search_window *__restrict__ windows,
                                                         const uint64_t *__restrict__ first, const sdf_search_interval *__restrict__ intervals,
                                                         const sdf_minimizer *__restrict__ r, int nr, long long len_r, int init_len,
                                                         const int32_t *__restrict__ limit, int n_limit, sdf_search_roll_rec *__restrict__ out) {
  __shared__ uint32_t keys[ROLL_MAX_KEYS];  // the keys, then the distinct keys; in the walk the span's locs
  __shared__ uint16_t slot[ROLL_MAX_SPAN];  // of the span's records (kNoSlot: status 2)
  __shared__ uint8_t bits[ROLL_MAX_KEYS];
  constexpr uint16_t kNoSlot = 0xFFFFu;
  const int lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
  if (t >= first[nq]) return;
  int i = search_wave_bound(nq + 1, [&](int x) { return first[x] <= t; }, lane) - 1;
  i = i < 0 ? 0 : i > nq - 1 ? nq - 1 : i;
  const sdf_search_window W = windows[i];
  const sdf_search_interval T = intervals[t];
  const long long start = T.start, span_last = (long long)T.end + init_len;
  const int lo = search_wave_bound(nr, [&](int x) { return (long long)r[x].loc < start; }, lane);
  int hi = search_wave_bound(nr, [&](int x) { return (long long)r[x].loc <= span_last; }, lane);
  hi = hi < lo ? lo : hi;
  const int nspan = hi - lo, nm = W.n_members;
  sdf_search_roll_rec R;
  R.ref_start = R.ref_end = R.winnow_start = R.winnow_end = R.jaccard = 0, R.flags = 0;
  if (nm > SEARCH_MAX_MEMBERS || nspan > ROLL_MAX_SPAN) R.flags = SDF_ROLL_WIDE;
  else if (nm < 1 || nm > nq - i || W.query_size < 0 || W.query_size >= n_limit) R.flags = SDF_ROLL_BADWINDOW;
  if (R.flags) {
    if (lane == 0) out[t] = R;
    return;
  }
  const int L = limit[W.query_size];
  // keys
  for (int j = lane; j < nm; j += 64) keys[j] = roll_key(q[i + j]);
  for (int x = lane; x < nspan; x += 64) {
    const sdf_minimizer M = r[lo + x];
    keys[nm + x] = M.status == 2 ? roll_key(q[i]) : roll_key(M);
  }
  const int nd = search_slots_setup(keys, bits, nm + nspan, lane);  // slots
  int B = 0;
  for (int j = lane; j < nm; j += 64) {
    const int sl = roll_slot(keys, nd, roll_key(q[i + j]));
    bits[sl] = 1;
    B = sl > B ? sl : B;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int other = __shfl_xor(B, o);
    B = other > B ? other : B;
  }
  B = __builtin_amdgcn_readfirstlane(B);
  for (int x = lane; x < nspan; x += 64) {
    const sdf_minimizer M = r[lo + x];
    slot[x] = M.status == 2 ? kNoSlot : (uint16_t)roll_slot(keys, nd, roll_key(M));
  }
  __syncthreads();
  int32_t *locs = (int32_t *)keys;
  for (int x = lane; x < nspan; x += 64) locs[x] = r[lo + x].loc;
  __syncthreads();
  if (!WALK) {
    if (lane == 0) R.winnow_start = lo, R.winnow_end = hi, R.jaccard = B + bits[B] + (nspan ? slot[0] + locs[0] : 0), out[t] = R;
    return;
  }
  // the walk: wave-uniform from here on
  SearchMap S{bits, nd, B, 0};
  long long best_s = 0, best_e = 0;
  int best_ws = 0, best_we = 0, best_J = 0;
  bool any = false;
  search_roll_walk(S, slot, locs, nspan, start, T.end, init_len, len_r, lane, [&](long long s, long long e, int ws, int we) {
    const int now = S.I >= L ? S.I : S.I - L;
    if (!any || now > best_J) best_s = s, best_e = e, best_ws = ws, best_we = we, best_J = now;
    any = true;
    return false;
  });
  if (lane == 0) {
    R.ref_start = (int32_t)best_s, R.ref_end = (int32_t)best_e;
    R.winnow_start = lo + best_ws, R.winnow_end = lo + best_we, R.jaccard = best_J;
    out[t] = R;
  }
}

template __global__ void search_roll_kernel<false>(const sdf_minimizer *, int, const sdf_search_window *, const uint64_t *,
                                                   const sdf_search_interval *, const sdf_minimizer *, int, long long, int, const int32_t *, int,
                                                   sdf_search_roll_rec *);
template __global__ void search_roll_kernel<true>(const sdf_minimizer *, int, const sdf_search_window *, const uint64_t *,
                                                  const sdf_search_interval *, const sdf_minimizer *, int, long long, int, const int32_t *, int,
                                                  sdf_search_roll_rec *);

}  // namespace sdf

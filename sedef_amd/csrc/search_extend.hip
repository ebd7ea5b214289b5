// Search extend: every rolled interval of sdf_search_roll grown to its hit -- the reference's extend() (src/search.cc:95-259)
// on its SlidingMap as it behaves; include/sedef_hip.h states the entry state, the four map operations, the stop tests and the
// do and undo steps.  One wavefront per interval, LDS only, built like search_roll.hip and from the same parts (search_dev.h:
// the keys' sort and slots, SearchMap, the roll's walk):
//   universe  the query records q[q0, q1) = the members and EXT_GROW records on either side of them; the reference records
//             r[r0, r1) = from the roll span's first record, or EXT_GROW records in front of the roll's winnow_start if that is
//             earlier, to EXT_GROW records behind its winnow_end.  No other record can be touched before the growth cap flags
//             the interval.  Their keys are sorted and compacted to slots as in the roll kernel (a status-2 reference record,
//             which no add or remove looks at, stands there as the first member's key; a status-2 QUERY record is a key like
//             any other);
//   entry     bits = 1 on the members, B their largest slot, I = 0; the roll's walk is replayed (search_roll_walk) up to the
//             evaluation at which it reaches the record's winnow_start and winnow_end;
//   extension wave-uniform like the walk: every lane carries the scalars and makes every write to bits[] itself, no barriers.
//             The locs lie in LDS where the keys were; the one record a range can reach beyond the universe is read from HBM.
// The wavefronts at or beyond first[nq] leave at once.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "search_dev.h"

namespace sdf {

__global__ __launch_bounds__(64) void search_extend_kernel(const sdf_minimizer *__restrict__ q, int nq, const sdf_search_window *__restrict__ windows,
                                                           const uint64_t *__restrict__ first, const sdf_search_interval *__restrict__ intervals,
                                                           const sdf_search_roll_rec *__restrict__ rolls, const sdf_filter_rec *__restrict__ filter,
                                                           const sdf_minimizer *__restrict__ r, int nr, long long len_q, long long len_r,
                                                           int init_len, const int32_t *__restrict__ limit, int n_limit, sdf_extend_params P,
                                                           sdf_search_hit *__restrict__ out) {
  __shared__ uint32_t keys[EXT_MAX_KEYS];  // the keys, then the distinct keys; afterwards the locs: the query's, then the reference's
  __shared__ uint16_t slot_q[EXT_MAX_Q];   // of the universe's records
  __shared__ uint16_t slot_r[EXT_MAX_R];   // (kNoSlot: status 2)
  __shared__ uint8_t bits[EXT_MAX_KEYS];
  constexpr uint16_t kNoSlot = 0xFFFFu;
  const int lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
  if (t >= first[nq]) return;
  int i = search_wave_bound(nq + 1, [&](int x) { return first[x] <= t; }, lane) - 1;
  i = i < 0 ? 0 : i > nq - 1 ? nq - 1 : i;
  const sdf_search_window W = windows[i];
  const sdf_search_interval T = intervals[t];
  const sdf_search_roll_rec Roll = rolls[t];
  const long long start = T.start;
  const int lo = search_wave_bound(nr, [&](int x) { return (long long)r[x].loc < start; }, lane);
  const int nm = W.n_members, rws0 = Roll.winnow_start, rwe0 = Roll.winnow_end;
  sdf_search_hit H{0, 0, 0, 0, 0, 0, 0, 0, 0, 0u};
  if (nm < 1 || nm > nq - i || W.query_size < 0 || W.query_size >= n_limit || extend_skips(Roll, filter ? &filter[t] : nullptr, lo, nr))
    H.flags = SDF_EXTEND_SKIPPED;
  else if (extend_replay_wide(Roll, nm, lo)) H.flags = SDF_EXTEND_WIDE;
  if (H.flags) {
    if (lane == 0) out[t] = H;
    return;
  }
  const int q0 = i - EXT_GROW > 0 ? i - EXT_GROW : 0, q1 = nq - (i + nm) > EXT_GROW ? i + nm + EXT_GROW : nq;
  const int back = rws0 - EXT_GROW < lo ? rws0 - EXT_GROW : lo;
  const int r0 = back > 0 ? back : 0, r1 = nr - rwe0 > EXT_GROW ? rwe0 + EXT_GROW : nr;
  const int nqu = q1 - q0, nru = r1 - r0;  // <= EXT_MAX_Q, <= EXT_MAX_R: rwe0 - lo <= ROLL_MAX_SPAN
  // keys
  for (int x = lane; x < nqu; x += 64) keys[x] = roll_key(q[q0 + x]);
  for (int x = lane; x < nru; x += 64) {
    const sdf_minimizer M = r[r0 + x];
    keys[nqu + x] = M.status == 2 ? roll_key(q[i]) : roll_key(M);
  }
  const int nd = search_slots_setup(keys, bits, nqu + nru, lane);
  // slots
  for (int x = lane; x < nqu; x += 64) slot_q[x] = (uint16_t)roll_slot(keys, nd, roll_key(q[q0 + x]));
  for (int x = lane; x < nru; x += 64) {
    const sdf_minimizer M = r[r0 + x];
    slot_r[x] = M.status == 2 ? kNoSlot : (uint16_t)roll_slot(keys, nd, roll_key(M));
  }
  __syncthreads();
  int B = 0;
  for (int j = lane; j < nm; j += 64) {
    const int sl = slot_q[i - q0 + j];
    bits[sl] = 1;
    B = sl > B ? sl : B;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int other = __shfl_xor(B, o);
    B = other > B ? other : B;
  }
  B = __builtin_amdgcn_readfirstlane(B);
  int32_t *locs_q = (int32_t *)keys, *locs_r = locs_q + nqu;
  for (int x = lane; x < nqu; x += 64) locs_q[x] = q[q0 + x].loc;
  for (int x = lane; x < nru; x += 64) locs_r[x] = r[r0 + x].loc;
  __syncthreads();
  // the entry state: wave-uniform from here on
  SearchMap S{bits, nd, B, 0};
  search_roll_walk(S, slot_r + (lo - r0), locs_r + (lo - r0), r1 - lo, start, T.end, init_len, len_r, lane,
                   [&](long long, long long, int ws, int we) { return ws >= rws0 - lo && we >= rwe0 - lo; });
  int qsz = W.query_size, L = limit[qsz];
  int qws = i, qwe = i + nm, rws = rws0, rwe = rwe0;
  bool wide = false, nolimit = false;
  auto q_loc = [&](int x) { return x >= q0 && x < q1 ? locs_q[x - q0] : q[x].loc; };
  auto r_loc = [&](int x) { return x >= r0 && x < r1 ? locs_r[x - r0] : r[x].loc; };
  auto add_to_query = [&](int x) {
    if (!S.add(__builtin_amdgcn_readfirstlane((int)slot_q[x - q0]), 1, qsz != 0, lane)) return;
    if (++qsz >= n_limit) {
      nolimit = true;
      return;
    }
    L = limit[qsz];
    const int up = S.above(S.B, lane);  // (B none, -1: the smallest stored slot)
    if (up < nd) S.B = up;
    S.I += S.full(S.B) ? 1 : 0;
  };
  auto remove_from_query = [&](int x) {
    if (!S.remove(__builtin_amdgcn_readfirstlane((int)slot_q[x - q0]), 1, qsz != 0, lane)) return;
    qsz -= qsz > 0 ? 1 : 0;
    L = limit[qsz];
    if (S.B < 0) return;
    S.I -= S.full(S.B) ? 1 : 0;
    S.B = S.below(S.B, lane);
  };
  auto add_to_reference = [&](int x) {
    const int sl = __builtin_amdgcn_readfirstlane((int)slot_r[x - r0]);
    if (sl != kNoSlot) S.add(sl, 2, qsz != 0, lane);
  };
  auto remove_from_reference = [&](int x) {
    const int sl = __builtin_amdgcn_readfirstlane((int)slot_r[x - r0]);
    if (sl != kNoSlot) S.remove(sl, 2, qsz != 0, lane);
  };
  auto J = [&]() { return S.I >= L ? S.I : S.I - L; };
  int qs = qws ? q_loc(qws - 1) + 1 : 0, qe = qwe < nq ? q_loc(qwe) : (int)len_q;
  int rs = rws ? r_loc(rws - 1) + 1 : 0, re = rwe < nr ? r_loc(rwe) : (int)len_r;
  while (!extend_stops(P, qs, qe, rs, re)) {
    bool extended = false;
    for (int way = 0; way < 3 && !extended; way++) {  // both_both, both_right, both_left
      const bool left = way != 1, right = way != 2;
      if (left && (!qws || !rws)) continue;
      if (right && (rwe >= nr || qwe >= nq)) continue;
      if ((left && (i - qws >= EXT_GROW || rws0 - rws >= EXT_GROW)) || (right && (qwe - (i + nm) >= EXT_GROW || rwe - rwe0 >= EXT_GROW))) {
        wide = true;
        break;
      }
      if (left) {
        add_to_query(--qws), qs = qws ? q_loc(qws - 1) + 1 : 0;
        add_to_reference(--rws), rs = rws ? r_loc(rws - 1) + 1 : 0;
      }
      if (right && !nolimit) {
        add_to_query(qwe++), qe = qwe < nq ? q_loc(qwe) : (int)len_q;
        add_to_reference(rwe++), re = rwe < nr ? r_loc(rwe) : (int)len_r;
      }
      if (nolimit) break;
      if (J() >= 0) {
        extended = true;
        break;
      }
      if (right) {  // the reference's undo: removes in its order, not a restore
        remove_from_reference(--rwe), re = r_loc(rwe);
        remove_from_query(--qwe), qe = q_loc(qwe);
      }
      if (left) {
        rs = r_loc(rws) + 1, remove_from_reference(rws++);
        qs = q_loc(qws) + 1, remove_from_query(qws++);
      }
    }
    if (!extended) break;
  }
  if (lane == 0) {
    if (nolimit) H.flags = SDF_EXTEND_NOLIMIT;
    else if (wide) H.flags = SDF_EXTEND_WIDE;
    else
      H = sdf_search_hit{qs, qe, rs, re, J(), qws, qwe, rws, rwe, 0u};
    out[t] = H;
  }
}

// one lane per hit: its filter task (sdf_search_hit_tasks_device)
__global__ void search_hit_tasks_kernel(const sdf_search_hit *__restrict__ hits, int n, const uint64_t *__restrict__ count, FilterTaskArgs A,
                                        sdf_filter_task *__restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  if (count && (uint64_t)t >= *count) out[t] = sdf_filter_task{0, 0, 0, 0, SDF_FILTER_SKIP, 0};
  else out[t] = hit_task_of(A, hits[t]);
}

}  // namespace sdf

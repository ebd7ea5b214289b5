// Search extend, the long form: the intervals search_extend_kernel flagged SDF_EXTEND_WIDE for their growth, completed on the
// device with a growth cap of long_grow <= SDF_EXTEND_LONG_MAX_GROW records an end (include/sedef_hip.h:
// sdf_search_extend_long_device).  The universe of such an interval does not fit a wavefront's LDS at seven bytes a key, so only
// bits[] -- one byte per DISTINCT key -- stays there; the keys are sorted and turned into slots in HBM, a batch of intervals at
// a time, each batch slot owning a fixed stride of U = SDF_SEARCH_MAX_MEMBERS + SDF_ROLL_MAX_SPAN + 4 * long_grow entries:
//   flag, list  one lane per record: is it a candidate; after an exclusive scan of the flags, the first n_long_max of them in
//               ascending t as {t, window, lo}
//   keys        one lane per universe entry: slot << 33 | pad << 32 | roll_key and the entry's index in its slot as the payload.
//               The universe is the short kernel's with long_grow for EXT_GROW: the query records, then the reference records,
//               then padding (pad = 1: roll_key may be all ones, so no 32-bit value can stand for "unused").  A status-2
//               reference record stands there as the first member's key, its payload marked: no add or remove looks at it
//   (sort)      hipcub::DeviceRadixSort::SortPairs over the batch: every slot's entries stay in its own stride
//   heads       1 where a key differs from its left neighbour or a stride begins; (scan) their inclusive sum
//   slots       the dense slot of an entry -- the sum at it minus the sum at its stride's start, so equal keys of neighbouring
//               strides get slots of their own -- scattered to slots[stride start + payload], 32 bits wide; nd per batch slot
//   walk        search_extend_kernel's walk, one wavefront per batch slot: the same SearchMap, search_roll_walk and
//               extend_stops; the slots and the locs are read from HBM through windows of 64 neighbouring entries that the
//               wavefront keeps in registers (ExtLongView), two per array -- one for either end of a range.
// Nothing here waits for the host: the number of launches and the workspace follow from n_long_max, long_grow and batch alone.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "search_dev.h"

namespace sdf {

namespace {
// Is record t (t < first[nq], t < n_max: the caller's) a candidate; *i its window, *lo the first record of r at or behind its start
__device__ __forceinline__ bool ext_long_candidate(const ExtLongArgs &A, const sdf_search_hit *__restrict__ hits, const uint32_t t, int *i, int *lo) {
  const sdf_search_hit H = hits[t];
  if (H.flags != SDF_EXTEND_WIDE || H.query_end != 0) return false;
  int a = 0, b = A.nq + 1;  // the first x with first[x] > t
  while (a < b) {
    const int mid = a + (b - a) / 2;
    if (A.first[mid] <= (uint64_t)t) a = mid + 1;
    else b = mid;
  }
  int w = a - 1;
  w = w < 0 ? 0 : w > A.nq - 1 ? A.nq - 1 : w;
  const sdf_search_window W = A.windows[w];
  if (W.n_members < 1 || W.n_members > A.nq - w || W.query_size < 0 || W.query_size >= A.n_limit) return false;
  const long long start = A.intervals[t].start;
  a = 0, b = A.nr;  // the first x with r[x].loc >= start
  while (a < b) {
    const int mid = a + (b - a) / 2;
    if ((long long)A.r[mid].loc < start) a = mid + 1;
    else b = mid;
  }
  const sdf_search_roll_rec Roll = A.rolls[t];
  if (extend_skips(Roll, A.filter ? &A.filter[t] : nullptr, a, A.nr) || extend_replay_wide(Roll, W.n_members, a)) return false;
  *i = w, *lo = a;
  return true;
}

// the universe of a taken candidate: q[q0, q1) and r[r0, r1), nqu + nru <= the stride
struct ExtLongGeom {
  int nm, rws0, rwe0, q0, q1, r0, r1, nqu, nru;
};
__device__ __forceinline__ ExtLongGeom ext_long_geom(const ExtLongArgs &A, const ExtLongCand &C) {
  ExtLongGeom G;
  const int i = C.i, grow = A.grow;
  G.nm = A.windows[i].n_members;
  const sdf_search_roll_rec Roll = A.rolls[C.t];
  G.rws0 = Roll.winnow_start, G.rwe0 = Roll.winnow_end;
  G.q0 = i - grow > 0 ? i - grow : 0, G.q1 = A.nq - (i + G.nm) > grow ? i + G.nm + grow : A.nq;
  const int back = G.rws0 - grow < C.lo ? G.rws0 - grow : C.lo;
  G.r0 = back > 0 ? back : 0, G.r1 = A.nr - G.rwe0 > grow ? G.rwe0 + grow : A.nr;
  G.nqu = G.q1 - G.q0, G.nru = G.r1 - G.r0;  // <= MAX_MEMBERS + 2 grow, <= MAX_SPAN + 2 grow: rwe0 - lo <= ROLL_MAX_SPAN
  return G;
}

// Element x of an array in HBM for the whole wavefront: load(y) is element y, y < n.  Every lane holds one of 64 neighbouring
// elements in a register and the wavefront reads the one it wants from there; two such windows, so that the two ends of a
// range, which move apart, do not chase each other out.  x is wave-uniform and at least 0.
template <class Load>
struct ExtLongView {
  Load load;
  int n, lane;
  int b0 = -64, b1 = -64, v0 = 0, v1 = 0, last = 1;
  __device__ __forceinline__ ExtLongView(Load l, int n_, int lane_) : load(l), n(n_), lane(lane_) {}
  __device__ __forceinline__ int operator[](const int x_) {
    const int x = __builtin_amdgcn_readfirstlane(x_), b = x & ~63;
    if (b == b0) {
      last = 0;
      return __builtin_amdgcn_readlane(v0, x & 63);
    }
    if (b == b1) {
      last = 1;
      return __builtin_amdgcn_readlane(v1, x & 63);
    }
    const int y = b + lane, v = y < n ? load(y) : 0;
    if (last) b0 = b, v0 = v, last = 0;
    else b1 = b, v1 = v, last = 1;
    return __builtin_amdgcn_readlane(v, x & 63);
  }
};
template <class Load>
__device__ __forceinline__ ExtLongView<Load> ext_long_view(Load load, int n, int lane) {
  return ExtLongView<Load>(load, n, lane);
}
}  // namespace

// one lane per record and one more: flag[t] = 1 on a candidate, flag[n] = 0 (the scan's total lands there)
__global__ void search_extend_long_flag_kernel(ExtLongArgs A, const sdf_search_hit *__restrict__ hits, int n, uint32_t *__restrict__ flag) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n) return;
  int i, lo;
  flag[t] = t < n && (uint64_t)t < A.first[A.nq] && ext_long_candidate(A, hits, (uint32_t)t, &i, &lo) ? 1u : 0u;
}

// pos: the exclusive scan of flag.  The candidates below n_long_max to list[] in ascending t; meta[0] = how many were taken;
// *left = how many were not
__global__ void search_extend_long_list_kernel(ExtLongArgs A, const sdf_search_hit *__restrict__ hits, const uint32_t *__restrict__ flag,
                                               const uint32_t *__restrict__ pos, int n, uint32_t n_long_max, ExtLongCand *__restrict__ list, uint32_t *__restrict__ meta,
                                               unsigned long long *__restrict__ left) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n) return;
  if (t == n) {
    const uint32_t total = pos[n], taken = total < n_long_max ? total : n_long_max;
    meta[0] = taken;
    if (left) *left = total - taken;
    return;
  }
  if (!flag[t] || pos[t] >= n_long_max) return;
  int i, lo;
  if (ext_long_candidate(A, hits, (uint32_t)t, &i, &lo)) list[pos[t]] = ExtLongCand{(uint32_t)t, i, lo};  // (it is: nothing wrote the hits in between)
}

// grid (the stride in blocks, the batch's slots): entry x of batch slot k, candidate cand_base + k
__global__ void search_extend_long_keys_kernel(ExtLongArgs A, const ExtLongCand *__restrict__ list, const uint32_t *__restrict__ meta,
                                               uint32_t cand_base, unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (x >= A.stride) return;
  const size_t at = (size_t)k * A.stride + x;
  const unsigned long long slot = (unsigned long long)k << kLongSlotShift, pad = 1ull << kLongPadBit;
  const uint32_t c = cand_base + k;
  if (c >= meta[0]) {
    keys[at] = slot | pad, vals[at] = (uint32_t)x;
    return;
  }
  const ExtLongCand C = list[c];
  const ExtLongGeom G = ext_long_geom(A, C);
  uint32_t payload = (uint32_t)x;
  unsigned long long key = slot | pad;
  if (x < G.nqu) {
    key = slot | roll_key(A.q[G.q0 + x]);
  } else if (x < G.nqu + G.nru) {
    const sdf_minimizer M = A.r[G.r0 + (x - G.nqu)];
    if (M.status == 2) key = slot | roll_key(A.q[C.i]), payload |= kLongPayloadNoSlot;
    else key = slot | roll_key(M);
  }
  keys[at] = key, vals[at] = payload;
}

__global__ void search_extend_long_heads_kernel(const unsigned long long *__restrict__ keys, int n, int stride, uint32_t *__restrict__ heads) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  heads[x] = x % stride == 0 || keys[x] != keys[x - 1] ? 1u : 0u;
}

// incl: the inclusive scan of the heads
__global__ void search_extend_long_slots_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                const uint32_t *__restrict__ incl, int n, int stride, uint32_t *__restrict__ slots,
                                                uint32_t *__restrict__ nds) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  const int k = x / stride;
  const size_t base = (size_t)k * stride;
  const unsigned long long pad = 1ull << kLongPadBit;
  if (keys[x] & pad) {  // the padding sorts behind the slot's keys
    if ((size_t)x == base) nds[k] = 0;
    return;
  }
  const uint32_t dense = incl[x] - incl[base], p = vals[x];
  slots[base + (p & ~kLongPayloadNoSlot)] = p & kLongPayloadNoSlot ? kLongNoSlot : dense;
  if ((size_t)x + 1 == base + stride || (keys[x + 1] & pad)) nds[k] = dense + 1;
}

__global__ __launch_bounds__(64) void search_extend_long_kernel(ExtLongArgs A, const ExtLongCand *__restrict__ list, const uint32_t *__restrict__ meta,
                                                                uint32_t cand_base, const uint32_t *__restrict__ slots,
                                                                const uint32_t *__restrict__ nds, long long len_q, long long len_r,
                                                                int init_len, const int32_t *__restrict__ limit, sdf_extend_params P,
                                                                sdf_search_hit *__restrict__ hits, unsigned long long *__restrict__ left) {
  __shared__ uint8_t bits[EXT_LONG_MAX_KEYS];
  const int lane = threadIdx.x, k = blockIdx.x;
  const uint32_t c = cand_base + k;
  if (c >= meta[0]) return;
  const ExtLongCand C = list[c];
  const ExtLongGeom G = ext_long_geom(A, C);
  const sdf_minimizer *__restrict__ q = A.q, *__restrict__ r = A.r;
  const int nq = A.nq, nr = A.nr, n_limit = A.n_limit, grow = A.grow;
  const int i = C.i, lo = C.lo, nm = G.nm, rws0 = G.rws0, rwe0 = G.rwe0, q0 = G.q0, r0 = G.r0, r1 = G.r1;
  const sdf_search_window W = A.windows[i];
  const sdf_search_interval T = A.intervals[C.t];
  const uint32_t *__restrict__ slot_q = slots + (size_t)k * A.stride, *__restrict__ slot_r = slot_q + G.nqu;
  const int nd = (int)nds[k];
  if (nd > EXT_LONG_MAX_KEYS) return;  // (cannot be: nd <= nqu + nru <= the stride)
  for (int x = lane; x < (nd + 3) / 4; x += 64) ((uint32_t *)bits)[x] = 0;
  __syncthreads();
  int B = 0;
  for (int j = lane; j < nm; j += 64) {
    const int sl = (int)slot_q[i - q0 + j];
    bits[sl] = 1;
    B = sl > B ? sl : B;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int other = __shfl_xor(B, o);
    B = other > B ? other : B;
  }
  B = __builtin_amdgcn_readfirstlane(B);
  __syncthreads();
  // the entry state: wave-uniform from here on
  SearchMap S{bits, nd, B, 0};
  search_roll_walk<-1>(S, ext_long_view([=](int y) { return (int)slot_r[lo - r0 + y]; }, r1 - lo, lane),
                       ext_long_view([=](int y) { return (int)r[lo + y].loc; }, r1 - lo, lane), r1 - lo, T.start, T.end, init_len, len_r, lane,
                       [&](long long, long long, int ws, int we) { return ws >= rws0 - lo && we >= rwe0 - lo; });
  auto vslot_q = ext_long_view([=](int y) { return (int)slot_q[y]; }, G.nqu, lane);
  auto vslot_r = ext_long_view([=](int y) { return (int)slot_r[y]; }, G.nru, lane);
  auto vloc_q = ext_long_view([=](int y) { return (int)q[y].loc; }, nq, lane);
  auto vloc_r = ext_long_view([=](int y) { return (int)r[y].loc; }, nr, lane);
  int qsz = W.query_size, L = limit[qsz];
  int qws = i, qwe = i + nm, rws = rws0, rwe = rwe0;
  bool capped = false, nolimit = false;
  auto q_loc = [&](int x) { return vloc_q[x]; };
  auto r_loc = [&](int x) { return vloc_r[x]; };
  auto add_to_query = [&](int x) {
    if (!S.add(vslot_q[x - q0], 1, qsz != 0, lane)) return;
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
    if (!S.remove(vslot_q[x - q0], 1, qsz != 0, lane)) return;
    qsz -= qsz > 0 ? 1 : 0;
    L = limit[qsz];
    if (S.B < 0) return;
    S.I -= S.full(S.B) ? 1 : 0;
    S.B = S.below(S.B, lane);
  };
  auto add_to_reference = [&](int x) {
    const int sl = vslot_r[x - r0];
    if (sl != (int)kLongNoSlot) S.add(sl, 2, qsz != 0, lane);
  };
  auto remove_from_reference = [&](int x) {
    const int sl = vslot_r[x - r0];
    if (sl != (int)kLongNoSlot) S.remove(sl, 2, qsz != 0, lane);
  };
  auto J = [&]() { return S.I >= L ? S.I : S.I - L; };
  int qs = qws ? q_loc(qws - 1) + 1 : 0, qe = qwe < nq ? q_loc(qwe) : (int)len_q;
  int rs = rws ? r_loc(rws - 1) + 1 : 0, re = rwe < nr ? r_loc(rwe) : (int)len_r;
  while (!extend_stops(P, qs, qe, rs, re)) {
    bool extended = false;
    for (int way = 0; way < 3 && !extended; way++) {  // both_both, both_right, both_left
      const bool go_left = way != 1, go_right = way != 2;
      if (go_left && (!qws || !rws)) continue;
      if (go_right && (rwe >= nr || qwe >= nq)) continue;
      if ((go_left && (i - qws >= grow || rws0 - rws >= grow)) || (go_right && (qwe - (i + nm) >= grow || rwe - rwe0 >= grow))) {
        capped = true;
        break;
      }
      if (go_left) {
        add_to_query(--qws), qs = qws ? q_loc(qws - 1) + 1 : 0;
        add_to_reference(--rws), rs = rws ? r_loc(rws - 1) + 1 : 0;
      }
      if (go_right && !nolimit) {
        add_to_query(qwe++), qe = qwe < nq ? q_loc(qwe) : (int)len_q;
        add_to_reference(rwe++), re = rwe < nr ? r_loc(rwe) : (int)len_r;
      }
      if (nolimit) break;
      if (J() >= 0) {
        extended = true;
        break;
      }
      if (go_right) {  // the reference's undo: removes in its order, not a restore
        remove_from_reference(--rwe), re = r_loc(rwe);
        remove_from_query(--qwe), qe = q_loc(qwe);
      }
      if (go_left) {
        rs = r_loc(rws) + 1, remove_from_reference(rws++);
        qs = q_loc(qws) + 1, remove_from_query(qws++);
      }
    }
    if (!extended) break;
  }
  if (lane == 0) {
    if (nolimit) hits[C.t] = sdf_search_hit{0, 0, 0, 0, 0, 0, 0, 0, 0, SDF_EXTEND_WIDE | SDF_EXTEND_NOLIMIT};
    else if (!capped) hits[C.t] = sdf_search_hit{qs, qe, rs, re, J(), qws, qwe, rws, rwe, SDF_EXTEND_WIDE};
    else if (left) atomicAdd(left, 1ull);  // the record stays as it is: zero, WIDE
  }
}

}  // namespace sdf

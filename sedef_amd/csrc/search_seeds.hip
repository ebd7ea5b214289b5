// Search seeding: for every query minimizer i the reference intervals in which the rest of `sedef search` would look -- the
// front half of search() (reference: src/search.cc:395-452) with an EMPTY tree; include/sedef_hip.h states the seven steps.
//
// Once per minimizer (one lane each, not once per window):
//   search_keys_kernel    key(j) = status << 32 | hash and j, for the library's radix sort;
//   search_prev_kernel    from the sorted keys: prev(j), the last minimizer before j with j's key (-1: none).  The distinct keys
//                         of a window [i, e) are the members with prev < i, so query_size is a count, whatever the extent;
//   search_lookup_kernel  the member extent e(i) (locs ascend: an upper bound) and j's group in r_sorted: lower and upper bound
//                         of its key, (start, size), size 0 when j does not seed, the group is absent or at / over the threshold.
// One wavefront per window, LDS only (search_window_kernel<EMIT>: the count pass, stats_cuts_scan_kernel over the counts, the
// emit pass -- the order minimizers.hip and stats_cuts.hip have):
//   counts    query_size, n_gathered (a sum over the members' records), WIDE -> out;
//   gather    the members' group sizes are prefix-summed into offs[] (LDS, 16-bit: at most 4,096 positions), and slot s of the
//             gathered positions finds its member by an upper bound in offs[] -- every lane carries the same load however the
//             sizes are spread.  A loc the same_genome filter removes is stored as the largest key and sorts behind the rest;
//   sort      a bitonic network on all 64 lanes, every compare-exchange ascending (chain.hip's, on 32-bit keys);
//   set       neighbours compared, compacted in place, 64 at a time (a round reads before it writes, and never writes behind
//             what it read);
//   merge     step 6 in closed form.  x and y both rise with a, so last.end is always the y of the LAST PASSING a before, and
//             an a that passes opens an interval exactly when there is no such a or x >= that y: a head flag from a ballot and
//             one LDS read, and a count.  A head writes its interval's start and the END of the interval before it; the last
//             end is the last passing y.  Step 7 can only move a start: with same_genome every candidate is >= qs + init_len,
//             so end = c + 1 lies above it, and x <= y holds by c[b] - c[a] <= init_len -- with an empty tree no interval
//             is ever dropped.
// An emit-pass wavefront whose window has no interval leaves at once.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "search_dev.h"
#include "stats_dev.h"

namespace sdf {

__device__ __forceinline__ unsigned long long search_key(const sdf_minimizer &M) {
  return (unsigned long long)(uint32_t)M.status << 32 | M.hash;
}

__global__ __launch_bounds__(256) void search_keys_kernel(const sdf_minimizer *__restrict__ q, int nq, unsigned long long *__restrict__ keys,
                                                          uint32_t *__restrict__ vals) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  keys[j] = search_key(q[j]);
  vals[j] = (uint32_t)j;
}

// (the sort is stable: equal keys lie in ascending j)
__global__ __launch_bounds__(256) void search_prev_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, int nq,
                                                          SearchLook *__restrict__ look) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nq) return;
  look[vals[p]].prev = p > 0 && keys[p - 1] == keys[p] ? (int32_t)vals[p - 1] : -1;
}

__global__ __launch_bounds__(256) void search_lookup_kernel(const sdf_minimizer *__restrict__ q, int nq, const sdf_minimizer *__restrict__ r,
                                                            int nr, uint32_t r_threshold, int init_len, int uppercase_seeds,
                                                            SearchLook *__restrict__ look) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  const sdf_minimizer M = q[j];
  const long long last = (long long)M.loc + init_len;  // the members of window j: locs <= last
  int lo = j + 1, hi = nq;                              // (j itself is one)
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if ((long long)q[mid].loc <= last) lo = mid + 1;
    else hi = mid;
  }
  look[j].end = lo;
  uint32_t start = 0, size = 0;
  if (!uppercase_seeds || M.status == 0) {
    const unsigned long long key = search_key(M);
    auto bound = [&](bool upper) {  // records with a key below `key` (upper: not above it)
      int a = 0, b = nr;
      while (a < b) {
        const int mid = a + (b - a) / 2;
        const unsigned long long k = search_key(r[mid]);
        if (k < key || (upper && k == key)) a = mid + 1;
        else b = mid;
      }
      return a;
    };
    const int g0 = bound(false), g1 = bound(true);
    if (g1 > g0 && (uint32_t)(g1 - g0) < r_threshold) start = (uint32_t)g0, size = (uint32_t)(g1 - g0);
  }
  look[j].start = start;
  look[j].size = size;
}

// (search_dev.h: a loc as a sort key and back, kSearchGone)
// EMIT false: windows[i] and counts[i] (the window's intervals); true: the intervals, from out[first[i]], none at or behind out[cap].
// FOUND (include/sedef_hip.h, the section of the found records): the visible records that meet the window are staged in LDS
// from the bins the window touches, and a gathered position that one of them covers at its member's loc is dropped like one
// the same_genome filter drops; more than FOUND_MAX of them: SDF_SEARCH_FOUND_WIDE, and the window is left like a WIDE one.
template <bool EMIT, bool FOUND>
__global__ __launch_bounds__(64) void search_window_kernel(const sdf_minimizer *__restrict__ q, int nq, long long len_q,
                                                           const sdf_minimizer *__restrict__ r, const SearchLook *__restrict__ look,
                                                           int init_len, int same_genome, const int32_t *__restrict__ limit, int n_limit,
                                                           sdf_search_window *__restrict__ windows, uint32_t *__restrict__ counts,
                                                           const uint64_t *__restrict__ first, sdf_search_interval *__restrict__ out,
                                                           uint64_t cap, FoundIndex F) {
  __shared__ uint32_t c[SEARCH_MAX_GATHER];
  __shared__ uint16_t offs[SEARCH_MAX_MEMBERS + 1];
  __shared__ sdf_search_found staged[FOUND_MAX];  // (FOUND alone refers to it)
  const int lane = threadIdx.x, i = blockIdx.x;
  uint64_t base = 0;
  if (EMIT) {
    base = first[i];
    if (first[i + 1] == base) return;
  }
  sdf_search_window W;
  W.query_size = W.n_members = W.n_gathered = W.n_candidates = 0, W.flags = 0;
  auto leave = [&](int intervals) {
    if (!EMIT && lane == 0) windows[i] = W, counts[i] = (uint32_t)intervals;
  };
  const long long qs = q[i].loc, floor_loc = qs + init_len;
  if (floor_loc > len_q) {
    W.flags = SDF_SEARCH_SHORT;
    return leave(0);
  }
  // the found records: every bin the window touches, 64 entries a round; a record is kept in the first of them that holds it,
  // so once however many bins it spans, and the COUNT of the kept ones decides FOUND_WIDE
  int n_found = 0;
  if constexpr (FOUND) {
    const uint32_t vis = F.visible[i] < F.nf ? F.visible[i] : F.nf;
    const int b0 = found_bin(qs), b1 = found_bin(floor_loc);
    for (int b = b0; b <= b1; b++) {
      unsigned long long k0 = F.start[b], k1 = F.start[b + 1];
      k1 = k1 < F.cap ? k1 : F.cap;
      for (; k0 < k1; k0 += 64) {
        const unsigned long long k = k0 + lane;
        sdf_search_found R{0, 0, 0, 0};
        bool take = false;
        if (k < k1) {
          const uint32_t id = F.entries[k];
          if (id < vis) {
            R = F.found[id];
            const int rb = found_bin(R.q_start);
            take = found_meets_window(R, qs, init_len) && b == (rb > b0 ? rb : b0);
          }
        }
        const unsigned long long m = __ballot(take);
        const int slot = n_found + __popcll(m & ((1ull << lane) - 1ull));
        if (take && slot < FOUND_MAX) staged[slot] = R;
        n_found += __popcll(m);
      }
    }
  }
  // counts: the members' records, 64 a round
  const int e = look[i].end, nm = e - i;
  long long gathered = 0;  // exact
  int run = 0;             // the same sum, every term and the sum itself held at SEARCH_MAX_GATHER + 1: the prefixes of a window that is not WIDE
  for (int j0 = i; j0 < e; j0 += 64) {
    const int j = j0 + lane;
    SearchLook K;
    K.start = K.size = 0, K.prev = i, K.end = 0;
    if (j < e) K = look[j];
    W.query_size += __popcll(__ballot(K.prev < i));
    long long s = K.size;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    gathered += s;
    const int sz = K.size > (uint32_t)SEARCH_MAX_GATHER ? SEARCH_MAX_GATHER + 1 : (int)K.size;
    const int in = stats_wave_scan(sz);
    if (j < e && nm <= SEARCH_MAX_MEMBERS) offs[j - i] = (uint16_t)(run + in - sz);  // (16 bits hold it unless the window is WIDE)
    run += __builtin_amdgcn_readlane(in, 63);
    run = run > SEARCH_MAX_GATHER ? SEARCH_MAX_GATHER + 1 : run;
  }
  W.n_members = nm;
  W.n_gathered = gathered > 0x7fffffffll ? 0x7fffffff : (int)gathered;
  if (nm > SEARCH_MAX_MEMBERS || gathered > SEARCH_MAX_GATHER) {
    W.flags = SDF_SEARCH_WIDE;
    if (W.query_size >= n_limit) W.flags |= SDF_SEARCH_NOLIMIT;
    if constexpr (FOUND) W.flags |= n_found > FOUND_MAX ? SDF_SEARCH_FOUND_WIDE : 0;
    return leave(0);
  }
  if constexpr (FOUND) {
    if (n_found > FOUND_MAX) {
      W.flags = SDF_SEARCH_FOUND_WIDE;
      if (W.query_size >= n_limit) W.flags |= SDF_SEARCH_NOLIMIT;
      return leave(0);
    }
  }
  const int ng = (int)gathered;
  __syncthreads();
  // gather: slot s belongs to the last member whose offset is <= s (a member without records shares its successor's offset)
  int gone = 0;
  for (int s = lane; s < ng; s += 64) {
    int lo = 0, hi = nm;  // the first member with offs > s lies in (lo, hi]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if ((int)offs[mid] <= s) lo = mid;
      else hi = mid;
    }
    const int loc = r[(long long)look[i + lo].start + (s - (int)offs[lo])].loc;
    bool keep = !same_genome || (long long)loc >= floor_loc;
    if constexpr (FOUND) {
      const long long at = q[i + lo].loc;  // the member's loc
      for (int f = 0; keep && f < n_found; f++) keep = !found_covers(staged[f], at, loc);
    }
    c[s] = keep ? search_loc_key(loc) : kSearchGone;
    gone += keep ? 0 : 1;
  }
  gone = stats_wave_sum(gone);
  __syncthreads();
  search_sort_u32(c, ng, lane);
  // the set: distinct keys to the front
  const int nv = ng - gone;
  const int nc = search_compact_u32(c, nv, lane);
  W.n_candidates = nc;
  if (W.query_size >= n_limit) {
    W.flags = SDF_SEARCH_NOLIMIT;
    return leave(0);
  }
  int L = limit[W.query_size];
  L = L < 1 ? 1 : L;
  // the merge: heads among the a that pass
  int heads = 0;
  bool any_pass = false;
  long long last_y = 0;  // y of the last a that passed in the rounds before
  for (int a0 = 0; a0 <= nc - L; a0 += 64) {
    const int a = a0 + lane;
    const bool valid = a <= nc - L;
    const long long ca = valid ? search_key_loc(c[a]) : 0, cb = valid ? search_key_loc(c[a + L - 1]) : 0;
    const bool pass = valid && cb - ca <= init_len;
    const unsigned long long m = __ballot(pass), below = m & ((1ull << lane) - 1ull);
    const long long y_before = below ? search_key_loc(c[a0 + 63 - __clzll(below)]) + 1 : last_y;
    const long long x = cb - init_len + 1 > 0 ? cb - init_len + 1 : 0;
    const bool head = pass && (!(below || any_pass) || x >= y_before);
    const unsigned long long hm = __ballot(head);
    if (EMIT && head) {
      const uint64_t k = base + (uint64_t)(heads + __popcll(hm & ((1ull << lane) - 1ull)));
      const long long start = same_genome && x < floor_loc ? floor_loc : x;
      if (k < cap) out[k].start = (int32_t)start;
      if (k > base && k - 1 < cap) out[k - 1].end = (int32_t)y_before;
    }
    heads += __popcll(hm);
    if (m) any_pass = true, last_y = search_key_loc(c[a0 + 63 - __clzll(m)]) + 1;
  }
  if (EMIT && lane == 0 && heads > 0 && base + (uint64_t)heads - 1 < cap) out[base + (uint64_t)heads - 1].end = (int32_t)last_y;
  leave(heads);
}

#define SDF_SEARCH_WINDOW_KERNEL(EMIT, FOUND)                                                                                            \
  template __global__ void search_window_kernel<EMIT, FOUND>(const sdf_minimizer *, int, long long, const sdf_minimizer *, const SearchLook *, \
                                                             int, int, const int32_t *, int, sdf_search_window *, uint32_t *,               \
                                                             const uint64_t *, sdf_search_interval *, uint64_t, FoundIndex);
SDF_SEARCH_WINDOW_KERNEL(false, false)
SDF_SEARCH_WINDOW_KERNEL(true, false)
SDF_SEARCH_WINDOW_KERNEL(false, true)
SDF_SEARCH_WINDOW_KERNEL(true, true)
#undef SDF_SEARCH_WINDOW_KERNEL

}  // namespace sdf

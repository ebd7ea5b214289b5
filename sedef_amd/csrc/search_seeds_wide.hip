// Search seeding, the windows search_window_kernel (search_seeds.hip) flags and leaves: SDF_SEARCH_WIDE for more than
// SEARCH_MAX_GATHER gathered positions, SDF_SEARCH_FOUND_WIDE for more than FOUND_MAX found records that meet the window.  Both
// limits are that kernel's LDS layout, one wavefront and 16 KiB; here ONE WORKGROUP of SEARCH_WIDE_THREADS = 256 lanes takes a
// window, with 32-bit keys for SEARCH_WIDE_MAX_GATHER = 32,768 positions (128 KiB), 32-bit offsets for the members and one chunk
// of SEARCH_WIDE_CHUNK found records: one workgroup on a CU, for windows that are the exception.  include/sedef_hip.h states the
// record a completed window gets (SDF_SEARCH_WIDE_DONE).
//
//   search_wide_list_kernel   after the count pass: the eligible windows (search_wide_eligible, sdf_kernels.h) in ascending
//                             order, the lowest n_wide_max of them, and their number: one workgroup, an ordered compaction --
//                             which windows stay behind does not depend on the order the lanes ran in;
//   search_window_wide_kernel<EMIT, FOUND>   workgroup b takes window wide[b]; the seven steps of search_window_kernel in its order:
//     counts   query_size and n_gathered: a sum per lane, 64 bits for the positions, added up over the workgroup; the members'
//              group sizes prefix-summed into offs[] (search_wg_scan: DPP inside a wavefront, the wavefronts' totals through LDS);
//     gather   slot s finds its member by an upper bound in offs[]; a loc the same_genome floor removes is stored as the
//              largest key (kSearchGone) and counted;
//     found    NOT capped: the records that meet the window are walked out of the bins 256 entries a round and compacted into
//              staged[]; whenever the next round's records would not fit, every gathered slot that is still there is tested
//              against the staged chunk (its member found again by the upper bound: the slots have no room for it), and the
//              chunk starts anew.  A position is dropped when ANY record covers it, so the chunks' order does not matter; a
//              dropped slot becomes kSearchGone and is counted once (a kept key equal to kSearchGone is the loc 2^31 - 1, which
//              no record covers: r_end is at most that);
//     sort     search_sort_u32_wg: search_sort_u32's network, 256 compare-exchanges a step;
//     set      search_compact_u32_wg: 256 keys a round, their places by search_wg_scan;
//     merge    the closed form of search_seeds.hip, 256 values of a a round.  An a that passes needs the y of the LAST PASSING a
//              before it.  Inside a wavefront that is the ballot's highest bit below the lane; ACROSS WAVEFRONTS every wavefront
//              publishes the index of its last passing a of the round in LDS (wl[], -1: none) and a lane without a
//              predecessor in its own wavefront takes the nearest earlier wavefront's that has one; ACROSS ROUNDS every lane
//              carries `last`, the index of the last passing a of all rounds before, taken from wl[] at the end of a round.  The
//              carry is an INDEX into c[], which the merge only reads: y = c[index] + 1 at any later time.  The heads' places
//              are an exclusive sum over the workgroup.
// EMIT false rewrites windows[i] and counts[i] of its window (in front of stats_cuts_scan_kernel), EMIT true writes its intervals
// from out[first[i]], none at or behind out[cap].  A window that is not what the list promises -- it never is -- is left as
// the plain kernel wrote it.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "search_dev.h"
#include "stats_dev.h"

namespace sdf {

__global__ __launch_bounds__(1024) void search_wide_list_kernel(const sdf_search_window *__restrict__ windows, int nq, uint32_t n_wide_max,
                                                                uint32_t *__restrict__ wide, unsigned long long *__restrict__ total,
                                                                unsigned long long *__restrict__ total_out) {
  __shared__ int ws[16];
  const int tid = threadIdx.x;
  unsigned long long count = 0;  // the eligible windows before this round
  for (int i0 = 0; i0 < nq; i0 += 1024) {
    const int i = i0 + tid;
    const bool mine = i < nq && search_wide_eligible(windows[i]);
    int all;
    const int at = search_wg_scan(mine ? 1 : 0, &all, ws, tid, 1024);
    if (mine && count + (unsigned long long)at < n_wide_max) wide[count + (unsigned long long)at] = (uint32_t)i;
    count += (unsigned long long)all;
  }
  if (tid == 0) {
    *total = count;
    if (total_out) *total_out = count;
  }
}

template <bool EMIT, bool FOUND>
__global__ __launch_bounds__(SEARCH_WIDE_THREADS) void search_window_wide_kernel(
    const sdf_minimizer *__restrict__ q, int nq, long long len_q, const sdf_minimizer *__restrict__ r, const SearchLook *__restrict__ look,
    int init_len, int same_genome, const int32_t *__restrict__ limit, int n_limit, sdf_search_window *__restrict__ windows,
    uint32_t *__restrict__ counts, const uint64_t *__restrict__ first, sdf_search_interval *__restrict__ out, uint64_t cap, FoundIndex F,
    const uint32_t *__restrict__ wide, const unsigned long long *__restrict__ n_wide, uint32_t n_wide_max) {
  constexpr int NT = SEARCH_WIDE_THREADS, NW = NT / 64;
  __shared__ uint32_t c[SEARCH_WIDE_MAX_GATHER];
  __shared__ uint32_t offs[SEARCH_MAX_MEMBERS + 1];
  __shared__ sdf_search_found staged[SEARCH_WIDE_CHUNK];  // (FOUND alone refers to it)
  __shared__ long long ws64[NW];
  __shared__ int ws[NW], wl[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long listed = *n_wide < n_wide_max ? *n_wide : (unsigned long long)n_wide_max;
  if (blockIdx.x >= listed) return;
  const int i = (int)wide[blockIdx.x];
  if (i < 0 || i >= nq) return;
  uint64_t base = 0;
  if (EMIT) {
    base = first[i];
    if (first[i + 1] == base) return;
  }
  const long long qs = q[i].loc, floor_loc = qs + init_len;
  const int e = look[i].end, nm = e - i;
  if (floor_loc > len_q || nm < 1 || nm > SEARCH_MAX_MEMBERS) return;
  // counts: the members' records, 256 a round
  sdf_search_window W;
  long long my_gathered = 0;
  int my_distinct = 0, run = 0;  // run: the sizes before this round, every term and the sum held at SEARCH_WIDE_MAX_GATHER + 1
  for (int j0 = i; j0 < e; j0 += NT) {
    const int j = j0 + tid;
    SearchLook K;
    K.start = K.size = 0, K.prev = i, K.end = 0;
    if (j < e) K = look[j];
    my_distinct += K.prev < i ? 1 : 0;
    my_gathered += (long long)K.size;
    const int sz = K.size > (uint32_t)SEARCH_WIDE_MAX_GATHER ? SEARCH_WIDE_MAX_GATHER + 1 : (int)K.size;
    int all;
    const int before = run + search_wg_scan(sz, &all, ws, tid, NT);
    if (j < e) offs[j - i] = (uint32_t)(before > SEARCH_WIDE_MAX_GATHER ? SEARCH_WIDE_MAX_GATHER + 1 : before);
    run = run + all > SEARCH_WIDE_MAX_GATHER ? SEARCH_WIDE_MAX_GATHER + 1 : run + all;
  }
  int distinct;
  (void)search_wg_scan(my_distinct, &distinct, ws, tid, NT);
  const long long gathered = search_wg_sum64(my_gathered, ws64, tid, NT);
  if (gathered > SEARCH_WIDE_MAX_GATHER || distinct >= n_limit) return;
  W.query_size = distinct, W.n_members = nm, W.n_gathered = (int)gathered, W.n_candidates = 0, W.flags = SDF_SEARCH_WIDE_DONE;
  const int ng = (int)gathered;
  __syncthreads();
  // slot s belongs to the last member whose offset is <= s (a member without records shares its successor's offset)
  auto member_of = [&](const int s) {
    int lo = 0, hi = nm;  // the first member with offs > s lies in (lo, hi]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if ((int)offs[mid] <= s) lo = mid;
      else hi = mid;
    }
    return lo;
  };
  int gone = 0;
  for (int s = tid; s < ng; s += NT) {
    const int lo = member_of(s);
    const int loc = r[(long long)look[i + lo].start + (s - (int)offs[lo])].loc;
    const bool keep = !same_genome || (long long)loc >= floor_loc;
    c[s] = keep ? search_loc_key(loc) : kSearchGone;
    gone += keep ? 0 : 1;
  }
  if constexpr (FOUND) {
    // the staged chunk against every slot that is still there (a lane tests the slots it gathered: tid, tid + 256, ...)
    auto apply = [&](const int n) {
      __syncthreads();
      for (int s = tid; s < ng; s += NT) {
        const uint32_t key = c[s];
        if (key == kSearchGone) continue;
        const long long at = q[i + member_of(s)].loc, pos = search_key_loc(key);
        bool covered = false;
        for (int f = 0; !covered && f < n; f++) covered = found_covers(staged[f], at, pos);
        if (covered) c[s] = kSearchGone, gone += 1;
      }
      __syncthreads();
    };
    const uint32_t vis = F.visible[i] < F.nf ? F.visible[i] : F.nf;
    const int b0 = found_bin(qs), b1 = found_bin(floor_loc);
    int n_staged = 0;
    for (int b = b0; b <= b1; b++) {
      unsigned long long k0 = F.start[b], k1 = F.start[b + 1];
      k1 = k1 < F.cap ? k1 : F.cap;
      for (; k0 < k1; k0 += NT) {
        const unsigned long long k = k0 + (unsigned long long)tid;
        sdf_search_found R{0, 0, 0, 0};
        bool take = false;
        if (k < k1) {
          const uint32_t id = F.entries[k];
          if (id < vis) {
            R = F.found[id];
            const int rb = found_bin(R.q_start);
            take = found_meets_window(R, qs, init_len) && b == (rb > b0 ? rb : b0);  // (kept in the first bin of the window that holds it)
          }
        }
        int all;
        const int at = search_wg_scan(take ? 1 : 0, &all, ws, tid, NT);
        if (n_staged + all > SEARCH_WIDE_CHUNK) {
          apply(n_staged);
          n_staged = 0;
        }
        if (take) staged[n_staged + at] = R;
        n_staged += all;
      }
    }
    if (n_staged) apply(n_staged);
  }
  int gone_all;
  (void)search_wg_scan(gone, &gone_all, ws, tid, NT);  // (its barriers stand between the slots' last writes and the sort)
  search_sort_u32_wg(c, ng, tid, NT);
  // the set: distinct keys to the front
  const int nc = search_compact_u32_wg(c, ng - gone_all, ws, tid, NT);
  W.n_candidates = nc;
  int L = limit[W.query_size];
  L = L < 1 ? 1 : L;
  // the merge: heads among the a that pass
  int heads = 0, last = -1;  // last: the last a that passed in the rounds before
  for (int a0 = 0; a0 <= nc - L; a0 += NT) {
    const int a = a0 + tid;
    const bool valid = a <= nc - L;
    const long long ca = valid ? search_key_loc(c[a]) : 0, cb = valid ? search_key_loc(c[a + L - 1]) : 0;
    const bool pass = valid && cb - ca <= init_len;
    const unsigned long long m = __ballot(pass), below = m & ((1ull << lane) - 1ull);
    __syncthreads();  // (the round before has read wl[])
    if (lane == 0) wl[wave] = m ? a + 63 - __clzll(m) : -1;
    __syncthreads();
    int prev = below ? a - lane + 63 - __clzll(below) : -1;
    for (int v = wave - 1; prev < 0 && v >= 0; v--) prev = wl[v];
    prev = prev < 0 ? last : prev;
    const long long y_before = prev >= 0 ? search_key_loc(c[prev]) + 1 : 0;
    const long long x = cb - init_len + 1 > 0 ? cb - init_len + 1 : 0;
    const bool head = pass && (prev < 0 || x >= y_before);
    int all;
    const int at = search_wg_scan(head ? 1 : 0, &all, ws, tid, NT);
    if (EMIT && head) {
      const uint64_t k = base + (uint64_t)(heads + at);
      const long long start = same_genome && x < floor_loc ? floor_loc : x;
      if (k < cap) out[k].start = (int32_t)start;
      if (k > base && k - 1 < cap) out[k - 1].end = (int32_t)y_before;
    }
    heads += all;
    for (int v = NW - 1; v >= 0; v--)
      if (wl[v] >= 0) {
        last = wl[v];
        break;
      }
  }
  if (EMIT && tid == 0 && heads > 0 && base + (uint64_t)heads - 1 < cap) out[base + (uint64_t)heads - 1].end = (int32_t)(search_key_loc(c[last]) + 1);
  if (!EMIT && tid == 0) windows[i] = W, counts[i] = (uint32_t)heads;
}

#define SDF_SEARCH_WINDOW_WIDE_KERNEL(EMIT, FOUND)                                                                                       \
  template __global__ void search_window_wide_kernel<EMIT, FOUND>(const sdf_minimizer *, int, long long, const sdf_minimizer *,           \
                                                                  const SearchLook *, int, int, const int32_t *, int, sdf_search_window *, \
                                                                  uint32_t *, const uint64_t *, sdf_search_interval *, uint64_t, FoundIndex, \
                                                                  const uint32_t *, const unsigned long long *, uint32_t);
SDF_SEARCH_WINDOW_WIDE_KERNEL(false, false)
SDF_SEARCH_WINDOW_WIDE_KERNEL(true, false)
SDF_SEARCH_WINDOW_WIDE_KERNEL(false, true)
SDF_SEARCH_WINDOW_WIDE_KERNEL(true, true)
#undef SDF_SEARCH_WINDOW_WIDE_KERNEL

}  // namespace sdf

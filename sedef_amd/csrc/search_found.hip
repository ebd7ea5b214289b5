// Search against the SDs already found: the two places where the reference reads its tree (src/search.cc:420-434 and
// is_overlap, :35-71), against an explicit list of found records; include/sedef_hip.h states the rules.
//
// The bin index over the query axis, rebuilt by every call (bin of a base: base >> FOUND_BIN_SHIFT, FOUND_BINS bins):
//   found_count_kernel   one lane per record, one atomic add per bin that [q_start, q_end) touches (none for an empty record);
//   the library's exclusive sum over the bins' counts: start[0 .. FOUND_BINS], start[FOUND_BINS] the entries of the list;
//   found_fill_kernel    one lane per record again: the counts serve as cursors, counted down, so a bin is filled from its end;
//                        an entry at or behind `cap` is not written, and lane 0 leaves the need in *need.
// The order inside a bin does not matter: every use is an existence test or a count of distinct records.
// search_window_kernel<.., true> (search_seeds.hip) reads the index for the exclusions;
//   search_overlap_kernel  one lane per rolled interval: its window by the binary search over first[] that
//                          search_filter_tasks_kernel uses, the one bin of q[i].loc, rules 1 to 5 on the entries below the
//                          interval's prefix; the verdict, and the skip task where it is 1 and the caller gave the tasks.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

__global__ __launch_bounds__(256) void found_count_kernel(const sdf_search_found *__restrict__ found, int nf,
                                                          unsigned long long *__restrict__ counts) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= nf) return;
  const sdf_search_found R = found[id];
  if (found_empty(R)) return;
  for (int b = found_bin(R.q_start), b1 = found_bin((long long)R.q_end - 1); b <= b1; b++) atomicAdd(&counts[b], 1ull);
}

__global__ __launch_bounds__(256) void found_fill_kernel(const sdf_search_found *__restrict__ found, int nf,
                                                         const unsigned long long *__restrict__ start, unsigned long long *__restrict__ cursors,
                                                         uint32_t *__restrict__ entries, unsigned long long cap,
                                                         unsigned long long *__restrict__ need) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id == 0 && need) *need = start[FOUND_BINS];
  if (id >= nf) return;
  const sdf_search_found R = found[id];
  if (found_empty(R)) return;
  for (int b = found_bin(R.q_start), b1 = found_bin((long long)R.q_end - 1); b <= b1; b++) {
    const unsigned long long at = start[b] + atomicAdd(&cursors[b], ~0ull) - 1ull;  // (the count before, counted down)
    if (at < cap) entries[at] = (uint32_t)id;
  }
}

__global__ __launch_bounds__(256) void search_overlap_kernel(const sdf_minimizer *__restrict__ q, int nq, const uint64_t *__restrict__ first,
                                                             const sdf_search_roll_rec *__restrict__ rolls, int n_max, FoundIndex F, int init_len,
                                                             int min_read_size, uint32_t *__restrict__ out, sdf_filter_task *__restrict__ tasks) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_max) return;
  if ((uint64_t)t >= first[nq]) {
    out[t] = 0;
    return;
  }
  int lo = 0, hi = nq;  // the last i in [0, nq) with first[i] <= t
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (first[mid] <= (uint64_t)t) lo = mid;
    else hi = mid;
  }
  const long long pf_pos = q[lo].loc, pf_end = pf_pos + init_len, pfp_pos = rolls[t].ref_start, pfp_end = rolls[t].ref_end;
  const uint32_t vis = F.visible[t] < F.nf ? F.visible[t] : F.nf;
  const int b = found_bin(pf_pos);
  unsigned long long k = F.start[b], k1 = F.start[b + 1];
  k1 = k1 < F.cap ? k1 : F.cap;
  bool hit = false;
  for (; k < k1 && !hit; k++) {
    const uint32_t id = F.entries[k];
    if (id >= vis) continue;
    const sdf_search_found R = F.found[id];
    hit = !found_empty(R) && found_covers(R, pf_pos, pfp_pos) && found_overlaps(R, pf_pos, pf_end, pfp_pos, pfp_end, min_read_size);
  }
  out[t] = hit ? 1u : 0u;
  if (hit && tasks) tasks[t] = sdf_filter_task{0, 0, 0, 0, SDF_FILTER_SKIP, 0};
}

}  // namespace sdf

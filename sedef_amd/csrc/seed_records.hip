// Search hits to seed records (include/sedef_hip.h: sdf_seed_records): what `sedef search` prints as a BED line and `align bucket`
// reads back through Hit::from_bed, as one 32-byte record per hit and without the text.
//
// A hit carries coordinates only; the chromosomes, the reference's length and the strand belong to its JOB (a chromosome pair
// of sdf_search_pairs_indexed), and the hits of job j are [first[j], first[j + 1]).  A lane takes hit t and finds its job by a
// binary search of first[] (seed_job_of, sdf_kernels.h: ceil(log2(n_jobs)) loads of a table every lane of the launch reads, so
// it stays in the cache), then applies seed_record -- the rule the host form applies too.  24 bytes read and 32 written a hit:
// the launch is bound by its traffic and by nothing else.  No LDS, no scratch, no atomics.  NOT MEASURED on its own.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

__global__ __launch_bounds__(256) void seed_records_kernel(const sdf_search_pair_hit *__restrict__ hits, const uint32_t n,
                                                           const uint64_t *__restrict__ first, const sdf_seed_job *__restrict__ jobs,
                                                           const size_t n_jobs, sdf_seed_hit *__restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // (n <= 2^30: the launch's lanes fit 32 bits)
  if (t >= n) return;
  const sdf_seed_job job = jobs[seed_job_of(first, n_jobs, t)];
  out[t] = seed_record(hits[t], job);  // (eight words, from vector registers)
}

}  // namespace sdf

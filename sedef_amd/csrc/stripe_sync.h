// What the wavefronts of a multi-wavefront task say to each other through HBM (stripes, banded stripes, chained strips):
// the exchanged words' memory order, giving a task up, taking a launch-order entry, and the placement probe.
#pragma once
#include <hip/hip_runtime.h>

#include "extz2_geom.h"

namespace sdf {

// The words stripes exchange: relaxed atomics of agent scope -- coherent across the XCDs' L2 caches, so that the protocol
// does not depend on a task's stripes sharing an XCD (that is a matter of speed: then the words stay in its L2).
template <typename T>
__device__ __forceinline__ T ld_agent(const T *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void st_agent(T *p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wait gives up after `spin_cap` polls (context field, SDF_STRIPE_SPIN_CAP in the environment of sdf_create; 2^24 by
// default: seconds).  With claimed entries (stripe_claim below) a stripe's left neighbour has always been taken by a
// workgroup that is running or done; taken by index (SDF_STRIPE_CLAIM=0, or a launch without counters) the protocol's forward
// progress rests on the dispatch order, which a part with another XCD count, or other launches holding the wavefront slots,
// may not honour -- and a wavefront preempted for good would stall its right neighbours either way.  The
// wavefront then marks its TASK as abandoned (n_cigar = -1 in the task's result record, which nothing else touches before
// the traceback; the task's index is appended to the list behind the give-up counter, once per task) and ends; the other
// stripes of the task see the mark within 64 polls and end too.  The batch call re-runs abandoned tasks on the
// one-wavefront / one-workgroup kernels (sdf_launch.hip: rerun_abandoned).
__device__ __forceinline__ void stripe_abandon(unsigned long long *gave_up, sdf_result *rec, int out_idx, int lane) {
  if (lane != 0) return;
  const int old = __hip_atomic_exchange(&rec->n_cigar, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old == -1) return;
  const unsigned long long slot = atomicAdd(gave_up, 1ull);
  if (slot < SDF_GAVEUP_CAP) reinterpret_cast<uint32_t *>(gave_up + SDF_GAVEUP_LIST)[slot] = (uint32_t)out_idx;
}
__device__ __forceinline__ bool stripe_abandoned(const sdf_result *rec) {
  return __builtin_amdgcn_readfirstlane(__hip_atomic_load(&rec->n_cigar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == -1;
}

// A workgroup's entry of the launch order.  The planner deals a launch's tasks to eight lists -- order[8 p + q] is entry p of
// list q -- so that the stripes of a task share an XCD's L2 (their edge words) and every stripe's left neighbour stands
// earlier in its list.  With `claim` (eight counters, zero at launch) a workgroup TAKES the next entry of the list of the
// XCD it finds itself on (HW_REG_XCC_ID), or of the next list that has one left: whatever the dispatcher does -- other
// launches' workgroups in between, another start XCD --, a task's stripes meet in one L2, and the neighbour a stripe waits
// for has been taken before it, by a workgroup that is running or done (forward progress no longer rests on the dispatch
// order).  Without `claim`: entry blockIdx.x, which is the same thing when workgroup i lands on XCD i mod 8.
// Debug (sdf_debug_placement): wavefronts started per (XCD, shader engine, CU, SIMD) by the kernels that call place_note().
// (What it showed, profiles/placement_probe.py: the 5,600 chain wavefronts of the hg19 mixture's heavy chunk land 4..7 to a SIMD
// -- mean 5.5 --, and a chain runs at the pace of its slowest block.  Workgroups of four wavefronts, one per SIMD of a CU, were
// tried against it: the dispatcher spreads them LESS evenly over the CUs, 35..56 per CU against 40..50, and the batch took
// 15.5 instead of 14.3-14.7 ms.)
extern __device__ unsigned *g_place;  // (one definition: extz2_stripe.hip)
__device__ __forceinline__ void place_note() {
  unsigned *p = g_place;
  if (p && threadIdx.x == 0) {
    const unsigned hw = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_HW_ID: SIMD 5:4, CU 11:8, SE 15:13
    const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;
    atomicAdd(p + ((xcc << 9) | (((hw >> 13) & 7u) << 6) | (((hw >> 8) & 15u) << 2) | ((hw >> 4) & 3u)), 1u);
  }
}

__device__ __forceinline__ int32_t stripe_claim(const int32_t *__restrict__ order, unsigned *__restrict__ claim) {
  if (!claim) return order[blockIdx.x];
  int32_t entry = (int32_t)(255u << 24);  // (idle)
  if (threadIdx.x == 0) {
    const unsigned per_list = gridDim.x / 8;
    const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;  // HW_REG_XCC_ID, bits 3:0
    for (unsigned a = 0; a < 8; ++a) {
      const unsigned q = (xcc + a) & 7u;
      const unsigned p = atomicAdd(&claim[q], 1u);
      if (p < per_list) {
        entry = order[8 * p + q];
        break;
      }
    }
  }
  return __builtin_amdgcn_readfirstlane(entry);  // (one-wavefront workgroups)
}

}  // namespace sdf

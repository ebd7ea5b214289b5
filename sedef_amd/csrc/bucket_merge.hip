// `sedef align bucket` on records (include/sedef_hip.h: sdf_bucket_merge): seed hits extended, sorted, merged, dealt.
//
// The reference (bucket_alignments_extern, src/align_main.cc:38-198; merge(), src/merge.cc:35-109) sorts the hits of a pair of
// chromosome groups and sweeps them one after the other, keeping the current run's survivors in a multimap by reference end.
// Three things make all of it but one loop free of a sequential dependency; the entry points (sdf_bucket_api.hip) rely on them,
// and tests/bucket_model.py states the sweep literally and in this closed form and compares the two:
//
//   RUNS.  The sweep opens a run on `last.query_end + merge_dist < h.query_start`, where `last` is the hit before with its
//   query end raised to that of everything before it in the run: a running maximum of query ends that are themselves maxima of
//   ORIGINAL (extended) query ends of the same run -- and a run only opens when the hit starts beyond that maximum, so nothing
//   of an earlier run is ever part of it.  The test is a prefix maximum of the original query ends over the non-self hits that
//   share (pair of groups, strand, names): one segmented max-scan (bucket_runs_kernel, bucket_new_run_kernel), then a sum.
//
//   ABSORPTION IS ORDER-FREE.  A window's multimap key is its own ref_end, so the lower_bound cut is the second clause of
//   bucket_apart again; each of the three clauses only turns false as the hit grows.  What a hit swallows is therefore the least
//   fixed point of "absorb every window that is not apart from the growing box", whatever order the windows are visited in:
//   64 lanes test 64 windows at once (bucket_sweep_kernel).
//
//   TIES AND THE FLUSH.  Two hits of equal sort key are never apart (each holds the other's starts), so they always merge and
//   the closure is the same whichever comes first; a stable radix sort may stand for the reference's std::sort wherever the
//   hits carry nothing but coordinates (seeds as `sedef search` writes them).  The multimap orders by ref_end with equal keys
//   in insertion order, a window's insertion order is its hit's place in the sort: the survivors leave in a stable sort by
//   (run, ref_end) of the slots (bucket_flush_keys_kernel).
//
// The deal needs no counter: a hit's bucket is (first bucket of its class + its rank within the class) % nbins, the first
// bucket of a class is (hits of the classes below) % nbins, and the two add up to the hit's place in a stable sort by class,
// modulo nbins (bucket_class_kernel, bucket_deal_kernel).
//
// Slots.  Slot i is hit i of the sort: its box (BucketBox) and a live word.  Self hits and the records the device form drops
// hold dead slots from the start; a hit that is swallowed dies; what is live at the end leaves.  Every array is indexed by
// lanes below n, the sweep reads and writes [run start, run end) of its own run only.
//
// bucket_sweep_kernel costs a run of m hits about m^2 / 128 steps of 64 window tests on ONE wavefront, dead slots included (no
// compaction within a run), each pass again while the hit grows: NOT MEASURED beyond profiles/bucket_merge.txt.  No LDS,
// no scratch.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

constexpr unsigned long long kBucketDeadKey = ~0ull;  // flush key of a slot that does not leave: behind every (run, ref_end)

// ---- a. a lane a seed: checks, Hit::extend, order_sides, the self flag, the two sort keys ----
__global__ __launch_bounds__(256) void bucket_prepare_kernel(const sdf_seed_hit *__restrict__ hits, const int n,
                                                             const int32_t *__restrict__ chr_group, const int n_chr,
                                                             const int32_t *__restrict__ group_pair_order, const int n_groups,
                                                             const double extend_ratio, const int max_extend, const int merge_dist,
                                                             BucketRec *__restrict__ recs, unsigned long long *__restrict__ key_lo,
                                                             unsigned long long *__restrict__ key_hi, uint32_t *__restrict__ place,
                                                             unsigned long long *__restrict__ n_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  BucketRec r = bucket_prepare(hits[i], chr_group, n_chr, group_pair_order, n_groups, extend_ratio, max_extend, merge_dist);
  if (r.flags & kBucketBad) {
    r = BucketRec{0, 0, 0, 0, 0, 0, kBucketBad, 0};  // (sorts in front of everything; its slot is dead)
    atomicAdd(n_out + 1, 1ull);
  }
  recs[i] = r;
  key_lo[i] = bucket_key_lo(r);
  key_hi[i] = bucket_key_hi(r);
  place[i] = (uint32_t)i;
}

// between the two sorts: key_hi in the order the first sort left
__global__ __launch_bounds__(256) void bucket_key_gather_kernel(const unsigned long long *__restrict__ key_hi,
                                                                const uint32_t *__restrict__ place, const int n,
                                                                unsigned long long *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = key_hi[place[i]];
}

// ---- c. the records in sorted order and the items of the segmented max-scan: segments are equal key_hi, values the
// extended query ends of the hits that take part ----
__global__ __launch_bounds__(256) void bucket_runs_kernel(const BucketRec *__restrict__ recs, const uint32_t *__restrict__ place,
                                                          const unsigned long long *__restrict__ key_hi, const int n,
                                                          BucketRec *__restrict__ sorted, BucketSeg *__restrict__ seg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const BucketRec r = recs[place[i]];
  sorted[i] = r;
  const bool dead = r.flags & (kBucketSelf | kBucketBad);
  seg[i] = BucketSeg{i == 0 || key_hi[i] != key_hi[i - 1], dead ? (int32_t)0x80000000 : r.q_end};
}

// behind the scan: new_run[0 .. n] (entry n: 0, the end of the sum), and every slot as the sweep finds it
__global__ __launch_bounds__(256) void bucket_new_run_kernel(const BucketRec *__restrict__ sorted, const BucketSeg *__restrict__ scan,
                                                             const int n, const int merge_dist, uint32_t *__restrict__ new_run,
                                                             BucketBox *__restrict__ box, uint32_t *__restrict__ live) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    new_run[n] = 0;
    return;
  }
  const BucketRec r = sorted[i];
  const bool dead = r.flags & (kBucketSelf | kBucketBad);
  const bool head = i == 0 || bucket_key_hi(r) != bucket_key_hi(sorted[i - 1]);
  // (the value of a dead hit is INT_MIN: behind nothing but dead hits every start lies beyond it)
  new_run[i] = !dead && (head || (long long)scan[i - 1].val + merge_dist < r.q_start);
  box[i] = BucketBox{r.q_start, r.q_end, r.r_start, r.r_end};
  live[i] = !dead;
}

// run_start[r] = the slot that opens run r; run_start[number of runs] = n
__global__ __launch_bounds__(256) void bucket_run_starts_kernel(const uint32_t *__restrict__ new_run, const uint32_t *__restrict__ run_of,
                                                                const int n, uint32_t *__restrict__ run_start) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n && (i == n || new_run[i])) run_start[run_of[i]] = (uint32_t)i;
}

// ---- d. the sweep: a wavefront per run of two or more slots ----
__device__ __forceinline__ int bucket_wave_min(int v) {
  for (int d = 32; d; d >>= 1) {
    const int o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int bucket_wave_max(int v) {
  for (int d = 32; d; d >>= 1) {
    const int o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// Slots [a, b) of one run.  Slot j is read and written by lane (j - a) & 63 alone -- its live word when it is swallowed, its
// box when its own hit has grown --, so a lane's program order is all the ordering the slots need.
__device__ __forceinline__ void bucket_sweep_run(BucketBox *__restrict__ box, uint32_t *__restrict__ live, const int a, const int b,
                                                 const int merge_dist, const int lane) {
  for (int i = a + 1; i < b; i++) {
    const int owner = (i - a) & 63;
    // (the slot's own lane holds what an earlier kernel wrote there; the others take it from that lane)
    BucketBox h{0, 0, 0, 0};
    uint32_t alive = 0;
    if (lane == owner) {
      alive = live[i];
      h = box[i];
    }
    if (!__shfl((int)alive, owner, 64)) continue;  // a self hit
    h.q_start = __shfl(h.q_start, owner, 64);
    h.q_end = __shfl(h.q_end, owner, 64);
    h.r_start = __shfl(h.r_start, owner, 64);
    h.r_end = __shfl(h.r_end, owner, 64);
    bool grown = false;
    for (bool grew = true; grew;) {  // passes over [a, i) until one absorbs nothing
      grew = false;
      for (int base = a; base < i; base += 64) {
        const int j = base + lane;
        BucketBox w{0, 0, 0, 0};
        bool take = false;
        if (j < i && live[j]) {
          w = box[j];
          take = !bucket_apart(w, h, merge_dist);
        }
        if (__ballot(take) == 0) continue;
        if (take) live[j] = 0;
        h.q_start = min(h.q_start, bucket_wave_min(take ? w.q_start : 0x7fffffff));
        h.q_end = max(h.q_end, bucket_wave_max(take ? w.q_end : (int)0x80000000));
        h.r_start = min(h.r_start, bucket_wave_min(take ? w.r_start : 0x7fffffff));
        h.r_end = max(h.r_end, bucket_wave_max(take ? w.r_end : (int)0x80000000));
        grew = grown = true;
      }
    }
    if (grown && lane == owner) box[i] = h;
  }
}

__global__ __launch_bounds__(256) void bucket_sweep_kernel(BucketBox *__restrict__ box, uint32_t *__restrict__ live,
                                                           const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ n_runs,
                                                           const int merge_dist) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6, waves = (long long)gridDim.x * 4;
  const long long runs = *n_runs;
  // 64 runs a look: a run of one slot is its own window
  for (long long r0 = wave * 64; r0 < runs; r0 += waves * 64) {
    const long long r = r0 + lane;
    int a = 0, b = 0;
    if (r < runs) a = (int)run_start[r], b = (int)run_start[r + 1];
    for (unsigned long long todo = __ballot(b - a >= 2); todo; todo &= todo - 1) {
      const int l = __ffsll(todo) - 1;
      bucket_sweep_run(box, live, __shfl(a, l, 64), __shfl(b, l, 64), merge_dist, lane);
    }
  }
}

// ---- e. flush and deal ----
// the survivors in the multimap's order: a stable sort by (run, ref_end); a dead slot goes behind them all
__global__ __launch_bounds__(256) void bucket_flush_keys_kernel(const BucketBox *__restrict__ box, const uint32_t *__restrict__ live,
                                                                const uint32_t *__restrict__ new_run, const uint32_t *__restrict__ run_of,
                                                                const int n, unsigned long long *__restrict__ key,
                                                                uint32_t *__restrict__ place) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // (run_of: the runs opened in front of slot i; a live slot lies in the last run opened at or in front of it)
  key[i] = live[i] ? (unsigned long long)(run_of[i] + new_run[i] - 1) << 32 | (uint32_t)box[i].r_end : kBucketDeadKey;
  place[i] = (uint32_t)i;
}

// the records in deal order, their classes as sort keys, and their number
__global__ __launch_bounds__(256) void bucket_class_kernel(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ place,
                                                           const BucketRec *__restrict__ sorted, const BucketBox *__restrict__ box,
                                                           const int n, sdf_bucket_hit *__restrict__ out, uint32_t *__restrict__ cls_key,
                                                           uint32_t *__restrict__ cls_place, unsigned long long *__restrict__ n_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const bool alive = key[j] != kBucketDeadKey, next_alive = j + 1 < n && key[j + 1] != kBucketDeadKey;
  uint32_t cls = kBucketDeadClass;
  if (alive) {
    const uint32_t slot = place[j];
    const BucketBox w = box[slot];
    const BucketRec r = sorted[slot];
    out[j] = sdf_bucket_hit{r.q_chr, w.q_start, w.q_end, r.r_chr, w.r_start, w.r_end, r.flags & SDF_SEED_RC, 0};
    cls = (uint32_t)bucket_class(w);
    if (!next_alive) n_out[0] = (unsigned long long)j + 1;
  } else if (j == 0) {
    n_out[0] = 0;
  }
  cls_key[j] = cls;
  cls_place[j] = (uint32_t)j;
}

// place p of the stable sort by class: the hits of the classes below, then the hit's rank within its own
__global__ __launch_bounds__(256) void bucket_deal_kernel(const uint32_t *__restrict__ cls_key, const uint32_t *__restrict__ cls_place,
                                                          const int n, const int nbins, sdf_bucket_hit *__restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n && cls_key[p] != kBucketDeadClass) out[cls_place[p]].bucket = p % nbins;
}

}  // namespace sdf

// The cuts of `sedef stats generate` (scope row f4) for a batch of finished alignments: the whole alignment's match
// counter, the cuts at assembly gaps and the two trims of every cut piece -- what the host did on fetched strings before
// the column counters of stats_cols.hip could run.
//
// Reference: Alignment(fa, fb, cigar) counts the matches (src/align.cc:90-105, ceq :29-35); split_alignment walks the
// columns for runs of >= 100 'N' in either sequence (src/stats_main.cc:163-211); subhit slices every piece and trims it
// with trim_back, then trim_front (src/stats_main.cc:33-84, src/align.cc:343-456).  Here nothing is expanded and nothing
// is walked serially: one wavefront takes one alignment, 64 CIGAR runs at a time, cut into units of up to eight columns
// of one run as in stats_cols.hip (same scans, same search of the unit offsets, stats_fetch8 for either strand).
//
// In column space (column i of side a is '-' inside an I run, of side b inside a D run):
//   * events.  A column is N for a side when toupper(c) == 'N' ('-' is not; a reversed side's character is
//     rev_dna(pool byte), so every byte that is not ACGTacgt is N there).  A maximal N run [s, e) of one side is an event at
//     e when e - s >= 100 and e < span.  Events are ordered by e, side a before side b.  With begin = 0, every event emits
//     the piece [begin, s) if s > begin, then begin = e; the last piece is [begin, span).  Without an event the alignment
//     is ONE piece [0, span), not trimmed.
//     The start of the N run that enters a unit is a max-scan of "column behind the last non-N column"; the begin an
//     event sees is a max-scan of the events' e; the piece's index is a sum-scan of the pieces emitted.
//   * trims.  With F(i) the sum of the columns' scores before column i -- match / mismatch for a pair column, gap_extend for
//     a gap column plus gap_open where the column before it is not a gap in the same sequence -- and
//     G(i) = F(i) - gap_open * [column i continues a gap], the score of columns [x, y) scanned from x is F(y) - G(x), and
//     scanned from y it is the same number (a scan pays gap_open at its first column if that is a gap, and once per gap
//     run it meets).  trim_back of [b, e) keeps [b, te), te - 1 the LAST argmax of F(i + 1) over the piece, if
//     F(te) - G(b) >= 0, else nothing; trim_front of [b, te) keeps [tb, te), tb the FIRST argmin of G over it, if
//     F(te) - G(tb) >= 0, else nothing -- and nothing as well when tb - b equals the a-bases of [b, te), the reference's
//     "nothing found" marker (src/align.cc:343; host/alignment.cc:325).  F is a sum-scan; the two arguments are wave
//     reductions of (value, column) keys.
//
// Three launches: stats_cuts_count_kernel (pieces per alignment, whole-alignment matches), stats_cuts_scan_kernel (piece
// offsets in task order), stats_cuts_emit_kernel (the records; an alignment without an event writes its one record from the
// counts, the others find their events again and walk every piece twice).  No segment path: an alignment of any number of
// runs is one wavefront's work.
#include <hip/hip_runtime.h>

#include "extz2_geom.h"
#include "sdf_kernels.h"
#include "stats_dev.h"

namespace sdf {

constexpr int CUTS_MIN_GAP = 100;  // Globals::Stats::MIN_ASSEMBLY_GAP_SIZE (src/globals.h:101)

// inclusive prefix maximum over the lanes, for values >= 0 (the DPP steps of stats_wave_scan; a lane a step does not
// write keeps the identity 0)
__device__ __forceinline__ int cuts_wave_scan_max(int v) {
  auto mx = [](int a, int b) { return a > b ? a : b; };
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
  return v;
}
// the value of the lane before (lane 0: 0)
__device__ __forceinline__ int cuts_lane_before(int v, int lane) {
  const int o = __builtin_amdgcn_ds_bpermute((lane - 1) << 2, v);
  return lane ? o : 0;
}
__device__ __forceinline__ long long cuts_wave_max64(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const long long o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ long long cuts_key(int value, int col) { return (long long)(((unsigned long long)(unsigned)value << 32) | (unsigned)col); }

struct CutsLds {  // per wavefront: the chunk's runs
  int unit[64], sa[64], sb[64], sl[64], sc[64], so[64];
};

// Every unit of the alignment that holds a column of [lo, hi), in column order, 64 at a time: f(col, cnt, kind, opens,
// wa, wb) is called by all lanes -- col: the unit's first column, cnt: its columns (0 for a lane past the last unit),
// kind: 0 pair, 1 gap in b, 2 gap in a, opens: the unit's first column is a gap and the column before it is none in the
// same sequence (or there is none; never for a lane past the last unit, whose sum is carried into the next chunk), wa / wb: the characters ('-' where the side has none).  Chunks and rounds of 64 units
// that hold no column of the range are passed over without a load.  Returns 1 for a CIGAR that does not fit its
// sequences (the checks of stats_count_alignment).
template <bool REV, class F>
__device__ __forceinline__ int cuts_walk(const sdf_stats_task &T, const char *__restrict__ pool, const uint32_t *__restrict__ cigars,
                                         CutsLds &L, const int lane, const int lo, const int hi, int &span, F &&f) {
  const char *a = pool + T.a_off, *b = pool + T.b_off;
  const uint32_t *cg = cigars + T.cigar_off;
  const int n_cigar = (int)T.n_cigar, a_len = (int)T.a_len, b_len = (int)T.b_len;
  const bool wide_a = a_len >= 8, wide_b = b_len >= 8;
  const uint32_t strand = REV ? (uint32_t)__builtin_amdgcn_readfirstlane((int)T.reserved) : 0u;
  const bool rc_a = (strand & SDF_STATS_A_RC) != 0, rc_b = (strand & SDF_STATS_B_RC) != 0;
  int ia = 0, ib = 0, col0 = 0, prev_kind = -1;  // wave-uniform
  for (int base = 0; base < n_cigar; base += 64) {
    const int k = base + lane;
    const uint32_t w = k < n_cigar ? cg[k] : 0u;
    const int op = (int)(w & 15u);
    const int len = k < n_cigar ? (int)(w >> 4) : 0;
    if (__any(op > 2 || len > (a_len > b_len ? a_len : b_len))) return 1;
    const int adv_a = op != 2 ? len : 0, adv_b = op != 1 ? len : 0, nunit = (len + 7) >> 3;
    const int in_u = stats_wave_scan(nunit), in_a = stats_wave_scan(adv_a), in_b = stats_wave_scan(adv_b), in_c = stats_wave_scan(len);
    const int total = __builtin_amdgcn_readlane(in_u, 63), tot_a = __builtin_amdgcn_readlane(in_a, 63),
              tot_b = __builtin_amdgcn_readlane(in_b, 63), tot_c = __builtin_amdgcn_readlane(in_c, 63);
    if (ia + tot_a > a_len || ib + tot_b > b_len) return 1;
    // the kind of the last run with columns before this one: a max-scan of (lane, op) keys
    const int in_k = cuts_wave_scan_max(len ? ((lane << 2) | op) + 1 : 0), ex_k = cuts_lane_before(in_k, lane);
    const int before = ex_k ? (ex_k - 1) & 3 : prev_kind;
    const int last_k = __builtin_amdgcn_readlane(in_k, 63);
    prev_kind = last_k ? (last_k - 1) & 3 : prev_kind;
    if (col0 < hi && col0 + tot_c > lo) {
      L.unit[lane] = in_u - nunit;
      L.sl[lane] = len;
      L.sa[lane] = op != 2 ? ia + in_a - adv_a : -1;
      L.sb[lane] = op != 1 ? ib + in_b - adv_b : -1;
      L.sc[lane] = col0 + in_c - len;
      L.so[lane] = op | (op != 0 && len != 0 && before != op ? 4 : 0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int u0 = 0; u0 < total; u0 += 64) {
        const bool valid = u0 + lane < total;
        const int u = valid ? u0 + lane : total - 1;
        int j = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1)
          if (L.unit[j + step] <= u) j += step;  // last run that starts at or before unit u: the one that holds it
        const int d = 8 * (u - L.unit[j]), left = L.sl[j] - d, col = L.sc[j] + d;
        const int cnt = valid ? (left < 8 ? left : 8) : 0;
        // the round's columns: from lane 0's unit to the end of the last unit
        const int r_lo = __builtin_amdgcn_readfirstlane(col);
        const int r_hi = u0 + 63 < total ? __builtin_amdgcn_readlane(col + cnt, 63) : col0 + tot_c;
        if (r_lo >= hi || r_hi <= lo) continue;  // (uniform)
        const int pa = L.sa[j], pb = L.sb[j], o = L.so[j];
        uint64_t wa = pa >= 0 ? stats_fetch8<REV>(a, pa + d, a_len, wide_a, rc_a) : STATS_DASHES;
        uint64_t wb = pb >= 0 ? stats_fetch8<REV>(b, pb + d, b_len, wide_b, rc_b) : STATS_DASHES;
        f(col, cnt, o & 3, valid && (o & 4) != 0 && d == 0, wa, wb);  // (a lane past the last unit opens no gap)
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    ia += tot_a, ib += tot_b, col0 += tot_c;
  }
  span = col0;
  return 0;
}

// a unit's columns as three bit masks (bit i: column i of the unit): N on side a, N on side b, match
// (same_base, host/alignment.cc: equal ignoring case and not N, on a pair column)
__device__ __forceinline__ void cuts_masks(uint64_t wa, uint64_t wb, int cnt, int kind, uint32_t &n_a, uint32_t &n_b, uint32_t &mt) {
  n_a = n_b = mt = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int ca = (int)(wa & 255u), cb = (int)(wb & 255u);
    wa >>= 8, wb >>= 8;
    const int ua = (unsigned)(ca - 'a') < 26u ? ca - 32 : ca, ub = (unsigned)(cb - 'a') < 26u ? cb - 32 : cb;
    n_a |= (uint32_t)(ua == 'N') << i;
    n_b |= (uint32_t)(ub == 'N') << i;
    mt |= (uint32_t)(ua == ub && ua != 'N') << i;
  }
  const uint32_t have = (1u << cnt) - 1u;
  n_a &= kind != 2 ? have : 0u;
  n_b &= kind != 1 ? have : 0u;
  mt &= kind == 0 ? have : 0u;
}

// The events of one alignment and the pieces they cut (see the head of the file).  EMIT: the pieces' column ranges are
// written to out[0 ..).  Returns 1 for a CIGAR that does not fit; pieces: how many; events: whether there was one;
// matches: of the whole alignment.
template <bool REV, bool EMIT>
__device__ __forceinline__ int cuts_events(const sdf_stats_task &T, const char *__restrict__ pool, const uint32_t *__restrict__ cigars,
                                           CutsLds &L, const int lane, sdf_stats_piece *__restrict__ out, int &pieces, int &events,
                                           int &matches, int &span) {
  int run_a = 0, run_b = 0, begin = 0, np = 0, nev = 0;  // wave-uniform: where the N run that reaches the round began, per side
  int m = 0;
  const int bad = cuts_walk<REV>(T, pool, cigars, L, lane, 0, 0x7fffffff, span,
                                 [&](int col, int cnt, int kind, bool, uint64_t wa, uint64_t wb) {
    uint32_t n_a, n_b, mt;
    cuts_masks(wa, wb, cnt, kind, n_a, n_b, mt);
    m += __popc(mt);
    const uint32_t have = (1u << cnt) - 1u, non_a = ~n_a & have, non_b = ~n_b & have;
    // the column behind the last column of the unit that is not N: where an N run that leaves the unit began
    const int end_a = non_a ? col + 32 - __clz(non_a) : 0, end_b = non_b ? col + 32 - __clz(non_b) : 0;
    const int in_ea = cuts_wave_scan_max(end_a), in_eb = cuts_wave_scan_max(end_b);
    const int ex_ea = cuts_lane_before(in_ea, lane), ex_eb = cuts_lane_before(in_eb, lane);
    const int s_a = ex_ea > run_a ? ex_ea : run_a, s_b = ex_eb > run_b ? ex_eb : run_b;
    const int l_a = __builtin_amdgcn_readlane(in_ea, 63), l_b = __builtin_amdgcn_readlane(in_eb, 63);
    run_a = l_a > run_a ? l_a : run_a, run_b = l_b > run_b ? l_b : run_b;
    // the N run that enters the unit ends at the unit's first column that is not N (a run that begins inside a unit of
    // eight columns is no event)
    const int e_a = col + __ffs(non_a) - 1, e_b = col + __ffs(non_b) - 1;
    const bool ev_a = non_a && e_a - s_a >= CUTS_MIN_GAP, ev_b = non_b && e_b - s_b >= CUTS_MIN_GAP;
    if (!__any(ev_a || ev_b)) return;  // (uniform)
    nev = 1;
    const int top = ev_a && ev_b ? (e_a > e_b ? e_a : e_b) : ev_a ? e_a : ev_b ? e_b : 0;
    const int in_t = cuts_wave_scan_max(top), ex_t = cuts_lane_before(in_t, lane);
    const int bg = ex_t > begin ? ex_t : begin;
    const int l_t = __builtin_amdgcn_readlane(in_t, 63);
    begin = l_t > begin ? l_t : begin;
    // this lane's events in order: by e, a before b
    const bool a_first = ev_a && (!ev_b || e_a <= e_b);
    const bool ev1 = ev_a || ev_b, ev2 = ev_a && ev_b;
    const int s1 = a_first ? s_a : s_b, e1 = a_first ? e_a : e_b, s2 = a_first ? s_b : s_a;
    const bool p1 = ev1 && s1 > bg, p2 = ev2 && s2 > e1;
    const int cnt_p = (int)p1 + (int)p2, in_p = stats_wave_scan(cnt_p);
    if (EMIT) {
      int at = np + in_p - cnt_p;
      if (p1) out[at].begin = bg, out[at].end = s1, ++at;
      if (p2) out[at].begin = e1, out[at].end = s2;
    }
    np += __builtin_amdgcn_readlane(in_p, 63);
  });
  if (EMIT && !bad && nev && lane == 0) out[np].begin = begin, out[np].end = span;
  pieces = nev ? np + 1 : 1;
  events = nev;
  matches = stats_wave_sum(m);
  return bad;
}

// trim_back, then trim_front, of columns [b, e): the kept range and its matches (tb == te: nothing is kept)
template <bool REV>
__device__ __forceinline__ void cuts_trim(const sdf_stats_task &T, const char *__restrict__ pool, const uint32_t *__restrict__ cigars,
                                          CutsLds &L, const int lane, const CutsScores sc, const int b, const int e, int &tb, int &te,
                                          int &matches) {
  constexpr long long kLowest = (long long)0x8000000000000000ull;
  int span;
  tb = te = b, matches = 0;
  // ---- trim_back: the last argmax of F(i + 1), and G(b) ----
  int carry = 0, g_b = 0;
  long long best = kLowest;
  auto scores = [&](int cnt, int kind, bool opens, uint32_t mt) {  // the unit's sum
    const int nm = __popc(mt);
    return kind == 0 ? nm * sc.match + (cnt - nm) * sc.mismatch : cnt * sc.gap_extend + (opens ? sc.gap_open : 0);
  };
  cuts_walk<REV>(T, pool, cigars, L, lane, b, e, span, [&](int col, int cnt, int kind, bool opens, uint64_t wa, uint64_t wb) {
    uint32_t n_a, n_b, mt;
    cuts_masks(wa, wb, cnt, kind, n_a, n_b, mt);
    const int sum = scores(cnt, kind, opens, mt), in_f = stats_wave_scan(sum);
    int f = carry + in_f - sum;
    carry += __builtin_amdgcn_readlane(in_f, 63);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int c = col + i;
      const bool in = i < cnt && c >= b && c < e, start = opens && i == 0;
      const int g = f - (kind != 0 && !start ? sc.gap_open : 0);
      f += kind == 0 ? ((mt >> i) & 1u ? sc.match : sc.mismatch) : sc.gap_extend + (start ? sc.gap_open : 0);
      const long long key = cuts_key(f, c);
      if (in && key > best) best = key;
      if (i < cnt && c == b) g_b = g;
    }
  });
  // (column b is in exactly one lane's unit: the others hold 0)
  g_b = stats_wave_sum(g_b);
  best = cuts_wave_max64(best);
  if (best == kLowest || (int)(best >> 32) - g_b < 0) return;
  const int keep_end = (int)(uint32_t)best + 1;
  // ---- trim_front of [b, keep_end): the first argmin of G, F(keep_end), the a-bases, and the matches from the argmin on ----
  int carry_m = 0, f_end = 0, a_bases = 0, m_at = 0;
  carry = 0;
  best = kLowest;  // (the maximum of (-G, -column) keys)
  cuts_walk<REV>(T, pool, cigars, L, lane, b, keep_end, span, [&](int col, int cnt, int kind, bool opens, uint64_t wa, uint64_t wb) {
    uint32_t n_a, n_b, mt;
    cuts_masks(wa, wb, cnt, kind, n_a, n_b, mt);
    const int lo_i = b - col > 0 ? (b - col < 8 ? b - col : 8) : 0, hi_i = keep_end - col < cnt ? (keep_end - col > 0 ? keep_end - col : 0) : cnt;
    const uint32_t in_mask = hi_i > lo_i ? ((1u << hi_i) - 1u) & ~((1u << lo_i) - 1u) : 0u;
    const int sum = scores(cnt, kind, opens, mt), in_f = stats_wave_scan(sum);
    const int nm = __popc(mt & in_mask), in_m = stats_wave_scan(nm);
    int f = carry + in_f - sum, mp = carry_m + in_m - nm;
    carry += __builtin_amdgcn_readlane(in_f, 63);
    carry_m += __builtin_amdgcn_readlane(in_m, 63);
    a_bases += kind != 2 ? __popc(in_mask) : 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int c = col + i;
      const bool in = (in_mask >> i) & 1u, start = opens && i == 0;
      const int g = f - (kind != 0 && !start ? sc.gap_open : 0);
      f += kind == 0 ? ((mt >> i) & 1u ? sc.match : sc.mismatch) : sc.gap_extend + (start ? sc.gap_open : 0);
      const long long key = cuts_key(-g, 0x7fffffff - c);
      if (in && key > best) best = key, m_at = mp;
      mp += in ? (int)((mt >> i) & 1u) : 0;
      if (in && c == keep_end - 1) f_end = f;
    }
  });
  f_end = stats_wave_sum(f_end);
  a_bases = stats_wave_sum(a_bases);
  const long long mine = best;
  best = cuts_wave_max64(best);
  // the lane that holds the argmin knows the matches before it
  const int owner = __ffsll((unsigned long long)__ballot(mine == best)) - 1;
  m_at = __shfl(m_at, owner);
  const int g_min = -(int)(best >> 32), first = 0x7fffffff - (int)(uint32_t)best;
  if (f_end - g_min < 0 || first - b == a_bases) return;
  tb = first, te = keep_end, matches = carry_m - m_at;
}

// ---- launch 1: pieces per alignment (bit 31: it has an event, bit 30: its CIGAR does not fit), whole-alignment matches ----
template <bool REV>
__global__ __launch_bounds__(64 * STATS_WAVES) void stats_cuts_count_kernel(const sdf_stats_task *__restrict__ tasks, int n,
                                                                            const char *__restrict__ pool,
                                                                            const uint32_t *__restrict__ cigars,
                                                                            uint32_t *__restrict__ counts, int32_t *__restrict__ whole) {
  __shared__ CutsLds lds[STATS_WAVES];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int task = blockIdx.x * STATS_WAVES + wv;
  if (task >= n) return;  // whole wavefronts leave; the kernel has no workgroup barrier
  const sdf_stats_task T = tasks[task];
  int pieces, events, matches, span;
  const int bad = cuts_events<REV, false>(T, pool, cigars, lds[wv], lane, nullptr, pieces, events, matches, span);
  if (lane == 0) {
    counts[task] = bad ? 1u | kCutsBad : (uint32_t)pieces | (events ? kCutsEvents : 0u);
    whole[2 * task] = matches, whole[2 * task + 1] = bad ? 0 : span;
  }
}

// ---- launch 2: first[i] = pieces of the alignments before i, first[n] = all (one workgroup of sixteen wavefronts) ----
__global__ __launch_bounds__(1024) void stats_cuts_scan_kernel(const uint32_t *__restrict__ counts, int n, uint64_t *__restrict__ first) {
  __shared__ int tot[16];
  const int wv = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (int base = 0; base < n; base += 1024) {  // (uniform trip count)
    const int i = base + (int)threadIdx.x;
    const int v = i < n ? (int)(counts[i] & kCutsCount) : 0;
    const int in = stats_wave_scan(v);
    if ((threadIdx.x & 63) == 63) tot[wv] = in;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) before += k < wv ? tot[k] : 0, all += tot[k];
    if (i < n) first[i] = carry + (uint64_t)(before + in - v);
    carry += (uint64_t)all;
    __syncthreads();
  }
  if (threadIdx.x == 0) first[n] = carry;
}

// ---- launch 3: the records.  An alignment whose pieces do not all lie below `cap` writes nothing. ----
template <bool REV>
__global__ __launch_bounds__(64 * STATS_WAVES) void stats_cuts_emit_kernel(const sdf_stats_task *__restrict__ tasks, int n,
                                                                           const char *__restrict__ pool,
                                                                           const uint32_t *__restrict__ cigars, CutsScores sc,
                                                                           const uint32_t *__restrict__ counts,
                                                                           const int32_t *__restrict__ whole,
                                                                           const uint64_t *__restrict__ first,
                                                                           sdf_stats_piece *__restrict__ out, uint64_t cap) {
  __shared__ CutsLds lds[STATS_WAVES];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int task = blockIdx.x * STATS_WAVES + wv;
  if (task >= n) return;
  const uint32_t c = counts[task];
  const uint64_t at = first[task];
  if (at + (c & kCutsCount) > cap) return;
  sdf_stats_piece *mine = out + at;
  if (!(c & kCutsEvents)) {  // one piece, as it is (or the record of a CIGAR that does not fit)
    if (lane == 0) {
      sdf_stats_piece R;
      R.begin = R.t_begin = 0, R.end = R.t_end = whole[2 * task + 1], R.matches = whole[2 * task];
      R.flags = c & kCutsBad ? 1 : 0, R.reserved[0] = R.reserved[1] = 0;
      *mine = R;
    }
    return;
  }
  const sdf_stats_task T = tasks[task];
  int pieces, events, matches, span;
  cuts_events<REV, true>(T, pool, cigars, lds[wv], lane, mine, pieces, events, matches, span);
  __threadfence();  // the lanes' ranges are read back below, by all of them
  for (int p = 0; p < pieces; p++) {
    const int b = __hip_atomic_load(&mine[p].begin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int e = __hip_atomic_load(&mine[p].end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int tb, te, m;
    cuts_trim<REV>(T, pool, cigars, lds[wv], lane, sc, b, e, tb, te, m);
    if (lane == 0) mine[p].t_begin = tb, mine[p].t_end = te, mine[p].matches = m, mine[p].flags = 0, mine[p].reserved[0] = mine[p].reserved[1] = 0;
  }
}

template __global__ void stats_cuts_count_kernel<false>(const sdf_stats_task *, int, const char *, const uint32_t *, uint32_t *, int32_t *);
template __global__ void stats_cuts_count_kernel<true>(const sdf_stats_task *, int, const char *, const uint32_t *, uint32_t *, int32_t *);
template __global__ void stats_cuts_emit_kernel<false>(const sdf_stats_task *, int, const char *, const uint32_t *, CutsScores,
                                                       const uint32_t *, const int32_t *, const uint64_t *, sdf_stats_piece *, uint64_t);
template __global__ void stats_cuts_emit_kernel<true>(const sdf_stats_task *, int, const char *, const uint32_t *, CutsScores,
                                                      const uint32_t *, const int32_t *, const uint64_t *, sdf_stats_piece *, uint64_t);

}  // namespace sdf

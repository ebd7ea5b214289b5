// Device helpers that several DP kernels share: the packed 16-bit forms, the recurrence of a packed register (SDF_CORE),
// fresh scores as byte permutes, the decode of the packed sequence pool, SDWA half selects, the best-cell order.
// Device-only code; sizes and bounds that the host needs too are in extz2_geom.h.
#pragma once
#include <hip/hip_runtime.h>

#include "extz2_geom.h"

namespace sdf {

// ---- packed 16-bit helpers of the DP kernels: every state byte of the reference is held as value << 8 in a
// 16-bit half, so the packed ALU reproduces the reference's wrap-around int8 arithmetic two cells at a time ----
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

#define SDF_OPQ(x) asm("" : "+v"(x))  // make a value opaque to instcombine (keeps the packed forms)

__device__ __forceinline__ unsigned pk_add(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ unsigned pk_sub(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ unsigned pk_maxi(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, a),
                                                                __builtin_bit_cast(i16x2, b)));
}
__device__ __forceinline__ unsigned pk_maxu(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                                                __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned pk_minu(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                                                __builtin_bit_cast(u16x2, b)));
}
// max(a - b, 0) per half: one v_pk_sub_u16 with the clamp bit (unsigned saturation)
__device__ __forceinline__ unsigned pk_subsat_u(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// min(x, 1) per half = "x != 0" as 0/1.  Written as the instruction itself: the optimiser would
// otherwise turn it into per-half compares + selects.
__device__ __forceinline__ unsigned pk_nonzero_(unsigned a, unsigned one_opaque) {
  return pk_minu(a, one_opaque);
}
#define pk_nonzero(a) pk_nonzero_((a), one2)
// F <- (F << 1) | bit, as the single instruction it is
__device__ __forceinline__ unsigned shl1_or(unsigned f, unsigned bit) {
  return (f << 1) + bit;  // bit 0 of f << 1 is clear: + == |, and it selects as one v_lshl_add_u32
}
__device__ __forceinline__ unsigned pk_mad(unsigned a, unsigned b, unsigned c) {
  return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b) +
                                          __builtin_bit_cast(u16x2, c));
}
__device__ __forceinline__ unsigned pk_ashr15(unsigned a) {
  return __builtin_bit_cast(unsigned, __builtin_bit_cast(i16x2, a) >> (i16x2){15, 15});
}
__device__ __forceinline__ unsigned pk_shl(unsigned a, unsigned n) {
  return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a)
                                          << (u16x2){(unsigned short)n, (unsigned short)n});
}

// ---- the packed sequence pool: ceil(len/16) words of 2-bit codes, then ceil(len/32) words of N mask ----
// code of position k (0..3); an N becomes NBITS | wild (the kernels differ in how they mark an N: the general kernel and
// the traceback take the wildcard's code itself, the window kernels set bits above it)
template <uint32_t NBITS>
__device__ __forceinline__ uint32_t pool_code(const uint32_t *codes, const uint32_t *nmask, int k, uint32_t wild) {
  const uint32_t c = (codes[k >> 4] >> ((k & 15) * 2)) & 3u;
  const uint32_t n = (nmask[k >> 5] >> (k & 31)) & 1u;
  return n ? (NBITS | wild) : c;
}
// 16-bit code: 0..3, or 0xff00 | wild for N
__device__ __forceinline__ uint32_t pool_code16(const uint32_t *codes, const uint32_t *nmask, int k, uint32_t wild) {
  return pool_code<0xff00u>(codes, nmask, k, wild);
}

// ---- SDWA half selects: dst half <- src half in the lanes a compare picks (SDWA keeps the other half).  The compare
// writes VCC and the SDWA select consumes it (no wait state needed between them on gfx9).  Each form is written once and
// generated for the low (WORD_0) and the high (WORD_1) half.
#define SDF_SDWA_SEL(W) "vcc dst_sel:" W " dst_unused:UNUSED_PRESERVE src0_sel:" W " src1_sel:" W
#define SDF_SEL_HALVES(W, HALF)                                                                                        \
  /* lanes in [lo, lo + len) ... */                                                                                   \
  __device__ __forceinline__ void sel_##HALF##_len(unsigned &dst, unsigned src, int lo, int len, int lane) {           \
    unsigned t;                                                                                                        \
    asm volatile(                                                                                                      \
        "v_subrev_u32 %1, %3, %5\n\t"                                                                                  \
        "v_cmp_gt_u32 vcc, %4, %1\n\t"                                                                                 \
        "v_cndmask_b32_sdwa %0, %0, %2, " SDF_SDWA_SEL(W) "\n\ts_nop 0"                                                \
        : "+v"(dst), "=&v"(t) : "v"(src), "s"(lo), "s"(len), "v"(lane) : "vcc");                                       \
  }                                                                                                                    \
  /* ... and in [lo, hi) */                                                                                            \
  __device__ __forceinline__ void sel_##HALF##_rng(unsigned &dst, unsigned src, int lo, int hi, int lane) {            \
    sel_##HALF##_len(dst, src, lo, hi > lo ? hi - lo : 0, lane);                                                       \
  }                                                                                                                    \
  /* (the range [0, bound): one signed compare) */                                                                     \
  __device__ __forceinline__ void sel_##HALF##_below(unsigned &dst, unsigned src, int bound, int lane) {               \
    asm volatile(                                                                                                      \
        "v_cmp_gt_i32 vcc, %2, %3\n\t"                                                                                 \
        "v_cndmask_b32_sdwa %0, %0, %1, " SDF_SDWA_SEL(W) "\n\ts_nop 0"                                                \
        : "+v"(dst) : "v"(src), "s"(bound), "v"(lane) : "vcc");                                                        \
  }
SDF_SEL_HALVES("WORD_0", lo)
SDF_SEL_HALVES("WORD_1", hi)
#undef SDF_SEL_HALVES

// both halves of one register: lo half where thr_lo <= lane, hi half where thr_hi <= lane (sel2_ge); where lane < thr (sel2_lt)
#define SDF_SEL2(NAME, CMP)                                                                                            \
  __device__ __forceinline__ void NAME(unsigned &dst, unsigned src, int thr_lo, int thr_hi, int lane) {                \
    asm volatile(                                                                                                      \
        CMP " vcc, %2, %4\n\t"                                                                                         \
        "v_cndmask_b32_sdwa %0, %0, %1, " SDF_SDWA_SEL("WORD_0") "\n\t"                                                \
        CMP " vcc, %3, %4\n\t"                                                                                         \
        "v_cndmask_b32_sdwa %0, %0, %1, " SDF_SDWA_SEL("WORD_1")                                                       \
        : "+v"(dst) : "v"(src), "s"(thr_lo), "s"(thr_hi), "v"(lane) : "vcc");                                          \
  }
SDF_SEL2(sel2_ge, "v_cmp_le_i32")
SDF_SEL2(sel2_lt, "v_cmp_gt_i32")
#undef SDF_SEL2
#undef SDF_SDWA_SEL

// value of slot `s` (0..127) of a packed register, as its 16-bit half
__device__ __forceinline__ unsigned slot_half(unsigned reg, int s) {
  const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)reg, s >> 1);
  return (s & 1) ? (w >> 16) : (w & 0xffffu);
}

// ---- fresh scores as byte permutes --------------------------------------------------------------------------------------
// Fresh (score + 2(q+e)) << 8 of the two halves of a lane's register k: ONE byte permute of the lane's two score tables
// TA[k], TB[k] by a selector made from the row's query bases (`sel`); WITH_N: the sequences hold an N somewhere, and a
// half an N selected (0xff: negative) is patched to the wildcard's score.  extz2_pair.hip (pair_qsel) has the story.
#define SDF_SCORE_PERM(z, k, sel, WITH_N)                               \
  {                                                                     \
    z = __builtin_amdgcn_perm(TB[k], TA[k], (sel));                     \
    if (WITH_N) {                                                       \
      unsigned nn_ = pk_ashr15(z);                                      \
      SDF_OPQ(nn_);                                                     \
      z = (z_wild & nn_) | (z & ~nn_);                                  \
    }                                                                   \
  }
// The kernels whose lanes hold TWO ADJACENT target positions per register (wave, stripe, banded stripe): a table of four score
// bytes per position -- against query base 0..3; an N in the target: the wildcard's score four times --, the row's two query
// bases as a selector (byte 1 = base of the even position: a byte of the first table; byte 3 = 4 + base of the odd one: a byte
// of the second; bytes 0, 2 = 0x0c: zero; an N: 0xff, patched afterwards where the sequences hold any N).
// code: what pool_code16 returns (0..3, N: 0xff00 | wild)
__device__ __forceinline__ unsigned score_table(const unsigned code, const unsigned mis4, const unsigned delta, const unsigned wild4) {
  return (code & 0xff00u) ? wild4 : mis4 ^ (delta << (8u * code));
}
// an entry of a query window of byte pairs (W[i] = bases of window positions i, i + 1) in selector form
__device__ __forceinline__ uint16_t qsel_pair(const uint32_t v0, const uint32_t v1) {
  return (uint16_t)(((v0 & 0xff00u) ? 0xffu : v0) | (((v1 & 0xff00u) ? 0xffu : v1 + 4u) << 8));
}
// the two selector bytes of a window entry -> the permute's selector 0x0c, s0, 0x0c, s1
__device__ __forceinline__ unsigned qsel_spread(const unsigned w16) {
  return __builtin_amdgcn_perm(0x0c0c0c0cu, w16, 0x01040004u);
}

// One anti-diagonal step of the recurrence for packed register k (two cells per lane), in the
// <<8 int16 domain; appends the four direction flags to the accumulators.
// Round 5: three of its differences are 32-bit subtracts (v_sub_u32: ~2.3 cycles against ~4.2 for v_pk_sub_i16,
// profiles/r05_ubench_valu_ops.txt).  They are exact on the packed halves for EVERY cell, the artefact cells of a band's
// edges included, because they never borrow: the score register only ever holds fresh scores z0 = (score + 2 (q + e)) << 8
// with q <= z0 >> 8 <= 127 (sdf_api.hip: core32_ok -- other scorings run on the general kernel), z1 = max_i(z0, a) is z0 or a
// larger non-negative value, zb = max_i(z1, b) likewise, and z3 = min_u(max_u(z1, b), cap) >= min(z1, cap) >= q << 8.  The
// other sums and differences involve u and v, which ARE negative in those cells: they keep the packed forms.
#define SDF_CORE(k)                                                     \
  {                                                                     \
    const unsigned a_ = pk_add(xt1[k], vt1[k]);                         \
    const unsigned bb_ = pk_add(Y[k], U[k]);                            \
    const unsigned z0_ = S[k];                                          \
    const unsigned z1_ = pk_maxi(z0_, a_);                              \
    const unsigned fa_ = z1_ - z0_; /* != 0 <=> a > z (signed); no borrow: z1 >= z0 >= 0 */ \
    const unsigned zb_ = pk_maxi(z1_, bb_);                             \
    const unsigned fb_ = zb_ - z1_; /* != 0 <=> b > max(z,a); no borrow */ \
    const unsigned z2_ = pk_maxu(z1_, bb_);                             \
    const unsigned z3_ = pk_minu(z2_, capv);                            \
    const unsigned un_ = pk_sub(z3_, vt1[k]);                           \
    const unsigned vn_ = pk_sub(z3_, U[k]);                             \
    const unsigned zq_ = z3_ - qv; /* no borrow: z3 >= q << 8 */         \
    const unsigned a2_ = pk_sub(a_, zq_);                               \
    const unsigned b2_ = pk_sub(bb_, zq_);                              \
    const unsigned xn_ = pk_maxi(a2_, 0u);                              \
    const unsigned yn_ = pk_maxi(b2_, 0u);                              \
    U[k] = un_;                                                         \
    V[k] = vn_;                                                         \
    X[k] = xn_;                                                         \
    Y[k] = yn_;                                                         \
    Fa[k] = shl1_or(Fa[k], pk_nonzero(fa_));                            \
    Fb[k] = shl1_or(Fb[k], pk_nonzero(fb_));                            \
    Fx[k] = shl1_or(Fx[k], pk_nonzero(xn_));                            \
    Fy[k] = shl1_or(Fy[k], pk_nonzero(yn_));                            \
  }

// ---- the best cell of a task (general kernel, pair kernel's TRACK flavour, banded stripes) ----
// a beats b: larger H; then earlier anti-diagonal; then the reference's in-row scan order
__device__ __forceinline__ bool beats(const BestCell &a, const BestCell &b) {
  if (a.H != b.H) return a.H > b.H;
  if (a.r != b.r) return a.r < b.r;
  return a.key < b.key;
}

__device__ __forceinline__ BestCell wave_best(BestCell c) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    BestCell o;
    o.H = __shfl_xor(c.H, off);
    o.r = __shfl_xor(c.r, off);
    o.key = __shfl_xor(c.key, off);
    o.t = __shfl_xor(c.t, off);
    if (beats(o, c)) c = o;
  }
  return c;
}

}  // namespace sdf

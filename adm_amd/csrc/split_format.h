// The two split number formats that carry f32 products on the 16-bit MFMAs -- the ONE statement of them: every kernel that produces
// or consumes a split operand (conv_wino2d_x6.hip, conv_gemm_x6.hip, conv_wgrad_x6.hip, attention_h3.hip, pack_weights.hip) takes
// the rule from here.
//
// gfx950 has no reduced-precision fast path for f32 matrix operands (v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate), so an
// f32 operand is written as a short sum of 16-bit terms whose pairwise products are exact in the f32 accumulator:
//   format 0 (bf16 x 3)  a = a0 + a1 + a2 EXACTLY, three bf16 terms by truncation (8 + 8 + 8 mantissa bits, the exponent range of
//      f32): a0 = top 16 bits of a, a1 = top 16 bits of a - a0, a2 = a - a0 - a1.  a b from SIX products, small ones first,
//      a0 b2 + a2 b0 + a1 b1 + a0 b1 + a1 b0 + a0 b0; the three below 2^-24 |a b| are dropped.  Needs nothing but the operands.
//      (Exactly: for |a| >= 2^-103 and for 0.  Below that a remainder is an f32 denormal and its truncation drops less than 2^-133.)
//   format 1 (fp16 x 2)  s a = h0 + h1, two fp16 terms by round-to-nearest: h0 = fp16(s a), h1 = fp16(s a - h0);
//      |s a - h0 - h1| <= 2^-24 |s a| while h1 is a normal fp16 number, <= 2^-25 absolutely below that.  a b from THREE products
//      (h0 h1' + h1 h0' + h0 h0'; h1 h1' <= 2^-24 |a b| is dropped), the two scales undone once in the epilogue.  Half the MFMAs,
//      fragment reads, split stores and weight DMA of format 0 at the same accuracy against fp64 (tools/fp16x3_accuracy.py).
//      s is a power of two from an UPPER BOUND of max |a| (split_scale): 16000 / bound < s <= 32000 / bound, so that s |a| <= 16000
//      and the Winograd transforms' sums of four values stay inside the fp16 range (65504).  Activations: the bound is a device
//      vector written by the kernel that produced them (include/adm_hip.h).  Weights: one scale per optimiser step
//      (PT_H3_SCALE); a scaled weight for which split_f16_overflow() holds raises a flag and the host falls back to format 0.
//
// Weight images (16-bit elements; 16 consecutive k of one row are 32 contiguous bytes, one (k chunk, term) image of 32 rows is the
// contiguous KB one LDS-DMA instruction moves):
//   wino_image_offset   [ey][cols/16][ex][term][rows][16]   the sixteen Winograd planes U[ey * 4 + ex][rows][cols] (conv_wino2d_x6.hip)
//   rows_image_offset   [cols/16][term][rows][16]           a [rows][cols] matrix (conv_gemm_x6.hip)
// Both give the element of term 0; term t lies t * split_term_stride(rows) further on.
#pragma once
#include "common.h"

constexpr int split_terms(int fmt) { return fmt ? 2 : 3; }

// power-of-two scale of format 1 from an upper bound of max |a|: s * amax <= 16000 < 2 s * amax (1 for a bound that is no positive
// finite number)
__host__ __device__ inline float split_scale(float amax) {
  if (!(amax > 0.f) || !(amax < 3e38f)) return 1.f;
  int e;
  frexpf(16000.f / amax, &e);                         // 16000 / amax = m 2^e, m in [0.5, 1)
  return ldexpf(1.f, e - 1);
}
// a scaled value that format 1 must not be given (the caller falls back to format 0); also true for NaN
__host__ __device__ inline bool split_f16_overflow(float a) { return !(__builtin_fabsf(a) < 65000.f); }

// ---- scalar forms (weight side; callable from the host)
__host__ __device__ inline float bf16_head(float a) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, a) & 0xFFFF0000u); }
__host__ __device__ inline unsigned short bf16_bits(float a) { return (unsigned short)(__builtin_bit_cast(unsigned, a) >> 16); }
__host__ __device__ inline void split3_store(float a, unsigned short* d, long term) {
  const float r1 = a - bf16_head(a), r2 = r1 - bf16_head(r1);
  d[0] = bf16_bits(a);
  d[term] = bf16_bits(r1);
  d[2 * term] = bf16_bits(r2);
}
__host__ __device__ inline void split2(float a, _Float16& h0, _Float16& h1) {      // a = the value already scaled
  h0 = (_Float16)a;
  h1 = (_Float16)(a - (float)h0);
}
__host__ __device__ inline void split2_store(float a, unsigned short* d, long term) {
  _Float16 h0, h1;
  split2(a, h0, h1);
  d[0] = __builtin_bit_cast(unsigned short, h0);
  d[term] = __builtin_bit_cast(unsigned short, h1);
}

// ---- the layouts of the weight images
__host__ __device__ inline long split_term_stride(int rows) { return (long)rows << 4; }
__host__ __device__ inline long wino_image_offset(int terms, int ey, int ex, int rows, int cols, int n, int c) {
  return ((((long)(ey * (cols >> 4) + (c >> 4)) * (4 * terms) + ex * terms) * rows + n) << 4) + (c & 15);
}
__host__ __device__ inline long rows_image_offset(int terms, int rows, int n, int c) {
  return ((((long)(c >> 4) * terms) * rows + n) << 4) + (c & 15);
}

#ifdef __HIPCC__
// ---- activation side: a channel quad -> packed dwords (two per term), next to the MFMAs of another wave of the same SIMD.
// All of that arithmetic is written with PLAIN (one value per lane) f32 instructions.  tools/overlap_probe2.hip: next to
// v_mfma_f32_32x32x16_bf16 of another wave on the same SIMD, v_add_f32 / v_and_b32 / v_perm_b32 are 91-96 % hidden, the PACKED forms
// (v_pk_add_f32, v_pk_fma_f32) not at all (0-3 %: they share the matrix pipe's data path) -- the packed form halves the instruction
// count and doubles the cost.  The compiler packs every f32x2-shaped add it sees, hence the inline assembly; the three *_x6 files are
// also compiled without packed-f32 instruction selection (csrc/Makefile, NOPK), the helpers mean the same without that flag.
__device__ __forceinline__ float plain_add(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float plain_sub(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ f32x4 plain_add4(f32x4 a, f32x4 b) { return f32x4{plain_add(a[0], b[0]), plain_add(a[1], b[1]), plain_add(a[2], b[2]), plain_add(a[3], b[3])}; }
__device__ __forceinline__ f32x4 plain_sub4(f32x4 a, f32x4 b) { return f32x4{plain_sub(a[0], b[0]), plain_sub(a[1], b[1]), plain_sub(a[2], b[2]), plain_sub(a[3], b[3])}; }

// the top halves of (lo, hi) in one dword
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) {
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
// v = v0 + v1 + v2 exactly, each term a bf16
__device__ __forceinline__ void split3_quad(const f32x4 v, u32x2& t0, u32x2& t1, u32x2& t2) {
  f32x4 h, mh;
#pragma unroll
  for (int i = 0; i < 4; ++i) h[i] = bf16_head(v[i]);
  const f32x4 r = plain_sub4(v, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) mh[i] = bf16_head(r[i]);
  const f32x4 r2 = plain_sub4(r, mh);
  t0 = u32x2{bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3])};
  t1 = u32x2{bf16_pack2(r[0], r[1]), bf16_pack2(r[2], r[3])};
  t2 = u32x2{bf16_pack2(r2[0], r2[1]), bf16_pack2(r2[2], r2[3])};
}
// v * s = h0 + h1
__device__ __forceinline__ void split2_quad(const f32x4 v, float s, u32x2& t0, u32x2& t1) {
  _Float16 h0[4], h1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split2(v[i] * s, h0[i], h1[i]);
  t0 = u32x2{__builtin_bit_cast(unsigned, f16x2{h0[0], h0[1]}), __builtin_bit_cast(unsigned, f16x2{h0[2], h0[3]})};
  t1 = u32x2{__builtin_bit_cast(unsigned, f16x2{h1[0], h1[1]}), __builtin_bit_cast(unsigned, f16x2{h1[2], h1[3]})};
}
// ... of eight values (an MFMA operand fragment): four dwords per term.  The same arithmetic written pair by pair, as
// attention_h3.hip had it: on the quad form, or on split2(), the attention kernels come out as different machine code.
__device__ __forceinline__ void split2_oct(const float (&v)[8], float s, u32x4& t0, u32x4& t1) {
  unsigned a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x0 = v[2 * i] * s, x1 = v[2 * i + 1] * s;
    const _Float16 h00 = (_Float16)x0, h01 = (_Float16)x1;
    const _Float16 h10 = (_Float16)(x0 - (float)h00), h11 = (_Float16)(x1 - (float)h01);
    a[i] = __builtin_bit_cast(unsigned, f16x2{h00, h01});
    b[i] = __builtin_bit_cast(unsigned, f16x2{h10, h11});
  }
  t0 = u32x4{a[0], a[1], a[2], a[3]};
  t1 = u32x4{b[0], b[1], b[2], b[3]};
}
#endif

// Forward kernels of the Swin condition encoder (unet/swin_transformer.py of the reference): the fused shifted-window attention
// core, LayerNorm with weight and bias over the last axis, and the PatchMerging gather fused with its LayerNorm(4C).
// Everything between them (qkv / proj / MLP / reduction Linears, GELU, residual adds) runs on the existing GEMM and elementwise
// kernels.  f32 throughout.
#include "common.h"

#define SWIN_WIN 7
#define SWIN_T 49          // tokens per window
#define SWIN_D 32          // head dimension
#define SWIN_WAVES 4       // (window, head) units per workgroup, one per wave

// ------------------------------------------------------------------------------------------------
// Window attention.  One wave owns one (window, head) unit; lane i < 49 owns query token i = (ty, tx) of the window.
// Padding, roll, partition, relative-position bias, the -100 mask and their inverses are index arithmetic:
//   rolled-frame coordinate  r = w * 7 + t          source coordinate (padded frame)  s = (r + shift) mod P
//   a token with s >= H (or W) is padding: as a key / value it equals the qkv bias, as a query it is not produced
//   region label along an axis (shift > 0): (r >= P - 7) + (r >= P - shift); two tokens whose labels differ get -100
// K and V of the head are staged once in LDS (read back as broadcasts: every lane reads the same key row), q lives in registers,
// the 49 scores of a row live in registers, so the softmax needs no cross-lane traffic.
// ------------------------------------------------------------------------------------------------
struct SwinAttnP {
  const float* qkv; const float* qkv_bias; const float* table; float* out;
  int B, H, W, C, heads, Ph, Pw, sh, sw, nWw, nWin;      // nWin = windows per image
  long units;                                            // B * nWin * heads
};

__global__ __launch_bounds__(SWIN_WAVES * 64) void swin_attn_kernel(SwinAttnP p) {
  __shared__ __attribute__((aligned(16))) float sK[SWIN_WAVES][SWIN_T * SWIN_D];
  __shared__ __attribute__((aligned(16))) float sV[SWIN_WAVES][SWIN_T * SWIN_D];
  __shared__ float sTab[SWIN_WAVES][176];
  __shared__ int sLab[SWIN_WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long unit = (long)blockIdx.x * SWIN_WAVES + wave;
  const bool active = unit < p.units;
  const int C3 = 3 * p.C;
  int head = 0, b = 0, wy = 0, wx = 0;
  if (active) {
    head = (int)(unit % p.heads);
    const long win = unit / p.heads;
    b = (int)(win / p.nWin);
    const int wi = (int)(win % p.nWin);
    wy = wi / p.nWw; wx = wi % p.nWw;
  }
  const size_t img = (size_t)b * p.H * p.W;
  if (active) {
    // K and V rows: 49 tokens x 8 float4 each
    for (int idx = lane; idx < SWIN_T * (SWIN_D / 4); idx += 64) {
      const int t = idx >> 3, c4 = idx & 7;
      const int sy = (wy * SWIN_WIN + t / SWIN_WIN + p.sh) % p.Ph, sx = (wx * SWIN_WIN + t % SWIN_WIN + p.sw) % p.Pw;
      const float* src = (sy < p.H && sx < p.W) ? p.qkv + (img + (size_t)sy * p.W + sx) * C3 : p.qkv_bias;
      const int off = head * SWIN_D + c4 * 4;
      *reinterpret_cast<f32x4*>(&sK[wave][t * SWIN_D + c4 * 4]) = *reinterpret_cast<const f32x4*>(src + p.C + off);
      *reinterpret_cast<f32x4*>(&sV[wave][t * SWIN_D + c4 * 4]) = *reinterpret_cast<const f32x4*>(src + 2 * p.C + off);
    }
    for (int idx = lane; idx < 169; idx += 64) sTab[wave][idx] = p.table[(size_t)idx * p.heads + head];
  }
  // this lane's token
  const int t = lane < SWIN_T ? lane : 0;
  const int ty = t / SWIN_WIN, tx = t % SWIN_WIN;
  const int ry = wy * SWIN_WIN + ty, rx = wx * SWIN_WIN + tx;
  const int ly = p.sh == 0 ? 0 : (ry >= p.Ph - SWIN_WIN) + (ry >= p.Ph - p.sh);
  const int lx = p.sw == 0 ? 0 : (rx >= p.Pw - SWIN_WIN) + (rx >= p.Pw - p.sw);
  const int lab = ly * 3 + lx;
  sLab[wave][lane] = lab;
  const int sy = (ry + p.sh) % p.Ph, sx = (rx + p.sw) % p.Pw;
  const bool valid = active && lane < SWIN_T && sy < p.H && sx < p.W;
  float q[SWIN_D];
  {
    const float* src = valid ? p.qkv + (img + (size_t)sy * p.W + sx) * C3 : p.qkv_bias;
    const float scale = 0.17677669529663687f;      // 32 ** -0.5
#pragma unroll
    for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + head * SWIN_D + c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[c4 * 4 + e] = v[e] * scale;
    }
  }
  __syncthreads();
  if (!valid) return;          // (no barrier follows)
  float s[SWIN_T];
  float m = -3.0e38f;
#pragma unroll
  for (int j = 0; j < SWIN_T; ++j) {
    float acc = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(&sK[wave][j * SWIN_D + c4 * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(q[c4 * 4 + e], kv[e], acc);
    }
    const int jy = j / SWIN_WIN, jx = j % SWIN_WIN;
    acc += sTab[wave][(ty - jy + SWIN_WIN - 1) * (2 * SWIN_WIN - 1) + (tx - jx + SWIN_WIN - 1)];
    acc += sLab[wave][j] != lab ? -100.0f : 0.0f;
    s[j] = acc;
    m = fmaxf(m, acc);
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < SWIN_T; ++j) {
    s[j] = expf(s[j] - m);
    sum += s[j];
  }
  const float inv = 1.0f / sum;
  float o[SWIN_D];
#pragma unroll
  for (int d = 0; d < SWIN_D; ++d) o[d] = 0.f;
#pragma unroll
  for (int j = 0; j < SWIN_T; ++j) {
#pragma unroll
    for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
      const f32x4 vv = *reinterpret_cast<const f32x4*>(&sV[wave][j * SWIN_D + c4 * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[c4 * 4 + e] = fmaf(s[j], vv[e], o[c4 * 4 + e]);
    }
  }
  float* dst = p.out + (img + (size_t)sy * p.W + sx) * p.C + head * SWIN_D;
#pragma unroll
  for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = o[c4 * 4 + e] * inv;
    *reinterpret_cast<f32x4*>(dst + c4 * 4) = v;
  }
}

extern "C" int adm_swin_attn_fwd(const float* qkv, const float* qkv_bias, const float* table, float* out, int B, int H, int W,
                                 int C, int heads, int window, int shift_h, int shift_w, hipStream_t stream) {
  if (!qkv || !qkv_bias || !table || !out || B <= 0 || H <= 0 || W <= 0 || heads <= 0) return ADM_EINVAL;
  if (window != SWIN_WIN || C != heads * SWIN_D) return ADM_EINVAL;          // specialised to window 7, head dimension 32
  if (shift_h < 0 || shift_h >= SWIN_WIN || shift_w < 0 || shift_w >= SWIN_WIN) return ADM_EINVAL;
  if (((uintptr_t)qkv | (uintptr_t)qkv_bias | (uintptr_t)out) & 15) return ADM_EINVAL;
  SwinAttnP p;
  p.qkv = qkv; p.qkv_bias = qkv_bias; p.table = table; p.out = out;
  p.B = B; p.H = H; p.W = W; p.C = C; p.heads = heads;
  p.Ph = (H + SWIN_WIN - 1) / SWIN_WIN * SWIN_WIN;
  p.Pw = (W + SWIN_WIN - 1) / SWIN_WIN * SWIN_WIN;
  p.sh = p.Ph > SWIN_WIN ? shift_h : 0;          // no shift along an axis that is a single window
  p.sw = p.Pw > SWIN_WIN ? shift_w : 0;
  p.nWw = p.Pw / SWIN_WIN;
  p.nWin = (p.Ph / SWIN_WIN) * p.nWw;
  p.units = (long)B * p.nWin * heads;
  const long blocks = (p.units + SWIN_WAVES - 1) / SWIN_WAVES;
  if (blocks > 0x7fffffffL) return ADM_EINVAL;
  hipLaunchKernelGGL(swin_attn_kernel, dim3((unsigned)blocks), dim3(SWIN_WAVES * 64), 0, stream, p);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// ------------------------------------------------------------------------------------------------
// LayerNorm over rows of up to 2048 floats, one wave per row, the row held in registers (<= 8 float4 per lane): the mean first
// (of the differences from the row's first element), then the variance as the mean of squared deviations from it, so a row that
// is mostly zeros or that sits on a large common offset loses nothing to cancellation.  MERGE: the row is gathered from the four pixels of a 2x2 cell (zeros past the edge).
// ------------------------------------------------------------------------------------------------
#define LN_ROWS 4          // rows (waves) per workgroup
#define LN_MAXQ 8          // float4 per lane: rows of up to 64 * 8 * 4 = 2048 floats

template <bool MERGE, int NQ>
__global__ __launch_bounds__(LN_ROWS * 64) void ln_affine_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ y, long M,
                                                                 int C, float eps, int H, int W, int Cin) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;
  const int C4 = C >> 2;
  int oy = 0, ox = 0, Wo = 0;
  long b = 0;
  if (MERGE) {
    const int Ho = (H + 1) >> 1;
    Wo = (W + 1) >> 1;
    b = row / ((long)Ho * Wo);
    const int r = (int)(row % ((long)Ho * Wo));
    oy = r / Wo; ox = r % Wo;
  }
  f32x4 v[NQ];
#pragma unroll
  for (int it = 0; it < NQ; ++it) {
    const int i4 = lane + 64 * it;
    v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i4 < C4) {
      if (MERGE) {
        const int c = i4 * 4, quad = c / Cin, ci = c - quad * Cin;          // quad: (0,0), (1,0), (0,1), (1,1) as (dy, dx)
        const int iy = 2 * oy + (quad & 1), ix = 2 * ox + (quad >> 1);
        if (iy < H && ix < W) v[it] = *reinterpret_cast<const f32x4*>(x + (((size_t)b * H + iy) * W + ix) * Cin + ci);
      } else {
        v[it] = *reinterpret_cast<const f32x4*>(x + (size_t)row * C + (size_t)i4 * 4);
      }
    }
  }
  // sums are taken of x - x0 (x0 = the row's first element): a large offset common to the row then costs the mean no digits
  const float x0 = __shfl(v[0][0], 0, 64);
  float sum = 0.f;
#pragma unroll
  for (int it = 0; it < NQ; ++it) {
    if (lane + 64 * it < C4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[it][e] -= x0;
      sum += (v[it][0] + v[it][1]) + (v[it][2] + v[it][3]);
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int it = 0; it < NQ; ++it) {
    if (lane + 64 * it < C4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[it][e] - mean;
        sq = fmaf(d, d, sq);
      }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
  for (int it = 0; it < NQ; ++it) {
    const int i4 = lane + 64 * it;
    if (i4 < C4) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(w + i4 * 4), bb = *reinterpret_cast<const f32x4*>(bias + i4 * 4);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[it][e] - mean) * rstd * g[e] + bb[e];
      *reinterpret_cast<f32x4*>(y + (size_t)row * C + (size_t)i4 * 4) = o;
    }
  }
}

// NQ = float4 per lane, the smallest of 1, 2, 4, 8 that covers the row: a 128-float row then holds 4 values per lane, not 32 slots
template <bool MERGE>
static void ln_launch(const float* x, const float* w, const float* b, float* y, long M, int C, float eps, int H, int W, int Cin,
                      unsigned blocks, hipStream_t stream) {
  const int q = (C / 4 + 63) / 64;
#define LN_GO(NQ) hipLaunchKernelGGL((ln_affine_kernel<MERGE, NQ>), dim3(blocks), dim3(LN_ROWS * 64), 0, stream, x, w, b, y, M, C, eps, H, W, Cin)
  if (q <= 1) LN_GO(1);
  else if (q <= 2) LN_GO(2);
  else if (q <= 4) LN_GO(4);
  else LN_GO(8);
#undef LN_GO
}

extern "C" int adm_ln_affine_fwd(const float* x, const float* w, const float* b, float* y, long M, int C, float eps,
                                 hipStream_t stream) {
  if (!x || !w || !b || !y || M <= 0 || C < 32 || C > 64 * LN_MAXQ * 4 || (C & 3)) return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b | (uintptr_t)y) & 15) return ADM_EINVAL;
  const long blocks = (M + LN_ROWS - 1) / LN_ROWS;
  if (blocks > 0x7fffffffL) return ADM_EINVAL;
  ln_launch<false>(x, w, b, y, M, C, eps, 0, 0, 0, (unsigned)blocks, stream);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_swin_merge_ln_fwd(const float* x, const float* w, const float* b, float* y, int B, int H, int W, int C,
                                     float eps, hipStream_t stream) {
  if (!x || !w || !b || !y || B <= 0 || H <= 0 || W <= 0 || C < 8 || (C & 3) || 4 * C > 64 * LN_MAXQ * 4) return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b | (uintptr_t)y) & 15) return ADM_EINVAL;
  const long M = (long)B * ((H + 1) / 2) * ((W + 1) / 2);
  const long blocks = (M + LN_ROWS - 1) / LN_ROWS;
  if (blocks > 0x7fffffffL) return ADM_EINVAL;
  ln_launch<true>(x, w, b, y, M, 4 * C, eps, H, W, C, (unsigned)blocks, stream);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

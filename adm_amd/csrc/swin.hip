// Kernels of the Swin condition encoder (unet/swin_transformer.py of the reference): the fused shifted-window attention
// core, LayerNorm with weight and bias over the last axis, the PatchMerging gather fused with its LayerNorm(4C), their backward
// kernels, and (at the end) the patch embedding of the single-channel variant fused with its LayerNorm, forward and backward.
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

// NQ = float4 per lane, the smallest of 1, 2, 4, 8 that covers the row: a 128-float row then holds 4 values per lane, not 32 slots.
// The one place the rule is written: ln_launch and ln_bwd_launch (plain and MERGE, whose row is 4 Cin floats) choose through it.
// form = (NQ, float4 of the row in its last used trip: 64 when the row fills that trip, fewer when lanes sit past the row's end);
// the row uses ceil(C / 256) of the NQ trips, the others are empty.  Supported C: 32 <= C <= 2048, C % 4 == 0.
static int ln_form(int C, int form[2]) {
  if (C < 32 || C > 64 * LN_MAXQ * 4 || (C & 3)) return ADM_EINVAL;
  const int C4 = C / 4, trips = (C4 + 63) / 64;
  form[0] = trips <= 1 ? 1 : trips <= 2 ? 2 : trips <= 4 ? 4 : 8;
  form[1] = C4 - 64 * (trips - 1);
  return ADM_OK;
}

extern "C" int adm_ln_form(int C, int* out) {
  int form[2];
  if (!out || ln_form(C, form) != ADM_OK) return ADM_EINVAL;
  out[0] = form[0]; out[1] = form[1];
  return ADM_OK;
}

template <bool MERGE>
static int ln_launch(const float* x, const float* w, const float* b, float* y, long M, int C, float eps, int H, int W, int Cin,
                     unsigned blocks, hipStream_t stream) {
  int form[2];
  if (ln_form(C, form) != ADM_OK) return ADM_EINVAL;
#define LN_GO(NQ) hipLaunchKernelGGL((ln_affine_kernel<MERGE, NQ>), dim3(blocks), dim3(LN_ROWS * 64), 0, stream, x, w, b, y, M, C, eps, H, W, Cin)
  switch (form[0]) {
    case 1: LN_GO(1); break;
    case 2: LN_GO(2); break;
    case 4: LN_GO(4); break;
    default: LN_GO(8); break;
  }
#undef LN_GO
  return ADM_OK;
}

extern "C" int adm_ln_affine_fwd(const float* x, const float* w, const float* b, float* y, long M, int C, float eps,
                                 hipStream_t stream) {
  if (!x || !w || !b || !y || M <= 0 || C < 32 || C > 64 * LN_MAXQ * 4 || (C & 3)) return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b | (uintptr_t)y) & 15) return ADM_EINVAL;
  const long blocks = (M + LN_ROWS - 1) / LN_ROWS;
  if (blocks > 0x7fffffffL) return ADM_EINVAL;
  if (ln_launch<false>(x, w, b, y, M, C, eps, 0, 0, 0, (unsigned)blocks, stream) != ADM_OK) return ADM_EINVAL;
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
  if (ln_launch<true>(x, w, b, y, M, 4 * C, eps, H, W, C, (unsigned)blocks, stream) != ADM_OK) return ADM_EINVAL;
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// ================================================================================================
// Backward kernels: the gradient of the window attention, of the two LayerNorm kernels, and stochastic depth.
// ================================================================================================

// ------------------------------------------------------------------------------------------------
// Window attention, backward.  One wave (one workgroup) owns one (window, head) unit, with the forward's index arithmetic.
// Nothing is saved by the forward: scores and softmax are recomputed.  With S = q k^T + table + mask, P = softmax(S), O = P V:
//   dP = dO V^T      D_i = sum_j P_ij dP_ij      dS = P (dP - D)      dq = scale * dS K      dK = dS^T q      dV = P^T dO
// Pass 1, lane = query i (K, V broadcast from LDS, q and dO in registers): row i of P and of dS go to LDS, dq to d_qkv.
// Pass 2, lane = key j (q, dO broadcast from LDS -- they take the place of K, V): dK_j, dV_j as sums over the column j of dS, P.
//   A real key stores them to d_qkv; a padding key's k / v ARE the qkv bias, so its dK, dV are summed (over the unit's padding
//   keys, in token order) into the unit's partial of d_qkv_bias.
// Fold, lane = table index: d_table[(dy + 6) * 13 + (dx + 6)] of the unit = sum of dS_ij over the pairs with i - j = (dy, dx).
// A padded query row is never produced: its dO is zero here, which zeroes its dS row and its share of dV.
// Per unit the partial is SWIN_PART floats: 169 table entries, 32 of dK, 32 of dV (padding keys).  swin_attn_bwd_reduce sums the
// partials in unit order, one thread per entry: no float atomics, the same bits every run.
// LDS per wave: 2 x 49 x 32 + 2 x 49 x 49 + table + labels = 32.7 KB, so four units are resident per CU (160 KB).
// ------------------------------------------------------------------------------------------------
#define SWIN_PART 240          // floats per unit partial (169 + 64, padded)

struct SwinAttnBwdP {
  const float* qkv; const float* qkv_bias; const float* table; const float* d_out;
  float* d_qkv; float* part;
  int B, H, W, C, heads, Ph, Pw, sh, sw, nWw, nWin;
  long units;
};

__global__ __launch_bounds__(64) void swin_attn_bwd_kernel(SwinAttnBwdP p) {
  __shared__ __attribute__((aligned(16))) float sA[SWIN_T * SWIN_D];          // K, then scaled q
  __shared__ __attribute__((aligned(16))) float sB[SWIN_T * SWIN_D];          // V, then dO
  __shared__ float sP[SWIN_T * SWIN_T];
  __shared__ float sDS[SWIN_T * SWIN_T];
  __shared__ float sTab[176];
  __shared__ int sLab[64];
  const int lane = threadIdx.x;
  const long unit = blockIdx.x;
  const int C3 = 3 * p.C;
  const int head = (int)(unit % p.heads);
  const long win = unit / p.heads;
  const int b = (int)(win / p.nWin);
  const int wi = (int)(win % p.nWin);
  const int wy = wi / p.nWw, wx = wi % p.nWw;
  const size_t img = (size_t)b * p.H * p.W;
  const float scale = 0.17677669529663687f;      // 32 ** -0.5
  for (int idx = lane; idx < SWIN_T * (SWIN_D / 4); idx += 64) {
    const int t = idx >> 3, c4 = idx & 7;
    const int sy = (wy * SWIN_WIN + t / SWIN_WIN + p.sh) % p.Ph, sx = (wx * SWIN_WIN + t % SWIN_WIN + p.sw) % p.Pw;
    const float* src = (sy < p.H && sx < p.W) ? p.qkv + (img + (size_t)sy * p.W + sx) * C3 : p.qkv_bias;
    const int off = head * SWIN_D + c4 * 4;
    *reinterpret_cast<f32x4*>(&sA[t * SWIN_D + c4 * 4]) = *reinterpret_cast<const f32x4*>(src + p.C + off);
    *reinterpret_cast<f32x4*>(&sB[t * SWIN_D + c4 * 4]) = *reinterpret_cast<const f32x4*>(src + 2 * p.C + off);
  }
  for (int idx = lane; idx < 169; idx += 64) sTab[idx] = p.table[(size_t)idx * p.heads + head];
  // this lane's token, as a query in pass 1 and as a key in pass 2
  const int t = lane < SWIN_T ? lane : 0;
  const int ty = t / SWIN_WIN, tx = t % SWIN_WIN;
  const int ry = wy * SWIN_WIN + ty, rx = wx * SWIN_WIN + tx;
  const int ly = p.sh == 0 ? 0 : (ry >= p.Ph - SWIN_WIN) + (ry >= p.Ph - p.sh);
  const int lx = p.sw == 0 ? 0 : (rx >= p.Pw - SWIN_WIN) + (rx >= p.Pw - p.sw);
  const int lab = ly * 3 + lx;
  sLab[lane] = lab;
  const int sy = (ry + p.sh) % p.Ph, sx = (rx + p.sw) % p.Pw;
  const bool tok = lane < SWIN_T;
  const bool valid = tok && sy < p.H && sx < p.W;
  const size_t pix = img + (size_t)sy * p.W + sx;          // used only where valid
  __syncthreads();
  // ---------------------------------------------------------------- pass 1: lane = query
  // (the row's scores, then its P, live in sP; its dP, then its dS, in sDS: register arrays of 49 made the compiler spill)
  if (tok) {
    float q[SWIN_D], g[SWIN_D];
    const float* src = valid ? p.qkv + pix * C3 : p.qkv_bias;
#pragma unroll
    for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + head * SWIN_D + c4 * 4);
      f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
      if (valid) d = *reinterpret_cast<const f32x4*>(p.d_out + pix * p.C + head * SWIN_D + c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[c4 * 4 + e] = v[e] * scale;
        g[c4 * 4 + e] = d[e];
      }
    }
    float* rowP = sP + lane * SWIN_T;
    float* rowS = sDS + lane * SWIN_T;
    float m = -3.0e38f;
    for (int jy = 0; jy < SWIN_WIN; ++jy) {
#pragma unroll
      for (int jx = 0; jx < SWIN_WIN; ++jx) {
        const int j = jy * SWIN_WIN + jx;
        float acc = 0.f, accp = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
          const f32x4 kv = *reinterpret_cast<const f32x4*>(&sA[j * SWIN_D + c4 * 4]);
          const f32x4 vv = *reinterpret_cast<const f32x4*>(&sB[j * SWIN_D + c4 * 4]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc = fmaf(q[c4 * 4 + e], kv[e], acc);
            accp = fmaf(g[c4 * 4 + e], vv[e], accp);
          }
        }
        acc += sTab[(ty - jy + SWIN_WIN - 1) * (2 * SWIN_WIN - 1) + (tx - jx + SWIN_WIN - 1)];
        acc += sLab[j] != lab ? -100.0f : 0.0f;
        rowP[j] = acc;
        rowS[j] = accp;
        m = fmaxf(m, acc);
      }
    }
    float sum = 0.f, D = 0.f;
    for (int j = 0; j < SWIN_T; ++j) {
      const float e = expf(rowP[j] - m);
      rowP[j] = e;
      sum += e;
      D = fmaf(e, rowS[j], D);
    }
    const float inv = 1.0f / sum;
    D *= inv;
    float dq[SWIN_D];
#pragma unroll
    for (int d = 0; d < SWIN_D; ++d) dq[d] = 0.f;
#pragma unroll 7
    for (int j = 0; j < SWIN_T; ++j) {
      const float pj = rowP[j] * inv;
      const float ds = pj * (rowS[j] - D);
      rowP[j] = pj;
      rowS[j] = ds;
#pragma unroll
      for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
        const f32x4 kv = *reinterpret_cast<const f32x4*>(&sA[j * SWIN_D + c4 * 4]);
#pragma unroll
        for (int e = 0; e < 4; ++e) dq[c4 * 4 + e] = fmaf(ds, kv[e], dq[c4 * 4 + e]);
      }
    }
    if (valid) {
      float* dst = p.d_qkv + pix * C3 + head * SWIN_D;
#pragma unroll
      for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = dq[c4 * 4 + e] * scale;
        *reinterpret_cast<f32x4*>(dst + c4 * 4) = v;
      }
    }
  }
  __syncthreads();
  // scaled q and dO of the unit take the place of K and V (a padding token: q = the bias, dO = 0)
  for (int idx = lane; idx < SWIN_T * (SWIN_D / 4); idx += 64) {
    const int tt = idx >> 3, c4 = idx & 7;
    const int yy = (wy * SWIN_WIN + tt / SWIN_WIN + p.sh) % p.Ph, xx = (wx * SWIN_WIN + tt % SWIN_WIN + p.sw) % p.Pw;
    const bool real = yy < p.H && xx < p.W;
    const size_t px = img + (size_t)yy * p.W + xx;
    const int off = head * SWIN_D + c4 * 4;
    f32x4 qv = *reinterpret_cast<const f32x4*>((real ? p.qkv + px * C3 : p.qkv_bias) + off);
    f32x4 gv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (real) gv = *reinterpret_cast<const f32x4*>(p.d_out + px * p.C + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) qv[e] *= scale;
    *reinterpret_cast<f32x4*>(&sA[tt * SWIN_D + c4 * 4]) = qv;
    *reinterpret_cast<f32x4*>(&sB[tt * SWIN_D + c4 * 4]) = gv;
  }
  __syncthreads();
  // ---------------------------------------------------------------- pass 2: lane = key
  float dk[SWIN_D], dv[SWIN_D];
#pragma unroll
  for (int d = 0; d < SWIN_D; ++d) dk[d] = dv[d] = 0.f;
#pragma unroll 7
  for (int i = 0; i < SWIN_T; ++i) {
    const float ds = sDS[i * SWIN_T + t], pr = sP[i * SWIN_T + t];
#pragma unroll
    for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
      const f32x4 qv = *reinterpret_cast<const f32x4*>(&sA[i * SWIN_D + c4 * 4]);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(&sB[i * SWIN_D + c4 * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dk[c4 * 4 + e] = fmaf(ds, qv[e], dk[c4 * 4 + e]);
        dv[c4 * 4 + e] = fmaf(pr, gv[e], dv[c4 * 4 + e]);
      }
    }
  }
  if (valid) {
    float* dst = p.d_qkv + pix * C3 + head * SWIN_D;
#pragma unroll
    for (int c4 = 0; c4 < SWIN_D / 4; ++c4) {
      *reinterpret_cast<f32x4*>(dst + p.C + c4 * 4) = f32x4{dk[c4 * 4], dk[c4 * 4 + 1], dk[c4 * 4 + 2], dk[c4 * 4 + 3]};
      *reinterpret_cast<f32x4*>(dst + 2 * p.C + c4 * 4) = f32x4{dv[c4 * 4], dv[c4 * 4 + 1], dv[c4 * 4 + 2], dv[c4 * 4 + 3]};
    }
  }
  // ---------------------------------------------------------------- fold: the unit's table partial
  float* part = p.part + (size_t)unit * SWIN_PART;
  for (int idx = lane; idx < 169; idx += 64) {
    const int oy = idx / (2 * SWIN_WIN - 1) - (SWIN_WIN - 1), ox = idx % (2 * SWIN_WIN - 1) - (SWIN_WIN - 1);
    float acc = 0.f;
    for (int iy = 0; iy < SWIN_WIN; ++iy) {
      const int jy = iy - oy;
      if (jy < 0 || jy >= SWIN_WIN) continue;
      for (int ix = 0; ix < SWIN_WIN; ++ix) {
        const int jx = ix - ox;
        if (jx < 0 || jx >= SWIN_WIN) continue;
        acc += sDS[(iy * SWIN_WIN + ix) * SWIN_T + jy * SWIN_WIN + jx];
      }
    }
    part[idx] = acc;
  }
  __syncthreads();          // q and dO have been read: their tiles now carry the padding keys' dK and dV
  if (tok) {
    const bool padk = !valid;
#pragma unroll
    for (int d = 0; d < SWIN_D; ++d) {
      sA[lane * SWIN_D + d] = padk ? dk[d] : 0.f;
      sB[lane * SWIN_D + d] = padk ? dv[d] : 0.f;
    }
  }
  __syncthreads();
  {
    const float* srcp = lane < SWIN_D ? sA : sB;
    const int c = lane & (SWIN_D - 1);
    float acc = 0.f;
    for (int j = 0; j < SWIN_T; ++j) acc += srcp[j * SWIN_D + c];
    part[169 + lane] = acc;
  }
}

// Sums the unit partials in unit order.  Thread (head, e): e < 169 -> d_table[e][head]; 169 <= e < 233 -> the K and V thirds of
// d_qkv_bias (the Q third is zero: a padding token is never a query).  acc_*: add to what the destination holds.
__global__ __launch_bounds__(256) void swin_attn_bwd_reduce(const float* __restrict__ part, float* __restrict__ d_table,
                                                            float* __restrict__ d_bias, long groups, int heads, int C,
                                                            int acc_table, int acc_bias) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= heads * SWIN_PART) return;
  const int head = gid / SWIN_PART, e = gid % SWIN_PART;
  if (e >= 169 + 2 * SWIN_D) return;
  float acc = 0.f;
  for (long n = 0; n < groups; ++n) acc += part[(size_t)(n * heads + head) * SWIN_PART + e];
  if (e < 169) {
    float* dst = d_table + (size_t)e * heads + head;
    *dst = acc_table ? *dst + acc : acc;
  } else {
    const int c = e - 169;                                   // [0, 32): dK, [32, 64): dV
    float* dst = d_bias + (c < SWIN_D ? C : 2 * C - SWIN_D) + head * SWIN_D + c;
    *dst = acc_bias ? *dst + acc : acc;
    if (c < SWIN_D && !acc_bias) d_bias[head * SWIN_D + c] = 0.f;
  }
}

extern "C" long adm_swin_attn_bwd_ws_floats(int B, int H, int W, int heads) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0) return 0;
  const long nWin = (long)((H + SWIN_WIN - 1) / SWIN_WIN) * ((W + SWIN_WIN - 1) / SWIN_WIN);
  return (long)B * nWin * heads * SWIN_PART;
}

extern "C" int adm_swin_attn_bwd(const float* qkv, const float* qkv_bias, const float* table, const float* d_out, float* d_qkv,
                                 float* d_table, float* d_qkv_bias, float* ws, int B, int H, int W, int C, int heads, int window,
                                 int shift_h, int shift_w, int acc_table, int acc_bias, hipStream_t stream) {
  if (!qkv || !qkv_bias || !table || !d_out || !d_qkv || !d_table || !d_qkv_bias || !ws) return ADM_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0) return ADM_EINVAL;
  if (window != SWIN_WIN || C != heads * SWIN_D) return ADM_EINVAL;
  if (shift_h < 0 || shift_h >= SWIN_WIN || shift_w < 0 || shift_w >= SWIN_WIN) return ADM_EINVAL;
  if (((uintptr_t)qkv | (uintptr_t)qkv_bias | (uintptr_t)d_out | (uintptr_t)d_qkv) & 15) return ADM_EINVAL;
  SwinAttnBwdP p;
  p.qkv = qkv; p.qkv_bias = qkv_bias; p.table = table; p.d_out = d_out; p.d_qkv = d_qkv; p.part = ws;
  p.B = B; p.H = H; p.W = W; p.C = C; p.heads = heads;
  p.Ph = (H + SWIN_WIN - 1) / SWIN_WIN * SWIN_WIN;
  p.Pw = (W + SWIN_WIN - 1) / SWIN_WIN * SWIN_WIN;
  p.sh = p.Ph > SWIN_WIN ? shift_h : 0;
  p.sw = p.Pw > SWIN_WIN ? shift_w : 0;
  p.nWw = p.Pw / SWIN_WIN;
  p.nWin = (p.Ph / SWIN_WIN) * p.nWw;
  p.units = (long)B * p.nWin * heads;
  if (p.units > 0x7fffffffL) return ADM_EINVAL;
  hipLaunchKernelGGL(swin_attn_bwd_kernel, dim3((unsigned)p.units), dim3(64), 0, stream, p);
  ADM_CHECK_LAUNCH();
  hipLaunchKernelGGL(swin_attn_bwd_reduce, dim3((unsigned)adm_cdiv((long)heads * SWIN_PART, 256)), dim3(256), 0, stream, ws, d_table,
                     d_qkv_bias, (long)B * p.nWin, heads, C, acc_table, acc_bias);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// ------------------------------------------------------------------------------------------------
// LayerNorm, backward.  With xh = (x - mean) * rstd (the forward's shifted two-pass statistics, recomputed) and g = dy * w:
//   dx = rstd * (g - mean(g) - xh * mean(g * xh))        dw = sum over rows of dy * xh        db = sum over rows of dy
// One wave per row; a wave walks rows wave, wave + NW, ... and keeps its dw / db share in registers, then writes it as the partial
// part[wave][2][C].  ln_bwd_reduce sums the NW partials in wave order (no atomics).  MERGE: x is gathered from the 2x2 cell as in
// the forward and dx goes back through the same gather -- every source pixel has one destination, a position past an odd edge none.
// ------------------------------------------------------------------------------------------------
#define LN_BWD_MAXBLOCKS 256

static long ln_bwd_blocks(long M) {
  long b = (M + 4 * LN_ROWS - 1) / (4 * LN_ROWS);          // >= 4 rows per wave
  return b < 1 ? 1 : b > LN_BWD_MAXBLOCKS ? LN_BWD_MAXBLOCKS : b;
}

extern "C" long adm_ln_bwd_ws_floats(long M, int C) { return M <= 0 || C <= 0 ? 0 : ln_bwd_blocks(M) * LN_ROWS * 2 * (long)C; }

template <bool MERGE, int NQ>
__global__ __launch_bounds__(LN_ROWS * 64) void ln_affine_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ dy, float* __restrict__ dx,
                                                                     float* __restrict__ part, long M, int C, float eps, int H,
                                                                     int W, int Cin) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  const long NW = (long)gridDim.x * LN_ROWS;
  const int C4 = C >> 2;
  const int Ho = (H + 1) >> 1, Wo = (W + 1) >> 1;
  f32x4 aw[NQ], ab[NQ];
#pragma unroll
  for (int it = 0; it < NQ; ++it) aw[it] = ab[it] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long row = wave; row < M; row += NW) {
    int oy = 0, ox = 0;
    long b = 0;
    if (MERGE) {
      b = row / ((long)Ho * Wo);
      const int r = (int)(row % ((long)Ho * Wo));
      oy = r / Wo; ox = r % Wo;
    }
    f32x4 v[NQ], d[NQ];
    long src[NQ];          // element offset of this lane's quad in x / dx, -1: past the edge
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      const int i4 = lane + 64 * it;
      v[it] = d[it] = f32x4{0.f, 0.f, 0.f, 0.f};
      src[it] = -1;
      if (i4 < C4) {
        if (MERGE) {
          const int c = i4 * 4, quad = c / Cin, ci = c - quad * Cin;
          const int iy = 2 * oy + (quad & 1), ix = 2 * ox + (quad >> 1);
          if (iy < H && ix < W) src[it] = (long)((((size_t)b * H + iy) * W + ix) * Cin + ci);
        } else {
          src[it] = (long)((size_t)row * C + (size_t)i4 * 4);
        }
        if (src[it] >= 0) v[it] = *reinterpret_cast<const f32x4*>(x + src[it]);
        d[it] = *reinterpret_cast<const f32x4*>(dy + (size_t)row * C + (size_t)i4 * 4);
      }
    }
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
          v[it][e] -= mean;
          sq = fmaf(v[it][e], v[it][e], sq);
        }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      if (lane + 64 * it < C4) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(w + (lane + 64 * it) * 4);          // (from cache: every row re-reads it)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[it][e] *= rstd;                                  // xh
          aw[it][e] = fmaf(d[it][e], v[it][e], aw[it][e]);
          ab[it][e] += d[it][e];
          d[it][e] *= g[e];                                  // from here on: dy * w
          s1 += d[it][e];
          s2 = fmaf(d[it][e], v[it][e], s2);
        }
      }
    }
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      if (lane + 64 * it < C4 && src[it] >= 0) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (d[it][e] - m1 - v[it][e] * m2);
        *reinterpret_cast<f32x4*>(dx + src[it]) = o;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < NQ; ++it) {
    const int i4 = lane + 64 * it;
    if (i4 < C4) {
      *reinterpret_cast<f32x4*>(part + (size_t)wave * 2 * C + (size_t)i4 * 4) = aw[it];
      *reinterpret_cast<f32x4*>(part + (size_t)wave * 2 * C + C + (size_t)i4 * 4) = ab[it];
    }
  }
}

__global__ __launch_bounds__(256) void ln_bwd_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                     long NW, int C, int acc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * C) return;
  float s = 0.f;
  for (long n = 0; n < NW; ++n) s += part[(size_t)n * 2 * C + i];
  float* dst = i < C ? dw + i : db + (i - C);
  *dst = acc ? *dst + s : s;
}

template <bool MERGE>
static int ln_bwd_launch(const float* x, const float* w, const float* dy, float* dx, float* part, long M, int C, float eps, int H,
                         int W, int Cin, unsigned blocks, hipStream_t stream) {
  int form[2];
  if (ln_form(C, form) != ADM_OK) return ADM_EINVAL;
#define LN_GO(NQ) hipLaunchKernelGGL((ln_affine_bwd_kernel<MERGE, NQ>), dim3(blocks), dim3(LN_ROWS * 64), 0, stream, x, w, dy, dx, part, M, C, eps, H, W, Cin)
  switch (form[0]) {
    case 1: LN_GO(1); break;
    case 2: LN_GO(2); break;
    case 4: LN_GO(4); break;
    default: LN_GO(8); break;
  }
#undef LN_GO
  return ADM_OK;
}

extern "C" int adm_ln_affine_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, float* ws,
                                 long M, int C, float eps, int accumulate, hipStream_t stream) {
  if (!x || !w || !dy || !dx || !dw || !db || !ws || M <= 0 || C < 32 || C > 64 * LN_MAXQ * 4 || (C & 3)) return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)ws) & 15) return ADM_EINVAL;
  const long blocks = ln_bwd_blocks(M);
  if (ln_bwd_launch<false>(x, w, dy, dx, ws, M, C, eps, 0, 0, 0, (unsigned)blocks, stream) != ADM_OK) return ADM_EINVAL;
  ADM_CHECK_LAUNCH();
  hipLaunchKernelGGL(ln_bwd_reduce, dim3((unsigned)adm_cdiv(2L * C, 256)), dim3(256), 0, stream, ws, dw, db, blocks * LN_ROWS, C,
                     accumulate);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_swin_merge_ln_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, float* ws,
                                     int B, int H, int W, int C, float eps, int accumulate, hipStream_t stream) {
  if (!x || !w || !dy || !dx || !dw || !db || !ws || B <= 0 || H <= 0 || W <= 0 || C < 8 || (C & 3) || 4 * C > 64 * LN_MAXQ * 4)
    return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)ws) & 15) return ADM_EINVAL;
  const long M = (long)B * ((H + 1) / 2) * ((W + 1) / 2);
  const long blocks = ln_bwd_blocks(M);
  if (ln_bwd_launch<true>(x, w, dy, dx, ws, M, 4 * C, eps, H, W, C, (unsigned)blocks, stream) != ADM_OK) return ADM_EINVAL;
  ADM_CHECK_LAUNCH();
  hipLaunchKernelGGL(ln_bwd_reduce, dim3((unsigned)adm_cdiv(8L * C, 256)), dim3(256), 0, stream, ws, dw, db, blocks * LN_ROWS, 4 * C,
                     accumulate);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// ------------------------------------------------------------------------------------------------
// Stochastic depth in "row" mode: y[b, :] = x[b, :] + s[b] * r[b, :], s[b] = keep_b / (1 - p) drawn by the caller.  x == nullptr:
// y = s[b] * r, the gradient of the branch.  A dropped row (s[b] == 0) copies x, bit for bit.  n = elements per sample, n % 4 == 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowscale_add_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                           const float* __restrict__ s, float* __restrict__ y, long n4, long total4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const float sc = s[i / n4];
  const f32x4 rv = reinterpret_cast<const f32x4*>(r)[i];
  f32x4 o;
  if (x) {
    o = reinterpret_cast<const f32x4*>(x)[i];
    if (sc != 0.f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf(sc, rv[e], o[e]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = sc == 0.f ? 0.f : sc * rv[e];
  }
  reinterpret_cast<f32x4*>(y)[i] = o;
}

extern "C" int adm_rowscale_add(const float* x, const float* r, const float* s, float* y, int B, long n, hipStream_t stream) {
  if (!r || !s || !y || B <= 0 || n <= 0 || (n & 3)) return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)r | (uintptr_t)y) & 15) return ADM_EINVAL;
  const long total4 = (long)B * (n / 4);
  const long blocks = (total4 + 255) / 256;
  if (blocks > 0x7fffffffL) return ADM_EINVAL;
  hipLaunchKernelGGL(rowscale_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, r, s, y, n / 4, total4);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// ================================================================================================
// Patch embedding of a ONE-channel image fused with its LayerNorm (first_coonv of the single-channel encoder):
//   x [B][1][H][W] -> conv 4x4 stride 4, no padding (16 FMAs + bias per output) -> LayerNorm over E -> y [B][H/4][W/4][E]
// in one launch, with neither a channel-padded copy of x nor the pre-norm tensor in memory.  No MFMA (K = 16): the kernel is bound
// by the store of y.  G = the power of two >= E / 4 (at most 64) lanes share a token, each lane owns Q float4 of its row (quads
// sub, sub + G of the row), so a wave covers 64 / G consecutive tokens and every store instruction writes whole contiguous rows in
// 16-byte pieces.  A lane keeps the 16 stem weights of its 4 * Q channels in registers and walks token groups wave, wave + NW, ...
// The LayerNorm runs on the conv outputs in registers: the mean across the G lanes, then the sum of squared deviations from it.
// E % 32 == 0, 32 <= E <= PE_MAXE.  Trailing rows / columns of x (H % 4, W % 4) are never read.
// ================================================================================================
#define PE_WAVES 4
#define PE_MAXE 512
#define PE_PART 19             // floats per channel of a backward partial: dW[16], db, dgamma, dbeta
#define PE_BWD_MAXBLOCKS 256

struct PatchP {
  const float* x;
  int H, W, Ht, Wt, E, vec;      // vec: rows of a patch are read as one float4 (W % 4 == 0 and x 16-byte aligned)
  long T;                        // B * Ht * Wt tokens
};

template <int G>
__device__ __forceinline__ float pe_group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void pe_load_patch(const PatchP& p, long t, float (&px)[16]) {
  const long hw = (long)p.Ht * p.Wt;
  const long b = t / hw;
  const int r = (int)(t - b * hw);
  const int ty = r / p.Wt, tx = r - ty * p.Wt;
  const float* src = p.x + ((size_t)b * p.H + 4 * (size_t)ty) * p.W + 4 * (size_t)tx;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (p.vec) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)i * p.W);
#pragma unroll
      for (int e = 0; e < 4; ++e) px[4 * i + e] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) px[4 * i + e] = src[(size_t)i * p.W + e];
    }
  }
}

// the stem weights [E][16] and bias of this lane's channels; a lane past the row (E / 4 is no power of two) holds zeros
template <int G, int Q>
__device__ __forceinline__ void pe_load_weights(const float* __restrict__ w, const float* __restrict__ cb, int sub, int E4,
                                                float (&wr)[Q][4][16], float (&br)[Q][4]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i4 = sub + G * q;
    const bool on = i4 < E4;
    const f32x4 bv = on ? *reinterpret_cast<const f32x4*>(cb + i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      br[q][j] = bv[j];
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const f32x4 v = on ? *reinterpret_cast<const f32x4*>(w + ((size_t)i4 * 4 + j) * 16 + k4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) wr[q][j][k4 * 4 + e] = v[e];
      }
    }
  }
}

// conv outputs of this lane's channels, centred on the token's mean (two passes over registers); returns 1 / sqrt(var + eps)
template <int G, int Q>
__device__ __forceinline__ float pe_conv_centre(const float (&wr)[Q][4][16], const float (&br)[Q][4], const float (&px)[16], int sub,
                                                int E4, float eps, float (&c)[Q][4]) {
  const float invE = 1.0f / (float)(E4 * 4);
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = br[q][j];
#pragma unroll
      for (int k = 0; k < 16; ++k) a = fmaf(wr[q][j][k], px[k], a);
      c[q][j] = a;
    }
    sum += (c[q][0] + c[q][1]) + (c[q][2] + c[q][3]);          // (zeros on a lane past the row)
  }
  const float mean = pe_group_sum<G>(sum) * invE;
  float sq = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const bool on = sub + G * q < E4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[q][j] = on ? c[q][j] - mean : 0.f;
      sq = fmaf(c[q][j], c[q][j], sq);
    }
  }
  return 1.0f / sqrtf(pe_group_sum<G>(sq) * invE + eps);
}

template <int G, int Q>
__global__ __launch_bounds__(PE_WAVES * 64) void patch_embed_ln_kernel(PatchP p, const float* __restrict__ w,
                                                                       const float* __restrict__ cb, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, float* __restrict__ y,
                                                                       float eps) {
  constexpr int TPW = 64 / G;          // tokens per wave and pass
  const int lane = threadIdx.x & 63, sub = lane & (G - 1), grp = lane / G;
  const int E4 = p.E >> 2;
  float wr[Q][4][16], br[Q][4];
  pe_load_weights<G, Q>(w, cb, sub, E4, wr, br);
  f32x4 gr[Q], be[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const bool on = sub + G * q < E4;
    gr[q] = on ? *reinterpret_cast<const f32x4*>(gamma + (sub + G * q) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    be[q] = on ? *reinterpret_cast<const f32x4*>(beta + (sub + G * q) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long NW = (long)gridDim.x * PE_WAVES;
  const long nTG = (p.T + TPW - 1) / TPW;
  for (long tg = (long)blockIdx.x * PE_WAVES + (threadIdx.x >> 6); tg < nTG; tg += NW) {          // (wave-uniform trip count)
    const long t = tg * TPW + grp;
    const bool live = t < p.T;          // a group past the last token recomputes the last one and stores nothing
    float px[16], c[Q][4];
    pe_load_patch(p, live ? t : p.T - 1, px);
    const float rstd = pe_conv_centre<G, Q>(wr, br, px, sub, E4, eps, c);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i4 = sub + G * q;
      if (live && i4 < E4) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = c[q][j] * rstd * gr[q][j] + be[q][j];
        *reinterpret_cast<f32x4*>(y + (size_t)t * p.E + (size_t)i4 * 4) = o;
      }
    }
  }
}

static int pe_params(PatchP& p, const float* x, int B, int H, int W, int E) {
  if (B <= 0 || H < 4 || W < 4 || E < 32 || E > PE_MAXE || (E & 31)) return ADM_EINVAL;
  p.x = x; p.H = H; p.W = W; p.Ht = H / 4; p.Wt = W / 4; p.E = E;
  p.vec = (W & 3) == 0 && ((uintptr_t)x & 15) == 0;
  p.T = (long)B * p.Ht * p.Wt;
  return ADM_OK;
}

// The one place the lane layout is chosen: PE_DISPATCH and pe_token_groups go through it.  form = (G, Q, E / 4 = float4 per token);
// G * Q > E / 4 means lanes past the row.  Supported E: E % 32 == 0, 32 <= E <= 512.
static int pe_form(int E, int form[3]) {
  if (E < 32 || E > PE_MAXE || (E & 31)) return ADM_EINVAL;
  form[0] = E <= 32 ? 8 : E <= 64 ? 16 : E <= 128 ? 32 : 64;
  form[1] = E <= 256 ? 1 : 2;
  form[2] = E / 4;
  return ADM_OK;
}

extern "C" int adm_patch_embed_form(int E, int* out) {
  int form[3];
  if (!out || pe_form(E, form) != ADM_OK) return ADM_EINVAL;
  for (int i = 0; i < 3; ++i) out[i] = form[i];
  return ADM_OK;
}

// G lanes per token, Q float4 per lane: 32 -> (8, 1), 64 -> (16, 1), 96 / 128 -> (32, 1), 160 .. 256 -> (64, 1), above -> (64, 2)
#define PE_DISPATCH(E)                                           \
  do {                                                           \
    int form_[3];                                                \
    if (pe_form((E), form_) != ADM_OK) return ADM_EINVAL;        \
    switch (form_[0] * 4 + form_[1]) {                           \
      case 8 * 4 + 1: PE_GO(8, 1); break;                        \
      case 16 * 4 + 1: PE_GO(16, 1); break;                      \
      case 32 * 4 + 1: PE_GO(32, 1); break;                      \
      case 64 * 4 + 1: PE_GO(64, 1); break;                      \
      case 64 * 4 + 2: PE_GO(64, 2); break;                      \
      default: return ADM_EINVAL;                                \
    }                                                            \
  } while (0)

static long pe_token_groups(long T, int E) {
  int form[3];
  if (pe_form(E, form) != ADM_OK) return 0;
  const int tpw = 64 / form[0];
  return (T + tpw - 1) / tpw;
}

extern "C" int adm_patch_embed_ln_fwd(const float* x, const float* w, const float* cb, const float* gamma, const float* beta,
                                      float* y, int B, int H, int W, int E, float eps, hipStream_t stream) {
  if (!x || !w || !cb || !gamma || !beta || !y) return ADM_EINVAL;
  PatchP p;
  if (pe_params(p, x, B, H, W, E) != ADM_OK) return ADM_EINVAL;
  if (((uintptr_t)w | (uintptr_t)cb | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) return ADM_EINVAL;
  long blocks = (pe_token_groups(p.T, E) + 8 * PE_WAVES - 1) / (8 * PE_WAVES);          // ~8 token groups per wave: the weights load once
  if (blocks > 0x7fffffffL) return ADM_EINVAL;
#define PE_GO(G, Q) hipLaunchKernelGGL((patch_embed_ln_kernel<G, Q>), dim3((unsigned)blocks), dim3(PE_WAVES * 64), 0, stream, p, w, cb, gamma, beta, y, eps)
  PE_DISPATCH(E);
#undef PE_GO
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// ------------------------------------------------------------------------------------------------
// Backward of the fused stem: dW [E][16], db, dgamma, dbeta [E] from x and dy; there is no dX (the condition image takes no
// gradient).  Nothing is saved by the forward: the conv outputs and the token statistics are recomputed from x, as above.
//   xh = (c - mean) * rstd      dgamma += dy * xh      dbeta += dy      g = dy * gamma
//   dc = rstd * (g - mean(g) - xh * mean(g * xh))      db += dc      dW[e][k] += dc[e] * patch[k]
// Same lane layout as the forward; a lane keeps its 4 * Q * 19 sums in registers over its token groups.  Then, in a fixed order:
// the 64 / G token slots of a wave are added by shuffles, the four waves of a workgroup add into LDS one after the other, the
// workgroup writes one partial [19 * E] (dW, db, dgamma, dbeta back to back), and patch_embed_bwd_reduce adds the partials in
// workgroup order.  No float atomics: the same bits every run.
// ------------------------------------------------------------------------------------------------
static long pe_bwd_blocks(long T, int E) {
  long b = (pe_token_groups(T, E) + 4 * PE_WAVES - 1) / (4 * PE_WAVES);
  return b < 1 ? 1 : b > PE_BWD_MAXBLOCKS ? PE_BWD_MAXBLOCKS : b;
}

extern "C" long adm_patch_embed_ln_bwd_ws_floats(int B, int H, int W, int E) {
  PatchP p;
  if (pe_params(p, nullptr, B, H, W, E) != ADM_OK) return 0;
  return pe_bwd_blocks(p.T, E) * PE_PART * (long)E;
}

template <int G, int Q>
__global__ __launch_bounds__(PE_WAVES * 64) void patch_embed_ln_bwd_kernel(PatchP p, const float* __restrict__ w,
                                                                           const float* __restrict__ cb,
                                                                           const float* __restrict__ gamma,
                                                                           const float* __restrict__ dy, float* __restrict__ part,
                                                                           float eps) {
  constexpr int TPW = 64 / G;
  __shared__ float sP[PE_PART * PE_MAXE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = lane & (G - 1), grp = lane / G;
  const int E = p.E, E4 = E >> 2;
  const float invE = 1.0f / (float)E;
  float wr[Q][4][16], br[Q][4];
  pe_load_weights<G, Q>(w, cb, sub, E4, wr, br);
  f32x4 gr[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q)
    gr[q] = sub + G * q < E4 ? *reinterpret_cast<const f32x4*>(gamma + (sub + G * q) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  float aW[Q][4][16], ab[Q][4], ag[Q][4], at[Q][4];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ab[q][j] = ag[q][j] = at[q][j] = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) aW[q][j][k] = 0.f;
    }
  }
  const long NW = (long)gridDim.x * PE_WAVES;
  const long nTG = (p.T + TPW - 1) / TPW;
  for (long tg = (long)blockIdx.x * PE_WAVES + wave; tg < nTG; tg += NW) {
    const long t = tg * TPW + grp;
    const bool live = t < p.T;          // a group past the last token runs on the last one with dy = 0: it adds zeros
    float px[16], c[Q][4];
    pe_load_patch(p, live ? t : p.T - 1, px);
    const float rstd = pe_conv_centre<G, Q>(wr, br, px, sub, E4, eps, c);
    f32x4 d[Q];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i4 = sub + G * q;
      d[q] = live && i4 < E4 ? *reinterpret_cast<const f32x4*>(dy + (size_t)t * E + (size_t)i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[q][j] *= rstd;                                   // xh
        ag[q][j] = fmaf(d[q][j], c[q][j], ag[q][j]);
        at[q][j] += d[q][j];
        d[q][j] *= gr[q][j];                               // from here on: dy * gamma
        s1 += d[q][j];
        s2 = fmaf(d[q][j], c[q][j], s2);
      }
    }
    const float m1 = pe_group_sum<G>(s1) * invE, m2 = pe_group_sum<G>(s2) * invE;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dc = rstd * (d[q][j] - m1 - c[q][j] * m2);
        const float dcv = sub + G * q < E4 ? dc : 0.f;          // (a lane past the row would add -rstd * m1)
        ab[q][j] += dcv;
#pragma unroll
        for (int k = 0; k < 16; ++k) aW[q][j][k] = fmaf(dcv, px[k], aW[q][j][k]);
      }
    }
  }
  // the token slots of the wave, in a fixed order: afterwards the lanes of slot 0 hold the wave's sums
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ab[q][j] += __shfl_xor(ab[q][j], o, 64);
        ag[q][j] += __shfl_xor(ag[q][j], o, 64);
        at[q][j] += __shfl_xor(at[q][j], o, 64);
#pragma unroll
        for (int k = 0; k < 16; ++k) aW[q][j][k] += __shfl_xor(aW[q][j][k], o, 64);
      }
    }
  }
  // the waves of the workgroup, one after the other
  for (int turn = 0; turn < PE_WAVES; ++turn) {
    if (wave == turn && grp == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int i4 = sub + G * q;
        if (i4 < E4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ch = i4 * 4 + j;
            float* pw = sP + ch * 16;
#pragma unroll
            for (int k = 0; k < 16; ++k) pw[k] = turn ? pw[k] + aW[q][j][k] : aW[q][j][k];
            sP[16 * E + ch] = turn ? sP[16 * E + ch] + ab[q][j] : ab[q][j];
            sP[17 * E + ch] = turn ? sP[17 * E + ch] + ag[q][j] : ag[q][j];
            sP[18 * E + ch] = turn ? sP[18 * E + ch] + at[q][j] : at[q][j];
          }
        }
      }
    }
    __syncthreads();
  }
  float* dst = part + (size_t)blockIdx.x * PE_PART * E;
  for (int i = threadIdx.x; i < PE_PART * E; i += PE_WAVES * 64) dst[i] = sP[i];
}

// acc: bit 0 dW, bit 1 db, bit 2 dgamma, bit 3 dbeta -- add to what the destination holds
__global__ __launch_bounds__(256) void patch_embed_bwd_reduce(const float* __restrict__ part, float* __restrict__ dW,
                                                              float* __restrict__ db, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, long nb, int E, int acc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= PE_PART * E) return;
  float s = 0.f;
  for (long n = 0; n < nb; ++n) s += part[(size_t)n * PE_PART * E + i];
  const int which = i < 16 * E ? 0 : (i - 16 * E) / E + 1;
  float* dst = which == 0 ? dW + i : which == 1 ? db + (i - 16 * E) : which == 2 ? dgamma + (i - 17 * E) : dbeta + (i - 18 * E);
  *dst = (acc >> which) & 1 ? *dst + s : s;
}

extern "C" int adm_patch_embed_ln_bwd(const float* x, const float* w, const float* cb, const float* gamma, const float* dy,
                                      float* dW, float* db, float* dgamma, float* dbeta, float* ws, int B, int H, int W, int E,
                                      float eps, int accumulate, hipStream_t stream) {
  if (!x || !w || !cb || !gamma || !dy || !dW || !db || !dgamma || !dbeta || !ws) return ADM_EINVAL;
  PatchP p;
  if (pe_params(p, x, B, H, W, E) != ADM_OK) return ADM_EINVAL;
  if (((uintptr_t)w | (uintptr_t)cb | (uintptr_t)gamma | (uintptr_t)dy) & 15) return ADM_EINVAL;
  const long blocks = pe_bwd_blocks(p.T, E);
#define PE_GO(G, Q) hipLaunchKernelGGL((patch_embed_ln_bwd_kernel<G, Q>), dim3((unsigned)blocks), dim3(PE_WAVES * 64), 0, stream, p, w, cb, gamma, dy, ws, eps)
  PE_DISPATCH(E);
#undef PE_GO
  ADM_CHECK_LAUNCH();
  hipLaunchKernelGGL(patch_embed_bwd_reduce, dim3((unsigned)adm_cdiv((long)PE_PART * E, 256)), dim3(256), 0, stream, ws, dW, db, dgamma,
                     dbeta, blocks, E, accumulate);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

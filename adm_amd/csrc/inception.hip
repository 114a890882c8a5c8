// Forward-only kernels of the InceptionV3 feature extractor behind FID / Inception score (adm_amd/metrics/).
//
//   adm_conv_rect_relu_fwd  implicit-GEMM conv for kh x kw filters (each side 1, 3, 5 or 7), stride 1 / 2, separate pad_h / pad_w,
//                           on the exact f32 MFMA; epilogue relu(acc + bias), written into a channel slice of a wider buffer
//   adm_pool3x3_fwd         3x3 max (stride 2 no padding / stride 1 pad 1 with -inf) and average (stride 1 pad 1, in-image count)
//   adm_global_avgpool_fwd  [B][H][W][C] -> [B][C], float64 accumulation in a fixed order
//   adm_tf1_resize_norm_u8  uint8 NCHW -> [B][299][299][32] f32, TensorFlow-1 bilinear resize + (v - 128) / 128, bit for bit
//   adm_feat_stats_accum    shifted float64 sums and outer products of feature rows, one thread per output element
//
// Everything is NHWC float32 with channels padded to 32.  The conv follows igemm_f32_kernel (conv_igemm.hip): LDS-DMA staging,
// XOR-swizzled 16-byte slots, v_mfma_f32_32x32x2_f32, and the buffer range check as the zero padding.  What differs is the tap
// geometry (a kh x kw window anchored at its top-left input pixel, which may lie outside the image) and the epilogue.
// This file is compiled with -ffp-contract=off (Makefile): the resize restates float32 arithmetic operation by operation.
#include "common.h"
#include "../../include/adm_hip.h"

namespace {

struct RectP {
  const float* x; const float* w; const float* bias; float* y;
  int M, N, Ho, Wo, Hin, Win, Cin, ldx, K, ldy, kh, kw, stride, pad_h, pad_w, act, tilesN, xbytes, wbytes;
};

constexpr int LDSS = 32;   // floats per LDS row (LDS-DMA writes linearly; the 16-byte slots of a row are XOR-swizzled)
typedef __attribute__((address_space(3))) void lds_void;

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv_rect_kernel(RectP p) {
  constexpr int MT = BM / (WM * 32), NT = BN / (WN * 32);
  constexpr int AI = BM / 32, BI = BN / 32;         // LDS-DMA instructions per wave per stage (8 rows each)
  static_assert(WM * WN == 4, "4 waves");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                       // [2][BM][LDSS]
  float* Bs = smem + 2 * BM * LDSS;       // [2][BN][LDSS]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int bid = adm_xcd_remap(blockIdx.x, gridDim.x);
  const int tilesM = gridDim.x / p.tilesN;
  const int tm = bid % tilesM, tn = bid / tilesM;
  const int m0 = tm * BM, n0 = tn * BN;

  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, p.wbytes, 0x00020000);
  constexpr unsigned OOB = 0x80000000u;   // past every extent the host accepts: the range check returns zeros
  // Per A row: the window's top-left input pixel (oy*stride - pad_h, ox*stride - pad_w), each biased by 64 and packed in 16 bits,
  // and the byte offset of that pixel.  The pixel may be outside the image, so the offset may be "negative": unsigned arithmetic
  // wraps, and a tap's offset is only used after its own coordinates passed the bounds test.
  unsigned a_org[AI], a_pix[AI], a_voff[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = (wid * AI + i) * 8 + (lane >> 3);
    const int ls = (lane & 7) ^ ((row >> 1) & 7);
    const int m = m0 + row;
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    const int ox = mm % p.Wo;
    const int t = mm / p.Wo;
    const int oy = t % p.Ho;
    const int b = t / p.Ho;
    const int iy0 = oy * p.stride - p.pad_h, ix0 = ox * p.stride - p.pad_w;
    a_org[i] = ok ? (((unsigned)(iy0 + 64) << 16) | (unsigned)(ix0 + 64)) : 0xFFFFFFFFu;   // rows past M: no tap is in the image
    a_pix[i] = (unsigned)(((b * p.Hin + iy0) * p.Win + ix0) * p.ldx + ls * 4) * 4u;
    a_voff[i] = OOB;
  }
  const int cchunks = p.Cin >> 5;
  const int KT = p.kh * p.kw * cchunks;
  unsigned b_voff[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int row = (wid * BI + i) * 8 + (lane >> 3);
    const int ls = (lane & 7) ^ ((row >> 1) & 7);
    const int n = n0 + row;
    b_voff[i] = (n < p.N) ? (unsigned)(n * p.K + ls * 4) * 4u : OOB;
  }

  int ld_tap = 0, ld_cc = 0;        // (tap, channel chunk) of the next stage to load
  auto issue_stage = [&](int buf) {
    const int tap = ld_tap;
    if (ld_cc == 0) {               // new tap: rebuild the per-row offsets (wave-uniform branch, every Cin/32 steps)
      const int dy = tap / p.kw, dx = tap - dy * p.kw;
      const int off = (dy * p.Win + dx) * p.ldx * 4;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const int iy = (int)(a_org[i] >> 16) - 64 + dy, ix = (int)(a_org[i] & 0xFFFFu) - 64 + dx;
        const bool v = (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
        a_voff[i] = v ? a_pix[i] + (unsigned)off : OOB;
      }
    }
    const int c0b = ld_cc << 7;                                  // 32 floats = 128 bytes per chunk
    const int kb = (tap * p.Cin) * 4 + c0b;
    float* la = As + buf * BM * LDSS + wid * AI * 8 * LDSS;
    float* lb = Bs + buf * BN * LDSS + wid * BI * 8 * LDSS;
#pragma unroll
    for (int i = 0; i < AI; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void*)(la + i * 8 * LDSS), 16, (int)a_voff[i], c0b, 0, 0);
#pragma unroll
    for (int i = 0; i < BI; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(lb + i * 8 * LDSS), 16, (int)b_voff[i], kb, 0, 0);
    if (++ld_cc == cchunks) { ld_cc = 0; ++ld_tap; }
  };
  int foff[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) foff[g] = lr * LDSS + (((2 * g + lh) ^ ((lr >> 1) & 7)) << 2);

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issue_stage(0);
  __syncthreads();

  for (int s = 0; s < KT; ++s) {
    const int buf = s & 1;
    if (s + 1 < KT) issue_stage(buf ^ 1);
    const float* Ab = As + buf * BM * LDSS + wm * MT * 32 * LDSS;
    const float* Bb = Bs + buf * BN * LDSS + wn * NT * 32 * LDSS;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 a[MT], b[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDSS + foff[g]);
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDSS + foff[g]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][k], b[j][k], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: C/D layout col = lane&31, row = (r&3) + 8 (r>>2) + 4 (lane>>5).  N is a multiple of 32, so a 32-column block
  // is inside or outside as a whole; the packed weight and bias rows of padded lanes are zero, so those lanes get relu(0) = 0.
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + (wn * NT + j) * 32 + lr;
    if (n >= p.N) continue;
    const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int mb = m0 + (wm * MT + i) * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        if (m < p.M) {
          float v = acc[i][j][r] + bv;
          if (p.act) v = fmaxf(v, 0.f);
          p.y[(long)m * p.ldy + n] = v;
        }
      }
    }
  }
}

template <int BM, int BN, int WM, int WN>
int launch_rect(RectP p, hipStream_t st) {
  static bool attr_set = false;
  constexpr int smem = 2 * (BM + BN) * LDSS * (int)sizeof(float);
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_rect_kernel<BM, BN, WM, WN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return ADM_ELAUNCH;
    attr_set = true;
  }
  p.tilesN = adm_cdiv(p.N, BN);
  const long grid = (long)adm_cdiv(p.M, BM) * p.tilesN;
  hipLaunchKernelGGL((conv_rect_kernel<BM, BN, WM, WN>), dim3((unsigned)grid), dim3(256), smem, st, p);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

bool side_ok(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

// ---------------------------------------------------------------------------------------------- pooling
// mode 0: max, stride 2, no padding; 1: max, stride 1, pad 1 (padding = -inf: out-of-image taps are skipped);
// 2: average, stride 1, pad 1, divided by the number of in-image taps.  One thread per output pixel and channel quad.
__global__ void pool3x3_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C, int ldx, int Ho,
                               int Wo, int ldy, int mode) {
  const int C4 = C >> 2;
  const long total = (long)B * Ho * Wo * C4;
  const int stride = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    long t = i / C4;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    f32x4 a;
    const float init = mode == 2 ? 0.f : -INFINITY;
    a[0] = a[1] = a[2] = a[3] = init;
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = oy * stride - pad + dy;
      if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = ox * stride - pad + dx;
        if ((unsigned)ix >= (unsigned)W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((long)(b * H + iy) * W + ix) * ldx + c);
        if (mode == 2) {
          a += v;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) a[q] = fmaxf(a[q], v[q]);
        }
        ++cnt;
      }
    }
    if (mode == 2) {
      const float d = (float)cnt;
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = a[q] / d;
    }
    *reinterpret_cast<f32x4*>(y + ((long)(b * Ho + oy) * Wo + ox) * ldy + c) = a;
  }
}

// [B][HW][ldx] -> [B][C]: 64 channels x 4 pixel slices per workgroup; slice s sums pixels s, s+4, ... in float64, then the four
// partial sums are added in slice order.  The order is fixed, so the result is the same bits every run.
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int HW, int C,
                                                             int ldx) {
  __shared__ double part[4][64];
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
  double s = 0.0;
  if (c < C) {
    const float* xb = x + (long)b * HW * ldx + c;
    for (int p = sl; p < HW; p += 4) s += (double)xb[(long)p * ldx];
  }
  part[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && c < C) {
    const double t = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
    y[(long)b * C + c] = (float)(t / (double)HW);
  }
}

// ---------------------------------------------------------------------------------------------- TensorFlow-1 resize
// out[oy][ox] per channel: gx = float(ox) * sx (f32 product), lo = trunc(gx), hi = min(lo + 1, W - 1), d = gx - float(lo);
// r0 = a + (b - a) * d on the two rows, then r0 + (r1 - r0) * dy, then (v - 128) / 128.  Every step is one rounded f32 operation.
__global__ void tf1_resize_kernel(const unsigned char* __restrict__ img, float* __restrict__ y, int B, int H, int W, float sy,
                                  float sx, int OS) {
  const long total = (long)B * OS * OS;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % OS);
    const long t = i / OS;
    const int oy = (int)(t % OS);
    const int b = (int)(t / OS);
    const float gx = __fmul_rn((float)ox, sx), gy = __fmul_rn((float)oy, sy);
    const int x0 = (int)gx, y0 = (int)gy;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float dx = __fsub_rn(gx, (float)x0), dy = __fsub_rn(gy, (float)y0);
    f32x4 o;
    o[3] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned char* pl = img + ((long)b * 3 + c) * H * W;
      const float v00 = (float)pl[(long)y0 * W + x0], v01 = (float)pl[(long)y0 * W + x1];
      const float v10 = (float)pl[(long)y1 * W + x0], v11 = (float)pl[(long)y1 * W + x1];
      const float r0 = __fadd_rn(v00, __fmul_rn(__fsub_rn(v01, v00), dx));
      const float r1 = __fadd_rn(v10, __fmul_rn(__fsub_rn(v11, v10), dx));
      const float v = __fadd_rn(r0, __fmul_rn(__fsub_rn(r1, r0), dy));
      o[c] = __fdiv_rn(__fsub_rn(v, 128.f), 128.f);
    }
    f32x4* dst = reinterpret_cast<f32x4*>(y + i * 32);
    f32x4 z;
    z[0] = z[1] = z[2] = z[3] = 0.f;
    dst[0] = o;
#pragma unroll
    for (int q = 1; q < 8; ++q) dst[q] = z;
  }
}

// ---------------------------------------------------------------------------------------------- feature statistics
__global__ void stats_shift_kernel(const float* __restrict__ x, double* __restrict__ c, int n, int D) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= D) return;
  double s = 0.0;
  for (int r = 0; r < n; ++r) s += (double)x[(long)r * D + j];
  c[j] = s / (double)n;
}
__global__ void stats_sum_kernel(const float* __restrict__ x, const double* __restrict__ c, double* __restrict__ sum, int n, int D) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= D) return;
  const double cj = c[j];
  double s = sum[j];
  for (int r = 0; r < n; ++r) s += (double)x[(long)r * D + j] - cj;
  sum[j] = s;
}
// outer[i][j] += sum_r (x[r][i] - c[i]) (x[r][j] - c[j]); a 16 x 16 tile of outputs per workgroup, one output per thread, rows staged
// through LDS 16 at a time.  Rows are added in order; nothing is shared between threads but the staged operands.
__global__ __launch_bounds__(256) void stats_outer_kernel(const float* __restrict__ x, const double* __restrict__ c,
                                                          double* __restrict__ outer, int n, int D) {
  __shared__ double sa[16][17], sb[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  const int i = i0 + ty, j = j0 + tx;
  // staging role: thread (ty, tx) loads row r0 + ty, column i0 + tx / j0 + tx
  const int ci = i0 + tx, cj = j0 + tx;
  const double cvi = ci < D ? c[ci] : 0.0, cvj = cj < D ? c[cj] : 0.0;
  double acc = (i < D && j < D) ? outer[(long)i * D + j] : 0.0;
  for (int r0 = 0; r0 < n; r0 += 16) {
    const int r = r0 + ty;
    sa[ty][tx] = (r < n && ci < D) ? (double)x[(long)r * D + ci] - cvi : 0.0;
    sb[ty][tx] = (r < n && cj < D) ? (double)x[(long)r * D + cj] - cvj : 0.0;
    __syncthreads();
    const int rn = min(16, n - r0);
    for (int k = 0; k < rn; ++k) acc += sa[k][ty] * sb[k][tx];
    __syncthreads();
  }
  if (i < D && j < D) outer[(long)i * D + j] = acc;
}

}  // namespace

extern "C" int adm_conv_rect_relu_fwd(const float* x, const float* wp, const float* bias, float* y, int B, int Hin, int Win,
                                      int Cin, int ldx, int N, int ldy, int yoff, int kh, int kw, int stride, int pad_h,
                                      int pad_w, int act, int tile, hipStream_t stream) {
  if (!x || !wp || !y || B <= 0 || Hin <= 0 || Win <= 0) return ADM_EINVAL;
  if (!side_ok(kh) || !side_ok(kw) || (stride != 1 && stride != 2)) return ADM_EINVAL;
  if (pad_h < 0 || pad_w < 0 || pad_h > kh / 2 || pad_w > kw / 2) return ADM_EINVAL;
  if (Cin <= 0 || (Cin & 31) || (ldx & 3) || ldx < Cin || N <= 0 || (N & 31) || yoff < 0 || (yoff & 31) || yoff + N > ldy)
    return ADM_EINVAL;
  if (Hin + 2 * pad_h < kh || Win + 2 * pad_w < kw) return ADM_EINVAL;
  if (Hin >= 32000 || Win >= 32000) return ADM_EINVAL;                 // packed 16-bit window origins
  if (((uintptr_t)x | (uintptr_t)wp) & 15) return ADM_EINVAL;
  const int Ho = (Hin + 2 * pad_h - kh) / stride + 1, Wo = (Win + 2 * pad_w - kw) / stride + 1;
  if ((long)B * Ho * Wo >= (1L << 31)) return ADM_EINVAL;
  RectP p;
  p.x = x; p.w = wp; p.bias = bias; p.y = y + yoff;
  p.M = B * Ho * Wo; p.N = N; p.Ho = Ho; p.Wo = Wo; p.Hin = Hin; p.Win = Win;
  p.Cin = Cin; p.ldx = ldx; p.K = kh * kw * Cin; p.ldy = ldy; p.kh = kh; p.kw = kw; p.stride = stride;
  p.pad_h = pad_h; p.pad_w = pad_w; p.act = act; p.tilesN = 0;
  // extent of x as the kernel may read it: the last pixel's Cin channels end the buffer (x may be a channel slice of a wider one)
  const long xb = (((long)B * Hin * Win - 1) * ldx + Cin) * 4, wb = (long)N * p.K * 4;
  if (xb >= (1L << 31) || wb >= (1L << 31)) return ADM_EINVAL;         // 32-bit buffer offsets; 0x80000000 must stay out of range
  p.xbytes = (int)xb; p.wbytes = (int)wb;
  if (tile < 0) {
    // the cost model of conv_igemm.hip: whole rounds of resident workgroups, weighted by the tile's measured efficiency
    struct Cand { int id, bm, bn, per_cu; double eff; };
    const Cand cands[4] = {{0, 128, 128, 2, 1.00}, {1, 128, 96, 2, 0.97}, {2, 64, 64, 4, 0.90}, {3, 128, 32, 4, 0.70}};
    double best = 1e300;
    for (const Cand& c : cands) {
      const long tiles = (long)adm_cdiv(p.M, c.bm) * adm_cdiv(N, c.bn);
      const long slots = 256L * c.per_cu;
      const long rounds = (tiles + slots - 1) / slots;
      const double t = (double)rounds * c.per_cu * c.bm * c.bn / c.eff;
      if (t < best) { best = t; tile = c.id; }
    }
  }
  switch (tile) {
    case 0: return launch_rect<128, 128, 2, 2>(p, stream);
    case 1: return launch_rect<128, 96, 4, 1>(p, stream);
    case 2: return launch_rect<64, 64, 2, 2>(p, stream);
    case 3: return launch_rect<128, 32, 4, 1>(p, stream);
    default: return ADM_EINVAL;
  }
}

extern "C" int adm_pool3x3_fwd(const float* x, float* y, int B, int H, int W, int C, int ldx, int ldy, int yoff, int mode,
                               hipStream_t stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || (ldx & 3) || (ldy & 3) || ldx < C) return ADM_EINVAL;
  if (mode < 0 || mode > 2 || yoff < 0 || (yoff & 3) || yoff + C > ldy) return ADM_EINVAL;
  if (mode == 0 && (H < 3 || W < 3)) return ADM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return ADM_EINVAL;
  const int Ho = mode == 0 ? (H - 3) / 2 + 1 : H, Wo = mode == 0 ? (W - 3) / 2 + 1 : W;
  if ((long)B * H * W >= (1L << 31)) return ADM_EINVAL;
  const long total = (long)B * Ho * Wo * (C >> 2);
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(pool3x3_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, y + yoff, B, H, W, C, ldx, Ho, Wo, ldy, mode);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_global_avgpool_fwd(const float* x, float* y, int B, int H, int W, int C, int ldx, hipStream_t stream) {
  if (!x || !y || B <= 0 || B > 65535 || H <= 0 || W <= 0 || C <= 0 || ldx < C || (long)H * W >= (1L << 31)) return ADM_EINVAL;
  hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)adm_cdiv(C, 64), (unsigned)B), dim3(256), 0, stream, x, y, H * W, C, ldx);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_tf1_resize_norm_u8(const unsigned char* img, float* y, int B, int H, int W, hipStream_t stream) {
  if (!img || !y || B <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384 || ((uintptr_t)y & 15)) return ADM_EINVAL;
  constexpr int OS = 299;
  if ((long)B * OS * OS * 32 >= (1L << 31)) return ADM_EINVAL;
  // the scale is the float32 rounding of the double quotient in / out, as the reference's torch.tensor(in / out, float32)
  const float sy = (float)((double)H / (double)OS), sx = (float)((double)W / (double)OS);
  const long total = (long)B * OS * OS;
  long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(tf1_resize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, img, y, B, H, W, sy, sx, OS);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_feat_stats_accum(const float* x, int n, int D, double* shift, double* sum, double* outer, int first,
                                    hipStream_t stream) {
  if (!x || !shift || !sum || !outer || n <= 0 || D <= 0 || D > 65535 * 16) return ADM_EINVAL;
  const int cb = adm_cdiv(D, 256);
  if (first) {
    hipLaunchKernelGGL(stats_shift_kernel, dim3(cb), dim3(256), 0, stream, x, shift, n, D);
    ADM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(stats_sum_kernel, dim3(cb), dim3(256), 0, stream, x, (const double*)shift, sum, n, D);
  ADM_CHECK_LAUNCH();
  const int tb = adm_cdiv(D, 16);
  hipLaunchKernelGGL(stats_outer_kernel, dim3(tb, tb), dim3(256), 0, stream, x, (const double*)shift, outer, n, D);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

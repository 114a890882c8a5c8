// The LPIPS branch of the pixel-space DDM loss (taming/modules/losses/lpips.py; ddm_const.py:351-358, ddm_const_2.py:242-251):
// everything around the VGG16 convolutions, which run on the conv kernels.  All kernels here are bandwidth-bound: 16-byte
// accesses on the NHWC side, wave64 shuffles for the per-position sums, and NO float atomics -- every sum has one fixed order,
// so the loss term and its gradient are bit-reproducible with and without ADM_DETERMINISTIC.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------------
// input: x_rec from the predictions, ScalingLayer, NCHW -> NHWC with 32 channels (3..31 zero)
// ---------------------------------------------------------------------------------------------------------------------------
// schedule: -1 the image itself (a = x), 0 'const' x_rec = -C_pred (ddm_const.py:326), 1 'const_2' x_rec = x_noisy - C_pred t - t noise_pred
// (ddm_const_2.py:217), 2 'linear' x_rec = x_noisy - K_pred t^2/2 - C_pred t - sqrt(t) noise_pred with a = theta_pred = [K_pred | C_pred],
// six channels (ddm_linear.py:173-176, 203-204).  Eight threads per pixel, one 16-byte store each: a wave writes 1 KiB contiguous.
__global__ __launch_bounds__(256) void lpips_input_kernel(const float* __restrict__ a, const float* __restrict__ n_pred,
                                                          const float* __restrict__ x_noisy, const float* __restrict__ t,
                                                          const float* __restrict__ shift, const float* __restrict__ scale,
                                                          f32x4* __restrict__ y, long pixels, int HW, int schedule) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long p = idx >> 3;
  if (p >= pixels) return;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if ((idx & 7) == 0) {
    const long b = p / HW, hw = p - b * HW;
    const float tb = schedule >= 1 ? t[b] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long i = (b * 3 + c) * HW + hw;
      float xr;
      if (schedule < 0) xr = a[i];
      else if (schedule == 0) xr = -a[i];
      else if (schedule == 1) xr = x_noisy[i] - a[i] * tb - tb * n_pred[i];
      else {
        const long ik = (b * 6 + c) * HW + hw;
        xr = ((x_noisy[i] - a[ik] * (tb * tb / 2.f)) - a[ik + 3L * HW] * tb) - sqrtf(tb) * n_pred[i];
      }
      v[c] = (xr - shift[c]) / scale[c];
    }
  }
  y[idx] = v;
}

// d x_rec = dy[.., c] / scale[c]; schedule -1: d_a = d x_rec; 0: d_c = -d x_rec; 1: d_c = d_n = -t d x_rec; 2: d_a = [-t^2/2 | -t] d x_rec
// (six channels), d_n = -sqrt(t) d x_rec.  One thread per pixel:
// one 16-byte load of the first four channels, three stores that are contiguous across the wave.
__global__ __launch_bounds__(256) void lpips_input_bwd_kernel(const f32x4* __restrict__ dy, const float* __restrict__ t,
                                                              const float* __restrict__ scale, float* __restrict__ d_a,
                                                              float* __restrict__ d_n, long pixels, int HW, int schedule) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const f32x4 g = dy[p * 8];
  const long b = p / HW, hw = p - b * HW;
  if (schedule == 2) {
    const float tb = t[b], mk = -(tb * tb / 2.f), ms = -sqrtf(tb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long i = (b * 3 + c) * HW + hw, ik = (b * 6 + c) * HW + hw;
      const float d = g[c] / scale[c];
      d_a[ik] = mk * d;
      d_a[ik + 3L * HW] = -tb * d;
      d_n[i] = ms * d;
    }
    return;
  }
  const float m = schedule < 0 ? 1.f : schedule == 0 ? -1.f : -t[b];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long i = (b * 3 + c) * HW + hw;
    const float d = m * (g[c] / scale[c]);
    d_a[i] = d;
    if (schedule == 1) d_n[i] = d;
  }
}

// One-channel image (the saliency map of the pixel-space recipe): ScalingLayer broadcasts it, (inp - shift) / scale with inp [B,1,H,W] and
// shift [1,3,1,1] gives three channels from the same x_rec (lpips.py:56-63).  a, n_pred, x_noisy are [B][1][HW]; schedules -1, 0, 1 as
// above (the linear schedule is not built for one channel).  Same store pattern: eight threads per pixel, one 16-byte store each.
__global__ __launch_bounds__(256) void lpips_input_c1_kernel(const float* __restrict__ a, const float* __restrict__ n_pred,
                                                             const float* __restrict__ x_noisy, const float* __restrict__ t,
                                                             const float* __restrict__ shift, const float* __restrict__ scale,
                                                             f32x4* __restrict__ y, long pixels, int HW, int schedule) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long p = idx >> 3;
  if (p >= pixels) return;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if ((idx & 7) == 0) {
    float xr;
    if (schedule < 0) xr = a[p];
    else if (schedule == 0) xr = -a[p];
    else {
      const float tb = t[p / HW];
      xr = x_noisy[p] - a[p] * tb - tb * n_pred[p];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (xr - shift[c]) / scale[c];
  }
  y[idx] = v;
}

// d x_rec = dy[.., 0] / scale[0] + dy[.., 1] / scale[1] + dy[.., 2] / scale[2], summed in that order (no atomics: one thread owns the
// pixel), then the schedule's factor as in lpips_input_bwd_kernel.  One 16-byte load, one (schedule 1: two) contiguous 4-byte stores.
__global__ __launch_bounds__(256) void lpips_input_c1_bwd_kernel(const f32x4* __restrict__ dy, const float* __restrict__ t,
                                                                 const float* __restrict__ scale, float* __restrict__ d_a,
                                                                 float* __restrict__ d_n, long pixels, int HW, int schedule) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const f32x4 g = dy[p * 8];
  const float m = schedule < 0 ? 1.f : schedule == 0 ? -1.f : -t[p / HW];
  const float d = m * ((g[0] / scale[0] + g[1] / scale[1]) + g[2] / scale[2]);
  d_a[p] = d;
  if (schedule == 1) d_n[p] = d;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2x2 max-pool, stride 2, NHWC
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2x2_fwd_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, long n, int Ho,
                                                             int Wo, int C4) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int q = (int)(idx % C4);
  long r = idx / C4;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const long b = r / Ho;
  const long row = (long)2 * Wo * C4;
  const f32x4* s = x + ((b * 2 * Ho + 2 * oy) * 2 * Wo + 2 * ox) * C4 + q;
  const f32x4 a = s[0], c = s[C4], d = s[row], e = s[row + C4];
  f32x4 m;
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = fmaxf(fmaxf(a[k], c[k]), fmaxf(d[k], e[k]));
  y[idx] = m;
}

// The gradient goes to the FIRST maximum of the window in the order (0,0), (0,1), (1,0), (1,1) -- what F.max_pool2d does on ties --
// found again from the saved input (no index tensor).  Every element of dx is written exactly once.
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ dy,
                                                             f32x4* __restrict__ dx, long n, int Ho, int Wo, int C4) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int q = (int)(idx % C4);
  long r = idx / C4;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const long b = r / Ho;
  const long row = (long)2 * Wo * C4;
  const long o = ((b * 2 * Ho + 2 * oy) * 2 * Wo + 2 * ox) * C4 + q;
  const f32x4 v0 = x[o], v1 = x[o + C4], v2 = x[o + row], v3 = x[o + row + C4];
  const f32x4 g = dy[idx];
  f32x4 g0, g1, g2, g3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int w = 0;
    float m = v0[k];
    if (v1[k] > m) { m = v1[k]; w = 1; }
    if (v2[k] > m) { m = v2[k]; w = 2; }
    if (v3[k] > m) { m = v3[k]; w = 3; }
    g0[k] = w == 0 ? g[k] : 0.f;
    g1[k] = w == 1 ? g[k] : 0.f;
    g2[k] = w == 2 ? g[k] : 0.f;
    g3[k] = w == 3 ? g[k] : 0.f;
  }
  dx[o] = g0;
  dx[o + C4] = g1;
  dx[o + row] = g2;
  dx[o + row + C4] = g3;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the head of one tap: normalize_tensor on both feature maps, squared difference, 1x1 `lin` conv, spatial mean (lpips.py:40-53,
// 115-121)
// ---------------------------------------------------------------------------------------------------------------------------
// Sixteen lanes share one position: lane l holds the channel quads l, l + 16, ... (NQ = C / 64 of them) of f0 and f1 in registers,
// so the norms come first and d = sum_c w_c (u_c - v_c)^2 is then formed directly (no expanded form, no cancellation).  A wave
// loads four neighbouring positions per instruction: NQ x 1 KiB contiguous for C = 64.
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

#define LPIPS_EPS 1e-10f

// grid (nblk, B): workgroup (j, b) sums d over positions [j * per, (j + 1) * per) of image b into part[b * nblk + j] in a fixed order
template <int NQ>
__global__ __launch_bounds__(256) void lpips_head_fwd_kernel(const f32x4* __restrict__ f0, const f32x4* __restrict__ f1,
                                                             const f32x4* __restrict__ w, float* __restrict__ part, int HW, int per) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int b = blockIdx.y, nblk = gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(p0 + per, HW);
  f32x4 wq[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) wq[i] = w[lane + 16 * i];
  float acc = 0.f;
  for (int p = p0 + grp; p < p0 + per; p += 16) {       // (uniform trip count: every lane takes part in the shuffles)
    const bool live = p < p1;
    const long o = ((long)b * HW + (live ? p : 0)) * (NQ * 16) + lane;
    f32x4 a[NQ], c[NQ];
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      a[i] = f0[o + 16 * i];
      c[i] = f1[o + 16 * i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s0 += a[i][k] * a[i][k];
        s1 += c[i][k] * c[i][k];
      }
    }
    const float r0 = 1.f / (sqrtf(group16_sum(s0)) + LPIPS_EPS), r1 = 1.f / (sqrtf(group16_sum(s1)) + LPIPS_EPS);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float e = a[i][k] * r0 - c[i][k] * r1;
        d += wq[i][k] * e * e;
      }
    d = group16_sum(d);
    if (live && lane == 0) acc += d;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(long)b * nblk + blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3]));
}

// out[b] = (accumulate ? out[b] : 0) + sum_j part[b][j] / HW: one wave per image, nblk <= 64
__global__ __launch_bounds__(64) void lpips_head_final_kernel(const float* __restrict__ part, float* __restrict__ out, int nblk,
                                                              float inv_hw, int accumulate) {
  const int b = blockIdx.x;
  float v = (int)threadIdx.x < nblk ? part[(long)b * nblk + threadIdx.x] : 0.f;
  v = wave_sum(v);
  if (threadIdx.x == 0) out[b] = (accumulate ? out[b] : 0.f) + v * inv_hw;
}

// d out[b] / d f0 at one position, times dout[b] / HW:  with n = |f0|, u = f0 / (n + eps), q_c = 2 w_c (u_c - v_c), S = sum_c q_c u_c
//   d f0_k = (q_k / (n + eps) - u_k S / n) dout[b] / HW
// At a position where f0 is entirely zero the reference's gradient is NaN (the derivative of sqrt at 0); this kernel returns ZERO
// there: such a position is a dead end of every ReLU before it, and a NaN would poison the whole step.
template <int NQ>
__global__ __launch_bounds__(256) void lpips_head_bwd_kernel(const f32x4* __restrict__ f0, const f32x4* __restrict__ f1,
                                                             const f32x4* __restrict__ w, const float* __restrict__ dout,
                                                             f32x4* __restrict__ df0, long positions, int HW, float inv_hw) {
  const int lane = threadIdx.x & 15;
  const long p = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = p < positions;
  const long o = (live ? p : 0) * (NQ * 16) + lane;
  f32x4 a[NQ], c[NQ];
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    a[i] = f0[o + 16 * i];
    c[i] = f1[o + 16 * i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s0 += a[i][k] * a[i][k];
      s1 += c[i][k] * c[i][k];
    }
  }
  const float n0 = sqrtf(group16_sum(s0));
  const float r0 = 1.f / (n0 + LPIPS_EPS), r1 = 1.f / (sqrtf(group16_sum(s1)) + LPIPS_EPS);
  float S = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const f32x4 wq = w[lane + 16 * i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float u = a[i][k] * r0;
      const float q = 2.f * wq[k] * (u - c[i][k] * r1);
      a[i][k] = u;
      c[i][k] = q;
      S += q * u;
    }
  }
  S = group16_sum(S);
  if (!live) return;
  const float g = dout[p / HW] * inv_hw;
  const float k1 = n0 > 0.f ? g * r0 : 0.f, k2 = n0 > 0.f ? g * S / n0 : 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    f32x4 d;
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = c[i][k] * k1 - a[i][k] * k2;
    df0[o + 16 * i] = d;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int adm_lpips_input(const float* a, const float* n_pred, const float* x_noisy, const float* t, const float* shift,
                               const float* scale, float* y, int B, int HW, int schedule, hipStream_t stream) {
  if (!a || !shift || !scale || !y || B <= 0 || HW <= 0 || schedule < -1 || schedule > 2 || !al16(y)) return ADM_EINVAL;
  if (schedule >= 1 && (!n_pred || !x_noisy || !t)) return ADM_EINVAL;
  const long pixels = (long)B * HW;
  hipLaunchKernelGGL(lpips_input_kernel, dim3(adm_cdiv(pixels * 8, 256)), dim3(256), 0, stream, a, n_pred, x_noisy, t, shift,
                     scale, reinterpret_cast<f32x4*>(y), pixels, HW, schedule);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_lpips_input_bwd(const float* dy, const float* t, const float* scale, float* d_a, float* d_n, int B, int HW,
                                   int schedule, hipStream_t stream) {
  if (!dy || !scale || !d_a || B <= 0 || HW <= 0 || schedule < -1 || schedule > 2 || !al16(dy)) return ADM_EINVAL;
  if (schedule >= 1 && (!t || !d_n)) return ADM_EINVAL;
  const long pixels = (long)B * HW;
  hipLaunchKernelGGL(lpips_input_bwd_kernel, dim3(adm_cdiv(pixels, 256)), dim3(256), 0, stream, reinterpret_cast<const f32x4*>(dy),
                     t, scale, d_a, d_n, pixels, HW, schedule);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_lpips_input_c1(const float* a, const float* n_pred, const float* x_noisy, const float* t, const float* shift,
                                  const float* scale, float* y, int B, int HW, int schedule, hipStream_t stream) {
  if (!a || !shift || !scale || !y || B <= 0 || HW <= 0 || schedule < -1 || schedule > 1 || !al16(y)) return ADM_EINVAL;
  if (schedule == 1 && (!n_pred || !x_noisy || !t)) return ADM_EINVAL;
  const long pixels = (long)B * HW;
  hipLaunchKernelGGL(lpips_input_c1_kernel, dim3(adm_cdiv(pixels * 8, 256)), dim3(256), 0, stream, a, n_pred, x_noisy, t, shift,
                     scale, reinterpret_cast<f32x4*>(y), pixels, HW, schedule);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_lpips_input_c1_bwd(const float* dy, const float* t, const float* scale, float* d_a, float* d_n, int B, int HW,
                                      int schedule, hipStream_t stream) {
  if (!dy || !scale || !d_a || B <= 0 || HW <= 0 || schedule < -1 || schedule > 1 || !al16(dy)) return ADM_EINVAL;
  if (schedule == 1 && (!t || !d_n)) return ADM_EINVAL;
  const long pixels = (long)B * HW;
  hipLaunchKernelGGL(lpips_input_c1_bwd_kernel, dim3(adm_cdiv(pixels, 256)), dim3(256), 0, stream,
                     reinterpret_cast<const f32x4*>(dy), t, scale, d_a, d_n, pixels, HW, schedule);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_maxpool2x2_fwd(const float* x, float* y, int B, int H, int W, int C, hipStream_t stream) {
  if (!x || !y || B <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1) || C <= 0 || (C & 3) || !al16(x) || !al16(y)) return ADM_EINVAL;
  const long n = (long)B * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_fwd_kernel, dim3(adm_cdiv(n, 256)), dim3(256), 0, stream, reinterpret_cast<const f32x4*>(x),
                     reinterpret_cast<f32x4*>(y), n, H / 2, W / 2, C / 4);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, hipStream_t stream) {
  if (!x || !dy || !dx || B <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1) || C <= 0 || (C & 3) || !al16(x) || !al16(dy) || !al16(dx))
    return ADM_EINVAL;
  const long n = (long)B * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3(adm_cdiv(n, 256)), dim3(256), 0, stream, reinterpret_cast<const f32x4*>(x),
                     reinterpret_cast<const f32x4*>(dy), reinterpret_cast<f32x4*>(dx), n, H / 2, W / 2, C / 4);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// workgroups per image of adm_lpips_head_fwd = floats per image of its `part` workspace
extern "C" int adm_lpips_head_blocks(int HW) {
  if (HW <= 0) return ADM_EINVAL;
  const int n = HW / 64;
  return n < 1 ? 1 : n > 64 ? 64 : n;
}

extern "C" int adm_lpips_head_fwd(const float* f0, const float* f1, const float* w, float* out, float* part, int B, int HW, int C,
                                  int accumulate, hipStream_t stream) {
  if (!f0 || !f1 || !w || !out || !part || B <= 0 || B > 65535 || HW <= 0 || !al16(f0) || !al16(f1) || !al16(w)) return ADM_EINVAL;
  const int nblk = adm_lpips_head_blocks(HW);
  const int per = (adm_cdiv(HW, nblk) + 15) / 16 * 16;
  const f32x4 *a = reinterpret_cast<const f32x4*>(f0), *c = reinterpret_cast<const f32x4*>(f1), *wq = reinterpret_cast<const f32x4*>(w);
  const dim3 grid(nblk, B);
  switch (C) {
    case 64: hipLaunchKernelGGL(lpips_head_fwd_kernel<1>, grid, dim3(256), 0, stream, a, c, wq, part, HW, per); break;
    case 128: hipLaunchKernelGGL(lpips_head_fwd_kernel<2>, grid, dim3(256), 0, stream, a, c, wq, part, HW, per); break;
    case 256: hipLaunchKernelGGL(lpips_head_fwd_kernel<4>, grid, dim3(256), 0, stream, a, c, wq, part, HW, per); break;
    case 512: hipLaunchKernelGGL(lpips_head_fwd_kernel<8>, grid, dim3(256), 0, stream, a, c, wq, part, HW, per); break;
    default: return ADM_EINVAL;
  }
  hipLaunchKernelGGL(lpips_head_final_kernel, dim3(B), dim3(64), 0, stream, part, out, nblk, 1.0f / (float)HW, accumulate);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_lpips_head_bwd(const float* f0, const float* f1, const float* w, const float* dout, float* df0, int B, int HW,
                                  int C, hipStream_t stream) {
  if (!f0 || !f1 || !w || !dout || !df0 || B <= 0 || HW <= 0 || !al16(f0) || !al16(f1) || !al16(w) || !al16(df0)) return ADM_EINVAL;
  const long positions = (long)B * HW;
  const f32x4 *a = reinterpret_cast<const f32x4*>(f0), *c = reinterpret_cast<const f32x4*>(f1), *wq = reinterpret_cast<const f32x4*>(w);
  f32x4* d = reinterpret_cast<f32x4*>(df0);
  const dim3 grid(adm_cdiv(positions, 16));
  const float inv = 1.0f / (float)HW;
  switch (C) {
    case 64: hipLaunchKernelGGL(lpips_head_bwd_kernel<1>, grid, dim3(256), 0, stream, a, c, wq, dout, d, positions, HW, inv); break;
    case 128: hipLaunchKernelGGL(lpips_head_bwd_kernel<2>, grid, dim3(256), 0, stream, a, c, wq, dout, d, positions, HW, inv); break;
    case 256: hipLaunchKernelGGL(lpips_head_bwd_kernel<4>, grid, dim3(256), 0, stream, a, c, wq, dout, d, positions, HW, inv); break;
    case 512: hipLaunchKernelGGL(lpips_head_bwd_kernel<8>, grid, dim3(256), 0, stream, a, c, wq, dout, d, positions, HW, inv); break;
    default: return ADM_EINVAL;
  }
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

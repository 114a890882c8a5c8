// The linear-drift DDM (ddm/ddm_linear.py): U(t) = K t^2 / 2 + C t with U(1) = -x0, i.e. C = -x0 - K / 2; the denoiser predicts
// theta = [K | C] (six channels) and the noise.  Schedule-side kernels, all bandwidth- and launch-bound on B x 3 x H x W tensors:
// one launch per logical step, 16-byte accesses wherever H W is a multiple of four (V = 4), a scalar form otherwise (V = 1).
// Layouts: NCHW; `n3` = 3 H W floats per image of x0 / noise / K / x_t / noise_pred, theta_pred has 2 n3 (K planes, then C planes).
#include "common.h"

namespace {

template <int V> struct Vec;
template <> struct Vec<4> { typedef f32x4 T; };
template <> struct Vec<1> { typedef float T; };
template <int V> __device__ __forceinline__ float lane(const typename Vec<V>::T& v, int j);
template <> __device__ __forceinline__ float lane<4>(const f32x4& v, int j) { return v[j]; }
template <> __device__ __forceinline__ float lane<1>(const float& v, int) { return v; }
template <int V> __device__ __forceinline__ void put(typename Vec<V>::T& v, int j, float f);
template <> __device__ __forceinline__ void put<4>(f32x4& v, int j, float f) { v[j] = f; }
template <> __device__ __forceinline__ void put<1>(float& v, int, float f) { v = f; }
template <int V> __device__ __forceinline__ typename Vec<V>::T ld(const float* p) { return *reinterpret_cast<const typename Vec<V>::T*>(p); }
template <int V> __device__ __forceinline__ void st(float* p, typename Vec<V>::T v) { *reinterpret_cast<typename Vec<V>::T*>(p) = v; }

__device__ __forceinline__ float clamp1(float k) { return fminf(fmaxf(k, -1.f), 1.f); }
__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// x_t = x0 + K/2 t^2 + C t + sqrt(t) eps,  K <- clamp(K, -1, 1),  C = -x0 - K/2   (ddm_linear.py:168-171, 198-200)
template <int V>
__global__ __launch_bounds__(256) void q_sample_linear_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                              const float* __restrict__ K, const float* __restrict__ t,
                                                              float* __restrict__ xt, long n3, long total) {
  typedef typename Vec<V>::T T;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (long)gridDim.x * 256 * V) {
    const float tt = t[i / n3], t2 = tt * tt, st_ = sqrtf(tt);
    T x = ld<V>(x0 + i), e = ld<V>(noise + i), k = ld<V>(K + i), o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float kh = clamp1(lane<V>(k, j)) / 2.f, xv = lane<V>(x, j);
      const float c = -1.f * xv - kh;
      put<V>(o, j, xv + kh * t2 + c * tt + st_ * lane<V>(e, j));
    }
    st<V>(xt + i, o);
  }
}

// The whole pixel-space loss of one image and its gradients in one pass (ddm_linear.py:201-240, MSE_Loss / MAE_Loss with their
// default 'mean' reduction).  With e1 = theta_pred - [K | C] (6 HW values), e2 = noise_pred - eps (3 HW) and
// d = x_rec - x0, x_rec = x_t - K_pred t^2/2 - C_pred t - sqrt(t) noise_pred:
//   per_simple[b] = w1 mean e1^2 + w2 mean e2^2                       (use_l1: [w1 (mean e1^2 + mean |e1|) + w2 (...)] / 2)
//   per_mae[b]    = mean |d|
// and, for the scalar  L = sum_b per_simple[b] / B + sum_b w3[b] per_mae[b]  (w3 carries the batch-coupled mean_b (1 - t_b)^2 / B),
//   d_theta, d_noise = dL / d theta_pred, dL / d noise_pred.
// grid (B, chunks): chunks == 1 gives each image one workgroup and a fixed summation order.
template <int V>
__global__ __launch_bounds__(256) void ddm_loss_linear_kernel(const float* __restrict__ theta, const float* __restrict__ np_,
                                                              const float* __restrict__ x0, const float* __restrict__ noise,
                                                              const float* __restrict__ K, const float* __restrict__ xt,
                                                              const float* __restrict__ t, const float* __restrict__ w,
                                                              float* __restrict__ per_simple, float* __restrict__ per_mae,
                                                              float* __restrict__ d_theta, float* __restrict__ d_n, float inv_b,
                                                              long n3, int use_l1) {
  typedef typename Vec<V>::T T;
  __shared__ float red[8];
  const int b = blockIdx.x;
  const float w1 = w[3 * b], w2 = w[3 * b + 1], w3 = w[3 * b + 2], tb = t[b];
  const float t2h = tb * tb / 2.f, sq = sqrtf(tb);
  const float m6 = 1.f / (float)(2 * n3), m3 = 1.f / (float)n3;
  // gradient factors: the squared terms, their L1 twins, the reconstruction term
  const float half = use_l1 ? 0.5f : 1.f;
  const float g1 = inv_b * half * w1 * m6, g2 = inv_b * half * w2 * m3, g3 = w3 * m3;
  float s1 = 0.f, a1 = 0.f, s2 = 0.f, a2 = 0.f, l1 = 0.f;
  const float* th = theta + (long)b * 2 * n3;
  float* dth = d_theta ? d_theta + (long)b * 2 * n3 : nullptr;
  for (long i = ((long)blockIdx.y * 256 + threadIdx.x) * V; i < n3; i += (long)gridDim.y * 256 * V) {
    const long k = (long)b * n3 + i;
    T kp = ld<V>(th + i), cp = ld<V>(th + n3 + i), e = ld<V>(np_ + k), x = ld<V>(x0 + k), ns = ld<V>(noise + k), kk = ld<V>(K + k),
      xn = ld<V>(xt + k), dk, dc, dn;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float kt = clamp1(lane<V>(kk, j)), xv = lane<V>(x, j);
      const float ct = -1.f * xv - kt / 2.f;
      const float ek = lane<V>(kp, j) - kt, ec = lane<V>(cp, j) - ct, en = lane<V>(e, j) - lane<V>(ns, j);
      const float d = (((lane<V>(xn, j) - lane<V>(kp, j) * t2h) - lane<V>(cp, j) * tb) - sq * lane<V>(e, j)) - xv;
      s1 += ek * ek + ec * ec;
      s2 += en * en;
      a1 += fabsf(ek) + fabsf(ec);
      a2 += fabsf(en);
      l1 += fabsf(d);
      const float sd = g3 * sgn(d);
      float gk = 2.f * g1 * ek, gc = 2.f * g1 * ec, gn = 2.f * g2 * en;
      if (use_l1) { gk += g1 * sgn(ek); gc += g1 * sgn(ec); gn += g2 * sgn(en); }
      put<V>(dk, j, gk - t2h * sd);
      put<V>(dc, j, gc - tb * sd);
      put<V>(dn, j, gn - sq * sd);
    }
    if (dth) {
      st<V>(dth + i, dk);
      st<V>(dth + n3 + i, dc);
      st<V>(d_n + k, dn);
    }
  }
  float simple = use_l1 ? 0.5f * (w1 * m6 * (s1 + a1) + w2 * m3 * (s2 + a2)) : w1 * m6 * s1 + w2 * m3 * s2;
  simple = wave_sum(simple);
  l1 = wave_sum(l1 * m3);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = simple; red[4 + (threadIdx.x >> 6)] = l1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float a = (red[0] + red[1]) + (red[2] + red[3]), c = (red[4] + red[5]) + (red[6] + red[7]);
    if (gridDim.y == 1) { per_simple[b] = a; per_mae[b] = c; }
    else { atomicAdd(&per_simple[b], a); atomicAdd(&per_mae[b], c); }
  }
}

// One Euler step of the reverse process on the fp32 state (ddm_linear.py:178-186, 299-304), per image t[b], s[b]:
//   K = clamp(K_pred, -1, 1);  x <- x + K s^2/2 - K t s - C s - s / sqrt(t) eps_pred + sqrt(s (t - s) / t) z
// last: clamp to +-scale_input, / scale_input, (x + 1) / 2   (:305-309)
template <int V>
__global__ __launch_bounds__(256) void sampler_step_linear_kernel(float* __restrict__ x, const float* __restrict__ theta,
                                                                  const float* __restrict__ np_, const float* __restrict__ z,
                                                                  const float* __restrict__ t, const float* __restrict__ s_,
                                                                  float scale_input, int last, long n3, long total) {
  typedef typename Vec<V>::T T;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (long)gridDim.x * 256 * V) {
    const long b = i / n3, r = i - b * n3;
    const float tt = t[b], s = s_[b];
    const float s2h = s * s, ts = tt * s, sn = s / sqrtf(tt), sigma = sqrtf(s * (tt - s) / tt);
    const float* th = theta + b * 2 * n3 + r;
    T xv = ld<V>(x + i), kp = ld<V>(th), cp = ld<V>(th + n3), e = ld<V>(np_ + i), zz = ld<V>(z + i), o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float k = clamp1(lane<V>(kp, j));
      float xn = (((lane<V>(xv, j) + k / 2.f * s2h) - k * ts) - lane<V>(cp, j) * s) - sn * lane<V>(e, j);
      xn += sigma * lane<V>(zz, j);
      if (last) {
        xn = fminf(fmaxf(xn, -scale_input), scale_input);
        if (scale_input != 1.f) xn = xn / scale_input;
        xn = (xn + 1.f) * 0.5f;
      }
      put<V>(o, j, xn);
    }
    st<V>(x + i, o);
  }
}

// NHWC [B HW][ldf] -> NCHW [B][C][HW] for a head of C <= 8 channels (the six-channel K | C head): one thread per pixel loads the
// first C channels with 16-byte loads and writes C plane elements, contiguous across the wave.  Nothing else is read.
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ f, int ldf, float* __restrict__ out, int C, int HW,
                                                           long pixels) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const f32x4* row = reinterpret_cast<const f32x4*>(f + p * ldf);
  const f32x4 lo = row[0];
  f32x4 hi = {0.f, 0.f, 0.f, 0.f};
  if (C > 4) hi = row[1];
  const long b = p / HW, hw = p - b * HW;
  float* o = out + b * C * HW + hw;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < C) o[(long)c * HW] = c < 4 ? lo[c & 3] : hi[c & 3];
}

// its adjoint: df[B HW][ldf] = dout (channels >= C zero), and the bound vector amax (may be NULL) raised to max |df|.  ldf / 4
// threads per pixel, one 16-byte store each.
__global__ __launch_bounds__(256) void nhwc_to_nchw_bwd_kernel(const float* __restrict__ dout, float* __restrict__ df, int ldf, int C, int HW,
                                                               long quads, float* __restrict__ amax) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int q4 = ldf >> 2;
  float am = 0.f;
  if (idx < quads) {
    const long p = idx / q4;
    const int q = (int)(idx - p * q4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (4 * q < C) {
      const long b = p / HW, hw = p - b * HW;
      const float* src = dout + b * C * HW + hw;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        if (c < C) { v[j] = src[(long)c * HW]; am = fmaxf(am, fabsf(v[j])); }
      }
    }
    reinterpret_cast<f32x4*>(df)[idx] = v;
  }
  adm_amax_commit(am, amax);
}

inline int grid_for(long items) {
  long b = (items + 255) / 256;
  if (b < 1) b = 1;
  if (b > 8192) b = 8192;
  return (int)b;
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int adm_q_sample_linear(const float* x0, const float* noise, const float* K, const float* t, float* xt, int B, long n3,
                                   hipStream_t stream) {
  if (!x0 || !noise || !K || !t || !xt || B <= 0 || n3 <= 0) return ADM_EINVAL;
  const long total = (long)B * n3;
  if (!(n3 & 3) && al16(x0) && al16(noise) && al16(K) && al16(xt))
    hipLaunchKernelGGL(q_sample_linear_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, stream, x0, noise, K, t, xt, n3, total);
  else
    hipLaunchKernelGGL(q_sample_linear_kernel<1>, dim3(grid_for(total)), dim3(256), 0, stream, x0, noise, K, t, xt, n3, total);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_ddm_loss_linear(const float* theta_pred, const float* n_pred, const float* x0, const float* noise, const float* K,
                                   const float* xt, const float* t, const float* w, float* per_simple, float* per_mae, float* d_theta,
                                   float* d_n, int B, long n3, int use_l1, hipStream_t stream) {
  if (!theta_pred || !n_pred || !x0 || !noise || !K || !xt || !t || !w || !per_simple || !per_mae || B <= 0 || n3 <= 0) return ADM_EINVAL;
  if ((d_theta == nullptr) != (d_n == nullptr)) return ADM_EINVAL;
  int chunks = 1;
  if (n3 > 65536) {           // large images: several workgroups per image, float atomics into zero-filled sums
    chunks = (int)((n3 + 4095) / 4096);
    if (chunks > 64) chunks = 64;
    if (hipMemsetAsync(per_simple, 0, sizeof(float) * B, stream) != hipSuccess) return ADM_ELAUNCH;
    if (hipMemsetAsync(per_mae, 0, sizeof(float) * B, stream) != hipSuccess) return ADM_ELAUNCH;
  }
  const float inv_b = 1.0f / (float)B;
  const bool vec = !(n3 & 3) && al16(theta_pred) && al16(n_pred) && al16(x0) && al16(noise) && al16(K) && al16(xt) && al16(d_theta) && al16(d_n);
  if (vec)
    hipLaunchKernelGGL(ddm_loss_linear_kernel<4>, dim3(B, chunks), dim3(256), 0, stream, theta_pred, n_pred, x0, noise, K, xt, t, w,
                       per_simple, per_mae, d_theta, d_n, inv_b, n3, use_l1);
  else
    hipLaunchKernelGGL(ddm_loss_linear_kernel<1>, dim3(B, chunks), dim3(256), 0, stream, theta_pred, n_pred, x0, noise, K, xt, t, w,
                       per_simple, per_mae, d_theta, d_n, inv_b, n3, use_l1);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_sampler_step_linear(float* x, const float* theta_pred, const float* n_pred, const float* z, const float* t,
                                       const float* s, float scale_input, int last, int B, long n3, hipStream_t stream) {
  if (!x || !theta_pred || !n_pred || !z || !t || !s || B <= 0 || n3 <= 0 || !(scale_input > 0.f)) return ADM_EINVAL;
  const long total = (long)B * n3;
  if (!(n3 & 3) && al16(x) && al16(theta_pred) && al16(n_pred) && al16(z))
    hipLaunchKernelGGL(sampler_step_linear_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, stream, x, theta_pred, n_pred, z, t, s,
                       scale_input, last, n3, total);
  else
    hipLaunchKernelGGL(sampler_step_linear_kernel<1>, dim3(grid_for(total)), dim3(256), 0, stream, x, theta_pred, n_pred, z, t, s,
                       scale_input, last, n3, total);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_nhwc_to_nchw(const float* f, int ldf, float* out, int B, int C, int HW, hipStream_t stream) {
  if (!f || !out || B <= 0 || C <= 0 || C > 8 || HW <= 0 || ldf < 8 || (ldf & 3) || !al16(f)) return ADM_EINVAL;
  const long pixels = (long)B * HW;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(adm_cdiv(pixels, 256)), dim3(256), 0, stream, f, ldf, out, C, HW, pixels);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_nhwc_to_nchw_bwd_amax(const float* dout, float* df, int ldf, float* amax, int B, int C, int HW, hipStream_t stream) {
  if (!dout || !df || B <= 0 || C <= 0 || HW <= 0 || ldf < C || (ldf & 3) || !al16(df)) return ADM_EINVAL;
  const long quads = (long)B * HW * (ldf >> 2);
  if (quads > (1L << 31) - 256) return ADM_EINVAL;
  hipLaunchKernelGGL(nhwc_to_nchw_bwd_kernel, dim3(adm_cdiv(quads, 256)), dim3(256), 0, stream, dout, df, ldf, C, HW, quads, amax);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

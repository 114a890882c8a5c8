// Training of the KL autoencoder (ddm/encoder_decoder.py AutoencoderKL.training_step with ddm/loss.py LPIPSWithDiscriminator):
// the small kernels between the convolutions -- posterior sample + KL, the reconstruction / NLL term, the hinge and generator
// terms on the PatchGAN logit map, LeakyReLU, the row-softmax backward of the single-head attention block, a 2-D transpose for
// its operands, the adaptive discriminator weight.  All bandwidth-bound: 16-byte accesses where the layout allows, grid-stride
// loops, no float atomics: every sum is a per-workgroup fp64 partial (fixed order inside the workgroup) summed in block order by
// a second launch, so two runs give the same bits.
#include "common.h"

namespace {

constexpr int kMaxBlocks = 1024;

inline int ae_blocks_for(long n) {
  long b = (n / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}
inline int ew_grid(long items) {
  long b = (items + 255) / 256;
  if (b < 1) b = 1;
  if (b > 8192) b = 8192;
  return (int)b;
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Sum of K doubles per thread over a 256-thread workgroup; thread 0 returns the totals in v (waves combined in wave order).
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red /* [4 * K] */) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum_d(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
  }
}

// Sum of part[i * stride] for i < n by one 256-thread workgroup, fixed order; every thread returns the total.
__device__ __forceinline__ double tree_sum(const double* __restrict__ part, int n, int stride, double* red /* [256] */) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += part[(long)i * stride];
  __syncthreads();
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// ---------------------------------------------------------------- posterior sample + KL
// z[p][c] = mean + exp(0.5 clamp(logvar, -30, 20)) eps for c < C, zero in the pad channels [C, ldz);
// part[b][block] = sum over this block's share of (mean^2 + var - 1 - logvar).  One thread per (pixel, quad of ldz).
__global__ __launch_bounds__(256) void posterior_kl_fwd_kernel(const float* __restrict__ mom, int ldm, const float* __restrict__ eps,
                                                               float* __restrict__ z, int ldz, double* __restrict__ part, long HW,
                                                               int C) {
  __shared__ double red[4];
  const int b = blockIdx.y, q4 = ldz >> 2;
  const long items = HW * q4;
  double acc[1] = {0.0};
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
    const long p = (long)b * HW + i / q4;
    const int q = (int)(i % q4);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (4 * q < C) {
      const float* row = mom + p * ldm;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        if (c < C) {
          const float mean = row[c], lv = fminf(fmaxf(row[C + c], -30.0f), 20.0f);
          const float sd = expf(0.5f * lv);
          o[j] = mean + sd * eps[p * C + c];
          s += ((mean * mean + sd * sd) - 1.0f) - lv;
        }
      }
    }
    *reinterpret_cast<f32x4*>(z + p * ldz + 4 * q) = o;
  }
  acc[0] = (double)s;
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(256) void posterior_kl_final_kernel(const double* __restrict__ part, float* __restrict__ kl, int nblocks) {
  __shared__ double red[256];
  const double t = tree_sum(part + (long)blockIdx.x * nblocks, nblocks, 1, red);
  if (threadIdx.x == 0) kl[blockIdx.x] = (float)(0.5 * t);
}

// dmom[p][0:C) = dz + dkl[b] mean;  dmom[p][C:2C) = dz eps std / 2 + dkl[b] (var - 1) / 2 where logvar lies in [-30, 20], else 0
// (the clamp); zero in [2C, ldm).  One thread per (pixel, quad of ldm).
__global__ __launch_bounds__(256) void posterior_kl_bwd_kernel(const float* __restrict__ mom, int ldm, const float* __restrict__ eps,
                                                               const float* __restrict__ dz, int lddz, const float* __restrict__ dkl,
                                                               float* __restrict__ dmom, long HW, long items, int C) {
  const int q4 = ldm >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
    const long p = i / q4;
    const int q = (int)(i % q4);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (4 * q < 2 * C) {
      const float* row = mom + p * ldm;
      const float gk = dkl ? dkl[p / HW] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = 4 * q + j;
        if (ch < C) {
          o[j] = (dz ? dz[p * lddz + ch] : 0.f) + gk * row[ch];
        } else if (ch < 2 * C) {
          const int c = ch - C;
          const float lv = row[ch];
          if (lv >= -30.0f && lv <= 20.0f) {
            const float sd = expf(0.5f * lv);
            o[j] = (dz ? dz[p * lddz + c] * eps[p * C + c] * 0.5f * sd : 0.f) + gk * 0.5f * (sd * sd - 1.0f);
          }
        }
      }
    }
    *reinterpret_cast<f32x4*>(dmom + p * ldm + 4 * q) = o;
  }
}

// ---------------------------------------------------------------- reconstruction / NLL
template <int V>
__global__ __launch_bounds__(256) void nll_fwd_kernel(const float* __restrict__ x, const float* __restrict__ r, double* __restrict__ part,
                                                      long n) {
  __shared__ double red[4];
  double acc[1] = {0.0};
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (long)gridDim.x * 256 * V) {
    float t = 0.f;
    if (V == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + i), c = *reinterpret_cast<const f32x4*>(r + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = a[j] - c[j]; t += fabsf(d) + d * d; }
    } else {
      const float d = x[i] - r[i];
      t = fabsf(d) + d * d;
    }
    acc[0] += (double)t;
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// out = {nll_loss, rec_loss, d nll / d logvar, gscale}:  S = sum rec + pw n_per sum_b p[b] (the [B,1,1,1] LPIPS value is broadcast
// over the n_per elements of its image), N = B n_per:  nll = (S e^-lv + N lv) / B,  rec = S / N,  dlv = (N - S e^-lv) / B,
// gscale = e^-lv / B  (= d nll / d rec per element; d nll / d p[b] = pw n_per gscale).
__global__ __launch_bounds__(256) void nll_final_kernel(const double* __restrict__ part, int nblocks, const float* __restrict__ p,
                                                        const float* __restrict__ logvar, float* __restrict__ out, int B, long n_per,
                                                        float pw) {
  __shared__ double red[256];
  const double S0 = tree_sum(part, nblocks, 1, red);
  if (threadIdx.x == 0) {
    double sp = 0.0;
    if (p) for (int b = 0; b < B; ++b) sp += (double)p[b];
    const double S = S0 + (double)pw * (double)n_per * sp, N = (double)B * (double)n_per, lv = (double)logvar[0], e = exp(-lv);
    out[0] = (float)((S * e + N * lv) / B);
    out[1] = (float)(S / N);
    out[2] = (float)((N - S * e) / B);
    out[3] = (float)(e / B);
  }
}

// g = gscale[0] mul (sign(r - x) + 2 (r - x))
template <int V>
__global__ __launch_bounds__(256) void nll_bwd_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                      const float* __restrict__ gscale, float mul, float* __restrict__ g, long n) {
  const float s = gscale[0] * mul;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (long)gridDim.x * 256 * V) {
    if (V == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + i), c = *reinterpret_cast<const f32x4*>(r + i);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = c[j] - a[j]; o[j] = s * (sgn(d) + 2.f * d); }
      *reinterpret_cast<f32x4*>(g + i) = o;
    } else {
      const float d = r[i] - x[i];
      g[i] = s * (sgn(d) + 2.f * d);
    }
  }
}

// ---------------------------------------------------------------- hinge / generator terms on the logit map
// logits [M][ld], channel 0 is the logit, the rest is the NHWC pad.  part[block][3] = sums of relu(1 - l), relu(1 + l), l.
__global__ __launch_bounds__(256) void logit_terms_fwd_kernel(const float* __restrict__ logits, int ld, double* __restrict__ part, long M) {
  __shared__ double red[12];
  float a = 0.f, b = 0.f, c = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long)gridDim.x * 256) {
    const float l = logits[i * ld];
    a += fmaxf(1.f - l, 0.f);
    b += fmaxf(1.f + l, 0.f);
    c += l;
  }
  double acc[3] = {(double)a, (double)b, (double)c};
  block_sum<3>(acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) part[(long)blockIdx.x * 3 + k] = acc[k];
  }
}

__global__ __launch_bounds__(256) void logit_terms_final_kernel(const double* __restrict__ part, int nblocks, float* __restrict__ out, long M) {
  __shared__ double red[256];
  for (int k = 0; k < 3; ++k) {
    const double t = tree_sum(part + k, nblocks, 3, red);
    if (threadIdx.x == 0) out[k] = (float)(t / (double)M);
  }
}

// dlogits [M][ld]: channel 0 = s * {mode 0: -(l < 1), 1: (l > -1), 2: 1} with s = mul (coef ? coef[0] : 1) / M; the pad is zero.
__global__ __launch_bounds__(256) void logit_terms_bwd_kernel(const float* __restrict__ logits, int ld, int mode,
                                                              const float* __restrict__ coef, float mul, float* __restrict__ dl, long M,
                                                              long items) {
  const int q4 = ld >> 2;
  const float s = mul * (coef ? coef[0] : 1.f) / (float)M;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
    const long p = i / q4;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (i == p * q4) {
      const float l = logits[p * ld];
      o[0] = mode == 0 ? (l < 1.f ? -s : 0.f) : mode == 1 ? (l > -1.f ? s : 0.f) : s;
    }
    *reinterpret_cast<f32x4*>(dl + i * 4) = o;
  }
}

// ---------------------------------------------------------------- LeakyReLU
__global__ __launch_bounds__(256) void leaky_relu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out,
                                                         long n4, float slope) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 o;
    if (dy) {
      const f32x4 g = reinterpret_cast<const f32x4*>(dy)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = v[j] > 0.f ? g[j] : slope * g[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = v[j] > 0.f ? v[j] : slope * v[j];
    }
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

// ---------------------------------------------------------------- row-softmax backward
// In place on dP: dS = scale P (dP - sum_j dP_j P_j) per row; one workgroup per row, both rows cached in registers (cols <= 8192).
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, int cols, long ld,
                                                               float scale) {
  __shared__ float red[4];
  const float* prow = P + (long)blockIdx.x * ld;
  float* drow = dP + (long)blockIdx.x * ld;
  const int tid = threadIdx.x, nv = cols >> 2;
  f32x4 pv[8], dv[8];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = tid + i * 256;
    if (q < nv) {
      pv[i] = *reinterpret_cast<const f32x4*>(prow + 4 * q);
      dv[i] = *reinterpret_cast<const f32x4*>(drow + 4 * q);
      dot += (pv[i][0] * dv[i][0] + pv[i][1] * dv[i][1]) + (pv[i][2] * dv[i][2] + pv[i][3] * dv[i][3]);
    }
  }
  dot = wave_sum(dot);
  if ((tid & 63) == 0) red[tid >> 6] = dot;
  __syncthreads();
  dot = (red[0] + red[1]) + (red[2] + red[3]);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = tid + i * 256;
    if (q < nv) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = scale * pv[i][j] * (dv[i][j] - dot);
      *reinterpret_cast<f32x4*>(drow + 4 * q) = o;
    }
  }
}

// longer rows: two passes over the pair of rows (they stay in the L2 between the passes)
__global__ __launch_bounds__(256) void softmax_rows_bwd_long_kernel(const float* __restrict__ P, float* __restrict__ dP, int cols, long ld,
                                                                    float scale) {
  __shared__ float red[4];
  const float* prow = P + (long)blockIdx.x * ld;
  float* drow = dP + (long)blockIdx.x * ld;
  const int tid = threadIdx.x, nv = cols >> 2;
  float dot = 0.f;
  for (int q = tid; q < nv; q += 256) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(prow + 4 * q), d = *reinterpret_cast<const f32x4*>(drow + 4 * q);
    dot += (p[0] * d[0] + p[1] * d[1]) + (p[2] * d[2] + p[3] * d[3]);
  }
  dot = wave_sum(dot);
  if ((tid & 63) == 0) red[tid >> 6] = dot;
  __syncthreads();
  dot = (red[0] + red[1]) + (red[2] + red[3]);
  for (int q = tid; q < nv; q += 256) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(prow + 4 * q), d = *reinterpret_cast<const f32x4*>(drow + 4 * q);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = scale * p[j] * (d[j] - dot);
    *reinterpret_cast<f32x4*>(drow + 4 * q) = o;
  }
}

// ---------------------------------------------------------------- transpose
// out[c][r] = in[r][c] through a 64 x 64 LDS tile (row stride 65: conflict-free column reads); 16-byte global accesses.
// rows, cols multiples of 4.
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
  __shared__ float tile[64][65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tq = threadIdx.x & 15, tr = threadIdx.x >> 4;      // 16 quads across, 16 rows per pass
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + tr + 16 * k, c = c0 + 4 * tq;
    if (r < rows && c < cols) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(in + (long)r * cols + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[tr + 16 * k][4 * tq + j] = v[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + tr + 16 * k, r = r0 + 4 * tq;      // output row c, output columns r .. r + 3
    if (c < cols && r < rows) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = tile[4 * tq + j][tr + 16 * k];
      *reinterpret_cast<f32x4*>(out + (long)c * rows + r) = v;
    }
  }
}

// ---------------------------------------------------------------- adaptive weight
__global__ __launch_bounds__(256) void sumsq_part_kernel(const float* __restrict__ g, double* __restrict__ part, long n) {
  __shared__ double red[4];
  float s = 0.f;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  if (blockIdx.x == 0 && (long)threadIdx.x < (n & 3)) { const float v = g[(n4 << 2) + threadIdx.x]; s += v * v; }
  double acc[1] = {(double)s};
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// out[0] = clamp(|a| / (|b| + 1e-4), 0, 1e4) * disc_weight   (LPIPSWithDiscriminator.calculate_adaptive_weight)
__global__ __launch_bounds__(256) void adaptive_weight_final_kernel(const double* __restrict__ part, int na, int nb, float disc_weight,
                                                                    float* __restrict__ out) {
  __shared__ double red[256];
  const double sa = tree_sum(part, na, 1, red);
  const double sb = tree_sum(part + na, nb, 1, red);
  if (threadIdx.x == 0) {
    float w = sqrtf((float)sa) / (sqrtf((float)sb) + 1e-4f);
    w = fminf(fmaxf(w, 0.f), 1e4f);
    out[0] = w * disc_weight;
  }
}

// out = a + coef[0] mul b
__global__ __launch_bounds__(256) void axpy_dev_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ coef,
                                                       float mul, float* __restrict__ out, long n4) {
  const float s = coef[0] * mul;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 u = reinterpret_cast<const f32x4*>(a)[i], v = reinterpret_cast<const f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(out)[i] = u + v * s;
  }
}

}  // namespace

extern "C" int adm_ae_blocks(long n) { return n > 0 ? ae_blocks_for(n) : 0; }

extern "C" int adm_posterior_kl_fwd(const float* moments, int ldm, const float* eps, float* z, int ldz, float* kl, double* part, int B,
                                    long HW, int C, hipStream_t stream) {
  if (!moments || !eps || !z || !kl || !part || B <= 0 || B > 65535 || HW <= 0 || C <= 0 || ldm < 2 * C || ldz < C || (ldz & 3) ||
      !al16(z))
    return ADM_EINVAL;
  const int nb = ae_blocks_for(HW * ldz);
  hipLaunchKernelGGL(posterior_kl_fwd_kernel, dim3(nb, B), dim3(256), 0, stream, moments, ldm, eps, z, ldz, part, HW, C);
  hipLaunchKernelGGL(posterior_kl_final_kernel, dim3(B), dim3(256), 0, stream, part, kl, nb);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_posterior_kl_bwd(const float* moments, int ldm, const float* eps, const float* dz, int lddz, const float* dkl,
                                    float* dmoments, int B, long HW, int C, hipStream_t stream) {
  if (!moments || !eps || !dmoments || B <= 0 || HW <= 0 || C <= 0 || ldm < 2 * C || (ldm & 3) || !al16(dmoments)) return ADM_EINVAL;
  if (dz && lddz < C) return ADM_EINVAL;
  const long items = (long)B * HW * (ldm >> 2);
  hipLaunchKernelGGL(posterior_kl_bwd_kernel, dim3(ew_grid(items)), dim3(256), 0, stream, moments, ldm, eps, dz, lddz, dkl, dmoments, HW,
                     items, C);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_ae_nll_fwd(const float* x, const float* r, const float* p, const float* logvar, float* out, double* part, int B,
                              long n_per, float pw, hipStream_t stream) {
  if (!x || !r || !logvar || !out || !part || B <= 0 || n_per <= 0) return ADM_EINVAL;
  const long n = (long)B * n_per;
  const int nb = ae_blocks_for(n);
  if (!(n & 3) && al16(x) && al16(r)) hipLaunchKernelGGL(nll_fwd_kernel<4>, dim3(nb), dim3(256), 0, stream, x, r, part, n);
  else hipLaunchKernelGGL(nll_fwd_kernel<1>, dim3(nb), dim3(256), 0, stream, x, r, part, n);
  hipLaunchKernelGGL(nll_final_kernel, dim3(1), dim3(256), 0, stream, part, nb, p, logvar, out, B, n_per, pw);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_ae_nll_bwd(const float* x, const float* r, const float* gscale, float mul, float* g, long n, hipStream_t stream) {
  if (!x || !r || !gscale || !g || n <= 0) return ADM_EINVAL;
  if (!(n & 3) && al16(x) && al16(r) && al16(g))
    hipLaunchKernelGGL(nll_bwd_kernel<4>, dim3(ew_grid(n / 4)), dim3(256), 0, stream, x, r, gscale, mul, g, n);
  else
    hipLaunchKernelGGL(nll_bwd_kernel<1>, dim3(ew_grid(n)), dim3(256), 0, stream, x, r, gscale, mul, g, n);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_logit_terms_fwd(const float* logits, int ld, float* out, double* part, long M, hipStream_t stream) {
  if (!logits || !out || !part || M <= 0 || ld < 1) return ADM_EINVAL;
  const int nb = ae_blocks_for(M);
  hipLaunchKernelGGL(logit_terms_fwd_kernel, dim3(nb), dim3(256), 0, stream, logits, ld, part, M);
  hipLaunchKernelGGL(logit_terms_final_kernel, dim3(1), dim3(256), 0, stream, part, nb, out, M);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_logit_terms_bwd(const float* logits, int ld, int mode, const float* coef, float mul, float* dlogits, long M,
                                   hipStream_t stream) {
  if (!logits || !dlogits || M <= 0 || ld < 4 || (ld & 3) || mode < 0 || mode > 2 || !al16(dlogits)) return ADM_EINVAL;
  const long items = M * (ld >> 2);
  hipLaunchKernelGGL(logit_terms_bwd_kernel, dim3(ew_grid(items)), dim3(256), 0, stream, logits, ld, mode, coef, mul, dlogits, M, items);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_leaky_relu_fwd(const float* x, float* y, long n, float slope, hipStream_t stream) {
  if (!x || !y || n <= 0 || (n & 3) || !al16(x) || !al16(y)) return ADM_EINVAL;
  hipLaunchKernelGGL(leaky_relu_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, x, (const float*)nullptr, y, n / 4, slope);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_leaky_relu_bwd(const float* x, const float* dy, float* dx, long n, float slope, hipStream_t stream) {
  if (!x || !dy || !dx || n <= 0 || (n & 3) || !al16(x) || !al16(dy) || !al16(dx)) return ADM_EINVAL;
  hipLaunchKernelGGL(leaky_relu_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, x, dy, dx, n / 4, slope);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_softmax_rows_bwd(const float* P, float* dP, long rows, int cols, long ld, float scale, hipStream_t stream) {
  if (!P || !dP || rows <= 0 || rows >= (1L << 31) || cols <= 0 || (cols & 3) || cols > (1 << 20) || ld < cols || (ld & 3)) return ADM_EINVAL;
  if (!al16(P) || !al16(dP)) return ADM_EINVAL;
  if (cols > 8192) hipLaunchKernelGGL(softmax_rows_bwd_long_kernel, dim3((unsigned)rows), dim3(256), 0, stream, P, dP, cols, ld, scale);
  else hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, stream, P, dP, cols, ld, scale);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_transpose2d(const float* in, float* out, int rows, int cols, hipStream_t stream) {
  if (!in || !out || rows <= 0 || cols <= 0 || (rows & 3) || (cols & 3) || !al16(in) || !al16(out)) return ADM_EINVAL;
  const int gx = (cols + 63) / 64, gy = (rows + 63) / 64;
  if (gy > 65535) return ADM_EINVAL;
  hipLaunchKernelGGL(transpose_kernel, dim3(gx, gy), dim3(256), 0, stream, in, out, rows, cols);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_adaptive_weight(const float* a, long na, const float* b, long nb, double* part, float disc_weight, float* out,
                                   hipStream_t stream) {
  if (!a || !b || !part || !out || na <= 0 || nb <= 0 || !al16(a) || !al16(b)) return ADM_EINVAL;
  const int ba = ae_blocks_for(na), bb = ae_blocks_for(nb);
  hipLaunchKernelGGL(sumsq_part_kernel, dim3(ba), dim3(256), 0, stream, a, part, na);
  hipLaunchKernelGGL(sumsq_part_kernel, dim3(bb), dim3(256), 0, stream, b, part + ba, nb);
  hipLaunchKernelGGL(adaptive_weight_final_kernel, dim3(1), dim3(256), 0, stream, part, ba, bb, disc_weight, out);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_axpy_dev(const float* a, const float* b, const float* coef, float mul, float* out, long n, hipStream_t stream) {
  if (!a || !b || !coef || !out || n <= 0 || (n & 3) || !al16(a) || !al16(b) || !al16(out)) return ADM_EINVAL;
  hipLaunchKernelGGL(axpy_dev_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, a, b, coef, mul, out, n / 4);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// The restoration score's sums (adm_amd/metrics/restoration.py): per image and plane the exact integer sum of squared differences
// behind PSNR and the float64 sum of the SSIM map, made in one launch.
//
// Prediction and target are [B][C][H][W], C = 1 or 3, each uint8 or float32 (quantised as the samplers' PNG writer does:
// rintf(fminf(fmaxf(v, 0), 1) * 255), ties to even; fmaxf returns its other operand for a NaN, so NaN counts as byte 0).  s =
// crop_border pixels are skipped on every side by addressing alone: the scored area is H' x W' = (H - 2s) x (W - 2s).
// Planes: for C = 3 R, G, B and Y = 16 + N / 255000 with the integer N = 65481 R + 128553 G + 24966 B (< 2^26); for C = 1 the one.
//   SSE   the sum over the H' x W' area of d^2, d = p - g for a byte plane and N_p - N_g for Y (the host scales by 255000^-2): an
//         integer below 2^52 x 2^24, returned as two words {lo, hi}, value = hi 2^32 + lo, 0 <= lo < 2^32;
//   SSIM  the sum over the (H' - 10) x (W' - 10) valid positions of the 11 x 11 Gaussian-window (sigma 1.5) SSIM value.
// restoration_sums_kernel: workgroup (tile, b) of 256 threads owns a T x T tile of valid positions of image b, T = 32, and runs the
// planes one after another:
//   load    the (T + 10)^2 halo of both images into LDS as doubles, quantising and forming N on the way in -- four pixels of a halo
//           row per thread, one 4-byte (uint8) or 16-byte (float32) load where that address is aligned, single loads otherwise.  The
//           same pass adds d^2 over the pixels the tile OWNS: its T x T corner of the halo, and for the last tile row / column also the
//           10-pixel fringe, so every pixel of the area has exactly one owner;
//   rows    the 11-tap filter along x of p, g, p^2, g^2, p g into LDS: (T + 10) x T x 5 doubles;
//   columns the 11-tap filter along y and the SSIM value in registers, summed per thread;
//   reduce  xor-shuffle tree per wave, the four waves in index order.
// That is 28 KB + 53 KB of the CU's 160 KB of LDS.  The filter runs in float64: in float32 the cancellation in w*x^2 - mu^2 at magnitude
// 65025 against C2 = 58.5 costs 7e-5 on a flat 255 / 254 pair.  The file is compiled without fma contraction (Makefile): with
// p = g the numerator (2 mu mu + C1)(2 s + C2) and the denominator (mu mu + mu mu + C1)(s + s + C2) are then the same doubles and every
// SSIM value is exactly 1.
// Across workgroups, adm_depth_metrics' scheme: thread 0 writes the tile's sums to partial[b][tile], then takes an integer ticket;
// the last workgroup of an image adds all partials -- thread t those of tiles t, t + 256, ..., then thread 0 the 256 subtotals in
// index order -- whichever workgroup that is: no float atomics, the same bits every run.  A tile's SSE (< 2^52 x 42^2 < 2^63) is
// carried as its 32-bit halves, summed separately (fewer than 2^17 tiles: < 2^49) and normalised at the end.  The ticket returns to zero.
#include <cmath>

#include "common.h"

namespace {

constexpr int T = ADM_RESTORATION_TILE, K = ADM_RESTORATION_WINDOW, HALO = T + K - 1, NT = 256, WAVES = NT / 64;
constexpr double C1 = 6.5025, C2 = 58.5225;          // (0.01 x 255)^2, (0.03 x 255)^2

struct Window { double w[K]; };

__device__ __forceinline__ int quant(float v) { return (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

// the bytes of elements i .. i + n - 1 (n <= 4) of a plane; one wide load where n = 4 and the address allows
template <bool F32>
__device__ __forceinline__ void load4(const void* base, long i, int n, int v[4]) {
  if (F32) {
    const float* p = static_cast<const float*>(base) + i;
    if (n == 4 && !(reinterpret_cast<uintptr_t>(p) & 15)) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = quant(f[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < n ? quant(p[j]) : 0;
    }
  } else {
    const uint8_t* p = static_cast<const uint8_t*>(base) + i;
    if (n == 4 && !(reinterpret_cast<uintptr_t>(p) & 3)) {
      const unsigned u = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (int)((u >> (8 * j)) & 255u);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < n ? (int)p[j] : 0;
    }
  }
}

// plane `pl` of one image at elements i .. i + n - 1: a channel's bytes, or (pl = 3) the integer N of Y from the three channels
template <bool F32>
__device__ __forceinline__ void plane4(const void* img, long hw, int pl, long i, int n, int v[4]) {
  if (pl < 3) {
    load4<F32>(img, pl * hw + i, n, v);
  } else {
    int r[4], g[4], b[4];
    load4<F32>(img, i, n, r);
    load4<F32>(img, hw + i, n, g);
    load4<F32>(img, 2 * hw + i, n, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 65481 * r[j] + 128553 * g[j] + 24966 * b[j];
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool PF, bool GF>
__global__ __launch_bounds__(NT) void restoration_sums_kernel(const void* __restrict__ pred, const void* __restrict__ target,
                                                              long long* __restrict__ sse, double* __restrict__ ssim,
                                                              long long* partial, int* ticket, int C, int H, int W, int s,
                                                              int tiles_x, Window win) {
  __shared__ double s_p[HALO][HALO], s_g[HALO][HALO];
  __shared__ double s_row[5][HALO][T];
  __shared__ double s_wd[WAVES];
  __shared__ unsigned long long s_wu[WAVES];
  __shared__ int s_last;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, tile = blockIdx.x, nblk = gridDim.x, tiles_y = nblk / tiles_x;
  const int P = C == 3 ? 4 : 1;
  const int Hs = H - 2 * s, Ws = W - 2 * s, Hv = Hs - (K - 1), Wv = Ws - (K - 1);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int oy0 = ty * T, ox0 = tx * T;
  const int th = min(T, Hv - oy0), tw = min(T, Wv - ox0);          // valid positions of this tile
  const int hh = th + K - 1, hw = tw + K - 1;                      // its halo
  const int own_h = ty == tiles_y - 1 ? hh : th, own_w = tx == tiles_x - 1 ? hw : tw;
  const long plane = (long)H * W;
  const void* pimg = PF ? static_cast<const void*>(static_cast<const float*>(pred) + (long)b * C * plane)
                        : static_cast<const void*>(static_cast<const uint8_t*>(pred) + (long)b * C * plane);
  const void* gimg = GF ? static_cast<const void*>(static_cast<const float*>(target) + (long)b * C * plane)
                        : static_cast<const void*>(static_cast<const uint8_t*>(target) + (long)b * C * plane);

  unsigned long long tile_sse[4] = {0, 0, 0, 0};          // thread 0's: the tile's sums per plane
  double tile_ssim[4] = {0.0, 0.0, 0.0, 0.0};

  for (int pl = 0; pl < P; ++pl) {
    // ---- load: halo rows in groups of four pixels; SSE over the owned pixels
    unsigned long long acc = 0;
    const int ng = (hw + 3) >> 2;
    for (int it = tid; it < hh * ng; it += NT) {
      const int ly = it / ng, gx = (it - ly * ng) << 2, n = min(4, hw - gx);
      const long i = (long)(s + oy0 + ly) * W + (s + ox0 + gx);
      int pv[4], gv[4];
      plane4<PF>(pimg, plane, pl, i, n, pv);
      plane4<GF>(gimg, plane, pl, i, n, gv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          s_p[ly][gx + j] = pl < 3 ? (double)pv[j] : 16.0 + (double)pv[j] / 255000.0;
          s_g[ly][gx + j] = pl < 3 ? (double)gv[j] : 16.0 + (double)gv[j] / 255000.0;
          if (ly < own_h && gx + j < own_w) {
            const long long d = (long long)pv[j] - gv[j];
            acc += (unsigned long long)(d * d);
          }
        }
      }
    }
    __syncthreads();
    // ---- rows: the 11 taps along x of p, g, p^2, g^2, p g
    for (int it = tid; it < hh * tw; it += NT) {
      const int ly = it / tw, ox = it - ly * tw;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double p = s_p[ly][ox + k], g = s_g[ly][ox + k], w = win.w[k];
        a0 += w * p; a1 += w * g; a2 += w * (p * p); a3 += w * (g * g); a4 += w * (p * g);
      }
      s_row[0][ly][ox] = a0; s_row[1][ly][ox] = a1; s_row[2][ly][ox] = a2; s_row[3][ly][ox] = a3; s_row[4][ly][ox] = a4;
    }
    __syncthreads();
    // ---- columns: the 11 taps along y, then the SSIM value
    double sum = 0.0;
    for (int it = tid; it < th * tw; it += NT) {
      const int oy = it / tw, ox = it - oy * tw;
      double mp = 0.0, mg = 0.0, pp = 0.0, gg = 0.0, pg = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double w = win.w[k];
        mp += w * s_row[0][oy + k][ox]; mg += w * s_row[1][oy + k][ox]; pp += w * s_row[2][oy + k][ox];
        gg += w * s_row[3][oy + k][ox]; pg += w * s_row[4][oy + k][ox];
      }
      const double mpp = mp * mp, mgg = mg * mg, mpg = mp * mg;
      const double vp = pp - mpp, vg = gg - mgg, cov = pg - mpg;
      sum += ((2.0 * mpg + C1) * (2.0 * cov + C2)) / ((mpp + mgg + C1) * (vp + vg + C2));
    }
    // ---- reduce: shuffle tree per wave, the waves in index order
    sum = wave_sum_d(sum);
    acc = wave_sum_u64(acc);
    if (lane == 0) { s_wd[wave] = sum; s_wu[wave] = acc; }
    __syncthreads();
    if (tid == 0) {
      double v = s_wd[0];
      unsigned long long u = s_wu[0];
      for (int w = 1; w < WAVES; ++w) { v += s_wd[w]; u += s_wu[w]; }
      tile_ssim[pl] = v; tile_sse[pl] = u;
    }
    __syncthreads();          // (the next plane overwrites the halo and s_wd)
  }

  if (tid == 0) {
    long long* mine = partial + ((long)b * nblk + tile) * P * 2;
    for (int pl = 0; pl < P; ++pl) {
      mine[2 * pl] = (long long)tile_sse[pl];
      mine[2 * pl + 1] = __double_as_longlong(tile_ssim[pl]);
    }
    __threadfence();                                           // the partials are visible device-wide before the ticket is taken
    const int taken = __hip_atomic_fetch_add(ticket + b, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = taken == nblk - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                             // ... and read only after every other workgroup's ticket
  // the halo's LDS is free now: the 256 subtotals of a plane
  unsigned long long* s_lo = reinterpret_cast<unsigned long long*>(&s_p[0][0]);
  unsigned long long* s_hi = s_lo + NT;
  double* s_d = &s_g[0][0];
  const long long* all = partial + (long)b * nblk * P * 2;
  for (int pl = 0; pl < P; ++pl) {
    unsigned long long lo = 0, hi = 0;
    double d = 0.0;
    for (int k = tid; k < nblk; k += NT) {
      const unsigned long long u =
          (unsigned long long)__hip_atomic_load(all + ((long)k * P + pl) * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lo += u & 0xffffffffull; hi += u >> 32;
      d += __longlong_as_double(__hip_atomic_load(all + ((long)k * P + pl) * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    s_lo[tid] = lo; s_hi[tid] = hi; s_d[tid] = d;
    __syncthreads();
    if (tid == 0) {
      lo = 0; hi = 0; d = 0.0;
      for (int t = 0; t < NT; ++t) { lo += s_lo[t]; hi += s_hi[t]; d += s_d[t]; }
      sse[((long)b * P + pl) * 2] = (long long)(lo & 0xffffffffull);
      sse[((long)b * P + pl) * 2 + 1] = (long long)(hi + (lo >> 32));
      ssim[(long)b * P + pl] = d;
    }
    __syncthreads();
  }
  if (tid == 0) ticket[b] = 0;
}

}  // namespace

extern "C" int adm_restoration_blocks(int Hs, int Ws) {
  if (Hs < K || Ws < K) return ADM_EINVAL;
  const long tiles = (long)adm_cdiv(Hs - (K - 1), T) * adm_cdiv(Ws - (K - 1), T);
  return tiles > 0x7fffffffL ? ADM_EINVAL : (int)tiles;
}

extern "C" int adm_restoration_sums(const void* pred, int pred_is_f32, const void* target, int target_is_f32, int64_t* sse,
                                    double* ssim, int64_t* partial, int* ticket, int B, int C, int H, int W, int crop_border,
                                    hipStream_t stream) {
  if (!pred || !target || !sse || !ssim || !partial || !ticket) return ADM_EINVAL;
  if (B < 1 || B > 65535 || (C != 1 && C != 3) || crop_border < 0 || H < 1 || W < 1) return ADM_EINVAL;
  if ((long)H * W > ADM_RESTORATION_MAX_PIXELS) return ADM_EINVAL;
  const long Hs = (long)H - 2L * crop_border, Ws = (long)W - 2L * crop_border;
  if (Hs < K || Ws < K) return ADM_EINVAL;
  if ((pred_is_f32 && (reinterpret_cast<uintptr_t>(pred) & 3)) || (target_is_f32 && (reinterpret_cast<uintptr_t>(target) & 3)))
    return ADM_EINVAL;
  if ((reinterpret_cast<uintptr_t>(sse) & 7) || (reinterpret_cast<uintptr_t>(ssim) & 7) || (reinterpret_cast<uintptr_t>(partial) & 7) ||
      (reinterpret_cast<uintptr_t>(ticket) & 3))
    return ADM_EINVAL;
  const int tiles_x = adm_cdiv(Ws - (K - 1), T), nblk = adm_restoration_blocks((int)Hs, (int)Ws);
  if (nblk < 1) return ADM_EINVAL;
  Window win;
  double total = 0.0;
  for (int k = 0; k < K; ++k) {
    const double x = k - (K - 1) / 2;
    win.w[k] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5));
    total += win.w[k];
  }
  for (int k = 0; k < K; ++k) win.w[k] /= total;
  long long* out = reinterpret_cast<long long*>(sse);
  long long* part = reinterpret_cast<long long*>(partial);
  const dim3 grid((unsigned)nblk, (unsigned)B), block(NT);
#define ADM_RESTORATION_LAUNCH(PF, GF)                                                                                          \
  hipLaunchKernelGGL((restoration_sums_kernel<PF, GF>), grid, block, 0, stream, pred, target, out, ssim, part, ticket, C, H, W, \
                     crop_border, tiles_x, win)
  if (pred_is_f32 && target_is_f32) ADM_RESTORATION_LAUNCH(true, true);
  else if (pred_is_f32) ADM_RESTORATION_LAUNCH(true, false);
  else if (target_is_f32) ADM_RESTORATION_LAUNCH(false, true);
  else ADM_RESTORATION_LAUNCH(false, false);
#undef ADM_RESTORATION_LAUNCH
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

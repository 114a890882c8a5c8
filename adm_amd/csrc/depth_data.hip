// Depth-estimation batches (ddm.data.NYUDv2DepthDataset, ddm/data.py:869-887 of the reference) and the depth score, on the device.
//
// depth_batch_kernel: one launch makes the batch from a uint8 HWC photo pool and a 16-BIT depth pool (little-endian, two bytes per
// pixel, millimetres): the fixed border box, the random crop at (top, left) inside it, one flip draw for both planes, then
// (u8 / 255) * 2 - 1 and (u16 / 10000) * 2 - 1 -- no resize, no clipping (a raw 65535 becomes 12.107).  The kernel moves a few MB and
// is bound by the stores: a sample's output rows are contiguous, so the threads of a sample walk its H * W / PX groups of PX
// consecutive pixels in order and every store instruction of a wave covers one contiguous run.  PX = 4 (W % 4 == 0, outputs 16-byte
// aligned): one 16-byte store per plane and thread.  PX = 1 otherwise: with W % 4 != 0 no row but the first starts on a 16-byte
// boundary, so that form writes scalars, one pixel per thread, still in consecutive addresses across the wave.  Source rows start at
// any byte (3 bytes per pixel, any left offset, reversed under flip) and at any even byte for the depth plane, so the reads are
// byte and 16-bit loads, never wider; they are a quarter of the traffic and neighbouring lanes share their cache lines.
// The arithmetic needs no -ffp-contract=off: the divisions are IEEE (hipcc's default for f32) and t * 2 is exact, so an fma of
// t * 2 - 1 rounds once exactly where the two separate operations do.
//
// depth_metrics_kernel: the per-image float64 sums behind abs-rel / RMSE / delta (adm_amd/metrics/depth.py).  Workgroup (j, b) sums
// a contiguous chunk of image b in a fixed order (thread-strided, then shuffles, then the waves in order) and writes its ten
// partials; the last workgroup of an image to finish -- an integer ticket, no float atomics -- adds the partials in index order, so
// the result is the same bits every run.  The ticket returns to zero, so the workspace is zero at rest.
//
// Every read of a pool is guarded by the pool's size and the image's own size, and the draws are clamped: wrong tables or draws give
// wrong pixels, never an access out of bounds.
#include "common.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int NQ = ADM_DEPTH_SUMS;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Box {
  int left, top, right, bottom;
};

template <int PX>
__global__ __launch_bounds__(NT) void depth_batch_kernel(
    const unsigned char* __restrict__ rgb_pool, long rgb_bytes, const int64_t* __restrict__ rgb_off, const int* __restrict__ rgb_hw,
    const unsigned short* __restrict__ depth_pool, long depth_px, const int64_t* __restrict__ depth_off,
    const int* __restrict__ depth_hw, int n_images, Box box, const int* __restrict__ idx, const int* __restrict__ top,
    const int* __restrict__ left, const int* __restrict__ flip, float* __restrict__ image, float* __restrict__ cond, int H, int W) {
  const int b = blockIdx.y;
  const int per_row = W / PX;                                  // PX == 4 only with W % 4 == 0
  const long g = (long)blockIdx.x * NT + threadIdx.x;          // group of PX consecutive pixels of sample b
  if (g >= (long)H * per_row) return;
  const int y = (int)(g / per_row), x0 = (int)(g % per_row) * PX;

  const int n = clampi(idx[b], 0, n_images - 1);
  const int t = clampi(top[b], 0, (box.bottom - box.top) - H), l = clampi(left[b], 0, (box.right - box.left) - W);
  const bool fl = flip[b] != 0;
  const int sy = box.top + t + y;
  const int sx0 = box.left + l + (fl ? W - 1 - x0 : x0), step = fl ? -1 : 1;          // the source column of output column x0 + i is sx0 + i * step
  const long plane = (long)H * W, o = (long)y * W + x0;

  if (image) {
    const int ih = depth_hw[2 * n], iw = depth_hw[2 * n + 1];
    const long base = depth_off[n] >> 1;                       // (offsets are even: checked on the host)
    float v[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const int sx = sx0 + i * step;
      const long p = base + (long)sy * iw + sx;
      const bool ok = sy >= 0 && sy < ih && sx >= 0 && sx < iw && p >= 0 && p < depth_px;
      v[i] = (float)(ok ? (int)depth_pool[p] : 0) / 10000.0f * 2.0f - 1.0f;
    }
    float* dst = image + (long)b * plane + o;
    if constexpr (PX == 4) {
      *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      dst[0] = v[0];
    }
  }
  if (cond) {
    const int ih = rgb_hw[2 * n], iw = rgb_hw[2 * n + 1];
    const long base = rgb_off[n];
    float v[3][PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const int sx = sx0 + i * step;
      const long p = base + ((long)sy * iw + sx) * 3;
      const bool ok = sy >= 0 && sy < ih && sx >= 0 && sx < iw && p >= 0 && p + 2 < rgb_bytes;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][i] = (float)(ok ? (int)rgb_pool[p + c] : 0) / 255.0f * 2.0f - 1.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* dst = cond + ((long)b * 3 + c) * plane + o;
      if constexpr (PX == 4) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
      } else {
        dst[0] = v[c][0];
      }
    }
  }
}

__global__ __launch_bounds__(NT) void depth_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           double* __restrict__ sums, double* partial, int* ticket, long hw,
                                                           long chunk, double min_depth, double max_depth) {
  __shared__ double s_wave[NT / 64][NQ];
  __shared__ int s_last;
  const int b = blockIdx.y, j = blockIdx.x, nblk = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long begin = (long)j * chunk, end = min(begin + chunk, hw);
  const float* pp = pred + (long)b * hw;
  const float* gp = gt + (long)b * hw;

  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (long i = begin + threadIdx.x; i < end; i += NT) {
    const double g = (double)gp[i] * 10.0;                     // metres
    if (!(g > min_depth && g < max_depth)) continue;           // (a NaN ground truth is invalid)
    double p = (double)pp[i] * 10.0;
    p = p < min_depth ? min_depth : (p > max_depth ? max_depth : p);
    const double d = p - g, dl = log(p) - log(g), r = fmax(p / g, g / p);
    acc[0] += 1.0;
    acc[1] += fabs(d) / g;
    acc[2] += d * d / g;
    acc[3] += d * d;
    acc[4] += dl * dl;
    acc[5] += dl;
    acc[6] += fabs(log10(p) - log10(g));
    acc[7] += r < 1.25 ? 1.0 : 0.0;
    acc[8] += r < 1.5625 ? 1.0 : 0.0;
    acc[9] += r < 1.953125 ? 1.0 : 0.0;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double v = wave_sum_d(acc[q]);
    if (lane == 0) s_wave[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* mine = partial + ((long)b * nblk + j) * NQ;
    for (int q = 0; q < NQ; ++q) {
      double v = s_wave[0][q];
      for (int w = 1; w < NT / 64; ++w) v += s_wave[w][q];
      mine[q] = v;
    }
    __threadfence();                                           // the partials are visible device-wide before the ticket is taken
    const int taken = __hip_atomic_fetch_add(ticket + b, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = taken == nblk - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                             // ... and read only after every other workgroup's ticket
  if (threadIdx.x < NQ) {
    const volatile double* all = partial + (long)b * nblk * NQ;
    double v = 0.0;
    for (int k = 0; k < nblk; ++k) v += all[(long)k * NQ + threadIdx.x];
    sums[(long)b * NQ + threadIdx.x] = v;
  }
  if (threadIdx.x == 0) ticket[b] = 0;
}

}  // namespace

extern "C" int adm_depth_batch(const uint8_t* rgb_pool, long rgb_bytes, const int64_t* rgb_off, const int* rgb_hw,
                               const uint8_t* depth_pool, long depth_bytes, const int64_t* depth_off, const int* depth_hw,
                               int n_images, int box_left, int box_top, int box_right, int box_bottom, const int* idx,
                               const int* top, const int* left, const int* flip, float* image, float* cond, int B, int H, int W,
                               hipStream_t stream) {
  if (!idx || !top || !left || !flip || (!image && !cond)) return ADM_EINVAL;
  if (cond && (!rgb_pool || !rgb_off || !rgb_hw || rgb_bytes <= 0)) return ADM_EINVAL;
  if (image && (!depth_pool || !depth_off || !depth_hw || depth_bytes <= 0 || (depth_bytes & 1) ||
                (reinterpret_cast<uintptr_t>(depth_pool) & 1)))
    return ADM_EINVAL;                                         // 16-bit loads
  if (n_images <= 0 || B <= 0 || B > 65535 || H <= 0 || W <= 0) return ADM_EINVAL;
  if (box_left < 0 || box_top < 0 || box_right - box_left < W || box_bottom - box_top < H) return ADM_EINVAL;
  const Box box{box_left, box_top, box_right, box_bottom};
  const bool vec = W % 4 == 0 && !(reinterpret_cast<uintptr_t>(image) & 15) && !(reinterpret_cast<uintptr_t>(cond) & 15);
  const long groups = (long)H * (vec ? W / 4 : W);
  if ((groups + NT - 1) / NT > 0x7fffffffL) return ADM_EINVAL;
  const dim3 grid((unsigned)((groups + NT - 1) / NT), B);
  const unsigned short* d16 = reinterpret_cast<const unsigned short*>(depth_pool);
  if (vec)
    hipLaunchKernelGGL(depth_batch_kernel<4>, grid, dim3(NT), 0, stream, rgb_pool, rgb_bytes, rgb_off, rgb_hw, d16, depth_bytes >> 1,
                       depth_off, depth_hw, n_images, box, idx, top, left, flip, image, cond, H, W);
  else
    hipLaunchKernelGGL(depth_batch_kernel<1>, grid, dim3(NT), 0, stream, rgb_pool, rgb_bytes, rgb_off, rgb_hw, d16, depth_bytes >> 1,
                       depth_off, depth_hw, n_images, box, idx, top, left, flip, image, cond, H, W);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_depth_metrics_blocks(long hw) {
  if (hw <= 0) return ADM_EINVAL;
  const long want = (hw + ADM_DEPTH_CHUNK - 1) / ADM_DEPTH_CHUNK;
  return (int)(want < ADM_DEPTH_MAX_BLOCKS ? want : ADM_DEPTH_MAX_BLOCKS);
}

extern "C" int adm_depth_metrics(const float* pred, const float* gt, double* sums, double* partial, int* ticket, int B, long hw,
                                 double min_depth, double max_depth, hipStream_t stream) {
  if (!pred || !gt || !sums || !partial || !ticket || B <= 0 || B > 65535 || hw <= 0) return ADM_EINVAL;
  if (!(min_depth > 0.0) || !(max_depth > min_depth)) return ADM_EINVAL;          // the logarithms need positive depths
  const int nblk = adm_depth_metrics_blocks(hw);
  const long chunk = (hw + nblk - 1) / nblk;
  hipLaunchKernelGGL(depth_metrics_kernel, dim3(nblk, B), dim3(NT), 0, stream, pred, gt, sums, partial, ticket, hw, chunk, min_depth,
                     max_depth);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

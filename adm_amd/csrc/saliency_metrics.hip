// The saliency score's integer tables (adm_amd/metrics/saliency.py): per image ONE table from which MAE, the F-, E- and S-measure
// all follow on the host, made in one launch.
//
// With prediction bytes p(y, x), map bytes m(y, x), g = [m > 128] and N = H W, per image:
//   head   = { nF, sum x g, sum y g, cx, cy }: the foreground count, its 0-based coordinate sums and the split point
//            cx = X + 1, cy = Y + 1 with X = (2 sum x g + nF) / (2 nF) (round half up, in integers), Y likewise; X = W / 2,
//            Y = H / 2 without foreground;
//   tables[q][c][v] = the number of pixels with byte v and class c = g in quadrant q = 2 [y >= cy] + [x >= cx].
// saliency_tables_kernel: one workgroup of 1024 threads per image, nothing shared between workgroups.
//   pass 1  the map alone: per-thread integer sums of g, x g, y g, an xor-shuffle tree per wave, the sixteen waves through LDS,
//           thread 0 divides -> cx, cy (integers: the same on every run, whatever the order);
//   pass 2  prediction and map (the map now from L2) into a 4 x 2 x 256 histogram of uint32 in LDS with LDS integer atomics;
//   then    the histogram goes out widened to int64 with plain stores -- no global atomics, no ticket, no float anywhere past the
//           quantiser.
// Alignment: image k starts at byte k N of both planes, for odd sizes on no 16-byte boundary.  A workgroup takes the `lead` bytes
// up to the map's next 16-byte boundary and the tail past the last whole 16-byte chunk one pixel per thread, and the chunks between
// with one 16-byte load of the map per thread; the prediction's chunk is one 16-byte load (four for float32) where ITS address is
// aligned too, which holds whenever both planes start on a 16-byte boundary, and single loads otherwise.  A chunk's (y, x) costs
// one division; the sixteen pixels step x and wrap.
// Contention: real maps are almost all 0 and 255, so neighbouring pixels -- a thread's sixteen, and the sixteen of its next trip --
// share one bin.  A thread therefore keeps (key, count) of its current RUN and issues one LDS atomic per run, not per pixel: on a
// saturated pair that is a handful of atomics per thread, on uniform-random bytes one per pixel, where the lanes spread over 256+
// bins and the banks anyway (tools/saliency_metrics_cost.py measures both).
// A float32 prediction is quantised as the samplers' PNG writer does: rintf(fminf(fmaxf(p, 0), 1) * 255), ties to even; fmaxf
// returns its other operand for a NaN, so NaN counts as byte 0.
#include "common.h"

namespace {

constexpr int NT = 1024, WAVES = NT / 64, BINS = ADM_SALIENCY_BINS;

__device__ __forceinline__ unsigned quant(float p) { return (unsigned)rintf(fminf(fmaxf(p, 0.f), 1.f) * 255.f); }

// the sixteen prediction bytes of pixels i .. i + 15, packed little-endian as the map's own 16-byte load is
template <bool F32>
__device__ __forceinline__ u32x4 pred16(const void* pred, long i, bool wide) {
  u32x4 r;
  if (F32) {
    const float* p = static_cast<const float*>(pred) + i;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      f32x4 f;
      if (wide) {
        f = *reinterpret_cast<const f32x4*>(p + 4 * w);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) f[b] = p[4 * w + b];
      }
      r[w] = quant(f[0]) | (quant(f[1]) << 8) | (quant(f[2]) << 16) | (quant(f[3]) << 24);
    }
  } else {
    const uint8_t* p = static_cast<const uint8_t*>(pred) + i;
    if (wide) {
      r = *reinterpret_cast<const u32x4*>(p);
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w)
        r[w] = (unsigned)p[4 * w] | ((unsigned)p[4 * w + 1] << 8) | ((unsigned)p[4 * w + 2] << 16) | ((unsigned)p[4 * w + 3] << 24);
    }
  }
  return r;
}

template <bool F32>
__device__ __forceinline__ unsigned pred1(const void* pred, long i) {
  return F32 ? quant(static_cast<const float*>(pred)[i]) : (unsigned)static_cast<const uint8_t*>(pred)[i];
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool F32>
__global__ __launch_bounds__(NT) void saliency_tables_kernel(const void* __restrict__ pred, const uint8_t* __restrict__ map,
                                                             long long* __restrict__ tables, long long* __restrict__ head, int H,
                                                             int W) {
  __shared__ unsigned hist[BINS];
  __shared__ unsigned long long red[3][WAVES];
  __shared__ unsigned split[2];

  const unsigned tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned N = (unsigned)H * (unsigned)W, Wu = (unsigned)W;          // N <= 2^24: the host checks
  const long base = (long)blockIdx.x * N;
  const uint8_t* m = map + base;
  const unsigned to_boundary = (unsigned)((0 - reinterpret_cast<uintptr_t>(m)) & 15);
  const unsigned lead = to_boundary < N ? to_boundary : N;
  const unsigned chunks = (N - lead) >> 4;
  const unsigned tail0 = lead + (chunks << 4);                             // N - tail0 < 16
  const uintptr_t pred_at = reinterpret_cast<uintptr_t>(pred) + (uintptr_t)(base + lead) * (F32 ? 4 : 1);
  const bool wide = (pred_at & 15) == 0;

  hist[tid] = 0;
  hist[tid + NT] = 0;

  // ---- pass 1: nF, sum x g, sum y g
  unsigned long long nf = 0, sx = 0, sy = 0;
  for (unsigned c = tid; c < chunks; c += NT) {
    const unsigned i0 = lead + (c << 4);
    unsigned y = i0 / Wu, x = i0 - y * Wu;
    const u32x4 mv = *reinterpret_cast<const u32x4*>(m + i0);
    unsigned cn = 0, cx = 0, cy = 0;                                       // 16 x 2^24 fits
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const bool g = ((mv[j >> 2] >> (8 * (j & 3))) & 255u) > 128u;
      cn += g; cx += g ? x : 0u; cy += g ? y : 0u;
      if (++x == Wu) { x = 0; ++y; }
    }
    nf += cn; sx += cx; sy += cy;
  }
  {
    const unsigned i = tid < lead ? tid : tail0 + (tid - lead);            // the lead pixels, then the tail's: fewer than 31
    if (i < N && m[i] > 128) {
      const unsigned y = i / Wu;
      nf += 1; sx += i - y * Wu; sy += y;
    }
  }
  nf = wave_sum_u64(nf); sx = wave_sum_u64(sx); sy = wave_sum_u64(sy);
  if (lane == 0) { red[0][wid] = nf; red[1][wid] = sx; red[2][wid] = sy; }
  __syncthreads();
  if (tid == 0) {
    unsigned long long a = 0, b = 0, c = 0;
    for (int w = 0; w < WAVES; ++w) { a += red[0][w]; b += red[1][w]; c += red[2][w]; }
    const unsigned X = a ? (unsigned)((2 * b + a) / (2 * a)) : Wu / 2, Y = a ? (unsigned)((2 * c + a) / (2 * a)) : (unsigned)H / 2;
    split[0] = X + 1; split[1] = Y + 1;
    long long* hd = head + (long)blockIdx.x * 5;
    hd[0] = (long long)a; hd[1] = (long long)b; hd[2] = (long long)c; hd[3] = X + 1; hd[4] = Y + 1;
  }
  __syncthreads();                                                         // (also: the histogram is zero)
  const unsigned cx = split[0], cy = split[1];

  // ---- pass 2: the histogram, one LDS atomic per run of equal keys
  unsigned cur = 0, cnt = 0;
  auto push = [&](unsigned key) {
    if (key != cur) {
      if (cnt) atomicAdd(&hist[cur], cnt);
      cur = key; cnt = 0;
    }
    ++cnt;
  };
  for (unsigned c = tid; c < chunks; c += NT) {
    const unsigned i0 = lead + (c << 4);
    unsigned y = i0 / Wu, x = i0 - y * Wu;
    const u32x4 mv = *reinterpret_cast<const u32x4*>(m + i0);
    const u32x4 pv = pred16<F32>(pred, base + i0, wide);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned mb = (mv[j >> 2] >> (8 * (j & 3))) & 255u, pb = (pv[j >> 2] >> (8 * (j & 3))) & 255u;
      push(((y >= cy ? 2u : 0u) + (x >= cx ? 1u : 0u)) * 512u + (mb > 128u ? 256u : 0u) + pb);
      if (++x == Wu) { x = 0; ++y; }
    }
  }
  {
    const unsigned i = tid < lead ? tid : tail0 + (tid - lead);
    if (i < N) {
      const unsigned y = i / Wu, x = i - y * Wu;
      push(((y >= cy ? 2u : 0u) + (x >= cx ? 1u : 0u)) * 512u + (m[i] > 128 ? 256u : 0u) + pred1<F32>(pred, base + i));
    }
  }
  if (cnt) atomicAdd(&hist[cur], cnt);
  __syncthreads();
  long long* out = tables + (long)blockIdx.x * BINS;
  out[tid] = (long long)hist[tid];
  out[tid + NT] = (long long)hist[tid + NT];
}

}  // namespace

extern "C" int adm_saliency_tables(const void* pred, int pred_is_f32, const uint8_t* map, int64_t* tables, int64_t* head, int B, int H,
                                   int W, hipStream_t stream) {
  if (!pred || !map || !tables || !head) return ADM_EINVAL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > ADM_SALIENCY_MAX_PIXELS) return ADM_EINVAL;
  if (pred_is_f32 && (reinterpret_cast<uintptr_t>(pred) & 3)) return ADM_EINVAL;
  if ((reinterpret_cast<uintptr_t>(tables) & 7) || (reinterpret_cast<uintptr_t>(head) & 7)) return ADM_EINVAL;
  long long* t = reinterpret_cast<long long*>(tables);
  long long* h = reinterpret_cast<long long*>(head);
  if (pred_is_f32)
    hipLaunchKernelGGL(saliency_tables_kernel<true>, dim3((unsigned)B), dim3(NT), 0, stream, pred, map, t, h, H, W);
  else
    hipLaunchKernelGGL(saliency_tables_kernel<false>, dim3((unsigned)B), dim3(NT), 0, stream, pred, map, t, h, H, W);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

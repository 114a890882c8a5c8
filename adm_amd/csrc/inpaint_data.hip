// In-painting training batches (ddm.data.InpaintDataset, ddm/data.py:384-476 of the reference) made on the device: the free-form
// masks of random_mask / RandomBrush and the {image, cond = mask * image, ori_mask} triple, from the uint8 image pool of
// sr_data.hip.  The reference draws with numpy and rasterises with PIL on the host, in a rejection loop; here
//   * inpaint_masks_kernel turns a fixed slot table of U[0,1) / N(0,1) draws (include/adm_hip.h) into primitive lists, in fp64 and in
//     the reference's operation order (this file is compiled with -ffp-contract=off: an fma would round a vertex differently
//     than the host does), and decides the rejection loop from the parameters: the first of ADM_INP_CANDIDATES candidates that
//     covers a pixel is kept;
//   * inpaint_batch_kernel rasterises in INTEGERS, so a NumPy restatement agrees bit for bit: rectangles, butt-ended bands
//     (0 <= dot <= L2, 4 cross^2 <= w^2 L2 in int64) and discs (4 d^2 <= (2 (w/2) + 1)^2); the two flips mirror the strokes.
// A workgroup owns an ADM_INP_TILE_H x ADM_INP_TILE_W tile of one sample: 32 consecutive x per row, so the pool's 3-byte pixels and
// the three output planes are read and written in runs along x.  The sample's primitives (about 1.2 KB) are staged once in
// LDS; 126 threads test each vertex's disc and each segment's band, by bounding boxes inflated by the half-width, against the
// tile, and the per-pixel integer tests run only over what survives.  A few MB per step, latency-bound: kept simple, no knobs.
//
// Every read of the pool is guarded by the pool's size and the image's own size, and every primitive count is clamped to its
// array, so wrong draws or lists give wrong pixels, never an access out of bounds.
#include "common.h"
#include "../../include/adm_hip.h"

#include <math.h>

namespace {

constexpr int K = ADM_INP_CANDIDATES, NR = ADM_INP_RECTS, NS = ADM_INP_STROKES, NV = ADM_INP_VERTS, NSEG = ADM_INP_SEGMENTS;
constexpr int NU = ADM_INP_NU, NZ = ADM_INP_NZ;
constexpr int TH = ADM_INP_TILE_H, TW = ADM_INP_TILE_W, NT = 256;
static_assert(TH * TW == NT, "one thread per pixel of the tile");
static_assert(NS * NV <= NT, "one thread per vertex in the culling pass");
static_assert(ADM_INP_U_RECT + 4 * NR == ADM_INP_U_NRECT_BIG && ADM_INP_U_STROKE + NS * ADM_INP_STROKE_U == ADM_INP_U_FLIP &&
              ADM_INP_U_FLIP + 2 == NU && NS * NSEG == NZ && NSEG + 1 == NV && ADM_INP_STROKE_U == 8 + NSEG, "slot table");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ double clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
// numpy's randint(lo, hi) on a uniform draw: lo + floor(u (hi - lo)), u < 1 so the result stays below hi
__device__ __forceinline__ int randint(float u, int lo, int hi) { return lo + (int)floor((double)u * (double)(hi - lo)); }

// Fill(max_size) (data.py:408-412): {x0, y0, x1, y1} clipped to the image; false when it covers no pixel
__device__ bool rect_of(const float* __restrict__ u, int max_size, int S, int* r) {
  const int w = randint(u[0], 0, max_size), h = randint(u[1], 0, max_size);
  const int ww = w / 2, hh = h / 2;
  const int x = randint(u[2], -ww, S - w + ww), y = randint(u[3], -hh, S - h + hh);
  r[0] = max(x, 0); r[1] = max(y, 0); r[2] = min(x + w, S); r[3] = min(y + h, S);
  return r[0] < r[2] && r[1] < r[3];
}

__global__ __launch_bounds__(64) void inpaint_masks_kernel(const float* __restrict__ u, const float* __restrict__ z,
                                                           int* __restrict__ rects, int* __restrict__ verts,
                                                           int* __restrict__ nverts, int* __restrict__ widths,
                                                           int* __restrict__ flips, int* __restrict__ chosen,
                                                           int* __restrict__ fallback, int B, int S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int r[4];
  // the rejection loop (data.py:406-421 with hole_range = [0, 1]): a candidate is redrawn iff nothing covers a pixel
  int k = 0;
  bool found = false;
  for (; k < K; ++k) {
    const float* uc = u + ((long)b * K + k) * NU;
    if (randint(uc[ADM_INP_U_NSTROKE], 0, NS + 1) > 0) found = true;          // a stroke always covers pixels of the image
    const int n_small = randint(uc[ADM_INP_U_NRECT_SMALL], 0, NR), n_big = randint(uc[ADM_INP_U_NRECT_BIG], 0, 2);
    for (int j = 0; j < n_small; ++j) found |= rect_of(uc + ADM_INP_U_RECT + 4 * j, S / 2, S, r);
    if (n_big) found |= rect_of(uc + ADM_INP_U_RECT + 4 * (NR - 1), S, S, r);
    if (found) break;
  }
  if (!found) {
    k = K - 1;
    atomicAdd(fallback, 1);
  }
  chosen[b] = k;
  const float* uc = u + ((long)b * K + k) * NU;
  const float* zc = z + ((long)b * K + k) * NZ;

  const int n_small = randint(uc[ADM_INP_U_NRECT_SMALL], 0, NR), n_big = randint(uc[ADM_INP_U_NRECT_BIG], 0, 2);
  for (int j = 0; j < NR; ++j) {
    const bool drawn = j < NR - 1 ? j < n_small : n_big > 0;
    const bool live = drawn && rect_of(uc + ADM_INP_U_RECT + 4 * j, j < NR - 1 ? S / 2 : S, S, r);
    for (int c = 0; c < 4; ++c) rects[((long)b * NR + j) * 4 + c] = live ? r[c] : 0;
  }

  // RandomBrush (data.py:424-476), python's operation order in fp64
  const double two_pi = 2 * M_PI, mean_angle = two_pi / 5, angle_range = two_pi / 15;
  const double avg = sqrt((double)(S * S + S * S)) / 8, scale = floor(avg / 2), rmax = 2 * avg;
  const int n_stroke = randint(uc[ADM_INP_U_NSTROKE], 0, NS + 1);
  for (int s = 0; s < NS; ++s) {
    const float* us = uc + ADM_INP_U_STROKE + s * ADM_INP_STROKE_U;
    int* v = verts + ((long)b * NS + s) * NV * 2;
    if (s >= n_stroke) {
      for (int i = 0; i < NV * 2; ++i) v[i] = 0;
      nverts[b * NS + s] = 0;
      widths[b * NS + s] = 0;
      continue;
    }
    const int nv = randint(us[0], 4, NV);
    const double amin = mean_angle - (0.0 + (angle_range - 0.0) * (double)us[1]);
    const double amax = mean_angle + (0.0 + (angle_range - 0.0) * (double)us[2]);
    int vx = randint(us[20], 0, S), vy = randint(us[21], 0, S);
    v[0] = vx; v[1] = vy;
    for (int i = 0; i < NSEG; ++i) {
      if (i >= nv) {
        v[2 * i + 2] = 0; v[2 * i + 3] = 0;
        continue;
      }
      double a = amin + (amax - amin) * (double)us[3 + i];
      if (i % 2 == 0) a = two_pi - a;
      const double rr = clipd(avg + scale * (double)zc[s * NSEG + i], 0.0, rmax);
      vx = (int)clipd((double)vx + rr * cos(a), 0.0, (double)S);
      vy = (int)clipd((double)vy + rr * sin(a), 0.0, (double)S);
      v[2 * i + 2] = vx; v[2 * i + 3] = vy;
    }
    nverts[b * NS + s] = nv + 1;
    widths[b * NS + s] = (int)(12.0 + (48.0 - 12.0) * (double)us[22]);
  }
  flips[2 * b] = uc[ADM_INP_U_FLIP] > 0.5f;
  flips[2 * b + 1] = uc[ADM_INP_U_FLIP + 1] > 0.5f;
}

__global__ __launch_bounds__(NT) void inpaint_batch_kernel(
    const unsigned char* __restrict__ pool, long pool_bytes, const int64_t* __restrict__ img_off, const int* __restrict__ img_hw,
    int n_images, const int* __restrict__ idx, const int* __restrict__ img_flip, const int* __restrict__ rects,
    const int* __restrict__ verts, const int* __restrict__ nverts, const int* __restrict__ widths, const int* __restrict__ flips,
    float* __restrict__ image, float* __restrict__ cond, float* __restrict__ ori_mask, int S) {
  __shared__ int s_rect[NR * 4], s_vert[NS * NV * 2], s_nv[NS], s_w[NS];
  __shared__ unsigned char s_live[NS * NV];          // bit 0: this vertex's disc reaches the tile; bit 1: the segment to the next vertex does

  const int tid = threadIdx.x;
  const int b = blockIdx.z, r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const bool fy = flips[2 * b] != 0, fx = flips[2 * b + 1] != 0;
  for (int i = tid; i < NR * 4; i += NT) s_rect[i] = rects[(long)b * NR * 4 + i];
  for (int i = tid; i < NS * NV * 2; i += NT) s_vert[i] = verts[(long)b * NS * NV * 2 + i];
  if (tid < NS) {
    s_nv[tid] = clampi(nverts[b * NS + tid], 0, NV);
    s_w[tid] = max(widths[b * NS + tid], 0);
  }
  __syncthreads();

  // the tile in the coordinates of the unflipped strokes, inclusive
  const int r1 = min(r0 + TH, S) - 1, c1 = min(c0 + TW, S) - 1;
  const int ty0 = fy ? S - 1 - r1 : r0, ty1 = fy ? S - 1 - r0 : r1, tx0 = fx ? S - 1 - c1 : c0, tx1 = fx ? S - 1 - c0 : c1;
  if (tid < NS * NV) {
    const int s = tid / NV, i = tid % NV, nv = s_nv[s], w = s_w[s];
    unsigned char live = 0;
    if (i < nv) {
      const int ax = s_vert[2 * tid], ay = s_vert[2 * tid + 1], rad = w / 2 + 1;
      if (ax + rad >= tx0 && ax - rad <= tx1 && ay + rad >= ty0 && ay - rad <= ty1) live |= 1;
      if (i + 1 < nv) {
        const int bx = s_vert[2 * tid + 2], by = s_vert[2 * tid + 3];
        if (max(ax, bx) + rad >= tx0 && min(ax, bx) - rad <= tx1 && max(ay, by) + rad >= ty0 && min(ay, by) - rad <= ty1) live |= 2;
      }
    }
    s_live[tid] = live;
  }
  __syncthreads();

  const int px = c0 + tid % TW, py = r0 + tid / TW;
  if (px >= S || py >= S) return;
  // the two flips mirror what RandomBrush returns, the strokes; the rectangles are filled into the mask itself (data.py:412, 418)
  const int qx = fx ? S - 1 - px : px, qy = fy ? S - 1 - py : py;
  bool hole = false;
  for (int j = 0; j < NR; ++j)
    hole |= px >= s_rect[4 * j] && px < s_rect[4 * j + 2] && py >= s_rect[4 * j + 1] && py < s_rect[4 * j + 3];
  for (int s = 0; s < NS && !hole; ++s) {
    const int nv = s_nv[s];
    const long w = s_w[s], d = 2 * (w / 2) + 1;
    for (int i = 0; i < nv; ++i) {
      const int live = s_live[s * NV + i];
      if (!live) continue;
      const long ex = qx - s_vert[2 * (s * NV + i)], ey = qy - s_vert[2 * (s * NV + i) + 1];
      if ((live & 1) && 4 * (ex * ex + ey * ey) <= d * d) hole = true;
      if (live & 2) {
        const long dx = s_vert[2 * (s * NV + i) + 2] - s_vert[2 * (s * NV + i)];
        const long dy = s_vert[2 * (s * NV + i) + 3] - s_vert[2 * (s * NV + i) + 1];
        const long L2 = dx * dx + dy * dy, dot = ex * dx + ey * dy, cross = ex * dy - ey * dx;
        if (L2 > 0 && dot >= 0 && dot <= L2 && 4 * cross * cross <= w * w * L2) hole = true;
      }
    }
  }
  const float m = hole ? 0.0f : 1.0f;

  // the pixel's three bytes: one 3-byte read, consecutive lanes read consecutive pixels
  const int n = clampi(idx[b], 0, n_images - 1);
  const int ih = img_hw[2 * n], iw = img_hw[2 * n + 1];
  const int sx = img_flip[b] != 0 ? S - 1 - px : px;
  const long g = img_off[n] + ((long)py * iw + sx) * 3;
  const bool ok = py < ih && sx < iw && g >= 0 && g + 2 < pool_bytes;
  const long plane = (long)S * S, o = (long)py * S + px;
  ori_mask[b * plane + o] = m;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = (float)(ok ? (int)pool[g + c] : 0) / 255.0f;          // ToTensor
    image[(b * 3L + c) * plane + o] = t * 2.0f - 1.0f;
    cond[(b * 3L + c) * plane + o] = (m * t) * 2.0f - 1.0f;
  }
}

__global__ __launch_bounds__(256) void inpaint_compose_kernel(const float* __restrict__ mask, const float* __restrict__ cond,
                                                              const float* __restrict__ x, float* __restrict__ out, int C, long hw,
                                                              long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float m = mask[i / (C * hw) * hw + i % hw];
    out[i] = m * ((cond[i] + 1.0f) * 0.5f) + (1.0f - m) * x[i];
  }
}

}  // namespace

extern "C" int adm_inpaint_masks(const float* u, const float* z, int* rects, int* verts, int* nverts, int* widths, int* flips,
                                 int* chosen, int* fallback, int B, int S, hipStream_t stream) {
  if (!u || !z || !rects || !verts || !nverts || !widths || !flips || !chosen || !fallback) return ADM_EINVAL;
  if (B <= 0 || B > 65535 || S < 2 || S > 4096) return ADM_EINVAL;
  hipLaunchKernelGGL(inpaint_masks_kernel, dim3(adm_cdiv(B, 64)), dim3(64), 0, stream, u, z, rects, verts, nverts, widths, flips,
                     chosen, fallback, B, S);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_inpaint_batch(const uint8_t* pool, long pool_bytes, const int64_t* img_off, const int* img_hw, int n_images,
                                 const int* idx, const int* img_flip, const int* rects, const int* verts, const int* nverts,
                                 const int* widths, const int* flips, float* image, float* cond, float* ori_mask, int B, int S,
                                 hipStream_t stream) {
  if (!pool || !img_off || !img_hw || !idx || !img_flip || !rects || !verts || !nverts || !widths || !flips || !image || !cond ||
      !ori_mask)
    return ADM_EINVAL;
  // S <= 4096: 4 cross^2 <= 4 (2 S^2)^2 = 2^54 stays inside int64
  if (pool_bytes <= 0 || n_images <= 0 || B <= 0 || B > 65535 || S < 2 || S > 4096) return ADM_EINVAL;
  hipLaunchKernelGGL(inpaint_batch_kernel, dim3(adm_cdiv(S, TW), adm_cdiv(S, TH), B), dim3(NT), 0, stream, pool, pool_bytes, img_off,
                     img_hw, n_images, idx, img_flip, rects, verts, nverts, widths, flips, image, cond, ori_mask, S);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_inpaint_compose(const float* mask, const float* cond, const float* x, float* out, int B, int C, long hw,
                                   hipStream_t stream) {
  if (!mask || !cond || !x || !out || B <= 0 || C <= 0 || hw <= 0) return ADM_EINVAL;
  const long n = (long)B * C * hw;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(inpaint_compose_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, mask, cond, x,
                     out, C, hw, n);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// Super-resolution training batches (ddm.data.SRDataset, ddm/data.py:645-658 of the reference) made on the device from a uint8
// image pool: random crop -> PIL's Image.resize of the crop (8 bits per channel) -> one horizontal flip of both images ->
// ToTensor, *2-1.  One launch makes the whole batch; the draws (idx, top, left, flip) are read from device memory.
//
// The resize -- arithmetic, tile, LDS staging and guards -- is resample_u8.h's: a workgroup owns one sample's ADM_SR_TILE_H x
// ADM_SR_TILE_W tile of low-resolution pixels, and the plane it resizes is the crop at (top, left).  What is particular here: ONE
// launch also writes `image`.  The tiles partition the crop's high-resolution pixels exactly (tile rows [r0, r1) own crop rows
// [r0*H/h, r1*H/h) in integer arithmetic, the same for columns), and a tile writes the normalised pixels it owns from the bytes it
// already holds.  For a down-scaling table the owned pixels always lie inside the staged rectangle; where a table leaves one outside
// it (up-scaling), that byte is read from the pool directly, guarded by the pool's size, so no second launch exists.  A few MB per
// step: latency-bound like augment.hip, kept simple, no knobs.
#include "resample_u8.h"

namespace {

using namespace resample_u8;

__global__ __launch_bounds__(NT) void sr_batch_kernel(
    const unsigned char* __restrict__ pool, long pool_dwords, const int64_t* __restrict__ img_off, const int* __restrict__ img_hw,
    int n_images, const int* __restrict__ idx, const int* __restrict__ top, const int* __restrict__ left,
    const int* __restrict__ flip, const int* __restrict__ hbounds, const int* __restrict__ hcoef, const int* __restrict__ vbounds,
    const int* __restrict__ vcoef, float* __restrict__ image, float* __restrict__ cond, unsigned char* __restrict__ cond_u8, int H,
    int W, int h, int w, Layout lay) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.z, r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const int nr = min(TH, h - r0), nc = min(TW, w - c0);

  const int n = clampi(idx[b], 0, n_images - 1);
  const int iw = img_hw[2 * n + 1];
  const int t = max(0, min(top[b], img_hw[2 * n] - H)), l = max(0, min(left[b], iw - W));
  const bool fl = flip[b] != 0;
  const long base = img_off[n];

  const Plane crop{pool, pool_dwords, base, iw, 3, t, l, H, W};
  const Table ht{hbounds, hcoef, lay.kh_cap}, vt{vbounds, vcoef, lay.kv_cap};
  const Staged st = resample_tile(crop, ht, vt, lay, r0, c0, nr, nc, [&](int y, int x, int c, int u) {
    const int xo = fl ? w - 1 - x : x;          // the flip follows the resize (data.py:651-652)
    cond[(((long)b * 3 + c) * h + y) * w + xo] = norm8(u);
    if (cond_u8) cond_u8[(((long)b * h + y) * w + xo) * 3 + c] = (unsigned char)u;
  });

  // the high-resolution pixels this tile owns
  const int oy0 = (int)((long)r0 * H / h), oy1 = (int)((long)(r0 + nr) * H / h);
  const int ox0 = (int)((long)c0 * W / w), ox1 = (int)((long)(c0 + nc) * W / w);
  const int oh = oy1 - oy0;
  for (int p = wave; p < 3 * oh; p += NT / 64) {
    const int c = p / oh, y = oy0 + p % oh;
    const int ry = y - st.sy0;
    const bool row_in = ry >= 0 && ry < st.nrows;
    const unsigned char* lrow = (row_in ? st.row(ry) : st.src) + c;
    const long grow = base + ((long)(t + y) * iw + l) * 3 + c;
    float* orow = image + (((long)b * 3 + c) * H + y) * W;
    for (int x = ox0 + lane; x < ox1; x += 64) {
      const int rx = x - st.sx0;
      int u;
      if (row_in && rx >= 0 && rx < st.ncols) {
        u = lrow[rx * 3];
      } else {
        const long g = grow + (long)x * 3;
        u = (g >= 0 && g < pool_dwords * 4) ? pool[g] : 0;
      }
      orow[fl ? W - 1 - x : x] = norm8(u);
    }
  }
}

}  // namespace

extern "C" int adm_sr_tile(int axis) { return axis == 0 ? TH : (axis == 1 ? TW : ADM_EINVAL); }

extern "C" int adm_sr_batch(const uint8_t* pool, long pool_bytes, const int64_t* img_off, const int* img_hw, int n_images,
                            const int* idx, const int* top, const int* left, const int* flip, const int* hbounds,
                            const int* hcoef, int kh, const int* vbounds, const int* vcoef, int kv, float* image, float* cond,
                            uint8_t* cond_u8, int B, int H, int W, int h, int w, hipStream_t stream) {
  if (!pool || !img_off || !img_hw || !idx || !top || !left || !flip || !hbounds || !hcoef || !vbounds || !vcoef || !image || !cond)
    return ADM_EINVAL;
  if (pool_bytes <= 0 || (pool_bytes & 3) || (reinterpret_cast<uintptr_t>(pool) & 3)) return ADM_EINVAL;      // dword loads
  if (n_images <= 0 || B <= 0 || B > 65535 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || kh <= 0 || kv <= 0) return ADM_EINVAL;
  const Layout lay = layout(h, w, H, W, kh, kv);
  if (lay.bytes() > kLdsBudget) return ADM_EINVAL;
  const dim3 grid(adm_cdiv(w, TW), adm_cdiv(h, TH), B);
  if (grid.y > 65535) return ADM_EINVAL;
  hipLaunchKernelGGL(sr_batch_kernel, grid, dim3(NT), (size_t)lay.bytes(), stream, pool, pool_bytes >> 2, img_off, img_hw, n_images,
                     idx, top, left, flip, hbounds, hcoef, vbounds, vcoef, image, cond, cond_u8, H, W, h, w, lay);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

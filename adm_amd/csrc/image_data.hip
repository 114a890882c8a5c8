// First-stage training images (ddm.data.ImageDataset, ddm/data.py:167-185 of the reference; the map of DUTSDataset and the photo of
// SketchDataset go through the same steps) made on the device from ONE uint8 pool: an image of C = 3 or C = 1 bytes per pixel, of
// ITS OWN size, resized to H x W with PIL's Image.resize (bilinear, antialiased, 8 bits per channel) -> horizontal flip ->
// ToTensor, *2-1.  One launch makes the whole batch; the draws (idx, flip) are read from device memory.
//
// This is the one-plane sibling of pair_resize_kernel (pair_data.hip): the resize -- arithmetic, tile, LDS staging and guards -- is
// resample_u8.h's, the table pool is adm_pair_resize_batch's with img_tab[2n + {0,1}] naming the width / height
// table of image n, and the LDS of a tile is adm_pair_resize_lds's figure.  A workgroup owns a tile of one sample (blockIdx.z = b).
// idx is clamped, a negative size counts as 0.
#include "resample_u8.h"

namespace {

using namespace resample_u8;

__global__ __launch_bounds__(NT) void image_resize_kernel(
    const unsigned char* __restrict__ pool, long pool_dwords, const int64_t* __restrict__ off, const int* __restrict__ hw,
    int n_images, int C, const int* __restrict__ tab, long tab_ints, const int* __restrict__ tab_dir, int n_tables,
    const int* __restrict__ img_tab, const int* __restrict__ idx, const int* __restrict__ flip, float* __restrict__ out,
    unsigned char* __restrict__ out_u8, int H, int W, Layout lay) {
  const int b = blockIdx.z, r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const int nr = min(TH, H - r0), nc = min(TW, W - c0);

  const int n = clampi(idx[b], 0, n_images - 1);
  const bool fl = flip[b] != 0;
  const int ih = max(hw[2 * n], 0), iw = max(hw[2 * n + 1], 0);
  const Plane src{pool, pool_dwords, off[n], iw, C, 0, 0, ih, iw};
  const Table ht = table_of(tab, tab_ints, tab_dir, n_tables, img_tab[2 * n], W, lay.kh_cap);
  const Table vt = table_of(tab, tab_ints, tab_dir, n_tables, img_tab[2 * n + 1], H, lay.kv_cap);

  resample_tile(src, ht, vt, lay, r0, c0, nr, nc, [&](int y, int x, int c, int u) {
    const int xo = fl ? W - 1 - x : x;          // the flip follows the resize (data.py:171-174)
    out[(((long)b * C + c) * H + y) * W + xo] = norm8(u);
    if (out_u8) out_u8[(((long)b * H + y) * W + xo) * C + c] = (unsigned char)u;
  });
}

}  // namespace

extern "C" int adm_image_resize_batch(const uint8_t* pool, long pool_bytes, const int64_t* off, const int* hw, int n_images, int C,
                                      const int* tab, long tab_ints, const int* tab_dir, int n_tables, const int* img_tab,
                                      int max_h, int max_w, int kh, int kv, const int* idx, const int* flip, float* out,
                                      uint8_t* out_u8, int B, int H, int W, hipStream_t stream) {
  if (!pool || !off || !hw || !tab || !tab_dir || !img_tab || !idx || !flip || !out) return ADM_EINVAL;
  if (pool_bytes <= 0 || (pool_bytes & 3) || (reinterpret_cast<uintptr_t>(pool) & 3)) return ADM_EINVAL;          // dword loads
  if (C != 1 && C != 3) return ADM_EINVAL;
  if (n_images <= 0 || n_tables <= 0 || tab_ints <= 0 || B <= 0 || B > 65535 || H <= 0 || W <= 0) return ADM_EINVAL;
  if (max_h <= 0 || max_w <= 0 || kh <= 0 || kv <= 0) return ADM_EINVAL;
  const long lds = adm_pair_resize_lds(H, W, max_h, max_w, kh, kv);
  if (lds <= 0 || lds > kLdsBudget) return ADM_EINVAL;
  const Layout lay = layout(H, W, max_h, max_w, kh, kv);
  const dim3 grid(adm_cdiv(W, TW), adm_cdiv(H, TH), B);
  if (grid.y > 65535) return ADM_EINVAL;
  hipLaunchKernelGGL(image_resize_kernel, grid, dim3(NT), (size_t)lds, stream, pool, pool_bytes >> 2, off, hw, n_images, C, tab,
                     tab_ints, tab_dir, n_tables, img_tab, idx, flip, out, out_u8, H, W, lay);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

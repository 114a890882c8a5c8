// Saliency training pairs (ddm.data.DUTSDataset, ddm/data.py:996-1026 of the reference) made on the device from two uint8 pools:
// an RGB photo and its grey ground-truth map, each of ITS OWN size, both resized to H x W with PIL's Image.resize (bilinear,
// antialiased, 8 bits per channel) -> one horizontal flip of both -> ToTensor, *2-1.  One launch makes the whole batch; the draws
// (idx, flip) are read from device memory.
//
// The resize -- arithmetic, tile, LDS staging and guards -- is resample_u8.h's.  What is particular here is where the tables come
// from: every sample has its own source size, so its own four 1-D tables.  A table depends on (in_size, out_size)
// only; the host builds one per distinct source width and height (adm_amd/ddm/pair_data.py) and concatenates them into one int32
// TABLE POOL, and img_tab[4n + {0,1,2,3}] names the width / height table of image n's photo and the width / height table of its
// map.  A workgroup owns a tile of ONE PLANE of one sample (blockIdx.z = 2 b + plane: the photo's three channels or the map's one),
// and the plane it resizes is the whole image.  idx is clamped, a negative size counts as 0.
#include "resample_u8.h"

namespace {

using namespace resample_u8;

__global__ __launch_bounds__(NT) void pair_resize_kernel(
    const unsigned char* __restrict__ rgb_pool, long rgb_dwords, const int64_t* __restrict__ rgb_off, const int* __restrict__ rgb_hw,
    const unsigned char* __restrict__ gray_pool, long gray_dwords, const int64_t* __restrict__ gray_off,
    const int* __restrict__ gray_hw, int n_images, const int* __restrict__ tab, long tab_ints, const int* __restrict__ tab_dir,
    int n_tables, const int* __restrict__ img_tab, const int* __restrict__ idx, const int* __restrict__ flip,
    float* __restrict__ rgb, float* __restrict__ gray, unsigned char* __restrict__ rgb_u8, unsigned char* __restrict__ gray_u8,
    int H, int W, Layout lay) {
  const int b = blockIdx.z >> 1, plane = blockIdx.z & 1, r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const int nr = min(TH, H - r0), nc = min(TW, W - c0);

  const int n = clampi(idx[b], 0, n_images - 1);
  const bool fl = flip[b] != 0;
  const int C = plane ? 1 : 3;
  const int* hw = plane ? gray_hw : rgb_hw;
  const int ih = max(hw[2 * n], 0), iw = max(hw[2 * n + 1], 0);
  const Plane src{plane ? gray_pool : rgb_pool, plane ? gray_dwords : rgb_dwords, plane ? gray_off[n] : rgb_off[n], iw, C, 0, 0, ih, iw};
  const Table ht = table_of(tab, tab_ints, tab_dir, n_tables, img_tab[4 * n + 2 * plane], W, lay.kh_cap);
  const Table vt = table_of(tab, tab_ints, tab_dir, n_tables, img_tab[4 * n + 2 * plane + 1], H, lay.kv_cap);

  float* out = plane ? gray : rgb;
  unsigned char* out_u8 = plane ? gray_u8 : rgb_u8;
  resample_tile(src, ht, vt, lay, r0, c0, nr, nc, [&](int y, int x, int c, int u) {
    const int xo = fl ? W - 1 - x : x;          // the flip follows the resize (data.py:982-985)
    out[(((long)b * C + c) * H + y) * W + xo] = norm8(u);
    if (out_u8) out_u8[(((long)b * H + y) * W + xo) * C + c] = (unsigned char)u;
  });
}

}  // namespace

extern "C" long adm_pair_resize_lds(int H, int W, int max_h, int max_w, int kh, int kv) {
  if (H <= 0 || W <= 0 || max_h <= 0 || max_w <= 0 || kh <= 0 || kv <= 0) return ADM_EINVAL;
  return layout(H, W, max_h, max_w, kh, kv).bytes();
}

extern "C" int adm_pair_resize_batch(const uint8_t* rgb_pool, long rgb_bytes, const int64_t* rgb_off, const int* rgb_hw,
                                     const uint8_t* gray_pool, long gray_bytes, const int64_t* gray_off, const int* gray_hw,
                                     int n_images, const int* tab, long tab_ints, const int* tab_dir, int n_tables,
                                     const int* img_tab, int max_h, int max_w, int kh, int kv, const int* idx, const int* flip,
                                     float* rgb, float* gray, uint8_t* rgb_u8, uint8_t* gray_u8, int B, int H, int W,
                                     hipStream_t stream) {
  if (!rgb_pool || !rgb_off || !rgb_hw || !gray_pool || !gray_off || !gray_hw || !tab || !tab_dir || !img_tab || !idx || !flip ||
      !rgb || !gray)
    return ADM_EINVAL;
  if (rgb_bytes <= 0 || (rgb_bytes & 3) || (reinterpret_cast<uintptr_t>(rgb_pool) & 3)) return ADM_EINVAL;          // dword loads
  if (gray_bytes <= 0 || (gray_bytes & 3) || (reinterpret_cast<uintptr_t>(gray_pool) & 3)) return ADM_EINVAL;
  if (n_images <= 0 || n_tables <= 0 || tab_ints <= 0 || B <= 0 || 2L * B > 65535 || H <= 0 || W <= 0) return ADM_EINVAL;
  if (max_h <= 0 || max_w <= 0 || kh <= 0 || kv <= 0) return ADM_EINVAL;
  const Layout lay = layout(H, W, max_h, max_w, kh, kv);
  if (lay.bytes() > kLdsBudget) return ADM_EINVAL;
  const dim3 grid(adm_cdiv(W, TW), adm_cdiv(H, TH), 2 * B);
  if (grid.y > 65535) return ADM_EINVAL;
  hipLaunchKernelGGL(pair_resize_kernel, grid, dim3(NT), (size_t)lay.bytes(), stream, rgb_pool, rgb_bytes >> 2, rgb_off, rgb_hw,
                     gray_pool, gray_bytes >> 2, gray_off, gray_hw, n_images, tab, tab_ints, tab_dir, n_tables, img_tab, idx, flip, rgb,
                     gray, rgb_u8, gray_u8, H, W, lay);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

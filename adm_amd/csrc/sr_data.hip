// Super-resolution training batches (ddm.data.SRDataset, ddm/data.py:645-658 of the reference) made on the device from a uint8
// image pool: random crop -> PIL's Image.resize of the crop (8 bits per channel) -> one horizontal flip of both images ->
// ToTensor, *2-1.  One launch makes the whole batch; the draws (idx, top, left, flip) are read from device memory.
//
// The resize is PIL's ImagingResample for 8-bit images restated in integers (DESIGN.md "SR batches"): coefficients rounded to
// 22 fractional bits (built on the host, adm_amd/ddm/sr_data.py), horizontal pass first, clipped to uint8, vertical pass over
// that uint8 intermediate, each pass clip8((2^21 + sum k*px) >> 22) in int32.  The output bytes are PIL's, bit for bit.
//
// A workgroup owns one sample's ADM_SR_TILE_H x ADM_SR_TILE_W tile of low-resolution pixels.  It loads the tile's source rectangle (its
// bounds come from the two tables: nothing here assumes a factor of 4) once into LDS as bytes, with dword loads of the
// 3-byte-per-pixel rows from the dword-aligned address below each row's start; runs the horizontal pass into a second uint8 LDS
// array and the vertical pass from there.  ONE launch also writes `image`: the tiles partition the crop's high-resolution pixels
// exactly (tile rows [r0, r1) own crop rows [r0*H/h, r1*H/h) in integer arithmetic, the same for columns), and a tile writes the
// normalised pixels it owns from the bytes it already holds.  For a down-scaling table the owned pixels always lie inside the
// loaded rectangle; where a table leaves one outside it (up-scaling), that byte is read from the pool directly, so no second
// launch exists.  A few MB per step: latency-bound like augment.hip, kept simple, no knobs.
//
// Every read of the pool is guarded by the pool's size and every window is clipped to the crop and to the LDS capacity the host
// wrapper sized, so draws or tables that are wrong give wrong pixels, never an access out of bounds.
#include "common.h"
#include "../../include/adm_hip.h"

namespace {

constexpr int TH = ADM_SR_TILE_H, TW = ADM_SR_TILE_W, NT = 256;
constexpr int kLdsBudget = 64 * 1024;
static_assert(TH * TW == NT, "one thread per low-resolution pixel of the tile");

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ float norm8(int u) { return (float)u / 255.0f * 2.0f - 1.0f; }      // ToTensor, then *2-1
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// window {start, length} of output coordinate i, clipped to [0, size) and to kmax taps
__device__ __forceinline__ void window(const int* __restrict__ bounds, int i, int size, int kmax, int& s, int& len) {
  s = clampi(bounds[2 * i], 0, size);
  len = clampi(bounds[2 * i + 1], 0, min(kmax, size - s));
}

__global__ __launch_bounds__(NT) void sr_batch_kernel(
    const unsigned char* __restrict__ pool, long pool_dwords, const int64_t* __restrict__ img_off, const int* __restrict__ img_hw,
    int n_images, const int* __restrict__ idx, const int* __restrict__ top, const int* __restrict__ left,
    const int* __restrict__ flip, const int* __restrict__ hbounds, const int* __restrict__ hcoef, int kh,
    const int* __restrict__ vbounds, const int* __restrict__ vcoef, int kv, float* __restrict__ image, float* __restrict__ cond,
    unsigned char* __restrict__ cond_u8, int H, int W, int h, int w, int cap_rows, int cap_cols) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* hk = reinterpret_cast<int*>(smem);          // [TW][kh]
  int* vk = hk + TW * kh;                          // [TH][kv]
  unsigned char* src = reinterpret_cast<unsigned char*>(vk + TH * kv);      // [cap_rows][src_stride], rows start dword-aligned
  const int src_stride = (cap_cols * 3 + 6) & ~3;
  unsigned char* tmp = src + cap_rows * src_stride;                         // [cap_rows][TW][3]: the horizontal pass

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.z, r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const int nr = min(TH, h - r0), nc = min(TW, w - c0);

  const int n = clampi(idx[b], 0, n_images - 1);
  const int iw = img_hw[2 * n + 1];
  const int t = max(0, min(top[b], img_hw[2 * n] - H)), l = max(0, min(left[b], iw - W));
  const bool fl = flip[b] != 0;
  const long base = img_off[n];
  const uint32_t* pool32 = reinterpret_cast<const uint32_t*>(pool);

  // the tile's source rectangle, in crop coordinates
  int sx0 = W, sx1 = 0, sy0 = H, sy1 = 0, s, len;
  for (int i = 0; i < nc; ++i) {
    window(hbounds, c0 + i, W, kh, s, len);
    sx0 = min(sx0, s); sx1 = max(sx1, s + len);
  }
  for (int i = 0; i < nr; ++i) {
    window(vbounds, r0 + i, H, kv, s, len);
    sy0 = min(sy0, s); sy1 = max(sy1, s + len);
  }
  const int ncols = clampi(sx1 - sx0, 0, cap_cols), nrows = clampi(sy1 - sy0, 0, cap_rows);
  // byte address in the pool of rectangle row r, column 0; its low two bits = where the row starts in its LDS dwords
  auto row_byte = [&](int r) -> long { return base + ((long)(t + sy0 + r) * iw + (l + sx0)) * 3; };

  for (int i = tid; i < nc * kh; i += NT) hk[i] = hcoef[(long)c0 * kh + i];
  for (int i = tid; i < nr * kv; i += NT) vk[i] = vcoef[(long)r0 * kv + i];
  for (int r = wave; r < nrows; r += NT / 64) {
    const long byte0 = row_byte(r), d0 = byte0 >> 2;
    const int nd = (int)(((byte0 & 3) + ncols * 3 + 3) >> 2);          // <= src_stride / 4
    uint32_t* dst = reinterpret_cast<uint32_t*>(src + r * src_stride);
    for (int d = lane; d < nd; d += 64) {
      const long g = d0 + d;
      dst[d] = (g >= 0 && g < pool_dwords) ? pool32[g] : 0u;
    }
  }
  __syncthreads();

  // horizontal pass: every rectangle row x tile column x channel
  for (int j = tid; j < nrows * nc * 3; j += NT) {
    const int c = j % 3, col = (j / 3) % nc, r = j / (3 * nc);
    window(hbounds, c0 + col, W, kh, s, len);
    len = min(len, sx0 + ncols - s);
    const unsigned char* p = src + r * src_stride + (int)(row_byte(r) & 3) + (s - sx0) * 3 + c;
    int acc = 1 << 21;
    for (int k = 0; k < len; ++k) acc += hk[col * kh + k] * (int)p[3 * k];
    tmp[(r * TW + col) * 3 + c] = (unsigned char)clip8(acc);
  }
  __syncthreads();

  // vertical pass: one thread per low-resolution pixel
  {
    const int col = tid % TW, row = tid / TW;
    if (col < nc && row < nr) {
      window(vbounds, r0 + row, H, kv, s, len);
      len = min(len, sy0 + nrows - s);
      const int xo = fl ? w - 1 - (c0 + col) : c0 + col;          // the flip follows the resize (data.py:651-652)
      for (int c = 0; c < 3; ++c) {
        const unsigned char* p = tmp + ((s - sy0) * TW + col) * 3 + c;
        int acc = 1 << 21;
        for (int k = 0; k < len; ++k) acc += vk[row * kv + k] * (int)p[k * TW * 3];
        const int u = clip8(acc);
        cond[(((long)b * 3 + c) * h + (r0 + row)) * w + xo] = norm8(u);
        if (cond_u8) cond_u8[(((long)b * h + (r0 + row)) * w + xo) * 3 + c] = (unsigned char)u;
      }
    }
  }

  // the high-resolution pixels this tile owns
  const int oy0 = (int)((long)r0 * H / h), oy1 = (int)((long)(r0 + nr) * H / h);
  const int ox0 = (int)((long)c0 * W / w), ox1 = (int)((long)(c0 + nc) * W / w);
  const int oh = oy1 - oy0;
  for (int p = wave; p < 3 * oh; p += NT / 64) {
    const int c = p / oh, y = oy0 + p % oh;
    const int ry = y - sy0;
    const bool row_in = ry >= 0 && ry < nrows;
    const unsigned char* lrow = src + (row_in ? ry * src_stride + (int)(row_byte(ry) & 3) : 0) + c;
    const long grow = base + ((long)(t + y) * iw + l) * 3 + c;
    float* orow = image + (((long)b * 3 + c) * H + y) * W;
    for (int x = ox0 + lane; x < ox1; x += 64) {
      const int rx = x - sx0;
      int u;
      if (row_in && rx >= 0 && rx < ncols) {
        u = lrow[rx * 3];
      } else {
        const long g = grow + (long)x * 3;
        u = (g >= 0 && g < pool_dwords * 4) ? pool[g] : 0;
      }
      orow[fl ? W - 1 - x : x] = norm8(u);
    }
  }
}

// rows / columns of the source rectangle no tile of T outputs can exceed: the T windows start at most (T-1)*size/out apart
// (+1 for the truncation of each end) and the last is at most k long
inline int sr_extent(int T, int size, int out, int k) {
  const long e = ((long)(T - 1) * size + out - 1) / out + k + 1;
  return (int)(e < size ? e : size);
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
  const int cap_cols = sr_extent(TW, W, w, kh), cap_rows = sr_extent(TH, H, h, kv);
  const long stride = (cap_cols * 3L + 6) & ~3L;
  const long lds = ((long)TW * kh + (long)TH * kv) * 4 + cap_rows * stride + (long)cap_rows * TW * 3;
  if (lds > kLdsBudget) return ADM_EINVAL;
  const dim3 grid(adm_cdiv(w, TW), adm_cdiv(h, TH), B);
  if (grid.y > 65535) return ADM_EINVAL;
  hipLaunchKernelGGL(sr_batch_kernel, grid, dim3(NT), (size_t)lds, stream, pool, pool_bytes >> 2, img_off, img_hw, n_images, idx,
                     top, left, flip, hbounds, hcoef, kh, vbounds, vcoef, kv, image, cond, cond_u8, H, W, h, w, cap_rows, cap_cols);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

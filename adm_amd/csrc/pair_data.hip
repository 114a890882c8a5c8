// Saliency training pairs (ddm.data.DUTSDataset, ddm/data.py:996-1026 of the reference) made on the device from two uint8 pools:
// an RGB photo and its grey ground-truth map, each of ITS OWN size, both resized to H x W with PIL's Image.resize (bilinear,
// antialiased, 8 bits per channel) -> one horizontal flip of both -> ToTensor, *2-1.  One launch makes the whole batch; the draws
// (idx, flip) are read from device memory.
//
// The arithmetic is sr_data.hip's: coefficients with 22 fractional bits, horizontal pass first, clipped to uint8,
// vertical pass over that uint8 intermediate, each pass clip8((2^21 + sum k*px) >> 22) in int32.  What differs is where the
// tables come from: every sample has its own source size, so its own four 1-D tables.  A table depends on
// (in_size, out_size) only; the host builds one per distinct source width and height (adm_amd/ddm/pair_data.py) and concatenates
// them into one int32 TABLE POOL -- table t = bounds [out][2] then coefficients [out][k] at tab[tab_dir[2t]], k = tab_dir[2t+1] --
// and img_tab[4n + {0,1,2,3}] names the width / height table of image n's photo and the width / height table of its map.
// Up-scaling (three taps) and the identity go through the same two passes: no shortcut that could change a byte.
//
// A workgroup owns a 16 x 16 tile of output pixels of ONE PLANE of one sample (blockIdx.z = 2 b + plane: the photo's three
// channels or the map's one): it loads the tile's source rectangle into LDS as bytes with dword loads, runs the horizontal pass
// into a second uint8 LDS array and the vertical pass from there.  A few MB per step: latency-bound, kept simple, no knobs.
//
// Every pool read is guarded by the pool's size, every table read by the table pool's size, every window is clipped to its image
// and to the LDS capacity the host wrapper sized, idx is clamped: wrong draws or tables give wrong pixels, never an access out
// of bounds.
#include "common.h"
#include "../../include/adm_hip.h"

namespace {

constexpr int TH = ADM_SR_TILE_H, TW = ADM_SR_TILE_W, NT = 256;
constexpr long kLdsBudget = 64 * 1024;
static_assert(TH * TW == NT, "one thread per output pixel of the tile");

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ float norm8(int u) { return (float)u / 255.0f * 2.0f - 1.0f; }      // ToTensor, then *2-1
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One 1-D table of the pool, checked against the pool: k = 0 (every window empty) when the directory entry does not fit.
struct Table {
  const int* bounds;      // [out][2]
  const int* coef;        // [out][k]
  int k;
};

__device__ __forceinline__ Table table_of(const int* __restrict__ tab, long tab_ints, const int* __restrict__ tab_dir,
                                          int n_tables, int t, int out, int kmax) {
  t = clampi(t, 0, n_tables - 1);
  const long off = tab_dir[2 * t];
  const int k = tab_dir[2 * t + 1];
  Table r;
  const bool ok = off >= 0 && k > 0 && k <= kmax && off + (long)out * (2 + k) <= tab_ints;
  r.bounds = tab + (ok ? off : 0);
  r.coef = r.bounds + 2 * out;
  r.k = ok ? k : 0;
  return r;
}

// window {start, length} of output coordinate i, clipped to [0, size) and to the table's k taps
__device__ __forceinline__ void window(const Table& t, int i, int size, int& s, int& len) {
  if (t.k == 0) { s = 0; len = 0; return; }
  s = clampi(t.bounds[2 * i], 0, size);
  len = clampi(t.bounds[2 * i + 1], 0, min(t.k, size - s));
}

__global__ __launch_bounds__(NT) void pair_resize_kernel(
    const unsigned char* __restrict__ rgb_pool, long rgb_dwords, const int64_t* __restrict__ rgb_off, const int* __restrict__ rgb_hw,
    const unsigned char* __restrict__ gray_pool, long gray_dwords, const int64_t* __restrict__ gray_off,
    const int* __restrict__ gray_hw, int n_images, const int* __restrict__ tab, long tab_ints, const int* __restrict__ tab_dir,
    int n_tables, const int* __restrict__ img_tab, const int* __restrict__ idx, const int* __restrict__ flip,
    float* __restrict__ rgb, float* __restrict__ gray, unsigned char* __restrict__ rgb_u8, unsigned char* __restrict__ gray_u8,
    int H, int W, int kh_max, int kv_max, int cap_rows, int cap_cols) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* hk = reinterpret_cast<int*>(smem);          // [TW][kh]
  int* vk = hk + TW * kh_max;                      // [TH][kv]
  unsigned char* src = reinterpret_cast<unsigned char*>(vk + TH * kv_max);      // [cap_rows][src_stride], rows start dword-aligned
  const int src_stride = (cap_cols * 3 + 6) & ~3;
  unsigned char* tmp = src + cap_rows * src_stride;                             // [cap_rows][TW][C]: the horizontal pass

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.z >> 1, plane = blockIdx.z & 1, r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const int nr = min(TH, H - r0), nc = min(TW, W - c0);

  const int n = clampi(idx[b], 0, n_images - 1);
  const bool fl = flip[b] != 0;
  const int C = plane ? 1 : 3;
  const unsigned char* pool = plane ? gray_pool : rgb_pool;
  const long pool_dwords = plane ? gray_dwords : rgb_dwords;
  const int* hw = plane ? gray_hw : rgb_hw;
  const int ih = max(hw[2 * n], 0), iw = max(hw[2 * n + 1], 0);
  const long base = plane ? gray_off[n] : rgb_off[n];
  const uint32_t* pool32 = reinterpret_cast<const uint32_t*>(pool);
  const Table ht = table_of(tab, tab_ints, tab_dir, n_tables, img_tab[4 * n + 2 * plane], W, kh_max);
  const Table vt = table_of(tab, tab_ints, tab_dir, n_tables, img_tab[4 * n + 2 * plane + 1], H, kv_max);
  const int kh = ht.k, kv = vt.k;

  // the tile's source rectangle, in image coordinates
  int sx0 = iw, sx1 = 0, sy0 = ih, sy1 = 0, s, len;
  for (int i = 0; i < nc; ++i) {
    window(ht, c0 + i, iw, s, len);
    sx0 = min(sx0, s); sx1 = max(sx1, s + len);
  }
  for (int i = 0; i < nr; ++i) {
    window(vt, r0 + i, ih, s, len);
    sy0 = min(sy0, s); sy1 = max(sy1, s + len);
  }
  const int ncols = clampi(sx1 - sx0, 0, cap_cols), nrows = clampi(sy1 - sy0, 0, cap_rows);
  // byte address in the pool of rectangle row r, column 0; its low two bits = where the row starts in its LDS dwords
  auto row_byte = [&](int r) -> long { return base + ((long)(sy0 + r) * iw + sx0) * C; };

  for (int i = tid; i < nc * kh; i += NT) hk[i] = ht.coef[(long)c0 * kh + i];
  for (int i = tid; i < nr * kv; i += NT) vk[i] = vt.coef[(long)r0 * kv + i];
  for (int r = wave; r < nrows; r += NT / 64) {
    const long byte0 = row_byte(r), d0 = byte0 >> 2;
    const int nd = (int)(((byte0 & 3) + ncols * C + 3) >> 2);          // <= src_stride / 4
    uint32_t* dst = reinterpret_cast<uint32_t*>(src + r * src_stride);
    for (int d = lane; d < nd; d += 64) {
      const long g = d0 + d;
      dst[d] = (g >= 0 && g < pool_dwords) ? pool32[g] : 0u;
    }
  }
  __syncthreads();

  // horizontal pass: every rectangle row x tile column x channel
  for (int j = tid; j < nrows * nc * C; j += NT) {
    const int c = j % C, col = (j / C) % nc, r = j / (C * nc);
    window(ht, c0 + col, iw, s, len);
    s = max(s, sx0);
    len = clampi(len, 0, sx0 + ncols - s);
    const unsigned char* p = src + r * src_stride + (int)(row_byte(r) & 3) + (s - sx0) * C + c;
    int acc = 1 << 21;
    for (int k = 0; k < len; ++k) acc += hk[col * kh + k] * (int)p[C * k];
    tmp[(r * TW + col) * C + c] = (unsigned char)clip8(acc);
  }
  __syncthreads();

  // vertical pass: one thread per output pixel
  const int col = tid % TW, row = tid / TW;
  if (col < nc && row < nr) {
    window(vt, r0 + row, ih, s, len);
    s = max(s, sy0);
    len = clampi(len, 0, sy0 + nrows - s);
    const int y = r0 + row, xo = fl ? W - 1 - (c0 + col) : c0 + col;          // the flip follows the resize (data.py:982-985)
    float* out = plane ? gray : rgb;
    unsigned char* out_u8 = plane ? gray_u8 : rgb_u8;
    for (int c = 0; c < C; ++c) {
      const unsigned char* p = tmp + ((s - sy0) * TW + col) * C + c;
      int acc = 1 << 21;
      for (int k = 0; k < len; ++k) acc += vk[row * kv + k] * (int)p[k * TW * C];
      const int u = clip8(acc);
      out[(((long)b * C + c) * H + y) * W + xo] = norm8(u);
      if (out_u8) out_u8[(((long)b * H + y) * W + xo) * C + c] = (unsigned char)u;
    }
  }
}

// rows / columns of the source rectangle no tile of T outputs can exceed: the T windows start at most (T-1)*size/out apart
// (+1 for the truncation of each end) and the last is at most k long (sr_data.hip's sr_extent)
inline long pair_extent(int T, int size, int out, int k) {
  const long e = ((long)(T - 1) * size + out - 1) / out + k + 1;
  return e < size ? e : size;
}

inline long pair_lds(int H, int W, int max_h, int max_w, int kh, int kv, long* cap_rows, long* cap_cols) {
  *cap_cols = pair_extent(TW, max_w, W, kh);
  *cap_rows = pair_extent(TH, max_h, H, kv);
  const long stride = (*cap_cols * 3L + 6) & ~3L;
  return ((long)TW * kh + (long)TH * kv) * 4 + *cap_rows * stride + *cap_rows * TW * 3;
}

}  // namespace

extern "C" long adm_pair_resize_lds(int H, int W, int max_h, int max_w, int kh, int kv) {
  if (H <= 0 || W <= 0 || max_h <= 0 || max_w <= 0 || kh <= 0 || kv <= 0) return ADM_EINVAL;
  long cr, cc;
  return pair_lds(H, W, max_h, max_w, kh, kv, &cr, &cc);
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
  long cap_rows, cap_cols;
  const long lds = pair_lds(H, W, max_h, max_w, kh, kv, &cap_rows, &cap_cols);
  if (lds > kLdsBudget) return ADM_EINVAL;
  const dim3 grid(adm_cdiv(W, TW), adm_cdiv(H, TH), 2 * B);
  if (grid.y > 65535) return ADM_EINVAL;
  hipLaunchKernelGGL(pair_resize_kernel, grid, dim3(NT), (size_t)lds, stream, rgb_pool, rgb_bytes >> 2, rgb_off, rgb_hw, gray_pool,
                     gray_bytes >> 2, gray_off, gray_hw, n_images, tab, tab_ints, tab_dir, n_tables, img_tab, idx, flip, rgb, gray,
                     rgb_u8, gray_u8, H, W, kh, kv, (int)cap_rows, (int)cap_cols);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// PIL's Image.resize for 8-bit images, byte for byte, for one tile of one plane: everything adm_sr_batch (sr_data.hip) and
// adm_pair_resize_batch (pair_data.hip) share, once.
//
// The resize is PIL's ImagingResample restated in integers: coefficients rounded to 22 fractional bits (built on the host,
// resample_table of adm_amd/ddm/sr_data.py), horizontal pass first, clipped to uint8, vertical pass over that uint8 intermediate,
// each pass clip8((2^21 + sum k*px) >> 22) in int32.  Up-scaling (three taps) and the identity go through the same two passes: no
// shortcut that could change a byte.
//
// A workgroup of NT threads owns a TH x TW tile of output pixels of one plane (3 bytes or 1 byte per pixel).  It loads the tile's
// source rectangle (its bounds come from the two tables: nothing here assumes a factor) once into LDS as bytes, with dword loads
// from the dword-aligned address below each row's start; runs the horizontal pass into a second uint8 LDS array and the vertical
// pass from there, and hands every finished byte to its caller, which does the stores.
//
// Every read of the pool is guarded by the pool's size, every table of a table pool by that pool's size, and every window is
// clipped to its region, to the staged rectangle and to the LDS capacity the host wrapper sized, so draws or tables that are wrong
// give wrong pixels, never an access out of bounds.
#pragma once
#include "common.h"
#include "../../include/adm_hip.h"

namespace resample_u8 {

constexpr int TH = ADM_SR_TILE_H, TW = ADM_SR_TILE_W, NT = 256;
constexpr long kLdsBudget = 64 * 1024;
static_assert(TH * TW == NT, "one thread per output pixel of the tile");

// ---- host-side sizing (plain C++) ----

// The LDS of one workgroup: hk [TW][kh_cap] and vk [TH][kv_cap] ints (a row holds its table's own k <= cap taps), src
// [cap_rows][stride()] bytes (rows start dword-aligned), tmp [cap_rows][TW][3] bytes (the horizontal pass).  The host wrapper sizes
// it and hands it to the kernel as it is.
struct Layout {
  int kh_cap, kv_cap, cap_rows, cap_cols;
  constexpr long stride() const { return (cap_cols * 3L + 6) & ~3L; }
  constexpr long bytes() const { return ((long)TW * kh_cap + (long)TH * kv_cap) * 4 + cap_rows * stride() + (long)cap_rows * TW * 3; }
};

// rows / columns of the source rectangle no tile of T outputs can exceed: the T windows start at most (T-1)*size/out apart
// (+1 for the truncation of each end) and the last is at most k long
inline int extent(int T, int size, int out, int k) {
  const long e = ((long)(T - 1) * size + out - 1) / out + k + 1;
  return (int)(e < size ? e : size);
}

// for out_h x out_w pixels from sources of at most src_h x src_w, through tables of at most kh / kv taps
inline Layout layout(int out_h, int out_w, int src_h, int src_w, int kh, int kv) {
  return {kh, kv, extent(TH, src_h, out_h, kv), extent(TW, src_w, out_w, kh)};
}

// ---- device side ----

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ float norm8(int u) { return (float)u / 255.0f * 2.0f - 1.0f; }      // ToTensor, then *2-1
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One 1-D table: k = 0 means every window is empty.  A launch with one table per axis fills it from its arguments (its host wrapper
// checks k > 0), a launch with a table pool through table_of.
struct Table {
  const int* bounds;      // [out][2]
  const int* coef;        // [out][k]
  int k;
};

// table t of a table pool -- bounds [out][2] then coefficients [out][k] at tab[tab_dir[2t]], k = tab_dir[2t+1] -- checked against
// the pool: k = 0 when the directory entry does not fit
__device__ __forceinline__ Table table_of(const int* __restrict__ tab, long tab_ints, const int* __restrict__ tab_dir,
                                          int n_tables, int t, int out, int kmax) {
  t = clampi(t, 0, n_tables - 1);
  const long off = tab_dir[2 * t];
  const int k = tab_dir[2 * t + 1];
  const bool ok = off >= 0 && k > 0 && k <= kmax && off + (long)out * (2 + k) <= tab_ints;
  const int* bounds = tab + (ok ? off : 0);
  return Table{bounds, bounds + 2 * out, ok ? k : 0};
}

// window {start, length} of output coordinate i, clipped to [0, size) and to the table's k taps
__device__ __forceinline__ void window(const Table& t, int i, int size, int& s, int& len) {
  if (t.k == 0) { s = 0; len = 0; return; }
  s = clampi(t.bounds[2 * i], 0, size);
  len = clampi(t.bounds[2 * i + 1], 0, min(t.k, size - s));
}

// One source plane: an image in a byte pool and the region of it the tables resize.
struct Plane {
  const unsigned char* pool;
  long pool_dwords;       // every read is guarded by it
  long base;              // byte offset of the image in the pool
  int pitch, C;           // pixels per image row, bytes per pixel (3 or 1)
  int y0, x0, h, w;       // origin and extent of the region the windows are clipped to
};

// The source rectangle a tile staged, in region coordinates, and where its bytes are in LDS.
struct Staged {
  int sx0, sy0, ncols, nrows;
  const unsigned char* src;
  int stride;
  long byte0, row_bytes;      // pool byte address of the rectangle's first pixel; bytes per image row
  // rectangle row r, column 0: the low two bits of its pool address = where the row starts in its LDS dwords
  __device__ __forceinline__ const unsigned char* row(int r) const { return src + r * stride + (int)((byte0 + r * row_bytes) & 3); }
};

// Tile rows [r0, r0 + nr) x columns [c0, c0 + nc) of plane p resized through ht / vt: store(row, col, c, u) is called once for
// every output pixel and channel with its finished byte u.  All NT threads of the workgroup call it.
template <class Store>
__device__ __forceinline__ Staged resample_tile(const Plane& p, const Table& ht, const Table& vt, const Layout& lay, int r0, int c0,
                                                int nr, int nc, Store&& store) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* hk = reinterpret_cast<int*>(smem);
  int* vk = hk + TW * lay.kh_cap;
  unsigned char* src = reinterpret_cast<unsigned char*>(vk + TH * lay.kv_cap);
  const int stride = (int)lay.stride();
  unsigned char* tmp = src + lay.cap_rows * stride;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, C = p.C, kh = ht.k, kv = vt.k;

  // the tile's source rectangle
  int sx0 = p.w, sx1 = 0, sy0 = p.h, sy1 = 0, s, len;
  for (int i = 0; i < nc; ++i) {
    window(ht, c0 + i, p.w, s, len);
    sx0 = min(sx0, s); sx1 = max(sx1, s + len);
  }
  for (int i = 0; i < nr; ++i) {
    window(vt, r0 + i, p.h, s, len);
    sy0 = min(sy0, s); sy1 = max(sy1, s + len);
  }
  Staged st;
  st.sx0 = sx0, st.sy0 = sy0, st.src = src, st.stride = stride;
  st.ncols = clampi(sx1 - sx0, 0, lay.cap_cols), st.nrows = clampi(sy1 - sy0, 0, lay.cap_rows);
  st.byte0 = p.base + ((long)(p.y0 + sy0) * p.pitch + (p.x0 + sx0)) * C, st.row_bytes = (long)p.pitch * C;
  const int ncols = st.ncols, nrows = st.nrows;

  for (int i = tid; i < nc * kh; i += NT) hk[i] = ht.coef[(long)c0 * kh + i];
  for (int i = tid; i < nr * kv; i += NT) vk[i] = vt.coef[(long)r0 * kv + i];
  const uint32_t* pool32 = reinterpret_cast<const uint32_t*>(p.pool);
  for (int r = wave; r < nrows; r += NT / 64) {
    const long byte0 = st.byte0 + r * st.row_bytes, d0 = byte0 >> 2;
    const int nd = (int)(((byte0 & 3) + ncols * C + 3) >> 2);          // <= stride / 4
    uint32_t* dst = reinterpret_cast<uint32_t*>(src + r * stride);
    for (int d = lane; d < nd; d += 64) {
      const long g = d0 + d;
      dst[d] = (g >= 0 && g < p.pool_dwords) ? pool32[g] : 0u;
    }
  }
  __syncthreads();

  // horizontal pass: every rectangle row x tile column x channel
  for (int j = tid; j < nrows * nc * C; j += NT) {
    const int c = j % C, col = (j / C) % nc, r = j / (C * nc);
    window(ht, c0 + col, p.w, s, len);
    s = max(s, sx0);
    len = clampi(len, 0, sx0 + ncols - s);
    const unsigned char* px = st.row(r) + (s - sx0) * C + c;
    int acc = 1 << 21;
    for (int k = 0; k < len; ++k) acc += hk[col * kh + k] * (int)px[C * k];
    tmp[(r * TW + col) * C + c] = (unsigned char)clip8(acc);
  }
  __syncthreads();

  // vertical pass: one thread per output pixel
  const int col = tid % TW, row = tid / TW;
  if (col < nc && row < nr) {
    window(vt, r0 + row, p.h, s, len);
    s = max(s, sy0);
    len = clampi(len, 0, sy0 + nrows - s);
    for (int c = 0; c < C; ++c) {
      const unsigned char* px = tmp + ((s - sy0) * TW + col) * C + c;
      int acc = 1 << 21;
      for (int k = 0; k < len; ++k) acc += vk[row * kv + k] * (int)px[k * TW * C];
      store(r0 + row, c0 + col, c, clip8(acc));
    }
  }
  return st;
}

}  // namespace resample_u8

// Weight / gradient layout transforms between the reference's parameter layout (OIHW,
// /root/reference/unet/uncond_unet.py:85) and the K-contiguous packed operands of the implicit-GEMM
// kernels.  Pure data movement over <= 11 MB per tensor; run once per optimiser step (or once per
// model for sampling), so simplicity beats tuning here.
#include "common.h"
#include "split_format.h"
#include <type_traits>

namespace {

// packed row (head, {q,k,v}, c) -> reference row (head, c, {q,k,v})   (uncond_unet.py:205)
__device__ __forceinline__ int qkv_to_ref(int n) {
  int h = n / 192, r = n - h * 192;
  int j = r >> 6, c = r & 63;
  return h * 192 + c * 3 + j;
}
__device__ __forceinline__ int qkv_to_packed(int n) {
  int h = n / 192, r = n - h * 192;
  int c = r / 3, j = r - c * 3;
  return h * 192 + j * 64 + c;
}

__global__ void pack_fwd_kernel(const float* __restrict__ w, float* __restrict__ out, int Co, int Ci, int taps,
                                int Co_pad, int Ci_pad, int qkv) {
  long total = (long)Co_pad * taps * Ci_pad;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    int ci = idx % Ci_pad;
    long t = idx / Ci_pad;
    int tap = t % taps;
    int cop = t / taps;
    float v = 0.f;
    if (cop < Co && ci < Ci) {
      int co = qkv ? qkv_to_ref(cop) : cop;
      v = w[((long)co * Ci + ci) * taps + tap];
    }
    out[idx] = v;
  }
}

// out[ci][taps-1-tap][co_packed] = w[co][ci][tap]
__global__ void pack_bwd_kernel(const float* __restrict__ w, float* __restrict__ out, int Co, int Ci, int taps,
                                int Co_pad, int Ci_pad, int qkv) {
  long total = (long)Ci_pad * taps * Co_pad;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    int cop = idx % Co_pad;
    long t = idx / Co_pad;
    int tapf = t % taps;
    int ci = t / taps;
    float v = 0.f;
    if (cop < Co && ci < Ci) {
      int co = qkv ? qkv_to_ref(cop) : cop;
      v = w[((long)co * Ci + ci) * taps + (taps - 1 - tapf)];
    }
    out[idx] = v;
  }
}

__global__ void unpack_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Co, int Ci, int taps,
                              int Ci_pad, int qkv, int accumulate, int splits, long split_stride) {
  long total = (long)Co * Ci * taps;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    int tap = idx % taps;
    long t = idx / taps;
    int ci = t % Ci;
    int co = t / Ci;
    int cop = qkv ? qkv_to_packed(co) : co;
    const long src = ((long)cop * taps + tap) * Ci_pad + ci;
    float v = dwp[src];
    for (int z = 1; z < splits; ++z) v += dwp[z * split_stride + src];      // fixed order: deterministic
    dw[idx] = accumulate ? dw[idx] + v : v;
  }
}

__global__ void permute_vec_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int n_pad, int qkv,
                                   int inverse) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pad) return;
  float v = 0.f;
  if (i < n) {
    int src = i;
    if (qkv) src = inverse ? qkv_to_packed(i) : qkv_to_ref(i);
    v = in[src];
  }
  out[i] = v;
}

// out[n] = sum_m a[m][n].  One block per 64-column strip x row-chunk; fp32 partials, atomics across chunks.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, float* __restrict__ out, int M,
                                                     int N, int ld, int rows_per_block) {
  __shared__ float part[4][64];
  int col = blockIdx.x * 64 + (threadIdx.x & 63);
  int ry = threadIdx.x >> 6;
  int m0 = blockIdx.y * rows_per_block;
  int m1 = min(M, m0 + rows_per_block);
  float s = 0.f;
  if (col < N)
    for (int m = m0 + ry; m < m1; m += 4) s += a[(long)m * ld + col];
  part[ry][threadIdx.x & 63] = s;
  __syncthreads();
  if (ry == 0 && col < N) {
    s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    atomicAdd(&out[col], s);
  }
}

// Destinations of the table kernel come out of an int64 table: said to be global memory, so that the stores are global_store_* and
// not flat_store_* (which also count against the LDS counter the tile reads wait on).
template <typename T> using gptr = __attribute__((address_space(1))) T*;
template <typename T> __device__ __forceinline__ gptr<T> table_ptr(long v) { return (gptr<T>)reinterpret_cast<T*>(v); }
// a[0..3] -> the three bf16 terms (split3_store's arithmetic), each as one 8-byte store
__device__ __forceinline__ void split3_store4(const float (&a)[4], gptr<unsigned short> d, long term) {
  unsigned t[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float r1 = a[j] - bf16_head(a[j]), r2 = r1 - bf16_head(r1);
    t[0][j] = bf16_bits(a[j]); t[1][j] = bf16_bits(r1); t[2][j] = bf16_bits(r2);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) *(gptr<u32x2>)(d + k * term) = u32x2{t[k][0] | (t[k][1] << 16), t[k][2] | (t[k][3] << 16)};
}
// a[0..3] (already scaled) -> the two fp16 terms (split2's arithmetic), each as one 8-byte store
__device__ __forceinline__ void split2_store4(const float (&a)[4], gptr<unsigned short> d, long term) {
  unsigned t[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    _Float16 h0, h1;
    split2(a[j], h0, h1);
    t[0][j] = __builtin_bit_cast(unsigned short, h0); t[1][j] = __builtin_bit_cast(unsigned short, h1);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) *(gptr<u32x2>)(d + k * term) = u32x2{t[k][0] | (t[k][1] << 16), t[k][2] | (t[k][3] << 16)};
}

// One launch for ALL layers of a model: table[e] = one row of PT_COLS int64 per layer (the columns: adm_pack_weight_table in
// include/adm_hip.h; adm_amd/ops.py fills them under the same names).  One workgroup per 32
// (out-channel) x 32 (in-channel) tile of one layer: the tile's taps-interleaved source runs (32*taps contiguous floats per
// out-channel) go through LDS once and leave as 128-byte row segments of every operand layout, so reads and writes are
// coalesced (the previous element-per-thread gather ran at 0.7 TB/s and cost 3.8 ms per optimiser step).
// The 16-bit images (split_format.h) leave as runs of four consecutive k of one row per (plane, term): thread (row = tid / 8,
// run = tid % 8) of the 32 x 32 tile, so that one store instruction of a wave covers eight rows of each of the tile's two k-chunks
// -- two contiguous 256-byte pieces of the [rows][16] blocks -- where the element-per-lane map wrote 2 bytes per lane into 64-byte
// pieces.  PT_FWD / PT_BWD may be 0: most layers never read their f32 operands (the split kernels read the images).
enum : int { PT_SRC, PT_FWD, PT_BWD, PT_CO, PT_CI, PT_TAPS, PT_CO_PAD, PT_CI_PAD, PT_QKV, PT_TILE_BEGIN, PT_WF, PT_WB, PT_W2F, PT_W2B, PT_W2F6,
             PT_W2B6, PT_G6F, PT_G6B, PT_W2FH, PT_W2BH, PT_H3_SCALE, PT_H3_FLAG, PT_G6FH, PT_G6BH, PT_COLS };
static_assert(PT_COLS == 24, "a row of adm_pack_weight_table has 24 columns (include/adm_hip.h)");
__global__ __launch_bounds__(256) void pack_table_kernel(const long* __restrict__ table, int n_entries) {
  __shared__ float tile[32][32 * 9 + 1];
  // layer of this tile: last row whose tile_begin <= blockIdx.x
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(long)mid * PT_COLS + PT_TILE_BEGIN] <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const long* t = table + (long)lo * PT_COLS;
  const gptr<const float> w = table_ptr<const float>(t[PT_SRC]);
  const gptr<float> fwd = table_ptr<float>(t[PT_FWD]);
  const gptr<float> bwd = table_ptr<float>(t[PT_BWD]);
  const int Co = (int)t[PT_CO], Ci = (int)t[PT_CI], taps = (int)t[PT_TAPS], Co_pad = (int)t[PT_CO_PAD], Ci_pad = (int)t[PT_CI_PAD], qkv = (int)t[PT_QKV];
  const gptr<float> wf = table_ptr<float>(t[PT_WF]);
  const gptr<float> wb = table_ptr<float>(t[PT_WB]);
  const int local = (int)((long)blockIdx.x - t[PT_TILE_BEGIN]);
  const int tiles_ci = Ci_pad >> 5;
  const int co0 = (local / tiles_ci) << 5, ci0 = (local % tiles_ci) << 5;
  const int run = 32 * taps;                       // floats per out-channel row of the tile
  const int n = 32 * run;
  // NB loads in flight per lane, then their NB LDS writes (one load per trip left the read side waiting out a memory round trip
  // 4 * taps times per tile); n / 256 = 4 * taps trips: twelve at a time for the 3x3 layers, four otherwise
  auto fill = [&](auto batch) {
    constexpr int NB = decltype(batch)::value;
    for (int e0 = threadIdx.x; e0 < n; e0 += 256 * NB) {
      float v[NB];
      int at[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int e = e0 + u * 256;
        const int r = e / run, c = e - r * run;    // c = ci_l * taps + tap
        const int cop = co0 + r, ci = ci0 + c / taps;
        v[u] = 0.f;
        if (cop < Co && ci < Ci) v[u] = w[((long)(qkv ? qkv_to_ref(cop) : cop) * Ci + ci0) * taps + c];
        at[u] = r * (32 * 9 + 1) + c;
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) (&tile[0][0])[at[u]] = v[u];
    }
  };
  if (taps % 3 == 0) fill(std::integral_constant<int, 12>{}); else fill(std::integral_constant<int, 4>{});
  __syncthreads();
  // 1x1 layers on conv_gemm_x6.hip: both operands in both split formats of split_format.h, rows_image_offset: three bf16 terms
  // (PT_G6F, PT_G6B) and two fp16 terms of scale * w (PT_G6FH, PT_G6BH)
  const gptr<unsigned short> g6f = table_ptr<unsigned short>(t[PT_G6F]);
  const gptr<unsigned short> g6b = table_ptr<unsigned short>(t[PT_G6B]);
  const gptr<unsigned short> g6fh = table_ptr<unsigned short>(t[PT_G6FH]);
  const gptr<unsigned short> g6bh = table_ptr<unsigned short>(t[PT_G6BH]);
  const float hscale = __uint_as_float((unsigned)t[PT_H3_SCALE]);
  bool hbad = false;                               // a scaled weight left the fp16 range
  if (fwd) {
    for (int e = threadIdx.x; e < n; e += 256) {   // forward operand [Co_pad][taps][Ci_pad]: ci fastest
      const int ci_l = e & 31, rest = e >> 5;
      const int tap = rest % taps, co_l = rest / taps;
      fwd[((long)(co0 + co_l) * taps + tap) * Ci_pad + ci0 + ci_l] = tile[co_l][ci_l * taps + tap];
    }
  }
  if (bwd) {
    for (int e = threadIdx.x; e < n; e += 256) {   // data-gradient operand [Ci_pad][taps flipped][Co_pad]: co fastest
      const int co_l = e & 31, rest = e >> 5;
      const int tapf = rest % taps, ci_l = rest / taps;
      bwd[((long)(ci0 + ci_l) * taps + tapf) * Co_pad + co0 + co_l] = tile[co_l][ci_l * taps + (taps - 1 - tapf)];
    }
  }
  // the image maps: row r4 of the tile, columns c4 .. c4 + 3 (one run of a 16-k chunk)
  const int r4 = threadIdx.x >> 3, c4 = (threadIdx.x & 7) << 2;
  if (taps == 1) {
#pragma unroll
    for (int which = 0; which < 2; ++which) {      // 0: rows = couts, k = cin; 1 (data gradient): rows = cins, k = cout
      const gptr<unsigned short> d6 = which ? g6b : g6f;
      const gptr<unsigned short> dh = which ? g6bh : g6fh;
      if (!d6 && !dh) continue;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = which ? tile[c4 + j][r4] : tile[r4][c4 + j];
      const int rows = which ? Ci_pad : Co_pad;
      const int nn = (which ? ci0 : co0) + r4, k = (which ? co0 : ci0) + c4;
      if (d6) split3_store4(v, d6 + rows_image_offset(3, rows, nn, k), split_term_stride(rows));
      if (dh) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = v[j] * hscale;
          hbad |= split_f16_overflow(v[j]);
        }
        split2_store4(v, dh + rows_image_offset(2, rows, nn, k), split_term_stride(rows));
      }
    }
  }
  int* __restrict__ hflag = reinterpret_cast<int*>(t[PT_H3_FLAG]);
  if (hbad && hflag) *hflag = 1;                   // the host falls back to the bf16 format
  if (taps != 9) return;
  // Winograd F(2,3) operands (conv_wino.hip): G g per filter row, u = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2)
  if (wf) {                                        // wf[xi][co][ky][ci]: ci fastest
    const long plane = (long)Co_pad * 3 * Ci_pad;
    for (int e = threadIdx.x; e < 32 * 3 * 32; e += 256) {
      const int ci_l = e & 31, rest = e >> 5;
      const int ky = rest % 3, co_l = rest / 3;
      const float* g = &tile[co_l][ci_l * 9 + ky * 3];
      const float g0 = g[0], g1 = g[1], g2 = g[2];
      const long o = ((long)(co0 + co_l) * 3 + ky) * Ci_pad + ci0 + ci_l;
      wf[o] = g0;
      wf[o + plane] = (g0 + g1 + g2) * 0.5f;
      wf[o + 2 * plane] = (g0 - g1 + g2) * 0.5f;
      wf[o + 3 * plane] = g2;
    }
  }
  // 2-D Winograd F(2x2, 3x3) operands (conv_wino2d.hip): U = G g G^T, plane ey * 4 + ex
  // ... and both split formats of them (split_format.h, wino_image_offset) for conv_wino2d_x6.hip: three bf16 terms (PT_W2F6, PT_W2B6)
  // and two fp16 terms of scale * U (PT_W2FH, PT_W2BH); 0 when unused
  const gptr<float> wf2 = table_ptr<float>(t[PT_W2F]);
  const gptr<float> wb2 = table_ptr<float>(t[PT_W2B]);
  const gptr<unsigned short> wf6 = table_ptr<unsigned short>(t[PT_W2F6]);
  const gptr<unsigned short> wb6 = table_ptr<unsigned short>(t[PT_W2B6]);
  const gptr<unsigned short> wfh = table_ptr<unsigned short>(t[PT_W2FH]);
  const gptr<unsigned short> wbh = table_ptr<unsigned short>(t[PT_W2BH]);
  // G g of the three filter rows of g (flipped for the data gradient): tr[a][ex]
  auto half_transform = [](const float* g, int which, float (&tr)[3][4]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int ra = which ? 2 - a : a;                // flipped filter for the data gradient
      const float g0 = which ? g[ra * 3 + 2] : g[ra * 3], g1 = g[ra * 3 + 1], g2 = which ? g[ra * 3] : g[ra * 3 + 2];
      tr[a][0] = g0; tr[a][1] = (g0 + g1 + g2) * 0.5f; tr[a][2] = (g0 - g1 + g2) * 0.5f; tr[a][3] = g2;
    }
  };
  if (wf2 || wb2) {                                  // the f32 planes: one element per lane, 128-byte row segments
    const long plane2 = (long)Co_pad * Ci_pad;
    for (int e = threadIdx.x; e < 32 * 32; e += 256) {
      // forward operand: ci fastest; data-gradient operand: co fastest -> two index maps over the same 32 x 32 tile
      for (int which = 0; which < 2; ++which) {
        const gptr<float> dst = which ? wb2 : wf2;
        if (!dst) continue;
        const int fast = e & 31, slow = e >> 5;
        const int co_l = which ? fast : slow, ci_l = which ? slow : fast;
        float tr[3][4];
        half_transform(&tile[co_l][ci_l * 9], which, tr);
        // (rows, cols) = (Co_pad, Ci_pad) forward, (Ci_pad, Co_pad) data gradient
        const int cols = which ? Co_pad : Ci_pad;
        const long o = (long)(which ? ci0 + ci_l : co0 + co_l) * cols + (which ? co0 + co_l : ci0 + ci_l);
#pragma unroll
        for (int ex = 0; ex < 4; ++ex) {
          const float c0 = tr[0][ex], c1 = tr[1][ex], c2 = tr[2][ex];
          const float u[4] = {c0, (c0 + c1 + c2) * 0.5f, (c0 - c1 + c2) * 0.5f, c2};
#pragma unroll
          for (int ey = 0; ey < 4; ++ey) dst[(long)(ey * 4 + ex) * plane2 + o] = u[ey];
        }
      }
    }
  }
  if (wf6 || wb6 || wfh || wbh) {                    // the split images: four k of one row per lane and (plane, term)
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      const gptr<unsigned short> dst6 = which ? wb6 : wf6;
      const gptr<unsigned short> dsth = which ? wbh : wfh;
      if (!dst6 && !dsth) continue;
      float tr[4][3][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) half_transform(which ? &tile[c4 + j][r4 * 9] : &tile[r4][(c4 + j) * 9], which, tr[j]);
      const int rows = which ? Ci_pad : Co_pad, cols = which ? Co_pad : Ci_pad;
      const int nn = (which ? ci0 : co0) + r4, c = (which ? co0 : ci0) + c4;
#pragma unroll
      for (int ex = 0; ex < 4; ++ex) {
        float u[4][4];                                 // u[j][ey]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float c0 = tr[j][0][ex], c1 = tr[j][1][ex], c2 = tr[j][2][ex];
          u[j][0] = c0; u[j][1] = (c0 + c1 + c2) * 0.5f; u[j][2] = (c0 - c1 + c2) * 0.5f; u[j][3] = c2;
        }
#pragma unroll
        for (int ey = 0; ey < 4; ++ey) {
          float v[4] = {u[0][ey], u[1][ey], u[2][ey], u[3][ey]};
          if (dst6) split3_store4(v, dst6 + wino_image_offset(3, ey, ex, rows, cols, nn, c), split_term_stride(rows));
          if (dsth) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[j] = v[j] * hscale;
              hbad |= split_f16_overflow(v[j]);
            }
            split2_store4(v, dsth + wino_image_offset(2, ey, ex, rows, cols, nn, c), split_term_stride(rows));
          }
        }
      }
    }
    if (hbad && hflag) *hflag = 1;                 // a scaled weight left the fp16 range: the host falls back to the bf16 format
  }
  if (wb) {                                        // wb[xi][ci][ky'][co]: co fastest; g'(ky', kx') = w(2-ky', 2-kx')
    const long plane = (long)Ci_pad * 3 * Co_pad;
    for (int e = threadIdx.x; e < 32 * 3 * 32; e += 256) {
      const int co_l = e & 31, rest = e >> 5;
      const int kyf = rest % 3, ci_l = rest / 3;
      const float* g = &tile[co_l][ci_l * 9 + (2 - kyf) * 3];
      const float g0 = g[2], g1 = g[1], g2 = g[0];
      const long o = ((long)(ci0 + ci_l) * 3 + kyf) * Co_pad + co0 + co_l;
      wb[o] = g0;
      wb[o + plane] = (g0 + g1 + g2) * 0.5f;
      wb[o + 2 * plane] = (g0 - g1 + g2) * 0.5f;
      wb[o + 3 * plane] = g2;
    }
  }
}

}  // namespace

extern "C" int adm_pack_weight_table(const long* table, int n_entries, long total_tiles, hipStream_t stream) {
  if (!table || n_entries <= 0 || total_tiles <= 0 || total_tiles >= (1L << 31)) return ADM_EINVAL;
  hipLaunchKernelGGL(pack_table_kernel, dim3((unsigned)total_tiles), dim3(256), 0, stream, table, n_entries);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_pack_weight(const float* w, float* wp_fwd, float* wp_bwd, int Co, int Ci, int ks, int Co_pad,
                               int Ci_pad, int qkv, hipStream_t stream) {
  if (!w || Co <= 0 || Ci <= 0 || ks < 1 || ks > 7 || Co_pad < Co || Ci_pad < Ci) return ADM_EINVAL;
  if (qkv && (Co % 192 != 0 || Co_pad != Co)) return ADM_EINVAL;
  int taps = ks * ks;
  long total = (long)Co_pad * taps * Ci_pad;
  int grid = (int)min((long)4096, (total + 255) / 256);
  if (wp_fwd) hipLaunchKernelGGL(pack_fwd_kernel, dim3(grid), dim3(256), 0, stream, w, wp_fwd, Co, Ci, taps, Co_pad, Ci_pad, qkv);
  if (wp_bwd) hipLaunchKernelGGL(pack_bwd_kernel, dim3(grid), dim3(256), 0, stream, w, wp_bwd, Co, Ci, taps, Co_pad, Ci_pad, qkv);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_unpack_wgrad(const float* dwp, float* dw, int Co, int Ci, int ks, int Co_pad, int Ci_pad, int qkv,
                                int accumulate, hipStream_t stream) {
  if (!dwp || !dw || Co <= 0 || Ci <= 0 || ks < 1 || ks > 7 || Co_pad < Co || Ci_pad < Ci) return ADM_EINVAL;
  if (qkv && (Co % 192 != 0)) return ADM_EINVAL;
  int taps = ks * ks;
  long total = (long)Co * Ci * taps;
  int grid = (int)min((long)4096, (total + 255) / 256);
  hipLaunchKernelGGL(unpack_kernel, dim3(grid), dim3(256), 0, stream, dwp, dw, Co, Ci, taps, Ci_pad, qkv, accumulate, 1, 0L);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

namespace {
__global__ void bias_splits_kernel(const float* __restrict__ bws, float* __restrict__ dbias, int n, int splits, long stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = bws[i];
  for (int z = 1; z < splits; ++z) v += bws[z * stride + i];
  dbias[i] += v;
}
}  // namespace

// Deterministic counterpart of the atomic split reduction: ws[splits][Co_pad][taps][Ci_pad] partial weight gradients (from
// adm_conv_wgrad_ws) are summed in split order and scattered to OIHW; bws[splits][Co_pad] bias partials are summed into
// dbias[0..Co_pad) (+=, the packed channel order the atomic path accumulates in).  bws / dbias may be NULL.
extern "C" int adm_unpack_wgrad_splits(const float* ws, int splits, float* dw, int Co, int Ci, int ks, int Co_pad, int Ci_pad,
                                       int qkv, int accumulate, const float* bws, float* dbias, hipStream_t stream) {
  if (!ws || !dw || splits < 1 || Co <= 0 || Ci <= 0 || ks < 1 || ks > 7 || Co_pad < Co || Ci_pad < Ci) return ADM_EINVAL;
  if (qkv && (Co % 192 != 0)) return ADM_EINVAL;
  if ((bws == nullptr) != (dbias == nullptr)) return ADM_EINVAL;
  int taps = ks * ks;
  long total = (long)Co * Ci * taps;
  int grid = (int)min((long)4096, (total + 255) / 256);
  hipLaunchKernelGGL(unpack_kernel, dim3(grid), dim3(256), 0, stream, ws, dw, Co, Ci, taps, Ci_pad, qkv, accumulate, splits,
                     (long)Co_pad * taps * Ci_pad);
  if (bws)
    hipLaunchKernelGGL(bias_splits_kernel, dim3((Co_pad + 255) / 256), dim3(256), 0, stream, bws, dbias, Co_pad, splits,
                       (long)Co_pad);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_permute_vec(const float* in, float* out, int n, int n_pad, int qkv, int inverse,
                               hipStream_t stream) {
  if (!in || !out || n <= 0 || n_pad < n) return ADM_EINVAL;
  if (qkv && n % 192 != 0) return ADM_EINVAL;
  hipLaunchKernelGGL(permute_vec_kernel, dim3((n_pad + 255) / 256), dim3(256), 0, stream, in, out, n, n_pad, qkv, inverse);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

extern "C" int adm_colsum(const float* a, float* out, int M, int N, int ld, int accumulate, hipStream_t stream) {
  if (!a || !out || M <= 0 || N <= 0 || ld < N) return ADM_EINVAL;
  if (!accumulate) {
    if (hipMemsetAsync(out, 0, sizeof(float) * N, stream) != hipSuccess) return ADM_ELAUNCH;
  }
  int strips = (N + 63) / 64;
  int chunks = max(1, min(adm_cdiv(M, 64), 2048 / strips));
  int rows = adm_cdiv(M, chunks);
  chunks = adm_cdiv(M, rows);
  hipLaunchKernelGGL(colsum_kernel, dim3(strips, chunks), dim3(256), 0, stream, a, out, M, N, ld, rows);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

namespace {
// out[(tap * Ci_pad + ci)][co] = w[co][ci][tap]: the B operand (rows = (tap, ci), K = co contiguous) of the GEMM form of a
// transposed convolution, col[m][(tap, ci)] = sum_co dy[m][co] w[co][ci][tap]
__global__ void pack_tconv_kernel(const float* __restrict__ w, float* __restrict__ out, int Co, int Ci, int taps, int Co_pad,
                                  int Ci_pad) {
  const long total = (long)taps * Ci_pad * Co_pad;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int co = idx % Co_pad;
    const long t = idx / Co_pad;
    const int ci = t % Ci_pad, tap = t / Ci_pad;
    out[idx] = (co < Co && ci < Ci) ? w[((long)co * Ci + ci) * taps + tap] : 0.f;
  }
}
}  // namespace

extern "C" int adm_pack_weight_tconv(const float* w, float* out, int Co, int Ci, int ks, int Co_pad, int Ci_pad,
                                     hipStream_t stream) {
  if (!w || !out || Co <= 0 || Ci <= 0 || ks < 1 || ks > 7 || Co_pad < Co || Ci_pad < Ci) return ADM_EINVAL;
  const long total = (long)ks * ks * Ci_pad * Co_pad;
  hipLaunchKernelGGL(pack_tconv_kernel, dim3((unsigned)min((long)4096, (total + 255) / 256)), dim3(256), 0, stream, w, out, Co, Ci,
                     ks * ks, Co_pad, Ci_pad);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

namespace {
// dw[co][ci][ky][kx] (+)= sum_z sum_ey Gt[ky][ey] * wx[z][co][ey][kx][ci],  Gt = G^T rows (1, 1/2, 1/2, 0) (0, 1/2, -1/2, 0) (0, 1/2, 1/2, 1)
__global__ void unpack_wino2d_kernel(const float* __restrict__ wx, float* __restrict__ dw, int Co, int Ci, int Ci_pad, int accumulate,
                                     int splits, long split_stride) {
  const long total = (long)Co * Ci * 3;      // one thread per (co, ci, kx): its three ky taps
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int kx = idx % 3;
    const long t = idx / 3;
    const int ci = t % Ci, co = t / Ci;
    float m[4];
#pragma unroll
    for (int ey = 0; ey < 4; ++ey) {
      const long src = (((long)co * 4 + ey) * 3 + kx) * Ci_pad + ci;
      float v = wx[src];
      for (int z = 1; z < splits; ++z) v += wx[z * split_stride + src];
      m[ey] = v;
    }
    const float h = 0.5f * (m[1] + m[2]);
    const float w[3] = {m[0] + h, 0.5f * (m[1] - m[2]), h + m[3]};
    float* o = dw + ((long)co * Ci + ci) * 9 + kx;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) o[ky * 3] = accumulate ? o[ky * 3] + w[ky] : w[ky];
  }
}
}  // namespace

// adm_unpack_wgrad (+ _splits) for the output of adm_conv_wgrad_wino2d / adm_conv_wgrad_ws(wino = 2): wx[splits][Co_pad][4][3][Ci_pad]
extern "C" int adm_unpack_wgrad_wino2d(const float* wx, int splits, float* dw, int Co, int Ci, int Co_pad, int Ci_pad, int accumulate,
                                       const float* bws, float* dbias, hipStream_t stream) {
  if (!wx || !dw || splits < 1 || Co <= 0 || Ci <= 0 || Co_pad < Co || Ci_pad < Ci) return ADM_EINVAL;
  if ((bws == nullptr) != (dbias == nullptr)) return ADM_EINVAL;
  const long total = (long)Co * Ci * 3;
  hipLaunchKernelGGL(unpack_wino2d_kernel, dim3((unsigned)min((long)4096, (total + 255) / 256)), dim3(256), 0, stream, wx, dw, Co, Ci,
                     Ci_pad, accumulate, splits, (long)Co_pad * 12 * Ci_pad);
  if (bws)
    hipLaunchKernelGGL(bias_splits_kernel, dim3((Co_pad + 255) / 256), dim3(256), 0, stream, bws, dbias, Co_pad, splits, (long)Co_pad);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

namespace {
// One launch for the weight gradients of ALL layers.  Row = 12 int64: {src, dst, Co, Ci, taps (0: 2-D Winograd planes), Ci_pad, qkv,
// accumulate, zero_src, block_begin, 0, 0}; block_begin = exclusive prefix sum of the rows' block counts (UT_ITEMS items per block;
// items = Co*Ci*taps, or Co*Ci*3 for the Winograd planes, as in unpack_kernel / unpack_wino2d_kernel).
constexpr int UT_ITEMS = 2048, UT_COLS = 12;
__global__ __launch_bounds__(256) void unpack_table_kernel(const long* __restrict__ table, int rows) {
  int lo = 0, hi = rows - 1;                        // last row whose block_begin <= blockIdx.x (uniform)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(long)mid * UT_COLS + 9] <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const long* r = table + (long)lo * UT_COLS;
  float* src = reinterpret_cast<float*>(r[0]);
  float* dw = reinterpret_cast<float*>(r[1]);
  const int Co = (int)r[2], Ci = (int)r[3], taps = (int)r[4], Ci_pad = (int)r[5], qkv = (int)r[6];
  const bool accumulate = r[7] != 0, zero = r[8] != 0;
  const long b0 = ((long)blockIdx.x - r[9]) * UT_ITEMS;
  if (taps > 0) {
    const long total = (long)Co * Ci * taps;
    for (long idx = b0 + threadIdx.x; idx < min(total, b0 + UT_ITEMS); idx += 256) {
      const int tap = idx % taps;
      const long t = idx / taps;
      const int ci = t % Ci, co = t / Ci;
      const int cop = qkv ? qkv_to_packed(co) : co;
      float* sp = src + ((long)cop * taps + tap) * Ci_pad + ci;
      const float v = *sp;
      if (zero) *sp = 0.f;
      dw[idx] = accumulate ? dw[idx] + v : v;
    }
  } else {
    const long total = (long)Co * Ci * 3;
    for (long idx = b0 + threadIdx.x; idx < min(total, b0 + UT_ITEMS); idx += 256) {
      const int kx = idx % 3;
      const long t = idx / 3;
      const int ci = t % Ci, co = t / Ci;
      float m[4];
#pragma unroll
      for (int ey = 0; ey < 4; ++ey) {
        float* sp = src + (((long)co * 4 + ey) * 3 + kx) * Ci_pad + ci;
        m[ey] = *sp;
        if (zero) *sp = 0.f;
      }
      const float h = 0.5f * (m[1] + m[2]);
      const float w[3] = {m[0] + h, 0.5f * (m[1] - m[2]), h + m[3]};
      float* o = dw + ((long)co * Ci + ci) * 9 + kx;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) o[ky * 3] = accumulate ? o[ky * 3] + w[ky] : w[ky];
    }
  }
}
}  // namespace

extern "C" int adm_unpack_wgrad_table(const long* table, int rows, long total_blocks, hipStream_t stream) {
  if (!table || rows <= 0 || total_blocks <= 0 || total_blocks >= (1L << 31)) return ADM_EINVAL;
  hipLaunchKernelGGL(unpack_table_kernel, dim3((unsigned)total_blocks), dim3(256), 0, stream, table, rows);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// Kernel Inception distance (adm_amd/metrics/kid.py): the polynomial-kernel sums of every subset in one launch.
//
// For subset s, X = f1[idx1[s]] and Y = f2[idx2[s]] (m rows of D floats each), k(a, b) = (gamma <a, b> + coef0)^degree:
//   sums[s] = { sum_{i != j} k(X_i, X_j),  sum_{i != j} k(Y_i, Y_j),  sum_{i, j} k(X_i, Y_j) }
// kid_tile_kernel: one workgroup per 128 x 128 tile of one of the three Gram blocks of one subset.  The tile structure is
// conv_rect_kernel's (inception.hip): LDS-DMA staging of 32-float K chunks into XOR-swizzled 16-byte slots, double buffered, and
// v_mfma_f32_32x32x2_f32 -- the exact f32 MFMA, so a dot product is an fmaf chain.  What differs:
//   - both operands are ROWS gathered through the index tables: a row's byte offset is idx * D * 4, looked up once per workgroup;
//     a row is D contiguous floats, so the gather costs no coalescing and no gathered copy of the features exists;
//   - no Gram matrix is written: the epilogue turns each accumulator into double(acc) * gamma + coef0, raises it to `degree` by
//     repeated multiplication and adds it up, all in float64;
//   - rows and columns at subset positions >= m (the ragged edge of the last tile) are MASKED in the epilogue -- their operands read
//     as zero, but a zero dot product is worth coef0^degree, not 0 -- and so is the diagonal i == j of XX and YY;
//   - XX and YY are symmetric: only tiles tj >= ti exist, and an off-diagonal tile's sum is doubled (exact in float64).
// The K tail (D % 32 != 0; D % 4 == 0, so a 16-byte slot is inside or outside a row as a whole) is zero-padded by pointing the slot
// past the buffer's extent: the range check returns zeros.  The same offset serves rows past m and, as a guard, an index outside
// [0, n): wrong tables give wrong sums, never an access outside the features.
// A workgroup's sum has a fixed order (a thread's 64 entries in register order, the xor-shuffle tree, the four waves in order) and
// goes to partial[s][tile]; kid_reduce_kernel, a second small launch, adds a subset's partials in index order.  No float atomics:
// the same bits every run.
#include "common.h"

namespace {

constexpr int BT = ADM_KID_TILE;   // tile edge: 2 x 2 waves of 64 x 64, each 2 x 2 MFMA blocks of 32 x 32
constexpr int LDSS = 32;           // floats per LDS row (LDS-DMA writes linearly; the 16-byte slots of a row are XOR-swizzled)
constexpr int MT = 2, NT = 2, RI = BT / 32;   // RI: LDS-DMA instructions per wave, operand and stage (8 rows each)
constexpr unsigned OOB = 0x80000000u;         // past every extent the host accepts: the range check returns zeros
typedef __attribute__((address_space(3))) void lds_void;

struct KidP {
  const float* f1; const float* f2; const int* idx1; const int* idx2; double* partial;
  int n1, n2, D, m, T, per, degree;
  unsigned bytes1, bytes2;
  double gamma, coef0;
};

__global__ __launch_bounds__(256) void kid_tile_kernel(KidP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                       // [2][BT][LDSS]
  float* Bs = smem + 2 * BT * LDSS;       // [2][BT][LDSS]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int bid = adm_xcd_remap(blockIdx.x, gridDim.x);      // a subset's tiles are neighbours: they share its rows in one L2
  const int s = bid / p.per, t = bid - s * p.per;
  const int nsym = p.T * (p.T + 1) / 2;
  int kind, ti, tj;                                          // 0: XX, 1: YY, 2: XY
  if (t < 2 * nsym) {
    kind = t >= nsym;
    int u = t - kind * nsym;
    ti = 0;
    while (u >= p.T - ti) { u -= p.T - ti; ++ti; }            // row ti of the upper triangle holds tiles tj = ti .. T-1
    tj = ti + u;
  } else {
    kind = 2;
    const int u = t - 2 * nsym;
    ti = u / p.T;
    tj = u - ti * p.T;
  }
  const bool a2 = kind == 1, b1 = kind == 0;                 // A rows come from f2 only for YY, B rows from f1 only for XX
  const float* fa = a2 ? p.f2 : p.f1;
  const float* fb = b1 ? p.f1 : p.f2;
  const int* ia = (a2 ? p.idx2 : p.idx1) + (long)s * p.m;
  const int* ib = (b1 ? p.idx1 : p.idx2) + (long)s * p.m;
  const int na = a2 ? p.n2 : p.n1, nb = b1 ? p.n1 : p.n2;
  const __amdgpu_buffer_rsrc_t rs_a =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(fa), 0, (int)(a2 ? p.bytes2 : p.bytes1), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(fb), 0, (int)(b1 ? p.bytes1 : p.bytes2), 0x00020000);
  const int m0 = ti * BT, n0 = tj * BT;

  // Per staged row: the byte offset of this lane's 16-byte slot in K chunk 0 (OOB for a row past m), and the slot's first k.
  unsigned a_base[RI], b_base[RI];
  int k_slot[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int row = (wid * RI + i) * 8 + (lane >> 3);
    const int ls = (lane & 7) ^ ((row >> 1) & 7);
    k_slot[i] = ls * 4;
    const int pa = m0 + row, pb = n0 + row;
    const int ra = pa < p.m ? ia[pa] : -1, rb = pb < p.m ? ib[pb] : -1;
    a_base[i] = (unsigned)ra < (unsigned)na ? ((unsigned)ra * (unsigned)p.D + ls * 4) * 4u : OOB;
    b_base[i] = (unsigned)rb < (unsigned)nb ? ((unsigned)rb * (unsigned)p.D + ls * 4) * 4u : OOB;
  }
  const int KT = (p.D + 31) >> 5;

  auto issue_stage = [&](int kc, int buf) {
    float* la = As + buf * BT * LDSS + wid * RI * 8 * LDSS;
    float* lb = Bs + buf * BT * LDSS + wid * RI * 8 * LDSS;
    const int k0 = kc << 5;
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      const bool in = k0 + k_slot[i] < p.D;                    // the K tail: slots past the row read as zero
      const unsigned va = (in && a_base[i] != OOB) ? a_base[i] + (unsigned)(k0 * 4) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_void*)(la + i * 8 * LDSS), 16, (int)va, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      const bool in = k0 + k_slot[i] < p.D;
      const unsigned vb = (in && b_base[i] != OOB) ? b_base[i] + (unsigned)(k0 * 4) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (lds_void*)(lb + i * 8 * LDSS), 16, (int)vb, 0, 0, 0);
    }
  };
  int foff[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) foff[g] = lr * LDSS + (((2 * g + lh) ^ ((lr >> 1) & 7)) << 2);

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issue_stage(0, 0);
  __syncthreads();

  for (int kc = 0; kc < KT; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < KT) issue_stage(kc + 1, buf ^ 1);
    const float* Ab = As + buf * BT * LDSS + wm * MT * 32 * LDSS;
    const float* Bb = Bs + buf * BT * LDSS + wn * NT * 32 * LDSS;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 a[MT], b[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDSS + foff[g]);
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDSS + foff[g]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][k], b[j][k], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: C/D layout col = lane&31, row = (r&3) + 8 (r>>2) + 4 (lane>>5); rows are positions of A, columns of B.
  const bool sym = kind != 2;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int pj = n0 + (wn * NT + j) * 32 + lr;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int pb = m0 + (wm * MT + i) * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pi = pb + (r & 3) + 8 * (r >> 2);
        const double b = (double)acc[i][j][r] * p.gamma + p.coef0;
        double v = b;
        for (int d = 1; d < p.degree; ++d) v *= b;
        const bool keep = pi < p.m && pj < p.m && !(sym && pi == pj);
        sum += keep ? v : 0.0;
      }
    }
  }
  double* s_wave = reinterpret_cast<double*>(smem);          // the staging buffers are free: the K loop ended on a barrier
  sum = wave_sum_d(sum);
  if (lane == 0) s_wave[wid] = sum;
  __syncthreads();
  if (tid == 0) {
    const double v = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    p.partial[(long)s * p.per + t] = (sym && tj != ti) ? 2.0 * v : v;
  }
}

// sums[s][q] = the partials of block q of subset s, added in index order (XX, YY: nsym tiles each, then XY: T * T)
__global__ __launch_bounds__(64) void kid_reduce_kernel(const double* __restrict__ partial, double* __restrict__ sums, int S, int T,
                                                        int per) {
  const int s = blockIdx.x, q = threadIdx.x;
  if (s >= S || q >= 3) return;
  const int nsym = T * (T + 1) / 2;
  const int begin = q * nsym, end = q == 2 ? per : begin + nsym;
  const double* mine = partial + (long)s * per;
  double v = 0.0;
  for (int k = begin; k < end; ++k) v += mine[k];
  sums[(long)s * 3 + q] = v;
}

}  // namespace

extern "C" int adm_kid_sums_tile(int which) { return which == 0 ? BT : (which > 0 ? 0 : ADM_EINVAL); }

extern "C" long adm_kid_sums_blocks(int m) {
  if (m < 2) return ADM_EINVAL;
  const long T = (m + BT - 1) / BT;
  return T * (T + 1) + T * T;
}

extern "C" int adm_kid_sums(const float* f1, int n1, const float* f2, int n2, int D, const int* idx1, const int* idx2, int S, int m,
                            int degree, double gamma, double coef0, double* sums, double* partial, hipStream_t stream) {
  if (!f1 || !f2 || !idx1 || !idx2 || !sums || !partial) return ADM_EINVAL;
  if ((reinterpret_cast<uintptr_t>(f1) & 15) || (reinterpret_cast<uintptr_t>(f2) & 15)) return ADM_EINVAL;   // 16-byte slots
  if (D <= 0 || D % 4 != 0 || n1 <= 0 || n2 <= 0 || S < 1 || m < 2 || m > n1 || m > n2) return ADM_EINVAL;
  if (degree < 1 || degree > 8) return ADM_EINVAL;
  const long bytes1 = (long)n1 * D * 4, bytes2 = (long)n2 * D * 4;
  if (bytes1 >= (long)OOB || bytes2 >= (long)OOB) return ADM_EINVAL;      // 32-bit buffer offsets, OOB past the extent
  const long per = adm_kid_sums_blocks(m);
  if (per * S > 0x7fffffffL) return ADM_EINVAL;
  KidP p;
  p.f1 = f1; p.f2 = f2; p.idx1 = idx1; p.idx2 = idx2; p.partial = partial;
  p.n1 = n1; p.n2 = n2; p.D = D; p.m = m; p.T = (m + BT - 1) / BT; p.per = (int)per; p.degree = degree;
  p.bytes1 = (unsigned)bytes1; p.bytes2 = (unsigned)bytes2;
  p.gamma = gamma; p.coef0 = coef0;
  static bool attr_set = false;
  constexpr int smem = 4 * BT * LDSS * (int)sizeof(float);
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&kid_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem) !=
        hipSuccess)
      return ADM_ELAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)(per * S)), dim3(256), smem, stream, p);
  ADM_CHECK_LAUNCH();
  hipLaunchKernelGGL(kid_reduce_kernel, dim3(S), dim3(64), 0, stream, partial, sums, S, p.T, p.per);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// 3x3 stride-1 convolution (forward and data gradient): 2-D Winograd F(2x2, 3x3) with the f32 products carried on the bf16 MFMA.
//
// The split number formats are stated in split_format.h.  Specific to this kernel: six v_mfma_f32_32x32x16_bf16 (6 x 32 cycles for
// K = 16) replace eight v_mfma_f32_32x32x2_f32 (8 x 64 cycles): 2.67x less matrix-pipe time at f32 accuracy (tools/bf16x6_probe.hip:
// the six products in a short accumulator chain started from C = 0 and added to the running sum with one f32 add measure BELOW the
// f32 MFMA's own rounding error against fp64, on zero-mean and on all-positive data; six truncating matrix adds into one
// long-running accumulator would be 3x worse on the latter).
//
// The algorithm is conv_wino2d.hip's (same transforms, four ex accumulator tiles per wave, output rows folded in registers);
// the loop order and the division of labour are not:
//   * the matrix pipe is no longer the bound, the data path is.  The f32 kernel's stages are as long as a global load takes
//     (every barrier of a __syncthreads also drains vmcnt), which the 2048-cycle f32 MFMA phase used to cover; a 768-cycle bf16
//     phase does not.  So the roles are split (512 threads, one workgroup per CU):
//       - waves 4-7 PRODUCE the A operand: thread = (tile, 16-byte channel quad); one register set per chunk of a K block holds
//         two rows of the tile's 4 x 4 patch (4 pixels each, raw buffer loads, range check = zero padding) -- these waves hold no
//         accumulators, so they have the registers for it.  A pass ey y-combines the two rows (r0 - r2, r1 + r2, r2 - r1, r1 - r3),
//         B^T-transforms in f32 exactly as before, splits into three bf16 terms (and / sub / and / sub per element, v_perm
//         packing) and writes to LDS (twelve ds_write_b64).  In whole K blocks every patch row is fetched ONCE per chunk: (r0, r2)
//         before pass 0, r1 over r0 after pass 0, nothing after pass 1, r3 over r2 after pass 2, the next block's (r0, r2) after
//         pass 3 -- four row loads (16 buffer_load_dwordx4) per chunk and tile, each one block pass (KB stages) ahead of its
//         first use.  A partial last block, the fused up-sampling (three passes; r1 and r2 are one source row) and the REUSE = 0
//         instantiations (adm_wino2d_x6_row_reuse(0): the A/B switch, bit-identical results) fetch the two rows of every stage
//         KB stages ahead instead: eight row loads per chunk, r1 and r2 three times each.  Measured against the kernel without the
//         reuse (B = 128): -5..9 % on the 64-cout fp16 form, -1..2 % on the bf16 form at 32 x 32, within +-3 % on the 96- and
//         128-cout forms, whose consumer waves are the critical path (their producers wait at the barrier for more than half
//         of a stage); DESIGN.md section 4;
//       - waves 0-3 CONSUME: 32 tiles x 32 couts each, six MFMAs per ex plane and stage.  Stages are ordered K block (KB chunks:
//         4 in the 64-cout forms, 3 in the 96- and 128-cout forms = their producer register sets) > ey > chunk: inside a
//         (block, ey) group the accumulators run on (<= 6 KB matrix adds each, the first from C = 0), at its
//         end the x / y output transforms are applied and the result is added to the output rows held in registers with f32 adds
//         -- the long-running sums see rounded f32 adds, not truncating matrix adds: measured against fp64 the error is at or
//         below the f32 MFMA kernel's (tests/test_hip_ops.py::test_conv_x6_error_vs_fp64).
//         These waves also issue the weight DMA (their only global accesses: the explicit vmcnt wait before a barrier
//         never touches the producers' prefetch);
//       - barriers are s_barrier with LDS-scoped fences (lgkmcnt only): the producers' loads stay in flight across them.
//   * LDS: A[2][4 ex][3 terms][64 tiles][16 ch] bf16 (2 x 24 KB) + B[4][4 ex][3 terms][64 couts][16 ch] (4 x 24 KB; weights are
//     split once per optimiser step at pack time into the K-chunk-tiled layout of adm_split3_bf16 -- one contiguous KB per DMA
//     instruction -- and arrive by LDS-DMA three stages ahead).  Rows are 32
//     bytes with the two 16-byte halves of rows 8-15 (mod 16) swapped, so that the 16 lanes of a fragment-read group hit all 64 banks
//     (un-swizzled: 40 % of the LDS cycles were bank conflicts, SQ_LDS_BANK_CONFLICT).
// Replaces F.conv2d of Conv2d.forward and its autograd data gradient (/root/reference/unet/uncond_unet.py:98-110).
#include "common.h"
#include "split_format.h"
#include <type_traits>

#ifndef X6_TL
#define X6_TL 0      // diagnostic build: per-stage timeline of one consumer and one producer wave of workgroup 0 into p.ws (tools/bench_wino2d_x6.cpp)
#endif
#ifndef X6_KB_N
#define X6_KB_N 4    // chunks per K block of the 64-cout forms (the row reuse is compiled in only at 4 = their producer register sets)
#endif
#ifndef X6_ABL
#define X6_ABL 0     // diagnostic builds (tools/bench_wino2d_x6.cpp): 1 no A global loads, 2 no A transform / split / LDS stores, 4 no B DMA, 8 no MFMAs, 16 no LDS fragment reads
#endif

namespace {

struct X6P {
  const float* x; const unsigned short* w; const float* bias; const float* res; float* y;
  int Mt, N, H, W, Hh, Wh, Cin, ldx, ldy, ldr, wrows, tilesN, xbytes, wbytes, plane;   // plane = wrows * Cin (elements of one [term] image)
  int splitk, chunks_per_split; float* ws;
  int ybytes, rbytes;                  // > 0: y / res fit 32-bit byte offsets (branch-free buffer epilogue)
  int up;                              // 1: x is [B][H/2][W/2][ldx] and the conv runs on its nearest x2 up-sampling (Conv2d(up=True))
  const float* amax_x; float wscale;   // fp16 format only: bound vector (adm_hip.h) of |x|; the weights' (power-of-two) scale
};

typedef __attribute__((address_space(3))) void x6_lds_void;
constexpr int X6P_T = 64, X6N = 64, X6K = 16;      // tiles x couts x K step
[[maybe_unused]] constexpr int X6_A_STAGE = 4 * 3 * X6P_T * X6K;    // bf16 elements per A sub-stage image (24 KB; the bf16 format)
[[maybe_unused]] constexpr int X6_B_STAGE = 4 * 3 * X6N * X6K;
// FMT (template parameter of the kernel) = the split number format of split_format.h: 0 three bf16 terms, six products; 1 two fp16
// terms of s a, three products, s from a bound of max |a| that the caller passes as a device vector (the GroupNorm kernel that
// produced the activation wrote it).  On the GPU: tests/test_hip_ops.py::test_conv_h3_error_vs_fp64; format 1 halves the MFMAs,
// the fragment reads, the split stores and the weight DMA of a stage: 1.25 -> 1.02 ms on 128 x 32 x 32 x 384 -> 384 (the
// experiment is tools/exp_wino2d_h3.hip of commit 29b1b0b).
// NB = 32-cout blocks per workgroup.  2: 64 couts, four consumer waves (512 threads).  4 (the "wide" form, fp16 format only): 128
// couts, EIGHT consumer waves, two per SIMD, next to the same four producer waves (768 threads, <= 168 registers): one A image
// (loads from L2, transform, split, LDS stores -- the part of a stage that does not shrink with the format) now feeds twice the
// MFMAs, and the launch pulls half the activation bytes out of the L2 (every cout tile re-reads the whole input: at Cin = 384 the
// 64-cout form reads 74 KB per pixel, ~9.5 TB/s over the launch, more than half of what the L2s deliver).
template <int FMT, int NB = 2> struct X6Fmt {
  static constexpr int TERMS = split_terms(FMT);
  static constexpr int NT = 32 * NB;                 // couts per workgroup
  static constexpr int CONS = 2 * NB;                // consumer waves: (2 tile halves) x (NB cout blocks)
  static constexpr int THREADS = (CONS + 4) * 64;
  static constexpr int A_STAGE = 4 * TERMS * X6P_T * X6K;
  static constexpr int B_STAGE = 4 * TERMS * NT * X6K;
  static constexpr int DMA_PER_WAVE = 2 * TERMS;     // 4 ex x TERMS images x NB 32-row blocks / CONS consumer waves
  static constexpr int RB = NB > 2 ? 3 : 4;         // weight ring depth (LDS: 2 x 16 + 3 x 32 KB wide; 2 x 16 + 4 x 16 KB fp16, 2 x 24 + 4 x 24 KB bf16)
  static constexpr int PD = NB > 2 ? 3 : 4;         // producer register sets = stages of loads in flight
  static constexpr int KB = NB > 2 ? 3 : X6_KB_N;   // chunks per K block: one producer register set per chunk of a block (the row reuse needs KB == PD)
};
constexpr int X6_RA = 2;                           // A ring depth (the weights' is X6Fmt::RB: RB - 1 stages ahead, a DMA queues behind the producers' loads)

// (this file is compiled WITHOUT packed-f32 instruction selection -- csrc/Makefile, NOPK -- so vector adds below are plain v_add_f32 /
//  v_sub_f32; the PRODUCER's arithmetic uses the explicit plain_add4 / plain_sub4 of split_format.h)
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) { return a - b; }
__device__ __forceinline__ f32x16 sub16(f32x16 a, f32x16 b) { return a - b; }

// producer, fp16 format: as x6_store below, two-term split of s v
__device__ __forceinline__ void h3_store(const f32x4 (&e)[4], unsigned short* la, float s) {
  if (X6_ABL & 2) return;
  const f32x4 v[4] = {plain_sub4(e[0], e[2]), plain_add4(e[1], e[2]), plain_sub4(e[2], e[1]), plain_sub4(e[1], e[3])};
#pragma unroll
  for (int ex = 0; ex < 4; ++ex) {
    u32x2 t0, t1;
    split2_quad(v[ex], s, t0, t1);
    *reinterpret_cast<u32x2*>(la + (ex * 2 + 0) * X6P_T * X6K) = t0;
    *reinterpret_cast<u32x2*>(la + (ex * 2 + 1) * X6P_T * X6K) = t1;
  }
}

// producer: y-combined rows e[4] (one per pixel of the patch row) -> B^T along x -> three-term split -> the [ex][term] images
__device__ __forceinline__ void x6_store(const f32x4 (&e)[4], unsigned short* la) {
  if (X6_ABL & 2) return;
  const f32x4 v[4] = {plain_sub4(e[0], e[2]), plain_add4(e[1], e[2]), plain_sub4(e[2], e[1]), plain_sub4(e[1], e[3])};
#pragma unroll
  for (int ex = 0; ex < 4; ++ex) {
    u32x2 t0, t1, t2;
    split3_quad(v[ex], t0, t1, t2);
    *reinterpret_cast<u32x2*>(la + (ex * 3 + 0) * X6P_T * X6K) = t0;
    *reinterpret_cast<u32x2*>(la + (ex * 3 + 1) * X6P_T * X6K) = t1;
    *reinterpret_cast<u32x2*>(la + (ex * 3 + 2) * X6P_T * X6K) = t2;
  }
}

// Stage order shared by all three roles: K blocks of KB chunks (X6Fmt::KB: 4 for the 64-cout forms, 3 for the 96- and 128-cout
// forms) outermost, the four ey passes inside a block, chunks innermost (a stage = one (ey, chunk) pair).  Inside a (block, ey)
// group the MFMA accumulators run on (<= 6 KB matrix adds each); at its end they are transformed and added to the output rows with
// f32 adds.
// With the fused nearest x2 up-sampling the patch rows r1 and r2 are the SAME source row, so the pass ey = 2 (r2 - r1) is
// identically zero and is skipped (three passes per block).
template <int KB> struct X6Seq {
  int k0, len, ey, cc, skip2;   // block start (chunk), block length, pass, chunk inside the block, skip pass 2
  __device__ __forceinline__ void init(int chunks, int up, int start = 0) { k0 = start; len = min(KB, chunks - start); ey = 0; cc = 0; skip2 = up; }
  __device__ __forceinline__ int chunk() const { return k0 + cc; }
  __device__ __forceinline__ bool done() const { return len <= 0; }
  __device__ __forceinline__ void next(int chunks) {
    if (++cc == len) {
      cc = 0;
      ++ey;
      if (skip2 && ey == 2) ++ey;
      if (ey == 4) { ey = 0; k0 += len; len = min(KB, chunks - k0); }
    }
  }
};

template <int FMT, int NB, int REUSE>
__global__ __launch_bounds__((2 * NB + 4) * 64) void wino2d_x6_kernel(X6P p) {
  using F = X6Fmt<FMT, NB>;
  using Seq = X6Seq<F::KB>;
  constexpr int TERMS = F::TERMS;
  float sa = 1.f, inv_scale = 1.f;                     // fp16 format: operand scale and the factor that undoes both scales in the epilogue
  if (FMT) { sa = split_scale(adm_amax_read(p.amax_x)); inv_scale = 1.f / (sa * p.wscale); }
  extern __shared__ __attribute__((aligned(16))) unsigned short smem6[];
  unsigned short* As = smem6;                          // [X6_RA][4 ex][3 terms][X6P_T][X6K]
  unsigned short* Bs = smem6 + X6_RA * F::A_STAGE;     // [RB][4 ex][3 terms][X6N][X6K]
  const int tid = threadIdx.x, lane = tid & 63, hw_wid = tid >> 6;
  const bool producer = hw_wid >= F::CONS;
  const int wid = producer ? hw_wid - F::CONS : hw_wid;      // role-local wave index
  const int bid = adm_xcd_remap(blockIdx.x, gridDim.x);
  const int tilesM = gridDim.x / p.tilesN;
  const int tm = bid % tilesM, tn = bid / tilesM;
  const int mt0 = tm * X6P_T, n0 = tn * F::NT;
  constexpr unsigned OOB = 0x80000000u;

  const int c_begin = (p.splitk > 1) ? (int)blockIdx.y * p.chunks_per_split : 0;
  const int chunks = (p.splitk > 1) ? min(p.chunks_per_split, (p.Cin >> 4) - c_begin) : (p.Cin >> 4);     // 16-channel chunks (even)
  const int S = (p.up ? 3 : 4) * chunks;              // stages (an even number: Cin is a multiple of 32)

  if (producer) {
    // ================================================================ producer waves: A operand
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, p.xbytes, 0x00020000);
    const int ptid = wid * 64 + lane;
    const int pl = ptid >> 2, aq = ptid & 3;          // tile, channel quad
    unsigned a_base = 0, colmask = 0, rowmask = 0;
    {
      const int t = mt0 + pl;
      if (t < p.Mt) {
        const int xp = t % p.Wh;
        const int u = t / p.Wh;
        const int ty = u % p.Hh, b = u / p.Hh;
        a_base = p.up ? (unsigned)((((long)b * p.Hh + ty) * p.Wh + xp) * p.ldx + aq * 4) * 4u        // source pixel (b, ty, xp)
                      : (unsigned)((((long)b * p.H + 2 * ty) * p.W + 2 * xp) * p.ldx + aq * 4) * 4u;
        colmask = (xp > 0 ? 1u : 0u) | 6u | (2 * xp + 2 < p.W ? 8u : 0u);
        rowmask = (ty > 0 ? 1u : 0u) | 6u | (2 * ty + 2 < p.H ? 8u : 0u);
      }
    }
    // rows are 32 bytes; a 16-lane group of a fragment read covers 16 rows at one 16-byte half, i.e. only half of the banks, unless
    // the halves of rows 8-15 (mod 16) are swapped: physical half = logical half ^ ((row >> 3) & 1), for A and B alike
    unsigned short* la = As + pl * X6K + ((((aq >> 1) ^ (pl >> 3)) & 1) << 3) + (aq & 1) * 4;
    constexpr int D = F::PD;                          // register sets
    f32x4 dA[D][4], dB[D][4];
    // y-combination of pass ey: 0: r0 - r2   1: r1 + r2   2: r2 - r1   3: r1 - r3, from the (A, B) halves of a register set
    auto combine = [&](int ey, const f32x4 (&a)[4], const f32x4 (&b)[4], f32x4 (&e)[4]) {
      if (ey == 1) {                                  // (wave-uniform, or a constant)
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = plain_add4(a[j], b[j]);
      } else if (ey == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = plain_sub4(b[j], a[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = plain_sub4(a[j], b[j]);
      }
    };
    int k_done = 0, t_done = 0;                       // chunks / stages the whole-block loop below has finished
    if constexpr (REUSE != 0 && F::KB == D) {
      // ---- whole K blocks, each patch row fetched once.  Set cc holds rows of chunk k0 + cc for the whole block: (r0, r2) when pass 0
      // starts; r1 replaces r0 in the A half after pass 0 (passes 1 and 2 combine r1 and r2 as they lie); r3 replaces r2 in the B half
      // after pass 2; the next block's (r0, r2) follow pass 3.  Every load is KB stages ahead of its first use, as in the generic body
      // below, which asks for two rows per stage (eight per chunk instead of four).  Every load of the loop is unconditional, so
      // the compiler's vmcnt in front of a stage's transform counts the later loads of the other sets and leaves them in flight.
      // Offsets: four registers for the columns at patch row 1 (column mask baked in) and four for row 0 (row mask too); rows 2
      // and 3 and the chunk go into the scalar offset.  Not for the fused up-sampling (three passes, r1 and r2 one source row).
      constexpr int KB = F::KB;
      const int nwhole = p.up ? 0 : chunks / KB;
      if (nwhole > 0) {
        const int rstride = p.W * p.ldx * 4;          // bytes per input row
        unsigned v0[4], vc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool cv = (colmask >> j) & 1u;
          const int cj = (j - 1) * p.ldx * 4;
          vc[j] = cv ? a_base + (unsigned)cj : OOB;
          v0[j] = (cv && (rowmask & 1u)) ? a_base + (unsigned)(cj - rstride) : OOB;
        }
        const unsigned k3 = (rowmask & 8u) ? 0u : OOB;     // row 3 below the image: out of range
        auto row = [&](f32x4 (&dst)[4], const unsigned (&vo)[4], unsigned kill, int soff) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (X6_ABL & 1) { dst[j] = f32x4{1.f, 2.f, (float)j, (float)soff}; continue; }
            dst[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)(vo[j] | kill), soff, 0));
          }
        };
#pragma unroll
        for (int cc = 0; cc < KB; ++cc) {
          row(dA[cc], v0, 0u, (c_begin + cc) << 6);   // 16 floats = 64 bytes per chunk
          row(dB[cc], vc, 0u, ((c_begin + cc) << 6) + rstride);
          __builtin_amdgcn_sched_barrier(0);          // (in the loop's order: the waits at its head are merged over both ways in)
        }
        for (int blk = 0; blk < nwhole; ++blk) {
          const int cb = (c_begin + blk * KB) << 6;
          const unsigned nx = blk + 1 < nwhole ? 0u : OOB;      // (uniform) no whole block follows: its rows are not asked for
#pragma unroll
          for (int ey = 0; ey < 4; ++ey) {
#pragma unroll
            for (int cc = 0; cc < KB; ++cc) {
              const int k = ey * KB + cc, ts = blk * 4 * KB + k;
              const bool tl = X6_TL && p.ws && blockIdx.x == 0 && tid == F::CONS * 64 && ts < 48;
              unsigned long long* TL = reinterpret_cast<unsigned long long*>(p.ws) + 1024 + ts * 4;
              if (tl) TL[0] = __builtin_readcyclecounter();
              f32x4 e[4];
              combine(ey, dA[cc], dB[cc], e);
              if (FMT) h3_store(e, la + (k & 1) * F::A_STAGE, sa);     // (4 * KB stages per block: an even number, so static slots)
              else x6_store(e, la + (k & 1) * F::A_STAGE);
              __builtin_amdgcn_sched_barrier(0);
              if (tl) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); TL[1] = __builtin_readcyclecounter(); }
              const int so = cb + (cc << 6);
              if (ey == 0) row(dA[cc], vc, 0u, so);
              if (ey == 2) row(dB[cc], vc, k3, so + 2 * rstride);
              if (ey == 3) { row(dA[cc], v0, nx, so + (KB << 6)); row(dB[cc], vc, nx, so + (KB << 6) + rstride); }
              __builtin_amdgcn_sched_barrier(0);
              if (tl) TL[2] = __builtin_readcyclecounter();
              adm_lds_barrier();
              if (tl) TL[3] = __builtin_readcyclecounter();
            }
          }
        }
        k_done = nwhole * KB; t_done = nwhole * 4 * KB;
      }
    }
    // ---- generic body: a partial last block, the fused up-sampling, REUSE = 0.  The loads of a stage (2 rows x 4 pixels) are issued
    // D stages ahead into register set (stage mod D).
    Seq ld; ld.init(chunks, p.up, k_done);
    unsigned a_voff[2][4];
    int voff_ey = -1;
    auto set_rows = [&]() {     // pass ey combines input rows (iA, iB): 0: +r0 -r2   1: +r1 +r2   2: -r1 +r2   3: +r1 -r3; past the end: nothing
      const int ey = ld.ey;
      const int iA = (ey == 0) ? 0 : 1, iB = (ey == 3) ? 3 : 2;
      const bool live = !ld.done();
      const bool vA = ((rowmask >> iA) & 1u) && live, vB = ((rowmask >> iB) & 1u) && live;
      // up-sampled row 2ty - 1 + i reads source row ty + (i + 1) / 2 - 1 = ty - 1, ty, ty, ty + 1 (columns likewise)
      const int offA = (p.up ? ((iA + 1) >> 1) - 1 : iA - 1) * (p.up ? p.Wh : p.W) * p.ldx * 4;
      const int offB = (p.up ? ((iB + 1) >> 1) - 1 : iB - 1) * (p.up ? p.Wh : p.W) * p.ldx * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool cv = (colmask >> j) & 1u;
        const int cj = (p.up ? ((j + 1) >> 1) - 1 : j - 1) * p.ldx * 4;
        a_voff[0][j] = (vA && cv) ? a_base + (unsigned)(offA + cj) : OOB;
        a_voff[1][j] = (vB && cv) ? a_base + (unsigned)(offB + cj) : OOB;
      }
      voff_ey = live ? ey : 4;
    };
    int set_ey[D];
    auto issue = [&](int d) {                         // next stage of the sequence -> register set d
      if (voff_ey != (ld.done() ? 4 : ld.ey)) set_rows();
      const int soff = (c_begin + ld.chunk()) << 6;   // 16 floats = 64 bytes per chunk
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (X6_ABL & 1) { dA[d][j] = f32x4{1.f, 2.f, 3.f, (float)soff}; dB[d][j] = f32x4{0.5f, 0.25f, (float)j, 1.f}; continue; }
        dA[d][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)a_voff[0][j], soff, 0));
        dB[d][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)a_voff[1][j], soff, 0));
      }
      set_ey[d] = ld.ey;
      if (!ld.done()) ld.next(chunks);
    };
    auto store = [&](int d, int slot) {
      f32x4 e[4];
      combine(set_ey[d], dA[d], dB[d], e);
      if (FMT) h3_store(e, la + slot * F::A_STAGE, sa);
      else x6_store(e, la + slot * F::A_STAGE);
    };
    const int S_gen = S - t_done;                     // (even, like t_done: slots stay static)
    if (S_gen <= 0) return;
#pragma unroll
    for (int d = 0; d < D; ++d) issue(d);
    __builtin_amdgcn_sched_barrier(0);
    // barrier t separates "A(t) written" from compute(t); A(t) lives in slot t & 1; set t % D is refilled with stage t + D
    constexpr int TRIP = (D & 1) ? 2 * D : D;         // stages per trip: static register sets AND static slots
    for (int t = 0; t < S_gen; t += TRIP) {
#pragma unroll
      for (int k = 0; k < TRIP; ++k) {
        const int d = k % D;
        if (t + k < S_gen) {                          // (uniform; S_gen is even, a multiple of 4 without the up-sampling)
          const bool tl = X6_TL && p.ws && blockIdx.x == 0 && tid == F::CONS * 64 && t_done + t + k < 48;
          unsigned long long* TL = reinterpret_cast<unsigned long long*>(p.ws) + 1024 + (t_done + t + k) * 4;
          if (tl) TL[0] = __builtin_readcyclecounter();
          store(d, k & 1);
          __builtin_amdgcn_sched_barrier(0);
          if (tl) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); TL[1] = __builtin_readcyclecounter(); }
          issue(d);                                   // stages past the end read nothing (all offsets out of range)
          __builtin_amdgcn_sched_barrier(0);
          if (tl) TL[2] = __builtin_readcyclecounter();
          adm_lds_barrier();
          if (tl) TL[3] = __builtin_readcyclecounter();
        }
      }
    }
    return;
  }

  // ================================================================== consumer waves: weight DMA, MFMA, output transform
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(p.w), 0, p.wbytes, 0x00020000);
  const int wm = wid / NB, wn = wid % NB;
  const int lr = lane & 31, lh = lane >> 5;
  if (p.splitk > 1) {
    p.y = p.ws + (long)blockIdx.y * ((long)p.Mt * 4) * p.N;
    p.ldy = p.N; p.bias = nullptr; p.res = nullptr;
    const long sb = (long)p.Mt * 4 * p.N * 4;
    p.ybytes = sb < (1L << 31) ? (int)sb : 0;
  }
  // B loader (LDS-DMA): 24 one-KB instructions per stage = (ex, term) image pt x 32-row half; wave w issues q = 6w .. 6w+5.
  // Lane l of an instruction covers row (q & 1) * 32 + (l >> 1), 16-byte half (l & 1) of the 32-byte row.
  constexpr int QW = F::DMA_PER_WAVE;                 // 6 (bf16) / 4 (fp16) one-KB instructions per wave and stage
  unsigned b_voff[QW];
#pragma unroll
  for (int i = 0; i < QW; ++i) {
    const int q = wid * QW + i, pt = q / NB;          // image (ex, term) and 32-row block q % NB of it
    const int row = (q % NB) * 32 + (lane >> 1);
    const int n = n0 + row;
    const int half = (lane ^ (row >> 3)) & 1;           // logical half stored at physical half (lane & 1)
    b_voff[i] = (n < p.wrows) ? (unsigned)((((long)pt * p.wrows + n) * 16 + half * 8) * 2) : OOB;
  }
  Seq lb; lb.init(chunks, p.up);
  int ld_slot = 0;
  auto issue_b = [&]() {                              // weights of the next stage of the sequence -> next ring slot
    const int kb = ((lb.ey * (p.Cin >> 4) + c_begin + lb.chunk()) * (4 * TERMS) * p.wrows) << 5;   // (ey, chunk) block of twelve [ex][term] images of wrows x 32 bytes
    unsigned short* dst = Bs + ld_slot * F::B_STAGE + (wid * QW) * 512;           // 512 elements = one KB per instruction
    if (!(X6_ABL & 4)) {
#pragma unroll
      for (int i = 0; i < QW; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (x6_lds_void*)(dst + i * 512), 16, (int)b_voff[i], kb, 0, 0);
    }
    lb.next(chunks);
    if (++ld_slot == F::RB) ld_slot = 0;
  };

  f32x16 acc[4];
  f32x16 Y[2][2];                                     // [output row][output column of the pair]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) Y[a][b][r] = 0.f;
  const int a_foff = (wm * 32 + lr) * X6K + ((lh ^ (lr >> 3)) & 1) * 8;   // fragment: row = tile / cout, 8 bf16 = 16 bytes at k = 8 (lane >> 5)
  const int b_foff = (wn * 32 + lr) * X6K + ((lh ^ (lr >> 3)) & 1) * 8;
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  Seq cs; cs.init(chunks, p.up);
  int slot_b = 0;
#pragma unroll
  for (int i = 0; i < F::RB - 1; ++i) issue_b();
  for (int t = 0; t < S; ++t) {
    const bool tl = X6_TL && p.ws && blockIdx.x == 0 && tid == 0 && t < 48;
    unsigned long long* TL = reinterpret_cast<unsigned long long*>(p.ws) + t * 4;
    if (tl) TL[0] = __builtin_readcyclecounter();
    // B(t) was issued three stages ago; B(t+1) and B(t+2) (six instructions each) may still be in flight.  Plain s_barrier +
    // explicit counters: a release fence would drain the weight prefetch (vmcnt(0)).
    if (F::RB == 4 && t + 2 < S) { if (FMT) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory"); else asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
    else if (t + 1 < S) { if (FMT) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory"); else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (tl) TL[1] = __builtin_readcyclecounter();
    if (t + F::RB - 1 < S) issue_b();
    const unsigned short* Ab = As + (t & 1) * F::A_STAGE + a_foff;
    const unsigned short* Bb = Bs + slot_b * F::B_STAGE + b_foff;
    if (++slot_b == F::RB) slot_b = 0;
    const bool first = cs.cc == 0;                    // first stage of a (block, ey) group: C = 0, no accumulator clearing
    // Fragment reads are issued ONE ex GROUP AHEAD of the MFMAs that use them (two register sets): left to itself the compiler
    // reads a group's six fragments right before its six MFMAs, so every group starts with an exposed LDS round trip (~130 cycles,
    // four times per stage) -- a read returns while the matrix pipe works only if it was issued before the chain it follows
    // (tools/overlap_probe2.hip: ds_read_b128 interleaved with MFMAs of the same wave costs ~6 cycles each, not a latency).
    u32x4 fa[NB > 2 ? 1 : 2][TERMS], fb[NB > 2 ? 1 : 2][TERMS];            // 8 bf16 / fp16 values per fragment
    auto frag = [&](int xi, int set) {
#pragma unroll
      for (int k = 0; k < TERMS; ++k) {
        if (X6_ABL & 16) {
          fa[set][k] = u32x4{0x3f803f80u, (unsigned)t, 0x3f803f80u, (unsigned)xi};
          fb[set][k] = u32x4{0x3f003f00u, (unsigned)k, 0x3f003f00u, (unsigned)lane};
          continue;
        }
        fa[set][k] = *reinterpret_cast<const u32x4*>(Ab + (xi * TERMS + k) * X6P_T * X6K);
        fb[set][k] = *reinterpret_cast<const u32x4*>(Bb + (xi * TERMS + k) * F::NT * X6K);
      }
    };
    auto products = [&](auto first_tag) {
      if (NB > 2) {
        // two consumer waves per SIMD; ONE fragment set: a second set (the 64-cout form's read-ahead) and a zero vector for the first
        // stage of a group do not fit next to 64 + 64 accumulator registers in 168 -- written with a read-ahead of the next group
        // (whole, or only of the fragments that are still live) the compiler spills into the loop: 0.80 -> 1.27 ms
#pragma unroll
        for (int xi = 0; xi < 4; ++xi) {
          frag(xi, 0);
          if (X6_ABL & 8) continue;
          const f16x8 a0 = __builtin_bit_cast(f16x8, fa[0][0]), a1 = __builtin_bit_cast(f16x8, fa[0][1]);
          const f16x8 b0 = __builtin_bit_cast(f16x8, fb[0][0]), b1 = __builtin_bit_cast(f16x8, fb[0][1]);
          f32x16 c;
          if (decltype(first_tag)::value) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(c) : "v"(a0), "v"(b1));
          else c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[xi], 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, c, 0, 0, 0);
          acc[xi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, c, 0, 0, 0);
        }
        return;
      }
      frag(0, 0);
#pragma unroll
      for (int xi = 0; xi < 4; ++xi) {
        const int cur = xi & 1;
        if (xi < 3) frag(xi + 1, cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);            // (keeps the next group's reads above this group's chain)
        if (X6_ABL & 8) continue;
        const f32x16 c0 = decltype(first_tag)::value ? zero : acc[xi];
        if (FMT) {                                  // three fp16 products, small ones first
          const f16x8 a0 = __builtin_bit_cast(f16x8, fa[cur][0]), a1 = __builtin_bit_cast(f16x8, fa[cur][1]);
          const f16x8 b0 = __builtin_bit_cast(f16x8, fb[cur][0]), b1 = __builtin_bit_cast(f16x8, fb[cur][1]);
          f32x16 c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, c0, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, c, 0, 0, 0);
          acc[xi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, c, 0, 0, 0);
        } else {                                    // six bf16 products, small ones first
          bf16x8 a[3], b[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) { a[k] = __builtin_bit_cast(bf16x8, fa[cur][k % TERMS]); b[k] = __builtin_bit_cast(bf16x8, fb[cur][k % TERMS]); }
          f32x16 c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c0, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
          acc[xi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (first) products(std::true_type{});            // (wave-uniform)
    else products(std::false_type{});
    if (tl) TL[2] = __builtin_readcyclecounter();
    const int ey = cs.ey;
    const bool last = cs.cc + 1 == cs.len;
    cs.next(chunks);
    if (last) {
      // end of a (block, ey) group: A^T along x (z0 = m0 + m1 + m2, z1 = m1 - m2 - m3), then A^T along y into the output rows
      // (row 0 += Z(ey = 0, 1, 2); row 1 += Z(1) - Z(2) - Z(3)) with f32 adds
      const f32x16 z0 = acc[0] + acc[1] + acc[2], z1 = sub16(sub16(acc[1], acc[2]), acc[3]);
      if (ey <= 2) { Y[0][0] += z0; Y[0][1] += z1; }
      if (ey == 1) { Y[1][0] += z0; Y[1][1] += z1; }
      if (ey >= 2) { Y[1][0] = sub16(Y[1][0], z0); Y[1][1] = sub16(Y[1][1], z1); }
    }
  }

  // ---- epilogue.  C/D layout col = lane&31 (cout), row = (r&3) + 8 (r>>2) + 4 (lane>>5) (tile)
  const int n = n0 + wn * 32 + lr;
  const float bv = (p.bias && n < p.N) ? p.bias[n] : 0.f;
  const int tb = mt0 + wm * 32 + 4 * lh;
  if (p.ybytes > 0) {
    // branch-free: residual loads and output stores through buffer descriptors, masked lanes at an out-of-range offset.  With `if`s
    // per element the compiler serialises the 64 residual loads of a thread, each waiting for the previous one -- tens of
    // microseconds per workgroup.
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res), 0, p.res ? p.rbytes : 0, 0x00020000);
    // One batch of loads, then one batch of stores.  A buffer load is never moved above an earlier buffer store and vmcnt counts
    // stores as well as loads, so a load / wait / store round per accumulator register is sixteen serial memory round trips per
    // wave.  Here: the offsets of pixel (b, 2ty, 2xp) of all sixteen registers (one VGPR each for y and the residual; the 2 x 2
    // outputs of a tile are reached through four uniform scalar offsets), all 64 residual loads into the registers the dead MFMA
    // accumulators leave free, the 64 values, all 64 stores with no wait between them.  Without a residual (the split-K partials
    // too) there is nothing to load and nothing to wait for: a second body, chosen by a workgroup-uniform branch.
    unsigned so_y[2][2], so_r[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        so_y[a][c] = ((unsigned)a * (unsigned)p.W + (unsigned)c) * (unsigned)p.ldy * 4u;
        so_r[a][c] = ((unsigned)a * (unsigned)p.W + (unsigned)c) * (unsigned)p.ldr * 4u;
      }
    auto epilogue = [&](auto res_tag) {
      constexpr bool RES = decltype(res_tag)::value;
      unsigned oy[16], orr[16];
      float v[16][2][2];
      const unsigned cmask = n < p.N ? 0u : OOB;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tb + (r & 3) + 8 * (r >> 2);
        const int xp = t % p.Wh;
        const int u = t / p.Wh;                    // = b * Hh + ty
        const unsigned px0 = ((unsigned)u * 2u) * (unsigned)p.W + 2u * (unsigned)xp;   // pixel (b, 2ty, 2xp): (b*H + 2ty) * W + 2xp
        const unsigned mask = (t < p.Mt ? 0u : OOB) | cmask;                           // masked lanes: an out-of-range offset
        oy[r] = max((px0 * (unsigned)p.ldy + (unsigned)n) * 4u, mask);
        orr[r] = max((px0 * (unsigned)p.ldr + (unsigned)n) * 4u, mask);
      }
      if (RES) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c)
              v[r][a][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_r, (int)orr[r], (int)so_r[a][c], 0));
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 2; ++c)      // (no residual: "+ 0", what a load through an empty descriptor gives; it turns a -0 into +0)
            v[r][a][c] = (FMT ? Y[a][c][r] * inv_scale : Y[a][c][r]) + bv + (RES ? v[r][a][c] : 0.f);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[r][a][c]), rs_y, (int)oy[r], (int)so_y[a][c], 0);
    };
    if (p.res) epilogue(std::true_type{});           // (workgroup-uniform)
    else epilogue(std::false_type{});
    return;
  }
  if (n >= p.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = tb + (r & 3) + 8 * (r >> 2);
    if (t >= p.Mt) continue;
    const int xp = t % p.Wh;
    const int u = t / p.Wh;                        // = b * Hh + ty
    const long px0 = ((long)u * 2) * p.W + 2 * xp; // pixel (b, 2ty, 2xp) in units of pixels: (b*H + 2ty) * W + 2xp
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const long px = px0 + (long)a * p.W;
      float y0 = (FMT ? Y[a][0][r] * inv_scale : Y[a][0][r]) + bv, y1 = (FMT ? Y[a][1][r] * inv_scale : Y[a][1][r]) + bv;
      if (p.res) { y0 += p.res[px * p.ldr + n]; y1 += p.res[(px + 1) * p.ldr + n]; }
      p.y[px * p.ldy + n] = y0;
      p.y[(px + 1) * p.ldy + n] = y1;
    }
  }
}

// Operand layout of the kernel: wino_image_offset (split_format.h), Wq6[ey][chunk][ex][term][n][16] -- the twelve 16-channel images a
// stage needs for its 64 rows are 64 x 32 contiguous bytes each, so one LDS-DMA instruction reads one whole KB (plane-major rows
// would be 32-byte pieces of 32 different 128-byte lines per instruction).
__global__ void split3_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int rows, int cols) {
  const long per = (long)rows * cols, total = per * 16;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int img = (int)(i / per);
    const long rc = i - img * per;
    const int n = (int)(rc / cols), c = (int)(rc - (long)n * cols);
    split3_store(src[i], dst + wino_image_offset(3, img >> 2, img & 3, rows, cols, n, c), split_term_stride(rows));
  }
}

// fp16 format: the two-term split of scale * src; *overflow is raised when a scaled value leaves the fp16 range (the caller then
// falls back to the bf16 format)
__global__ void split2_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int rows, int cols, float scale,
                              int* __restrict__ overflow) {
  const long per = (long)rows * cols, total = per * 16;
  bool bad = false;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int img = (int)(i / per);
    const long rc = i - img * per;
    const int n = (int)(rc / cols), c = (int)(rc - (long)n * cols);
    const float a = src[i] * scale;
    bad |= split_f16_overflow(a);
    split2_store(a, dst + wino_image_offset(2, img >> 2, img & 3, rows, cols, n, c), split_term_stride(rows));
  }
  if (bad && overflow) *overflow = 1;
}

}  // namespace

// dst (bf16 bit patterns, 48 * rows * cols of them, layout [ey][cols/16][ex][term][rows][16]) <- the exact three-term split
// a = a0 + a1 + a2 of the sixteen Winograd planes src[ey * 4 + ex][rows][cols] (f32); cols % 16 == 0
extern "C" int adm_split3_bf16(const float* src, void* dst, int rows, int cols, hipStream_t stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || (cols & 15)) return ADM_EINVAL;
  const long total = (long)rows * cols * 16;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(split3_kernel, dim3(grid), dim3(256), 0, stream, src, static_cast<unsigned short*>(dst), rows, cols);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// fp16 format of the weight operand (see X6Fmt<1>): dst = 32 * rows * cols fp16 values, layout [ey][cols/16][ex][term(2)][rows][16]
extern "C" int adm_split2_f16(const float* src, void* dst, int rows, int cols, float scale, int* overflow, hipStream_t stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || (cols & 15) || !(scale > 0.f)) return ADM_EINVAL;
  const long total = (long)rows * cols * 16;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(split2_kernel, dim3(grid), dim3(256), 0, stream, src, static_cast<unsigned short*>(dst), rows, cols, scale, overflow);
  ADM_CHECK_LAUNCH();
  return ADM_OK;
}

// Same contract as adm_conv_fwd_wino2d, with wq6 = adm_split3_bf16 of the adm_pack_weight_wino2d operand (16 planes of
// wrows x Cin).
static int g_h3_wide = -1;      // -1: chosen per launch, 0: never, 1: whenever the launch qualifies (fp16 format, no split-K)
extern "C" int adm_wino2d_h3_wide(int v) { const int old = g_h3_wide; g_h3_wide = v; return old; }
static int g_row_reuse = 1;     // 1: whole K blocks fetch each patch row once (REUSE = 1 instantiations), 0: two rows per stage everywhere
extern "C" int adm_wino2d_x6_row_reuse(int v) { const int old = g_row_reuse; if (v >= 0) g_row_reuse = v ? 1 : 0; return old; }

// one form of the kernel: both instantiations (row reuse on / off) get their LDS size once, the switch picks one per launch
template <int FMT, int NB> static int x6_launch_form(const X6P& p, unsigned gx, unsigned gy, hipStream_t stream) {
  using F = X6Fmt<FMT, NB>;
  constexpr int smem = (X6_RA * F::A_STAGE + F::RB * F::B_STAGE) * (int)sizeof(unsigned short);
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wino2d_x6_kernel<FMT, NB, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&wino2d_x6_kernel<FMT, NB, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return ADM_ELAUNCH;
    attr_set = true;
  }
  if (g_row_reuse) hipLaunchKernelGGL((wino2d_x6_kernel<FMT, NB, 1>), dim3(gx, gy), dim3(F::THREADS), smem, stream, p);
  else hipLaunchKernelGGL((wino2d_x6_kernel<FMT, NB, 0>), dim3(gx, gy), dim3(F::THREADS), smem, stream, p);
  return ADM_OK;
}

static int wino2d_x6_launch(const float* x, const void* wq6, const float* bias, const float* res, float* y, float* ws, long ws_floats,
                            int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr, int up, hipStream_t stream,
                            const float* amax_x = nullptr, float wscale = 0.f) {
  const bool h3 = amax_x != nullptr;                   // fp16 format: wq6 is the adm_split2_f16 image (scale wscale), amax_x >= max |x| on the device
  if (!x || !wq6 || !y || B <= 0 || H < 2 || W < 2 || (W & 1) || (H & 1)) return ADM_EINVAL;
  if ((Cin & 31) || (ldx & 3) || N <= 0 || wrows < N) return ADM_EINVAL;      // an even number of 16-channel chunks
  if (((uintptr_t)x | (uintptr_t)wq6) & 15) return ADM_EINVAL;
  X6P p;
  p.x = x; p.w = static_cast<const unsigned short*>(wq6); p.bias = bias; p.res = res; p.y = y;
  const long Mt = (long)B * (H / 2) * (W / 2);
  const long xb = (long)B * H * W * ldx * 4 / (up ? 4 : 1), wb = (h3 ? 32L : 48L) * wrows * Cin * 2;
  if (h3 && !(wscale > 0.f)) return ADM_EINVAL;
  if (Mt >= (1L << 30) || xb >= (1L << 31) || wb >= (1L << 31)) return ADM_EINVAL;
  p.Mt = (int)Mt; p.N = N; p.H = H; p.W = W; p.Hh = H / 2; p.Wh = W / 2; p.Cin = Cin; p.ldx = ldx; p.ldy = ldy; p.ldr = ldr;
  p.wrows = wrows; p.xbytes = (int)xb; p.wbytes = (int)wb; p.plane = wrows * Cin; p.up = up ? 1 : 0;
  p.amax_x = amax_x; p.wscale = wscale;
  p.tilesN = adm_cdiv(N, X6N);
  const long mtiles = adm_cdiv(Mt, X6P_T);
  p.splitk = 1; p.chunks_per_split = 0; p.ws = X6_TL ? ws : nullptr;
  const long yb = (long)B * H * W * ldy * 4, rb = res ? (long)B * H * W * ldr * 4 : 0;
  p.ybytes = (yb < (1L << 31) && rb < (1L << 31)) ? (int)yb : 0;
  p.rbytes = (int)rb;
  const int sk = (ws && !(N & 3) && !(ldy & 3) && (!res || !(ldr & 3))) ? adm_wino2d_x6_splitk(B, H, W, Cin, N) : 1;
  if (sk > 1 && ws_floats >= (long)sk * Mt * 4 * N) {
    const int chunks = Cin >> 4;
    p.chunks_per_split = ((chunks + sk - 1) / sk + 1) & ~1;        // the producer double-buffers chunk pairs
    p.splitk = (chunks + p.chunks_per_split - 1) / p.chunks_per_split;
    p.ws = ws;
  }
  // 64, 96 or 128 couts per workgroup (four, six, eight consumer waves).  What a CU fetches per stage bounds all three forms: 32 KB of
  // activations + 16 / 24 / 32 KB of weights, 24 B/clk at the measured stage times against the ~30 B/clk a CU gets out of its L2; one
  // workgroup per CU, so a launch takes (rounds of 256 workgroups) x (bytes per stage) -- the 96 form priced a little above its bytes
  // (its six consumer waves load two SIMDs more than the others).  This model orders every shape of tools/bench_wino2d_x6.cpp
  // correctly (B = 128, ms for 64 / 96 / 128 couts: 32x32 384->384 0.91 / 0.90 / 0.81, 192->192 0.27 / 0.26 / 0.29, 576->192
  // 0.72 / 0.60 / 0.65, 192->576 0.75 / 0.63 / 0.59; 16x16 384->384 0.26 / 0.20 / 0.22; 8x8 384->384 0.083 / 0.100 / 0.108).
  // The table was fitted before the row reuse (16 instead of 32 KB of activations per stage since); it was not re-fitted, and it
  // still orders those shapes correctly (0.84 / 0.78 / 0.68, 0.25 / 0.22 / 0.25, 0.65 / 0.60 / 0.66, 0.67 / 0.61 / 0.58;
  // 0.23 / 0.20 / 0.22; 0.078 / 0.097 / 0.107).
  int form = 2;
  if (h3 && p.splitk == 1 && g_h3_wide != 0 && N > X6N) {
    if (g_h3_wide == 1) form = 4;
    else if (g_h3_wide == 3) form = 3;
    else {
      const long cost[3] = {48, 60, 64};
      long best = -1;
      for (int nb = 2; nb <= 4; ++nb) {
        const long t = (mtiles * adm_cdiv(N, 32 * nb) + 255) / 256 * cost[nb - 2];
        if (best < 0 || t < best) { best = t; form = nb; }
      }
    }
  }
  int rc;
  if (form == 3) {
    p.tilesN = adm_cdiv(N, X6Fmt<1, 3>::NT);
    rc = x6_launch_form<1, 3>(p, (unsigned)(mtiles * p.tilesN), 1, stream);
  } else if (form == 4) {
    p.tilesN = adm_cdiv(N, X6Fmt<1, 4>::NT);
    rc = x6_launch_form<1, 4>(p, (unsigned)(mtiles * p.tilesN), 1, stream);
  } else if (h3) {
    rc = x6_launch_form<1, 2>(p, (unsigned)(mtiles * p.tilesN), (unsigned)p.splitk, stream);
  } else {
    rc = x6_launch_form<0, 2>(p, (unsigned)(mtiles * p.tilesN), (unsigned)p.splitk, stream);
  }
  if (rc != ADM_OK) return rc;
  ADM_CHECK_LAUNCH();
  if (p.splitk > 1) return adm_splitk_reduce(ws, bias, res, y, Mt * 4, N, ldy, ldr, p.splitk, stream);
  return ADM_OK;
}

// fp16 format (three fp16 products per f32 product): wqh = adm_split2_f16(planes, scale = wscale), amax_x = device scalar >= max |x|
// (an upper bound; too large only costs precision on the smallest values); up != 0: the fused nearest x2 form
extern "C" int adm_conv_fwd_wino2d_h3(const float* x, const void* wqh, const float* bias, const float* res, float* y, float* ws,
                                      long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                                      const float* amax_x, float wscale, int up, hipStream_t stream) {
  if (!amax_x) return ADM_EINVAL;
  return wino2d_x6_launch(x, wqh, bias, res, y, ws, ws_floats, B, H, W, Cin, ldx, N, wrows, ldy, ldr, up, stream, amax_x, wscale);
}

extern "C" int adm_conv_fwd_wino2d_x6(const float* x, const void* wq6, const float* bias, const float* res, float* y, float* ws,
                                      long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                                      hipStream_t stream) {
  return wino2d_x6_launch(x, wq6, bias, res, y, ws, ws_floats, B, H, W, Cin, ldx, N, wrows, ldy, ldr, 0, stream);
}

// Conv2d(up=True): the same convolution on the nearest x2 up-sampling of x[B][H/2][W/2][ldx]; H x W is the OUTPUT grid (even)
extern "C" int adm_conv_fwd_wino2d_x6_up(const float* x, const void* wq6, const float* bias, const float* res, float* y, float* ws,
                                         long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                                         hipStream_t stream) {
  return wino2d_x6_launch(x, wq6, bias, res, y, ws, ws_floats, B, H, W, Cin, ldx, N, wrows, ldy, ldr, 1, stream);
}

// Split count over the input channels for launches with fewer workgroups than CUs (one workgroup per CU here)
extern "C" int adm_wino2d_x6_splitk(int B, int H, int W, int Cin, int N) {
  const long wgs = (long)adm_cdiv((long)B * (H / 2) * (W / 2), X6P_T) * adm_cdiv(N, X6N);
  const int chunks = Cin >> 4;
  if (wgs >= 192 || chunks < 8) return 1;
  // one workgroup per CU: the launch takes (rounds of 256 workgroups) x (stages of a split + ~12 stages' worth of prologue and
  // epilogue).  Round 2 took min(768 / wgs, chunks / 4, 6) splits: 48 workgroups x 6 = 288 = a second round for 32 of them.
  int best = 1;
  long best_t = (wgs + 255) / 256 * (4L * chunks + 12);
  for (int s = 2; s <= 6 && s <= chunks / 4; ++s) {
    const int cps = ((chunks + s - 1) / s + 1) & ~1;            // (the producer double-buffers chunk pairs)
    const int splits = (chunks + cps - 1) / cps;
    const long t = (wgs * splits + 255) / 256 * (4L * cps + 12);
    if (t < best_t) { best_t = t; best = s; }
  }
  return best;
}

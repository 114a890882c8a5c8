/* adm_hip.h -- C ABI of libadm_hip.so: the MI355X (gfx950) hot path of DDM's UNet + analytic schedule.
 *
 * The reference (zacz08/ADM, a DDM fork) has no FFI / plugin ABI: its hot path is PyTorch ATen calls
 * made from Python modules.  This header therefore defines the boundary a
 * maintainer binds instead of those ATen calls; each entry point cites the reference lines whose
 * arithmetic it replaces (paths relative to /root/reference).  INTEGRATION.md shows the ctypes
 * binding and the two-line change in the reference's modules.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated; activations are NHWC
 *     ([B][H][W][C], C contiguous; "ld*" = floats between consecutive pixels, >= C)
 *   - no allocation, no synchronisation, no host<->device copies inside any call: work is enqueued on
 *     `stream` (a hipStream_t) and the call returns; graph-capture safe
 *   - return 0 on success, -22 (EINVAL) for a shape/alignment the kernels do not support,
 *     -5 if the launch itself failed.  Nothing falls back to another implementation.
 *   - channel counts seen by the GEMM-shaped kernels are multiples of 32 (the host pads 3 -> 32 for
 *     the stem / heads; packed weights carry the zero padding)
 */
#ifndef ADM_HIP_H
#define ADM_HIP_H
#include <stdint.h>
/* identical to HIP's own typedef, so this header needs no HIP include (C11 allows the repeat) */
typedef struct ihipStream_t* hipStream_t;

#ifdef __cplusplus
/* A BOUND VECTOR (the `amax` arguments below): ADM_AMAX_SLOTS floats at a stride of ADM_AMAX_STRIDE floats (one cache line each), zeroed by
 * the caller; the bound is the maximum of the slots.  The kernels that produce a tensor raise the slots with atomicMax, every wave
 * on its own slot (tens of thousands of waves raising ONE address serialise in the L2: 185 us for a 22 us launch); the kernels that
 * consume the tensor read all slots once per workgroup. */
#define ADM_AMAX_SLOTS 64
#define ADM_AMAX_STRIDE 32
#define ADM_AMAX_FLOATS (ADM_AMAX_SLOTS * ADM_AMAX_STRIDE)

extern "C" {
#endif

int adm_version(void);

/* ---------------- convolution / Linear: fp32-MFMA implicit GEMM ------------------------------ */

/* y[B,H,W,N] = conv_{ks x ks, pad ks/2}(x) + bias (+ res).   Replaces Conv2d.forward
 * (unet/uncond_unet.py:91-113: F.conv2d, the up branch's conv_transpose2d-with-ones == nearest x2
 * when up=1, bias add) and Linear.forward (:62-66, as ks=1,H=W=1).  x is [B,Hin,Win,ldx] with
 * (Hin,Win) = (H,W) or (H/2,W/2) when up.  wp = adm_pack_weight output [wrows][ks*ks*Cin].
 * res (optional) [B*H*W][ldr] is added in the epilogue (the block's residual / skip add, :201, :209).
 * tile: -1 = heuristic, 0..3 force a tile shape (tests). */
int adm_conv_fwd(const float* x, const float* wp, const float* bias, const float* res, float* y,
                 int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                 int ks, int up, int tile, hipStream_t stream);

/* adm_conv_fwd with a stride and explicit top/left zero padding: tap (ky, kx) of output (oy, ox) reads input
 * (oy*stride + ky - pad_lo, ox*stride + kx - pad_lo); anything outside the Hin x Win image is zero (this is the
 * bottom/right padding).  The KL-f4 autoencoder's Downsample -- F.pad(x, (0,1,0,1)) + Conv2d(3x3, stride 2, padding 0),
 * /root/reference/ddm/encoder_decoder.py:78-96 -- is stride 2, pad_lo 0, Hout = Hin/2.  Forward only (the first stage is
 * frozen: /root/reference/ddm/ddm_const_2.py:436-440). */
int adm_conv_fwd_strided(const float* x, const float* wp, const float* bias, const float* res, float* y,
                         int B, int Hin, int Win, int Hout, int Wout, int Cin, int ldx, int N, int wrows,
                         int ldy, int ldr, int ks, int stride, int pad_lo, hipStream_t stream);

/* 3x3 stride-1 conv (forward / data gradient) through a 1-D Winograd F(2,3) transform along x: 1.5x fewer MFMA flops than
 * adm_conv_fwd, same NHWC contract (up = 0, ks = 3), W even, Cin % 16 == 0.  wq = adm_pack_weight_wino's operand
 * [4][wrows][3][Cin] (G g applied at pack time: 1, (g0+g1+g2)/2, (g0-g1+g2)/2, 1).  fp32 throughout; not bit-identical to the
 * direct kernel (different summation), same tolerance.  F.conv2d of Conv2d.forward, uncond_unet.py:98-110. */
int adm_conv_fwd_wino(const float* x, const float* wq, const float* bias, const float* res, float* y, int B, int H, int W,
                      int Cin, int ldx, int N, int wrows, int ldy, int ldr, hipStream_t stream);
/* adm_conv_fwd_wino with the nearest-x2 up-sampling of Conv2d(up=True) fused into the loader: x is [B][H/2][W/2][ldx],
 * H x W is the OUTPUT grid (both even).  uncond_unet.py:98-104. */
int adm_conv_fwd_wino_up(const float* x, const float* wq, const float* bias, const float* res, float* y, int B, int H, int W,
                         int Cin, int ldx, int N, int wrows, int ldy, int ldr, hipStream_t stream);
/* OIHW [Co][Ci][3][3] -> wf [4][Co_pad][3][Ci_pad] (forward) and wb [4][Ci_pad][3][Co_pad] (data gradient: taps flipped,
 * channels transposed); either may be NULL. */
int adm_pack_weight_wino(const float* w, float* wf, float* wb, int Co, int Ci, int Co_pad, int Ci_pad, hipStream_t stream);

/* Deterministic split-K for the small-M layers (4x4 resolution, embedding Linears): adm_conv_splitk(M, N, K) is the
 * number of K slices the library would use (1 = none); adm_conv_fwd_ws is adm_conv_fwd with a workspace of at least
 * splitk*M*N floats: partial tiles are written there and summed (+ bias, + res) in a fixed order by a second launch. */
int adm_conv_splitk(int M, int N, int K);
int adm_conv_fwd_ws(const float* x, const float* wp, const float* bias, const float* res, float* y, float* ws,
                    long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr, int ks,
                    int up, hipStream_t stream);

/* dwp[Cout][ks*ks][Cin] = sum_pixels dy[p][co] * x[p+tap][ci]  (atomic fp32 accumulation over
 * `splits` pixel ranges; dwp is overwritten: the call zero-fills it when it splits).  The weight-gradient of the conv above
 * (autograd of F.conv2d in the reference).  Cout, Cin multiples of 32. */
int adm_conv_wgrad(const float* x, const float* dy, float* dwp, int B, int H, int W, int Cin, int ldx,
                   int Cout, int lddy, int ks, int up, int splits, hipStream_t stream);

/* adm_conv_wgrad that also accumulates the conv's bias gradient, dbias[co] += sum_pixels dy[p][co] (fp32 atomics; the
 * caller zero-fills or passes the gradient buffer to accumulate into): the dy tiles already pass through registers, so
 * no separate reduction pass over dy is needed.  dbias == NULL is adm_conv_wgrad. */
int adm_conv_wgrad_bias(const float* x, const float* dy, float* dwp, float* dbias, int B, int H, int W, int Cin, int ldx,
                        int Cout, int lddy, int ks, int up, int splits, hipStream_t stream);

/* adm_conv_wgrad_bias for 3x3 stride-1 convs through the transposed Winograd form F(3,2) along x (1.5x fewer MFMA flops;
 * fp32; power-of-two H and W >= 2).  Same outputs: dwp[Cout][9][Cin] (zero-filled by the call when it splits) and the
 * optional dbias accumulation.  Autograd of F.conv2d's weight, uncond_unet.py:98-110. */
int adm_conv_wgrad_wino(const float* x, const float* dy, float* dwp, float* dbias, int B, int H, int W, int Cin, int ldx,
                        int Cout, int lddy, int splits, hipStream_t stream);

/* adm_conv_wgrad_wino for Conv2d(up=True): x is the HALF-resolution input [B][H/2][W/2][ldx], H x W is dy's grid. */
int adm_conv_wgrad_wino_up(const float* x, const float* dy, float* dwp, float* dbias, int B, int H, int W, int Cin, int ldx,
                           int Cout, int lddy, int splits, hipStream_t stream);

/* 2-D Winograd F(2x2, 3x3) forward / data gradient (conv_wino2d.hip): 2.25x fewer MFMA flops than adm_conv_fwd, 1.5x fewer
 * than adm_conv_fwd_wino; H and W even, Cin % 16 == 0.  wq = adm_pack_weight_wino2d operand: wf[16][Co_pad][Ci_pad] (forward)
 * or wb[16][Ci_pad][Co_pad] (data gradient, taps flipped), plane index ey * 4 + ex of U = G g G^T. */
int adm_pack_weight_wino2d(const float* w, float* wf, float* wb, int Co, int Ci, int Co_pad, int Ci_pad, hipStream_t stream);
int adm_conv_fwd_wino2d(const float* x, const float* wq, const float* bias, const float* res, float* y, float* ws, long ws_floats,
                        int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr, hipStream_t stream);
/* f32 products on the bf16 MFMA through the exact three-term bf16 split (conv_wino2d_x6.hip): same contract as
 * adm_conv_fwd_wino2d with wq6 = adm_split3_bf16(adm_pack_weight_wino2d operand).
 * Replaces F.conv2d of Conv2d.forward + its data gradient (/root/reference/unet/uncond_unet.py:98-110). */
int adm_conv_fwd_wino2d_x6(const float* x, const void* wq6, const float* bias, const float* res, float* y, float* ws,
                           long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                           hipStream_t stream);
/* ... on the nearest x2 up-sampling of x[B][H/2][W/2][ldx] (Conv2d(up=True), uncond_unet.py:105-108); H x W = the output grid */
int adm_conv_fwd_wino2d_x6_up(const float* x, const void* wq6, const float* bias, const float* res, float* y, float* ws,
                              long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                              hipStream_t stream);
int adm_wino2d_x6_splitk(int B, int H, int W, int Cin, int N);
/* The same convolution on THREE fp16 products per f32 product (conv_wino2d_x6.hip, X6Fmt<1>): operands are split into two fp16 terms
 * by round-to-nearest after a power-of-two scaling, s a = h0 + h1 with |s a - h0 - h1| <= 2^-24 |s a| (h1 normal), and
 * a b ~ (h0 h0' + h0 h1' + h1 h0') / (s s').  wqh = adm_split2_f16 of the adm_pack_weight_wino2d planes with scale `wscale` (a power
 * of two; *overflow is raised if a scaled weight leaves the fp16 range), layout [ey][cols/16][ex][term(2)][rows][16].  amax_x: a bound
 * vector (above) of |x| over the whole input (e.g. written by adm_gn_fwd_amax, which produced x); the kernel derives the activation scale
 * from it so that the Winograd input transform (sums of four values) stays inside the fp16 range.  Error against fp64: that of the
 * six-bf16-product form (tools/fp16x3_accuracy.py, tests/test_hip_ops.py).  up != 0: Conv2d(up=True) as adm_conv_fwd_wino2d_x6_up.
 * Replaces F.conv2d of uncond_unet.py:98-110 like the other forms. */
int adm_split2_f16(const float* src, void* dst, int rows, int cols, float scale, int* overflow, hipStream_t stream);
int adm_conv_fwd_wino2d_h3(const float* x, const void* wqh, const float* bias, const float* res, float* y, float* ws,
                           long ws_floats, int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr,
                           const float* amax_x, float wscale, int up, hipStream_t stream);
/* dst (48 * rows * cols bf16, layout [ey][cols/16][ex][term][rows][16]) <- exact split a = a0 + a1 + a2 of the sixteen Winograd
 * planes src[ey * 4 + ex][rows][cols] (f32) */
int adm_split3_bf16(const float* src, void* dst, int rows, int cols, hipStream_t stream);
/* 1x1 conv / pixel-wise linear map with the f32 products on the bf16 MFMA by exact three-term splitting (conv_gemm_x6.hip):
 * y[M][ldy] = x[M][ldx] (K channels) . w^T (+ bias) (+ res), w6 = adm_split3_rows of the packed operand [wrows >= N][K] (f32, row
 * stride ld) = [K/16][3][wrows][16] bf16.  K % 32 == 0.  Replaces F.conv2d (1x1) + its data gradient (uncond_unet.py:98-110). */
int adm_gemm_x6(const float* x, const void* w6, const float* bias, const float* res, float* y, long M, int K, int ldx, int N, int wrows,
                int ldy, int ldr, hipStream_t stream);
int adm_split3_rows(const float* src, void* dst, int rows, int cols, int ld, hipStream_t stream);
/* adm_gemm_x6 that also raises the bound vector amax_y (above) to max |y| */
int adm_gemm_x6_amax(const float* x, const void* w6, const float* bias, const float* res, float* y, long M, int K, int ldx, int N,
                     int wrows, int ldy, int ldr, float* amax_y, hipStream_t stream);
/* ... on the fp16 format (two fp16 terms per operand, three MFMAs per f32 product, as adm_conv_fwd_wino2d_h3): wh = adm_split2_rows_f16 of
 * the packed operand = [K/16][2][wrows][16] fp16 of wscale * w (*overflow raised if a scaled weight leaves the fp16 range), amax_x = bound
 * vector of |x|, amax_y (may be NULL) = bound vector raised to max |y|.  Same replacement (uncond_unet.py:98-110). */
int adm_gemm_x6_h3(const float* x, const void* wh, const float* bias, const float* res, float* y, long M, int K, int ldx, int N, int wrows,
                   int ldy, int ldr, const float* amax_x, float wscale, float* amax_y, hipStream_t stream);
int adm_split2_rows_f16(const float* src, void* dst, int rows, int cols, int ld, float scale, int* overflow, hipStream_t stream);
/* The 2-D Winograd weight gradient with the f32 products on the bf16 MFMA by exact three-term splitting (conv_wgrad_x6.hip): same
 * contract as adm_conv_wgrad_wino2d (dwp2[Cout][4 ey][3 kx][Cin] -> adm_unpack_wgrad_wino2d; dbias += column sums of dy; splits = 0:
 * chosen by the launcher; H, W powers of two >= 2).  _ws: deterministic mode, split z stores its partial planes at ws[z][Cout][12][Cin]
 * and its bias partial at bws[z][Cout]; splits must be adm_conv_wgrad_x6_plan(...).
 * Replaces the autograd weight gradient of Conv2d.forward (/root/reference/unet/uncond_unet.py:98-110). */
int adm_conv_wgrad_x6(const float* x, const float* dy, float* dwp2, float* dbias, int B, int H, int W, int Cin, int ldx, int Cout,
                      int lddy, int splits, hipStream_t stream);
/* _up: weight gradient of Conv2d(up=True): x is the conv's half-resolution input [B][H/2][W/2][ldx], H x W is dy's grid */
int adm_conv_wgrad_x6_up(const float* x, const float* dy, float* dwp2, float* dbias, int B, int H, int W, int Cin, int ldx, int Cout,
                         int lddy, int splits, hipStream_t stream);
int adm_conv_wgrad_x6_ws(const float* x, const float* dy, float* ws, float* bws, int B, int H, int W, int Cin, int ldx, int Cout,
                         int lddy, int splits, int up, hipStream_t stream);
int adm_conv_wgrad_x6_plan(int B, int H, int W, int Cin, int Cout);
/* Weight gradient of a 1x1 conv on the same kernel (conv_wgrad_x6.hip, MODE 1): dwp[Cout][Cin] (+)= sum over P pixels of
 * dy[p][co] x[p][ci] (-> adm_unpack_wgrad with ks = 1), dbias += column sums of dy; _ws / _plan as for adm_conv_wgrad_x6. */
int adm_gemm_wgrad_x6(const float* x, const float* dy, float* dwp, float* dbias, long P, int Cin, int ldx, int Cout, int lddy,
                      int splits, hipStream_t stream);
int adm_gemm_wgrad_x6_ws(const float* x, const float* dy, float* ws, float* bws, long P, int Cin, int ldx, int Cout, int lddy,
                         int splits, hipStream_t stream);
int adm_gemm_wgrad_x6_plan(long P, int Cin, int Cout);
/* The same two weight gradients with x stored as bf16 (the opt-in bf16 mode's GroupNorm outputs, adm_gn_fwd_bf16out): x16 =
 * [B][H][W][ldx] bf16 ([B][H/2][W/2][ldx] when up); products exact in x, three-term exact in dy, f32 accumulate. */
int adm_conv_wgrad_x6_bf16a(const void* x16, const float* dy, float* dwp2, float* dbias, int B, int H, int W, int Cin, int ldx,
                            int Cout, int lddy, int splits, int up, hipStream_t stream);
int adm_gemm_wgrad_x6_bf16a(const void* x16, const float* dy, float* dwp, float* dbias, long P, int Cin, int ldx, int Cout, int lddy,
                            int splits, hipStream_t stream);
/* ... and on the fp16 format of adm_conv_fwd_wino2d_h3 (two fp16 terms per operand, three products): amax_x / amax_dy = bound vectors
 * (above) of |x| / |dy|, written by the kernels that produced the tensors; det != 0 = the _ws contract (dwp = ws, dbias = bws,
 * splits from the _plan call).  Replaces the same autograd weight gradient (/root/reference/unet/uncond_unet.py:98-110). */
int adm_conv_wgrad_x6_h3(const float* x, const float* dy, float* dwp2, float* dbias, int B, int H, int W, int Cin, int ldx, int Cout,
                         int lddy, int splits, int up, int det, const float* amax_x, const float* amax_dy, hipStream_t stream);
int adm_gemm_wgrad_x6_h3(const float* x, const float* dy, float* dwp, float* dbias, long P, int Cin, int ldx, int Cout, int lddy,
                         int splits, int det, const float* amax_x, const float* amax_dy, hipStream_t stream);
/* the split count adm_conv_wgrad_x6_h3 takes for splits <= 0 and det == 0: where its 128-cout workgroups qualify, the minimum of a time
 * model (rounds of 256 workgroups x (stages of a split + the atomic epilogue)) where that beats the fill rule of adm_conv_wgrad_x6_plan
 * by more than 5 %, else the fill rule's count; >= 6 stages of 16 tiles per split, <= 64 */
int adm_conv_wgrad_x6_h3_plan(int B, int H, int W, int Cin, int Cout);
/* kernel variant of adm_conv_fwd_wino2d: -1 (default) chosen per launch, 1 wave-specialised (producer / consumer waves), 0 symmetric;
 * returns the old value */
int adm_wino2d_variant(int ws);
/* form of adm_conv_fwd_wino2d_h3's kernel: -1 (default) chosen per launch, 1 the 128-cout workgroups (eight consumer waves) / 3 the 96-cout
 * workgroups (six) wherever the launch qualifies (no split-K), 0 always 64-cout workgroups; returns the old value */
int adm_wino2d_h3_wide(int v);
/* producer of adm_conv_fwd_wino2d_x6 / _h3's kernel: 1 (default) whole K blocks fetch each of the four patch rows of a tile and
 * 16-channel chunk once and keep it in registers across the four ey passes, 0 every pass fetches its two rows (eight row loads per
 * chunk).  Both settings run the same arithmetic in the same order: outputs are bit-identical.  Returns the old value; a negative v
 * only queries. */
int adm_wino2d_x6_row_reuse(int v);
/* form of adm_conv_wgrad_x6_h3 / adm_gemm_wgrad_x6_h3's kernel: -1 (default) / 2: 128 couts per workgroup (sixteen waves) where the launch
 * qualifies (more than 64 couts, not the deterministic workspace mode), 1: always 64; returns the old value */
int adm_wgrad_h3_blocks(int v);
/* split count (>= 1) adm_conv_fwd_wino2d uses when given a workspace of that many B*H*W*N-float slices (small maps) */
int adm_wino2d_splitk(int B, int H, int W, int Cin, int N);

/* 2-D Winograd F(3x3, 2x2) weight gradient (conv_wgrad_wino.hip, MODE 2): 1.5x fewer MFMA flops than adm_conv_wgrad_wino.  H, W
 * powers of two, H >= 2.  dwp2[Cout][4 ey][3 kx][Cin] holds the x-folded transform planes; adm_unpack_wgrad_wino2d applies the
 * y half of G^T while scattering to OIHW (splits = 1, bws = dbias = NULL for the atomic path; the workspace form of
 * adm_conv_wgrad_ws(wino = 2) otherwise). */
int adm_conv_wgrad_wino2d(const float* x, const float* dy, float* dwp2, float* dbias, int B, int H, int W, int Cin, int ldx,
                          int Cout, int lddy, int splits, hipStream_t stream);
int adm_unpack_wgrad_wino2d(const float* wx, int splits, float* dw, int Co, int Ci, int Co_pad, int Ci_pad, int accumulate,
                            const float* bws, float* dbias, hipStream_t stream);

/* Deterministic weight gradients (bitwise reproducible backward; SURVEY.md section 5.2 "run twice, bit-compare").  The
 * kernels above combine their pixel-range splits with fp32 atomics.  Here split z writes its partial tile with plain stores
 * to ws[z][Cout][ks*ks][Cin] (and its bias partial to bws[z][Cout], bws may be NULL) and adm_unpack_wgrad_splits sums the
 * splits in a fixed order.  adm_conv_wgrad_plan returns the split count the launcher picks (>= 1) for the direct
 * (wino = 0), Winograd F(3,2) (wino = 1: ks = 3, power-of-two H and W) or 2-D F(3x3,2x2) (wino = 2; ws planes are then
 * [Cout][12][Cin], see adm_conv_wgrad_wino2d) kernel; pass it as `splits`. */
int adm_conv_wgrad_plan(int B, int H, int W, int Cin, int Cout, int ks, int up, int wino);
int adm_conv_wgrad_ws(const float* x, const float* dy, float* ws, float* bws, int B, int H, int W, int Cin, int ldx, int Cout,
                      int lddy, int ks, int up, int splits, int wino, hipStream_t stream);

/* ---- reduced-precision option (BASELINE.json configs[2], "bf16"): same contracts as adm_conv_fwd / adm_conv_wgrad,
 * tensors stay fp32 in HBM, the contraction runs on v_mfma_f32_32x32x16_bf16 (operands rounded to bf16 on their way
 * into LDS, fp32 accumulation).  wp16 = the adm_pack_weight layouts converted with adm_f32_to_bf16.  Cin % 64 == 0
 * for adm_conv_fwd_bf16.  Never selected implicitly: the host opts in (adm_amd.ops.set_compute_precision). */
int adm_conv_fwd_bf16(const float* x, const unsigned short* wp16, const float* bias, const float* res, float* y,
                      int B, int H, int W, int Cin, int ldx, int N, int wrows, int ldy, int ldr, int ks, int up,
                      int tile, hipStream_t stream);
int adm_conv_wgrad_bf16(const float* x, const float* dy, float* dwp, int B, int H, int W, int Cin, int ldx, int Cout,
                        int lddy, int ks, int up, int splits, hipStream_t stream);
/* bf16-STORAGE variants (BASELINE configs[2]): the activation operand is already bf16 in HBM (written by adm_gn_fwd_bf16out), so
 * the kernels read half the bytes and skip the conversion; results are bit-identical to the f32-activation entry points above. */
int adm_conv_fwd_bf16a(const void* x16, const unsigned short* wp16, const float* bias, const float* res, float* y, int B, int H, int W,
                       int Cin, int ldx, int N, int wrows, int ldy, int ldr, int ks, int up, int tile, hipStream_t stream);
int adm_conv_wgrad_bf16a(const void* x16, const float* dy, float* dwp, int B, int H, int W, int Cin, int ldx, int Cout, int lddy, int ks,
                         int up, int splits, hipStream_t stream);
/* adm_gn_fwd with y stored as bf16 (round to nearest even): y16[B][HW][C] */
int adm_gn_fwd_bf16out(const float* x, float* stats, double* ws, const float* gamma, const float* beta, const float* ss,
                       long ss_bstride, void* y16, int B, int HW, int C, int G, float eps, int silu, float drop_p, uint64_t seed,
                       hipStream_t stream);
int adm_f32_to_bf16(const float* src, unsigned short* dst, long n, hipStream_t stream);
/* Host queries of the two launch plans above (no launch; the launchers call the same functions).  adm_conv_bf16_tile: the form
 * adm_conv_fwd_bf16 / _bf16a take with tile = -1 at M = B*H*W output pixels and N couts: 0 = 128x128, 1 = 128x96, 2 = 64x64.
 * adm_conv_wgrad_bf16_plan: out = {TM, TN, splits, chunk} of adm_conv_wgrad_bf16 / _bf16a at P = B*H*W pixels: the cout x cin tile,
 * the number of pixel ranges after rounding (> 1: fp32 atomics) and the pixels per range (a multiple of 64); `splits` as passed to
 * the launcher (<= 0: chosen by it). */
int adm_conv_bf16_tile(long M, int N);
int adm_conv_wgrad_bf16_plan(long P, int Cin, int Cout, int ks, int splits, int* out);

/* OIHW [Co][Ci][ks][ks] (the reference's parameter layout, uncond_unet.py:85) ->
 *   wp_fwd [Co_pad][ks*ks][Ci_pad]            (B operand of adm_conv_fwd)
 *   wp_bwd [Ci_pad][ks*ks flipped][Co_pad]    (B operand of adm_conv_fwd computing dL/dx)
 * zero padded.  qkv != 0: rows are permuted from the reference's (head, c, {q,k,v}) interleave
 * (uncond_unet.py:205) to (head, {q,k,v}, c) so q/k/v are contiguous 64-float runs.
 * Either output may be NULL. */
int adm_pack_weight(const float* w, float* wp_fwd, float* wp_bwd, int Co, int Ci, int ks, int Co_pad, int Ci_pad,
                    int qkv, hipStream_t stream);
/* adm_pack_weight (+ adm_pack_weight_wino) for every layer of a model in ONE launch (used after each optimiser step).
 * table = device array of n_entries rows of 24 int64 (the PT_* names of csrc/pack_weights.hip and adm_amd/ops.py):
 *    0 src          the OIHW / [out, in] parameter
 *    1 fwd          wp_fwd of adm_pack_weight; 0 when unused
 *    2 bwd          wp_bwd of adm_pack_weight; 0 when unused
 *    3 Co, 4 Ci, 5 taps = ks*ks, 6 Co_pad, 7 Ci_pad, 8 qkv   as adm_pack_weight
 *    9 tile_begin   exclusive prefix sum of (Co_pad/32)*(Ci_pad/32) in row order; total_tiles = the sum over all rows
 *   10 wf, 11 wb    1-D Winograd operands of adm_pack_weight_wino (forward, data gradient)
 *   12 w2f, 13 w2b  f32 2-D Winograd planes of adm_pack_weight_wino2d
 *   14 w2f6, 15 w2b6   their three-term bf16 splits, as adm_split3_bf16
 *   16 g6f, 17 g6b  three-term bf16 splits of the 1x1 operands fwd / bwd, as adm_split3_rows
 *   18 w2fh, 19 w2bh   two-term fp16 images of scale * (2-D Winograd planes), as adm_split2_f16
 *   20 h3_scale     that scale (a power of two; the formats: adm_amd/csrc/split_format.h): the bits of a float in the low 32 bits
 *   21 h3_flag      int* raised to 1 when a scaled weight of columns 18, 19, 22, 23 leaves the fp16 range; 0 = none
 *   22 g6fh, 23 g6bh   two-term fp16 images of scale * (1x1 operands), as adm_split2_rows_f16
 * Columns 1, 2, 10-19, 22 and 23 are destinations and may be 0, each on its own (not derived: nothing is written for it, the
 * others are); 10-15, 18 and 19 are read for 3x3 layers only, 16, 17, 22 and 23 for 1x1 layers only.  The 16-bit images (14-19, 22,
 * 23) are written with 8-byte stores and must be 8-byte aligned. */
int adm_pack_weight_table(const long* table, int n_entries, long total_tiles, hipStream_t stream);
/* inverse of the fwd packing for gradients: dw OIHW = (accumulate ? dw : 0) + dwp */
int adm_unpack_wgrad(const float* dwp, float* dw, int Co, int Ci, int ks, int Co_pad, int Ci_pad, int qkv,
                     int accumulate, hipStream_t stream);
/* adm_unpack_wgrad over the `splits` partial gradients of adm_conv_wgrad_ws, summed in split order; bias partials
 * bws[splits][Co_pad] are summed into dbias[0..Co_pad) (+=, packed channel order); bws and dbias may both be NULL. */
int adm_unpack_wgrad_splits(const float* ws, int splits, float* dw, int Co, int Ci, int ks, int Co_pad, int Ci_pad, int qkv,
                            int accumulate, const float* bws, float* dbias, hipStream_t stream);
/* adm_unpack_wgrad / adm_unpack_wgrad_wino2d (splits = 1) for the weight gradients of ALL layers in ONE launch, issued once at the
 * end of the backward pass.  table = device array of `rows` rows of 12 int64: {src, dst, Co, Ci, taps, Ci_pad, qkv, accumulate,
 * zero_src, block_begin, 0, 0}; taps = ks*ks for the plain packed layout [Co_pad][taps][Ci_pad], 0 for the 2-D Winograd planes
 * [Co_pad][4 ey][3 kx][Ci_pad]; a row owns ceil(items / 2048) blocks (items = Co*Ci*taps, or Co*Ci*3), block_begin = exclusive
 * prefix sum, total_blocks = the sum.  zero_src != 0 clears every workspace element after reading it: with workspaces that are zero
 * at rest the weight-gradient entry points take splits = -1 ("chosen by the launcher, workspace already zero") and enqueue no memset. */
int adm_unpack_wgrad_table(const long* table, int rows, long total_blocks, hipStream_t stream);
/* out[i] = in[perm(i)] over n_pad entries (zero beyond n); qkv permutation of bias vectors.
 * inverse=1 maps packed order back to the reference order. */
int adm_permute_vec(const float* in, float* out, int n, int n_pad, int qkv, int inverse, hipStream_t stream);
/* out[n] (+)= sum_m a[m][n]: bias gradients. */
int adm_colsum(const float* a, float* out, int M, int N, int ld, int accumulate, hipStream_t stream);

/* ---------------- GroupNorm (+ adaptive scale/shift) + SiLU (+ dropout) ----------------------- */

/* stats[b][g] = {mean, rstd} of x[b, :, g*cpg:(g+1)*cpg]; ws: scratch of B*splits*G*2 doubles
 * (splits = adm_gn_splits(HW, C)).  F.group_norm's moments (uncond_unet.py:128). */
/* 1 (default): one-launch register-resident GroupNorm where a plan exists; 0: always the multi-pass kernels.  Returns the old value. */
int adm_gn_fused(int on);
int adm_gn_splits(int HW, int C);
/* The launch plan of adm_gn_fwd / adm_gn_bwd at (HW, C, G) under the current adm_gn_fused switch, no launch:
 * out[0..4] = {Cc, threads, rows, MAXR, S}.  One-launch path: slab width in channels, workgroup size, rows per thread, the
 * register-resident template taken (2 / 8 / 14), S = 1.  Multi-pass path: Cc = 0, threads per workgroup, rows per split, MAXR = 0,
 * S = adm_gn_splits(HW, C).  ADM_EINVAL for a shape the kernels refuse. */
int adm_gn_plan(int HW, int C, int G, int* out);
int adm_gn_stats(const float* x, float* stats, double* ws, int B, int HW, int C, int G, float eps, hipStream_t stream);
/* y = act( (xhat*gamma + beta) * (1 + scale[b,c]) + shift[b,c] ) * dropmask
 * xhat = (x - mean) * rstd.  ss = [.., 2C] rows of (scale | shift) or NULL (uncond_unet.py:191-196);
 * ss_bstride = floats between batch rows (0 = broadcast one row: sampling runs the embedding at batch 1).
 * silu: apply SiLU.  drop_p > 0: inverted dropout with the stateless mask (seed, element index)
 * (uncond_unet.py:200). */
int adm_gn_apply(const float* x, const float* stats, const float* gamma, const float* beta, const float* ss,
                 long ss_bstride, float* y, int B, int HW, int C, int G, int silu, float drop_p, uint64_t seed,
                 hipStream_t stream);
/* adm_gn_stats + adm_gn_apply in one call (same arguments); feature maps of HW <= 256 pixels run as ONE launch that keeps
 * its slab in registers between the reduction and the apply pass (x is read once).  stats is written either way. */
int adm_gn_fwd(const float* x, float* stats, double* ws, const float* gamma, const float* beta, const float* ss,
               long ss_bstride, float* y, int B, int HW, int C, int G, float eps, int silu, float drop_p, uint64_t seed,
               hipStream_t stream);
/* adm_gn_fwd that also raises the bound vector amax (above; zeroed by the caller) to max |y| with one atomicMax per wave: the scale basis
 * of the fp16-format convolution that consumes y (adm_conv_fwd_wino2d_h3). */
int adm_gn_fwd_amax(const float* x, float* stats, double* ws, const float* gamma, const float* beta, const float* ss,
                    long ss_bstride, float* y, float* amax, int B, int HW, int C, int G, float eps, int silu, float drop_p,
                    uint64_t seed, hipStream_t stream);
/* Backward of adm_gn_apply.  Pass 1 reduces per (b,c): r1 = sum du, r2 = sum du*xhat into red[B][C][2]
 * (du = dy * mask * act'(u)); pass 2 writes dx and, when the pointers are non-NULL, dss[B][2C]
 * (d scale | d shift; row stride = ss_bstride when that is non-zero: ss and dss may be column slices of one wide buffer),
 * dgamma[C], dbeta[C] (accumulated: caller zero-fills dgamma/dbeta). */
int adm_gn_bwd(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta,
               const float* ss, long ss_bstride, float* dx, float* dss, float* dgamma, float* dbeta, float* red,
               int B, int HW, int C, int G, int silu, float drop_p, uint64_t seed, hipStream_t stream);

/* The batch reduction of dgamma / dbeta for EVERY GroupNorm layer of a backward pass in one launch: adm_gn_bwd / adm_gn_bwd_add
 * called with dgamma = dbeta = NULL leave the per-image sums tot[B][C][2] at red + B*S*C*2 floats (S = adm_gn_splits(HW, C)); the
 * caller keeps `red` (and ss) alive and queues a row.  table = device array of `rows` rows of 8 int64: {tot, ss (0: none),
 * ss_bstride, dgamma, dbeta, B, C, block_begin}; a row owns ceil(C / 32) blocks, block_begin = exclusive prefix sum, total_blocks =
 * the sum.  dgamma[c] += sum_b (1 + scale[b][c]) tot[b][c][1], dbeta[c] += ... tot[b][c][0]: the same order as the per-layer pass. */
int adm_gn_bwd_param_table(const long* table, int rows, long total_blocks, hipStream_t stream);

/* adm_gn_bwd with dx = (GroupNorm input gradient) + addend[B][HW][C] (addend may be NULL): the block input also feeds the
 * residual branch (uncond_unet.py:189, 201), and adding that branch's gradient here saves autograd's separate
 * read-read-write pass over the activation. */
int adm_gn_bwd_add(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta,
                   const float* ss, long ss_bstride, const float* addend, float* dx, float* dss, float* dgamma, float* dbeta,
                   float* red, int B, int HW, int C, int G, int silu, float drop_p, uint64_t seed, hipStream_t stream);
/* ... that also raises the bound vector amax (zeroed by the caller) to max |dx|: the data-gradient convolution that consumes dx
 * can then run on the fp16 format (adm_conv_fwd_wino2d_h3 with the data-gradient weight image). */
int adm_gn_bwd_add_amax(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta,
                        const float* ss, long ss_bstride, const float* addend, float* dx, float* dss, float* dgamma, float* dbeta,
                        float* red, float* amax, int B, int HW, int C, int G, int silu, float drop_p, uint64_t seed,
                        hipStream_t stream);
/* The concat forms, for a block whose input is z = (a | scale_b * b) along the channels (adm_concat2: a[M][Ca], b[M][Cb], M = B HW,
 * Ca and Cb multiples of 4, C = Ca + Cb): the GroupNorm kernels sit on both sides of that copy and pick a source / destination per thread.
 * adm_gn_fwd_cat_amax = adm_concat2(a, b -> z, amax_z) + adm_gn_fwd_amax(z -> y, amax) without the copy pass: the moments pass (the one
 * launch of a small map) reads a and b in place of z and writes z and its bound.  adm_gn_bwd_add_cat_amax = adm_gn_bwd_add_amax(x = z ->
 * dz, amax) + adm_split2(dz -> da, db) without dz: the dx pass stores da = dz[:, :Ca] and db = scale_b * dz[:, Ca:]; amax bounds |dz|
 * (so |da|, and |db| when |scale_b| <= 1).  amax_z and amax may be NULL.  Results are bit-identical to the two-call forms. */
int adm_gn_fwd_cat_amax(const float* a, int Ca, const float* b, int Cb, float scale_b, float* z, float* amax_z, float* stats, double* ws,
                        const float* gamma, const float* beta, const float* ss, long ss_bstride, float* y, float* amax, int B, int HW,
                        int G, float eps, int silu, float drop_p, uint64_t seed, hipStream_t stream);
int adm_gn_bwd_add_cat_amax(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta, const float* ss,
                            long ss_bstride, const float* addend, float* da, int Ca, float* db, int Cb, float scale_b, float* dss,
                            float* dgamma, float* dbeta, float* red, float* amax, int B, int HW, int G, int silu, float drop_p,
                            uint64_t seed, hipStream_t stream);

/* ---------------- KL autoencoder (first stage) helpers ---------------------------------------- */

/* In-place s[r][0:cols] = softmax(scale * s[r][0:cols]) for `rows` rows of stride ld: the single-head
 * (d = C = 512) attention of the autoencoder's mid block, whose QK^T and PV products run on adm_conv_fwd
 * (/root/reference/ddm/encoder_decoder.py:190-213).  cols % 4 == 0, cols <= 8192. */
int adm_softmax_rows(float* s, long rows, int cols, long ld, float scale, hipStream_t stream);
/* z[m][c] = zscale * (mean + exp(0.5*clamp(logvar,-30,20)) * eps[m*C+c]); moments rows = (mean[0:C] | logvar[C:2C]);
 * eps == NULL gives the mode.  DiagonalGaussianDistribution.sample (/root/reference/ddm/encoder_decoder.py:855-867). */
int adm_posterior_sample(const float* moments, int ldm, const float* eps, float* z, int ldz, long M, int C,
                         float zscale, hipStream_t stream);

/* ---------------- self-attention core -------------------------------------------------------- */

/* qkv [B][L][heads*192] packed (head, {q,k,v}, 64); out [B][L][heads*64].
 * out = softmax_k(q.k / 8) v per (b, head): uncond_unet.py:205-208.  L <= 32 or a multiple of 32; sequences beyond
 * 256 (L = 1024 at the 32x32 level of the 64x64-latent configs) run in 256-row chunks with an online softmax. */
int adm_attn_fwd(const float* qkv, float* out, float* lse, int B, int L, int heads, hipStream_t stream);
/* lse [B*heads][L] = log-sum-exp per query saved by the forward (may be NULL there when no backward
 * follows); delta [B*heads][L] scratch.  dqkv has the qkv layout.  Autograd of :205-208. */
int adm_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta,
                 int B, int L, int heads, hipStream_t stream);
/* adm_attn_fwd with both matrix products on the fp16 split format (attention_h3.hip: three fp16 MFMAs per f32 product, as
 * adm_conv_fwd_wino2d_h3): amax = bound vector of |qkv|; L in {32, 64, 128, 256} or a multiple of 256 (ADM_EINVAL otherwise).  Same replacement (:205-208). */
int adm_attn_fwd_h3(const float* qkv, float* out, float* lse, const float* amax, int B, int L, int heads, hipStream_t stream);
/* adm_attn_bwd on the same format: amax_qkv / amax_dout = bound vectors of |qkv| and |dout|, amax_dqkv (may be NULL) = bound vector
 * raised to max |dqkv|; L as above.  Autograd of :205-208. */
int adm_attn_bwd_h3(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta,
                    const float* amax_qkv, const float* amax_dout, float* amax_dqkv, int B, int L, int heads, hipStream_t stream);
/* ... that also raises the bound vector amax to max |dqkv| (the qkv conv's gradients then run on the fp16 format) */
int adm_attn_bwd_amax(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta, float* amax,
                      int B, int L, int heads, hipStream_t stream);
/* Host query of the form a sequence length runs on (no launch; the entry points above choose their kernel through the same
 * function).  family 0 = adm_attn_fwd / adm_attn_bwd / adm_attn_bwd_amax, 1 = adm_attn_fwd_h3, 2 = adm_attn_bwd_h3.  out[0] = waves
 * per workgroup (32 queries or keys each), out[1] = rows of the other side per LDS fill, out[2] = grid.y (workgroups per (b, head)),
 * out[3] = 1 for the chunked form (L > 256: a workgroup owns one of grid.y 256-row chunks and passes all chunks of the other side
 * through LDS), else 0.  ADM_EINVAL for an L the family refuses. */
int adm_attn_form(int family, int L, int* out);

/* ---------------- resampling / layout / elementwise ------------------------------------------ */

/* mode 0: y[B,H/2,W/2,C] = scale * sum_{2x2} x   (down: scale .25, uncond_unet.py:107-108;
 *         also the backward of up with scale 1)
 * mode 1: y[B,2H,2W,C]   = scale * x[y/2,x/2]    (up: uncond_unet.py:105-106; backward of down with .25)
 * acc != 0: y += ... */
int adm_resample2x(const float* x, float* y, int B, int H, int W, int C, int mode, float scale, int acc,
                   hipStream_t stream);
/* y[B,H,W,Cpad] = mul[b] * x_nchw (channels >= C zero); x is fp32 or fp64 (x_is_f64).
 * EDMPrecond's `c_in * x` + .to(float32) (uncond_unet.py:616, 628) fused with NCHW->NHWC. */
int adm_nchw_to_nhwc(const void* x, int x_is_f64, const float* mul, long mul_bstride, float* y, int B, int C, int HW,
                     int Cpad, hipStream_t stream);
/* ... that also raises the bound vector amax to max |y| (the stem conv then runs on the fp16 format) */
int adm_nchw_to_nhwc_amax(const void* x, int x_is_f64, const float* mul, long mul_bstride, float* y, float* amax, int B, int C, int HW,
                          int Cpad, hipStream_t stream);
/* out_nchw[b,c,p] = a[b] * x_nchw[b,c,p] + s[b] * f_nhwc[b,p,c]   (D = c_skip x + c_out F, :631-632).
 * x == NULL (then a may be NULL): out = s[b] * f -- the adjoint of adm_nchw_to_nhwc, i.e. dL/dx through `c_in * x` (the tensors
 * EDMPrecond.forward returns take part in autograd w.r.t. x, uncond_unet.py:614-635). */
int adm_precond_out(const void* x, int x_is_f64, const float* f, int ldf, const float* a, const float* s,
                    long coef_bstride, float* out, int B, int C, int HW, hipStream_t stream);
/* backward of the two above w.r.t. f:  df_nhwc[b,p,c<C] = s[b] * dout_nchw[b,c,p], zero for c >= C */
int adm_precond_out_bwd(const float* dout, const float* s, long coef_bstride, float* df, int ldf, int B, int C,
                        int HW, hipStream_t stream);
/* ... that also raises the bound vector amax to max |df| (the output conv's gradients then run on the fp16 format) */
int adm_precond_out_bwd_amax(const float* dout, const float* s, long coef_bstride, float* df, int ldf, float* amax, int B, int C,
                             int HW, hipStream_t stream);
/* emb[b][0:C/2] = cos(t[b] f_i), emb[b][C/2:] = sin(t[b] f_i), f_i = (1/10000)^(i/(C/2))
 * (PositionalEmbedding, uncond_unet.py:224-230) */
int adm_pos_embedding(const float* t, float* emb, int B, int C, hipStream_t stream);
/* y = silu(x) ; dx = dy * silu'(x) */
int adm_silu_fwd(const float* x, float* y, long n, hipStream_t stream);
int adm_silu_bwd(const float* x, const float* dy, float* dx, long n, hipStream_t stream);
/* y = a + b (n floats); y may alias a */
int adm_add(const float* a, const float* b, float* y, long n, hipStream_t stream);
/* y = a + b (+ c when non-NULL), n % 4 == 0, 16-byte aligned: the sum of the gradients autograd would otherwise add pairwise for a
 * tensor with several consumers -- the encoder outputs feed the next block and both decoders' concatenations
 * (uncond_unet.py:548-571). */
int adm_add3(const float* a, const float* b, const float* c, float* y, float* amax, long n, hipStream_t stream);     /* amax (may be NULL): a bound vector, raised to max |y| */
/* dst[m][dst_off + c] (+)= scale * src[m][src_off + c], c < C: channel concat / slice copies
 * (torch.cat, :571, :578; `scale` carries uncond_unet_sd_3's skip-tuning ratio) */
int adm_copy_channels(const float* src, int lds, int src_off, float* dst, int ldd, int dst_off, long M, int C,
                      float scale, int acc, hipStream_t stream);
/* torch.cat((a, scale_b * b), channel axis) of two NHWC tensors in ONE launch (uncond_unet.py:571; `scale_b` = uncond_unet_sd_3's
 * skip-tuning ratio), amax (may be NULL) = bound vector raised to max |y|; adm_split2 = its adjoint (da = dy[:, :Ca], db = scale_b dy[:, Ca:]) */
int adm_concat2(const float* a, int Ca, const float* b, int Cb, float* y, long M, float scale_b, float* amax, hipStream_t stream);
int adm_split2(const float* dy, float* da, int Ca, float* db, int Cb, long M, float scale_b, hipStream_t stream);
/* out[b,i] = a[b] * x[b,i] + s[b] * y[b,i]  (x may be NULL -> s*y only; x fp32 or fp64): the
 * single-decoder variants' D_y = (x - (sigma-1) D_x) / g(sigma)  (uncond_unet_sd.py:602) and its backward */
int adm_axpby_b(const void* x, int x_is_f64, const float* y, const float* a, const float* s, long coef_bstride,
                float* out, int B, long n, hipStream_t stream);

/* SpatialAtt (uncond_unet.py:27-37) after the 384->1 `map` conv:  att [B][HW][ldatt] (channel 0),
 * y[b,p,c] = softsign( sum_j softmax_j(q_p k_j) att_j ) * h[b,p,c] + xres[b,p,c]
 * q = qw*att+qb, k = kw*att+kb; qk = {qw,qb,kw,kb} on device.  HW <= 64. */
int adm_spatial_att_fwd(const float* att, int ldatt, const float* qk, const float* h, const float* xres, float* y,
                        int B, int HW, int C, hipStream_t stream);
/* dh, datt (channel 0 of [B][HW][ldatt], other channels zeroed), dqk[4] (accumulated).  dqk_part = [B][4] workspace:
 * per-image partials summed in image order (deterministic); NULL = fp32 atomics. */
int adm_spatial_att_bwd(const float* att, int ldatt, const float* qk, const float* h, const float* dy, float* dh,
                        float* datt, float* dqk, float* dqk_part, int B, int HW, int C, hipStream_t stream);

/* ---------------- analytic schedule (ddm/ddm_const.py, ddm/ddm_const_2.py) -------------------- */

/* schedule 0 = 'const' (sqrt(t) noise gain), 1 = 'const_2' (t).
 * x_t = x0 + C t + g(t) eps with C = -x0   (ddm_const.py:284-287 / ddm_const_2.py:173-176); NCHW, n per image */
int adm_q_sample(const float* x0, const float* noise, const float* t, float* xt, int B, long n, int schedule,
                 hipStream_t stream);
/* Weighted SSE loss and its gradients (ddm_const.py:335-358 with ddm/loss.py MSE_Loss 'sum'):
 * per_sample[b] = w1[b] sum (Cp+x0)^2 + w2[b] sum (Np-noise)^2 ; dCp = gscale*2 w1 (Cp + x0) ; dNp likewise.
 * w = [B][2] weights precomputed on device.  per_sample is fp64 [B], zero-filled by the call: the f32 terms are summed in fp64 (one
 * workgroup per sample up to n = 65536: bitwise reproducible; above, up to 64 chunks per sample meet in fp64 atomics). */
int adm_ddm_loss(const float* c_pred, const float* n_pred, const float* x0, const float* noise, const float* w,
                 double* per_sample, float* d_c, float* d_n, float gscale, int B, long n, hipStream_t stream);
/* Latent-space loss (LatentDiffusion.p_losses, ddm_const_2.py:527-596, schedule const_2): the two weighted SSE terms
 * of adm_ddm_loss plus w3[b] * sum |x_rec - x0| with x_rec = xt - Cp t - t Np.  w = [B][3] = (w1, w2, w3).
 * per_sample[b] = SSE part, per_l1[b] = un-weighted L1 sum; dCp = gscale (2 w1 (Cp + x0) - w3 t sign(x_rec - x0)),
 * dNp = gscale (2 w2 (Np - noise) - w3 t sign(x_rec - x0)).  Both sums are fp64 [B], zero-filled by the call. */
int adm_ddm_loss_latent(const float* c_pred, const float* n_pred, const float* x0, const float* noise, const float* xt,
                        const float* t, const float* w, double* per_sample, double* per_l1, float* d_c, float* d_n,
                        float gscale, int B, long n, int schedule, int use_l1,
                        hipStream_t stream);
/* Pixel-space loss with use_l1 (ddm_const.py:343-348 / ddm_const_2.py:235-240): the L1 twins are per-sample MEANS over n = C H W,
 * loss_simple_b = [w1 (SSE_C + L1_C / n) + w2 (SSE_eps + L1_eps / n)] / 2.  sums = fp64 [B][4] = un-weighted (SSE_C, SSE_eps, L1_C,
 * L1_eps), zero-filled by the call; the caller combines them.  dCp = gscale 0.5 w1 (2 (Cp + x0) + sign(Cp + x0) / n), dNp likewise
 * with w2 and Np - noise; sign(0) = 0.  w = [B][2].  d_c and d_n may both be NULL (no gradients).  Chunking as adm_ddm_loss. */
int adm_ddm_loss_l1(const float* c_pred, const float* n_pred, const float* x0, const float* noise, const float* w, double* sums,
                    float* d_c, float* d_n, float gscale, int B, long n, hipStream_t stream);
/* One deterministic sampler update in fp64 (ddm_const.py:450-455 / ddm_const_2.py:363-368):
 * x0 = x - C t - eps g(t); [clamp]; x_next = x0 + C t' + eps g(t');  if last: clamp, /scale, (x+1)/2 */
int adm_sampler_step(double* x, const float* c_pred, const float* n_pred, double t_cur, double t_next, int schedule,
                     int clip_x0, double scale_input, int last, long n, hipStream_t stream);

/* One stochastic sampler update in fp64 (ddm_const.py:296-303, 410-414 / ddm_const_2.py:185-197, 324-328):
 * x0 = x - C t - g(t) eps; [clamp]; C' = -x0; x <- mean(x, C', eps, t, s) + sigma(t, s) z, per-image t[B], s[B];
 * z = the N(0,1) draw (device fp64).  last: final clamp, /scale, (x+1)/2. */
int adm_sampler_step_stochastic(double* x, const float* c_pred, const float* n_pred, const double* z, const double* t,
                                const double* s, int schedule, int clip_x0, double scale_input, int last, int B, long n,
                                hipStream_t stream);

/* ---------------- linear-drift schedule (ddm/ddm_linear.py): U(t) = K t^2/2 + C t, C = -x0 - K/2 ---------------- */

/* x_t = x0 + K t^2/2 + C t + sqrt(t) eps with K clamped to [-1, 1] on read and C = -x0 - K/2 (ddm_linear.py:168-171, 198-200).
 * NCHW, n3 floats per image; t [B]. */
int adm_q_sample_linear(const float* x0, const float* noise, const float* K, const float* t, float* xt, int B, long n3,
                        hipStream_t stream);
/* DDPM.p_losses of ddm_linear.py:201-240 without its LPIPS summand, forward and both gradients in one launch.  theta_pred
 * [B][2 n3] = (K_pred | C_pred), the other tensors [B][n3]; K is clamped to [-1, 1] on read; w = [B][3] = (w1, w2, w3).
 * per_simple[b] = w1 mean (theta_pred - [K | C])^2 + w2 mean (n_pred - noise)^2, with use_l1 the mean-|.| twins added and the sum halved;
 * per_mae[b] = mean |x_rec - x0|, x_rec = xt - K_pred t^2/2 - C_pred t - sqrt(t) n_pred.
 * d_theta, d_n (both or neither) = gradients of  sum_b per_simple[b] / B + sum_b w3[b] per_mae[b]. */
int adm_ddm_loss_linear(const float* theta_pred, const float* n_pred, const float* x0, const float* noise, const float* K,
                        const float* xt, const float* t, const float* w, float* per_simple, float* per_mae, float* d_theta,
                        float* d_n, int B, long n3, int use_l1, hipStream_t stream);
/* One reverse step on the fp32 state (ddm_linear.py:178-186, 299-304), per-image t[B], s[B], z = the N(0,1) draw:
 * K = clamp(K_pred, -1, 1); x <- x + K s^2/2 - K t s - C_pred s - s / sqrt(t) n_pred + sqrt(s (t - s) / t) z.
 * last: clamp to +-scale_input, / scale_input, (x + 1) / 2. */
int adm_sampler_step_linear(float* x, const float* theta_pred, const float* n_pred, const float* z, const float* t,
                            const float* s, float scale_input, int last, int B, long n3, hipStream_t stream);
/* out_nchw[b,c,p] = f_nhwc[b,p,c] for a head of C <= 8 channels (the K | C head without preconditioning: no skip term, so the
 * network input is not read); ldf % 4 == 0, ldf >= 8. */
int adm_nhwc_to_nchw(const float* f, int ldf, float* out, int B, int C, int HW, hipStream_t stream);
/* its adjoint: df_nhwc[b,p,c<C] = dout_nchw[b,c,p], zero for c >= C; amax (may be NULL) is raised to max |df| (the head conv's
 * gradients then run on the fp16 format). */
int adm_nhwc_to_nchw_bwd_amax(const float* dout, float* df, int ldf, float* amax, int B, int C, int HW, hipStream_t stream);

/* ---------------- augmentation of x_start (use_augment: True) ------------------------------- */

/* Execution half of AugmentPipe for the transforms DDM enables (/root/reference/ddm/augment.py:161-172, 236-276;
 * instantiated at ddm_const.py:179-180 / ddm_const_2.py:112-113): per-image x/y flips, reflect padding by the batch-wide
 * `margin` = {mx0, my0, mx1, my1} (DEVICE ints: no host read-back), sym6 x2 up-sampling, bilinear affine resampling with
 * theta[N][2][3] (normalised coordinates, align_corners = False, zeros outside), sym6 x2 down-sampling and crop.
 * images / out: NCHW fp32 [N][C][H][W]; flips: int32 [N][2]; ws: adm_aug_workspace_floats(N, C, H, W) floats. */
long adm_aug_workspace_floats(int N, int C, int H, int W);
int adm_augment_geometric(const float* images, const int* flips, const int* margin, const float* theta, float* ws,
                          float* out, int N, int C, int H, int W, hipStream_t stream);

/* ---------------- super-resolution batches (ddm/data.py:645-658, SRDataset.__getitem__) ----------------
 * One launch makes a batch from a uint8 image pool in device memory: sample b is the H x W crop at (top[b], left[b]) of image
 * idx[b]; `image` [B][3][H][W] = (u8 / 255) * 2 - 1 of the crop, `cond` [B][3][h][w] = the same mapping of the crop resized to
 * h x w with PIL's 8-bit two-pass arithmetic (horizontal pass clip8((2^21 + sum k*px) >> 22) into uint8, vertical pass over that),
 * `cond_u8` [B][h][w][3] (may be NULL) = the resized bytes.  flip[b] != 0 mirrors the columns of both outputs, after the resize.
 *   pool: packed HWC uint8 images, 4-byte aligned, pool_bytes a multiple of 4; image n starts at byte img_off[n] and is
 *   img_hw[2n] x img_hw[2n+1] pixels.  idx / top / left / flip: int32 [B], read on the device (out-of-range draws are clamped).
 *   hbounds [w][2] / vbounds [h][2] = {window start, window length} in crop coordinates; hcoef [w][kh] / vcoef [h][kv] = int32
 *   coefficients with 22 fractional bits, kh / kv = the longest window (adm_amd/ddm/sr_data.py resample_table).
 * A workgroup makes an ADM_SR_TILE_H x ADM_SR_TILE_W tile of `cond` from LDS; ADM_EINVAL, without launching, when the tile's
 * source rectangle (sized from H/h, W/w, kh, kv) needs more than 64 KiB of LDS.  adm_sr_tile(0 / 1) = the tile's rows / columns.
 * The resize itself, shared with adm_pair_resize_batch, is adm_amd/csrc/resample_u8.h. */
#define ADM_SR_TILE_H 16
#define ADM_SR_TILE_W 16
int adm_sr_tile(int axis);
int adm_sr_batch(const uint8_t* pool, long pool_bytes, const int64_t* img_off, const int* img_hw, int n_images, const int* idx,
                 const int* top, const int* left, const int* flip, const int* hbounds, const int* hcoef, int kh,
                 const int* vbounds, const int* vcoef, int kv, float* image, float* cond, uint8_t* cond_u8, int B, int H, int W,
                 int h, int w, hipStream_t stream);

/* ---------------- saliency pairs (ddm/data.py:996-1026, DUTSDataset.__getitem__) ----------------
 * One launch makes a batch from TWO uint8 pools in device memory (adm_sr_batch's layout each: packed, 4-byte aligned, a multiple of
 * 4 bytes): sample b is image n = idx[b] (clamped to [0, n_images)): `rgb` [B][3][H][W] = (u8 / 255) * 2 - 1 of the rgb_hw[2n] x
 * rgb_hw[2n+1] HWC photo at byte rgb_off[n] resized to H x W, `gray` [B][1][H][W] the same of the gray_hw[2n] x gray_hw[2n+1]
 * one-byte-per-pixel map at byte gray_off[n] (the two sizes need not agree), both with PIL's 8-bit two-pass arithmetic as in
 * adm_sr_batch; `rgb_u8` [B][H][W][3] / `gray_u8` [B][H][W] (each may be NULL) = the resized bytes.  flip[b] != 0 mirrors the
 * columns of every output, after the resize.
 *   tab: the int32 table pool of tab_ints ints; table t starts at tab[tab_dir[2t]] as bounds [out][2] = {window start, window
 *   length} followed by coefficients [out][k], k = tab_dir[2t+1] (22 fractional bits; adm_amd/ddm/sr_data.py resample_table);
 *   img_tab [n_images][4] = table of the photo's width -> W, of its height -> H, of the map's width -> W, of its height -> H.
 *   max_h / max_w: the largest source height / width of either pool, kh / kv: the longest horizontal / vertical table; they size
 *   the LDS rectangle of an ADM_SR_TILE_H x ADM_SR_TILE_W tile.  adm_pair_resize_lds = the LDS bytes that takes; above 64 KiB
 *   (a source more than about 7 times the target) adm_pair_resize_batch returns ADM_EINVAL without launching.
 * A table or an image that lies about its size gives wrong pixels, never an access outside the pools. */
long adm_pair_resize_lds(int H, int W, int max_h, int max_w, int kh, int kv);
int adm_pair_resize_batch(const uint8_t* rgb_pool, long rgb_bytes, const int64_t* rgb_off, const int* rgb_hw,
                          const uint8_t* gray_pool, long gray_bytes, const int64_t* gray_off, const int* gray_hw, int n_images,
                          const int* tab, long tab_ints, const int* tab_dir, int n_tables, const int* img_tab, int max_h,
                          int max_w, int kh, int kv, const int* idx, const int* flip, float* rgb, float* gray, uint8_t* rgb_u8,
                          uint8_t* gray_u8, int B, int H, int W, hipStream_t stream);

/* ---------------- first-stage images (ddm/data.py:167-185, ImageDataset.__getitem__; the map of DUTSDataset, the photo of
 * SketchDataset) ----------------
 * The one-plane sibling of adm_pair_resize_batch: one launch makes a batch from ONE uint8 pool of images with C = 3 (HWC) or C = 1
 * bytes per pixel (adm_sr_batch's layout: packed, 4-byte aligned, a multiple of 4 bytes).  Sample b is image n = idx[b] (clamped
 * to [0, n_images)): `out` [B][C][H][W] = (u8 / 255) * 2 - 1 of the hw[2n] x hw[2n+1] image at byte off[n] resized to H x W with
 * PIL's 8-bit two-pass arithmetic, `out_u8` [B][H][W][C] (may be NULL) = the resized bytes.  flip[b] != 0 mirrors the columns of
 * both outputs, after the resize.
 *   tab / tab_dir: the table pool of adm_pair_resize_batch; img_tab [n_images][2] = table of the image's width -> W, of its
 *   height -> H.  max_h / max_w / kh / kv size the LDS rectangle as there (adm_pair_resize_lds).
 * ADM_EINVAL, without launching: a null pointer (out_u8 excepted), a pool that is not dword-aligned or not a multiple of 4 bytes,
 * C not 1 or 3, B > 65535, more than 65535 rows of tiles, more than 64 KiB of LDS.
 * A table or an image that lies about its size gives wrong pixels, never an access outside the pools. */
int adm_image_resize_batch(const uint8_t* pool, long pool_bytes, const int64_t* off, const int* hw, int n_images, int C,
                           const int* tab, long tab_ints, const int* tab_dir, int n_tables, const int* img_tab, int max_h,
                           int max_w, int kh, int kv, const int* idx, const int* flip, float* out, uint8_t* out_u8, int B, int H,
                           int W, hipStream_t stream);

/* ---------------- in-painting batches (ddm/data.py:384-476, InpaintDataset.__getitem__ / random_mask / RandomBrush) ----------------
 * A mask is hole = 0 / keep = 1 on integer pixel coordinates of an S x S image, defined in integers: a pixel is a
 * hole when a clipped rectangle, a stroke segment (butt-ended band: 0 <= dot <= L2 and 4 cross^2 <= w^2 L2, int64) or a stroke
 * vertex (disc: 4 d^2 <= (2 (w / 2) + 1)^2) covers it; the two flip bits mirror the STROKES along axis 0 / axis 1 (RandomBrush flips
 * the mask it returns, data.py:472-475), never the rectangles.
 *
 * Draws: per sample ADM_INP_CANDIDATES candidate slabs of ADM_INP_NU uniform and ADM_INP_NZ normal float32 draws, consumed by the
 * reference's calls in FIXED slots (a slot belongs to one call whether or not that call happens):
 *   u[ADM_INP_U_NRECT_SMALL]                    count of rectangles of max_size S/2 (0..3)
 *   u[ADM_INP_U_RECT + 4 j + {0,1,2,3}]         w, h, x, y of rectangle j (j = 0..2 small, j = 3 the one of max_size S)
 *   u[ADM_INP_U_NRECT_BIG]                      count of rectangles of max_size S (0..1)
 *   u[ADM_INP_U_NSTROKE]                        count of strokes (0..7)
 *   u[ADM_INP_U_STROKE + ADM_INP_STROKE_U k + ...]   stroke k: +0 num_vertex, +1 / +2 angle_min / angle_max, +3 .. +19 the angles,
 *                                               +20 / +21 the first vertex x / y, +22 the width, +23 / +24 two discarded draws
 *   u[ADM_INP_U_FLIP + {0,1}]                   the flips along axis 0 / axis 1
 *   z[ADM_INP_SEGMENTS k + i]                   the radius draw of segment i of stroke k
 * adm_inpaint_masks (B threads, fp64 without contraction) turns them into primitive lists and keeps, per sample, the first
 * candidate that covers a pixel (decided from the parameters); if none does it keeps the last, whose mask is all ones, and adds
 * one to fallback[0].  rects int32 [B][4][4] = {x0, y0, x1, y1} clipped to the image (x0 >= x1: empty); verts int32
 * [B][7][18][2] = {x, y} in [0, S]; nverts / widths int32 [B][7] (nverts 0: no stroke); flips int32 [B][2]; chosen int32 [B].
 *
 * adm_inpaint_batch: one launch, a workgroup per ADM_INP_TILE_H x ADM_INP_TILE_W tile of one sample, the sample's primitives
 * staged in LDS and culled against the tile.  Image idx[b] of the pool (adm_sr_batch's layout; it must be S x S) gives `image`
 * [B][3][S][S] = u8 / 255 * 2 - 1 (columns mirrored when img_flip[b] != 0), `cond` = (mask * (u8 / 255)) * 2 - 1 of the same
 * pixels, `ori_mask` [B][1][S][S]; each float is rounded once per operation (no fma), as the host expression is.
 *
 * adm_inpaint_compose: out[b][c][p] = mask[b][p] * ((cond + 1) / 2) + (1 - mask[b][p]) * x[b][c][p], each operation rounded
 * (ddm_const_2.py:629); hw = pixels of a plane. */
#define ADM_INP_CANDIDATES 4
#define ADM_INP_RECTS 4
#define ADM_INP_STROKES 7
#define ADM_INP_VERTS 18
#define ADM_INP_SEGMENTS 17
#define ADM_INP_U_NRECT_SMALL 0
#define ADM_INP_U_RECT 1
#define ADM_INP_U_NRECT_BIG 17
#define ADM_INP_U_NSTROKE 18
#define ADM_INP_U_STROKE 19
#define ADM_INP_STROKE_U 25
#define ADM_INP_U_FLIP 194
#define ADM_INP_NU 196
#define ADM_INP_NZ 119
#define ADM_INP_TILE_H 8
#define ADM_INP_TILE_W 32
int adm_inpaint_masks(const float* u, const float* z, int* rects, int* verts, int* nverts, int* widths, int* flips, int* chosen,
                      int* fallback, int B, int S, hipStream_t stream);
int adm_inpaint_batch(const uint8_t* pool, long pool_bytes, const int64_t* img_off, const int* img_hw, int n_images, const int* idx,
                      const int* img_flip, const int* rects, const int* verts, const int* nverts, const int* widths,
                      const int* flips, float* image, float* cond, float* ori_mask, int B, int S, hipStream_t stream);
int adm_inpaint_compose(const float* mask, const float* cond, const float* x, float* out, int B, int C, long hw,
                        hipStream_t stream);

/* ---------------- optimiser (train_uncond_dpm.py:292-310, ddm/ema.py:158-188) ---------------- */

/* sumsq[0] += sum g^2.  partials = workspace of adm_sumsq_blocks(n) doubles: per-workgroup partial sums combined in a
 * fixed order by a second launch (the norm, hence the clip factor and the update, are bitwise reproducible); NULL = one
 * launch with fp64 atomics. */
int adm_sumsq_blocks(long n);
int adm_sumsq(const float* g, double* sumsq, double* partials, long n, hipStream_t stream);
/* AdamW step on flat buffers with the clip factor computed on device from sumsq[0]:
 * g *= min(1, max_norm/(sqrt(sumsq)+1e-6)); decoupled weight decay; optional EMA lerp
 * (ema += (1-decay)(p-ema)) fused into the same pass when ema != NULL.  beta1, beta2 and ema_decay are doubles: 1 - beta, the bias
 * corrections 1 - beta^step and the EMA weight are formed from them in double on the host and rounded to float once. */
int adm_adamw_step(float* p, const float* g, float* m, float* v, float* ema, const double* sumsq, long n, float lr,
                   double beta1, double beta2, float eps, float wd, float max_norm, int step, double ema_decay,
                   float grad_scale, hipStream_t stream);


/* ================================================================================================
 * Conditional super-resolution denoiser (BASELINE configs[4]):
 * the operators /root/reference/unet/cond_unet_sd.py needs beyond the unconditional UNet's.  NHWC fp32.
 * ================================================================================================ */

/* adm_conv_wgrad for a strided conv with explicit top/left padding (Downsample = Conv2d(C, C', 4, 2, 1), cond_unet_sd.py:341-342;
 * also the 7x7 stem with stride 1, pad_lo 3, and stride-1 convs whose output is smaller than their input): tap (ky, kx) of output (oy, ox) reads x(oy*stride + ky - pad_lo, ...).  The forward
 * is adm_conv_fwd_strided (ks up to 7). */
int adm_conv_wgrad_strided(const float* x, const float* dy, float* dwp, float* dbias, int B, int Hin, int Win, int Hout, int Wout,
                           int Cin, int ldx, int Cout, int lddy, int ks, int stride, int pad_lo, hipStream_t stream);
/* ... in the deterministic workspace form of adm_conv_wgrad_ws: `splits` = adm_conv_wgrad_plan(B, Hout, Wout, Cin, Cout, ks, 0, 0)
 * partial tiles ws[splits][Cout][ks*ks][Cin] (bias partials bws[splits][Cout], may be NULL) for adm_unpack_wgrad_splits. */
int adm_conv_wgrad_strided_ws(const float* x, const float* dy, float* ws, float* bws, int B, int Hin, int Win, int Hout, int Wout,
                              int Cin, int ldx, int Cout, int lddy, int ks, int stride, int pad_lo, int splits, hipStream_t stream);
/* B operand of the GEMM form of the transposed conv (data gradient of a strided conv): out[(tap*Ci_pad + ci)][co] = w[co][ci][tap];
 * col[m][(tap, ci)] = adm_conv_fwd(dy as a 1x1 conv with this operand), then adm_col2im gathers dx. */
int adm_pack_weight_tconv(const float* w, float* out, int Co, int Ci, int ks, int Co_pad, int Ci_pad, hipStream_t stream);
int adm_col2im(const float* col, float* dx, int B, int Hin, int Win, int Ho, int Wo, int C, int ks, int stride, int pad_lo,
               hipStream_t stream);

/* WeightStandardizedConv2d (cond_unet_sd.py:344-357): wn[o][:] = (w[o][:] - mean_o) * rsqrt(var_o + eps) over the K = Cin*kh*kw
 * values of output channel o; stats[o] = (mean, rstd).  Backward: dw (+)= rstd (dwn - mean(dwn) - wn mean(dwn wn)). */
int adm_ws_fwd(const float* w, float* wn, float* stats, int O, int K, float eps, hipStream_t stream);
int adm_ws_bwd(const float* w, const float* stats, const float* dwn, float* dw, int O, int K, int accumulate, hipStream_t stream);

/* LayerNorm over the channels of every pixel with gain g and no bias (cond_unet_sd.py:359-368): x, y [M][C]. */
int adm_lnc_blocks(long M);
int adm_lnc_fwd(const float* x, const float* g, float* y, long M, int C, float eps, hipStream_t stream);
/* part = workspace of adm_lnc_blocks(M) * C doubles */
int adm_lnc_bwd(const float* x, const float* dy, const float* g, float* dx, float* dg, double* part, long M, int C, float eps,
                int accumulate, hipStream_t stream);

/* nn.BatchNorm2d of RelationNet.input_conv{1,2} (cond_unet_sd.py:247-254) on [M][C] rows.  training: batch statistics, running
 * statistics updated in place (momentum, unbiased variance), mr[c] = (mean, rstd) saved for the backward; else mr from the running
 * statistics.  part = adm_bn_blocks(M) * 2 C doubles; sums = 2 C floats. */
int adm_bn_blocks(long M);
int adm_bn_fwd(const float* x, const float* gamma, const float* beta, float* run_mean, float* run_var, float* mr, float* y,
               double* part, long M, int C, float eps, float momentum, int training, hipStream_t stream);
int adm_bn_bwd(const float* x, const float* dy, const float* mr, const float* gamma, float* dx, float* dgamma, float* dbeta,
               double* part, float* sums, long M, int C, int training, int accumulate, hipStream_t stream);

/* F.interpolate(mode='bilinear', align_corners=...) (cond_unet_sd.py:196, 235, 824): x [B][Hi][Wi][C] -> channels
 * [coff, coff + C) of y [B][Ho][Wo][ldy]; the backward is the exact adjoint in gather form (no atomics). */
int adm_bilinear_fwd(const float* x, float* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int ldy, int coff, int align_corners,
                     hipStream_t stream);
int adm_bilinear_bwd(const float* dy, float* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, int lddy, int coff,
                     int align_corners, hipStream_t stream);

/* act: 0 identity, 1 ReLU, 2 GELU (erf form), followed by dropout(p) with the stateless hash of the GroupNorm kernels. */
int adm_act_fwd(const float* x, float* y, long n, int act, float drop_p, uint64_t seed, hipStream_t stream);
int adm_act_bwd(const float* x, const float* dy, float* dx, long n, int act, float drop_p, uint64_t seed, hipStream_t stream);
/* GaussianFourierProjection (cond_unet_sd.py:396-405): out[b] = [sin(2 pi x_b W), cos(2 pi x_b W)], W [D] */
int adm_fourier_features(const float* x, const float* W, float* out, int B, int D, hipStream_t stream);

/* adm_spatial_att_fwd / _bwd for maps of up to 2560 pixels (the 16x16 bottleneck of the SR denoiser): nothing of the HW x HW
 * softmax is stored; gate [B][HW][2] carries (pooled value, log-sum-exp) per row to the backward. */
int adm_spatial_att_big_fwd(const float* att, int ldatt, const float* qk, const float* h, const float* xres, float* y, float* gate,
                            int B, int HW, int C, hipStream_t stream);
int adm_spatial_att_big_bwd(const float* att, int ldatt, const float* qk, const float* h, const float* dy, const float* gate,
                            float* dh, float* datt, float* dqk, float* dqk_part, int B, int HW, int C, hipStream_t stream);

/* softmax(scale q k^T) v per (image, head) with separate query / key lengths; head h = columns [h*D, (h+1)*D) of rows with
 * strides ldq / ldk / ldv / ldo; D in {4, 8, 12, 16, 24, 32, 48, 64, 96}.  RelationNet's windowed cross-attention (cond_unet_sd.py:221-231,
 * scale 1) and the bottleneck Attention (:532-554, scale 32^-0.5).  lse [B*H][Lq][2] = (row maximum,
 * log sum exp(s - maximum)), kept apart so that a maximum of a few hundred does not round the sum; delta = workspace [B*H][Lq]. */
int adm_mha_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Lq, int Lk, int H, int D, int ldq,
                int ldk, int ldv, int ldo, float scale, hipStream_t stream);
int adm_mha_bwd(const float* q, const float* k, const float* v, const float* o, const float* dO, const float* lse, float* dq,
                float* dk, float* dv, float* delta, int B, int Lq, int Lk, int H, int D, int ldq, int ldk, int ldv, int ldo, int lddq,
                int lddk, int lddv, float scale, hipStream_t stream);

/* LinearAttention core (cond_unet_sd.py:516-529): qkv [B][N][384] = (q | k | v) of 4 heads x 32 -> out [B][N][128];
 * ctx [B][4][32][32] and kst [B][128][2] are saved for the backward; ws = adm_linattn_ws_floats(B, N) floats;
 * dctx [B][4][32][32] and S [B][128] are workspaces of the backward. */
long adm_linattn_ws_floats(int B, int N);
int adm_linattn_fwd(const float* qkv, float* out, float* ctx, float* kst, float* ws, int B, int N, hipStream_t stream);
int adm_linattn_bwd(const float* qkv, const float* dout, const float* ctx, const float* kst, float* dqkv, float* dctx, float* S,
                    float* ws, int B, int N, hipStream_t stream);


/* ================================================================================================
 * LPIPS term of the pixel-space loss (ddm_const.py:351-358 / ddm_const_2.py:242-251 with
 * taming/modules/losses/lpips.py): everything around the VGG16 convolutions, which are adm_conv_fwd* calls.
 * No float atomics: every sum has a fixed order.
 * ================================================================================================ */

/* y[B][HW][32] = (x_rec - shift) / scale in channels 0..2, zero in 3..31 (ScalingLayer, lpips.py:56-63, fused with the layout change).
 * schedule -1: x_rec = a (an image, e.g. the target x_start); 0 'const': x_rec = -a with a = C_pred (ddm_const.py:326);
 * 1 'const_2': x_rec = x_noisy - a t - t n_pred (ddm_const_2.py:217), t [B].  a, n_pred, x_noisy are NCHW [B][3][HW]; shift, scale: 3 floats.
 * 2 'linear': a = theta_pred [B][6][HW] = (K_pred | C_pred), x_rec = x_noisy - K_pred t^2/2 - C_pred t - sqrt(t) n_pred (ddm_linear.py:173-176). */
int adm_lpips_input(const float* a, const float* n_pred, const float* x_noisy, const float* t, const float* shift,
                    const float* scale, float* y, int B, int HW, int schedule, hipStream_t stream);
/* its adjoint: d_a (and, schedules 1 and 2, d_n) in NCHW from dy [B][HW][32]; schedule 2: d_a has six channels (-t^2/2 | -t) d x_rec,
 * d_n = -sqrt(t) d x_rec. */
int adm_lpips_input_bwd(const float* dy, const float* t, const float* scale, float* d_a, float* d_n, int B, int HW,
                        int schedule, hipStream_t stream);

/* The same for a one-channel image: a, n_pred, x_noisy are [B][1][HW] and ScalingLayer's broadcast gives channels 0..2 =
 * (x_rec - shift[c]) / scale[c] from the one x_rec (lpips.py:56-63).  Schedules -1, 0 and 1 only; 2 returns ADM_EINVAL.
 * The adjoint sums d x_rec = dy0 / scale0 + dy1 / scale1 + dy2 / scale2 in that fixed order (no atomics) and applies the schedule's
 * factor; schedule 1 also writes d_n.  d_a, d_n: [B][1][HW]. */
int adm_lpips_input_c1(const float* a, const float* n_pred, const float* x_noisy, const float* t, const float* shift,
                       const float* scale, float* y, int B, int HW, int schedule, hipStream_t stream);
int adm_lpips_input_c1_bwd(const float* dy, const float* t, const float* scale, float* d_a, float* d_n, int B, int HW,
                           int schedule, hipStream_t stream);

/* nn.MaxPool2d(2, 2) of VGG16 `features` on NHWC: x [B][H][W][C] -> y [B][H/2][W/2][C]; H, W even, C % 4 == 0.  The backward
 * finds the maximum again from x (no index tensor) and gives the gradient to the first one in the order (0,0), (0,1), (1,0), (1,1),
 * as F.max_pool2d does on ties. */
int adm_maxpool2x2_fwd(const float* x, float* y, int B, int H, int W, int C, hipStream_t stream);
int adm_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, hipStream_t stream);

/* One tap of LPIPS.forward (lpips.py:45-53, 115-121): out[b] (+)= mean_p sum_c w[c] (f0/(|f0|+1e-10) - f1/(|f1|+1e-10))^2 with the
 * norms over the channels of position p; f0, f1 [B][HW][C], C in {64, 128, 256, 512}; part = workspace of
 * B * adm_lpips_head_blocks(HW) floats.  The backward is with respect to f0 only: df0 = d out[b] / d f0 * dout[b]; where f0 is zero in
 * every channel of a position (the reference's gradient is NaN there) it is zero. */
int adm_lpips_head_blocks(int HW);
int adm_lpips_head_fwd(const float* f0, const float* f1, const float* w, float* out, float* part, int B, int HW, int C,
                       int accumulate, hipStream_t stream);
int adm_lpips_head_bwd(const float* f0, const float* f1, const float* w, const float* dout, float* df0, int B, int HW, int C,
                       hipStream_t stream);


/* ================================================================================================
 * Training of the KL autoencoder (ddm/encoder_decoder.py AutoencoderKL.training_step with ddm/loss.py
 * LPIPSWithDiscriminator): the kernels between the convolutions.  No float atomics: every sum is a per-workgroup fp64
 * partial, summed in workgroup order by a second launch.  adm_ae_blocks(n) = the number of partials of an n-element sum.
 * ================================================================================================ */
int adm_ae_blocks(long n);

/* DiagonalGaussianDistribution.sample + .kl (encoder_decoder.py:854-892) on NHWC moments [B*HW][ldm] = (mean[0:C] | logvar[C:2C]):
 * z[B*HW][ldz] = mean + exp(0.5 clamp(logvar, -30, 20)) eps in channels [0, C), zero in [C, ldz); eps [B*HW][C];
 * kl[b] = 0.5 sum (mean^2 + var - 1 - logvar).  part = B * adm_ae_blocks(HW * ldz) doubles. */
int adm_posterior_kl_fwd(const float* moments, int ldm, const float* eps, float* z, int ldz, float* kl, double* part, int B,
                         long HW, int C, hipStream_t stream);
/* its adjoint: dmoments [B*HW][ldm] from dz [B*HW][lddz] (channels [0, C) are read; may be NULL) and dkl [B] (may be NULL); the
 * clamp passes no gradient outside [-30, 20], as torch.clamp; channels [2C, ldm) are zero. */
int adm_posterior_kl_bwd(const float* moments, int ldm, const float* eps, const float* dz, int lddz, const float* dkl,
                         float* dmoments, int B, long HW, int C, hipStream_t stream);

/* Reconstruction term of LPIPSWithDiscriminator.forward (loss.py): x, r [B][n_per]; p [B] = the LPIPS values (NULL: none), which
 * the reference broadcasts over the n_per elements of their image; logvar = one device float.  With
 * S = sum (|x - r| + (x - r)^2) + pw n_per sum_b p[b] and N = B n_per:
 *   out[0] = nll_loss = (S exp(-logvar) + N logvar) / B      out[1] = rec_loss = S / N
 *   out[2] = d nll_loss / d logvar = (N - S exp(-logvar)) / B
 *   out[3] = exp(-logvar) / B = d nll_loss / d (one element of rec_loss);  d nll_loss / d p[b] = pw n_per out[3]
 * part = adm_ae_blocks(B * n_per) doubles. */
int adm_ae_nll_fwd(const float* x, const float* r, const float* p, const float* logvar, float* out, double* part, int B,
                   long n_per, float pw, hipStream_t stream);
/* g = gscale[0] mul (sign(r - x) + 2 (r - x)): the gradient of the elementwise part with respect to r; gscale = one device float */
int adm_ae_nll_bwd(const float* x, const float* r, const float* gscale, float mul, float* g, long n, hipStream_t stream);

/* PatchGAN logit map [M][ld] (NHWC, channel 0 is the logit, the rest padding): out = {mean relu(1 - l), mean relu(1 + l), mean l}
 * (hinge_d_loss halves, -g_loss); part = 3 adm_ae_blocks(M) doubles. */
int adm_logit_terms_fwd(const float* logits, int ld, float* out, double* part, long M, hipStream_t stream);
/* dlogits [M][ld] = s d out[mode] / d logits in channel 0 and zero in the padding; s = mul (coef ? coef[0] : 1), coef = one device
 * float or NULL. */
int adm_logit_terms_bwd(const float* logits, int ld, int mode, const float* coef, float mul, float* dlogits, long M,
                        hipStream_t stream);

/* nn.LeakyReLU(slope): y = x > 0 ? x : slope x; n % 4 == 0. */
int adm_leaky_relu_fwd(const float* x, float* y, long n, float slope, hipStream_t stream);
int adm_leaky_relu_bwd(const float* x, const float* dy, float* dx, long n, float slope, hipStream_t stream);

/* Backward of adm_softmax_rows, in place on dP: dS = scale P (dP - rowsum(dP P)); P, dP [rows][ld], cols % 4 == 0. */
int adm_softmax_rows_bwd(const float* P, float* dP, long rows, int cols, long ld, float scale, hipStream_t stream);
/* out[cols][rows] = in[rows][cols]^T; rows, cols multiples of 4 (operands of the attention block's NT / TN products). */
int adm_transpose2d(const float* in, float* out, int rows, int cols, hipStream_t stream);

/* calculate_adaptive_weight (loss.py): out[0] = clamp(|a| / (|b| + 1e-4), 0, 1e4) disc_weight for two gradient buffers of na / nb
 * floats; part = adm_ae_blocks(na) + adm_ae_blocks(nb) doubles. */
int adm_adaptive_weight(const float* a, long na, const float* b, long nb, double* part, float disc_weight, float* out,
                        hipStream_t stream);
/* out = a + coef[0] mul b with coef one device float (the adaptive weight); n % 4 == 0. */
int adm_axpy_dev(const float* a, const float* b, const float* coef, float mul, float* out, long n, hipStream_t stream);

/* ================================================================================================
 * Forward of the Swin condition encoder (unet/swin_transformer.py of the reference; csrc/swin.hip).
 * ================================================================================================ */

/* shifted_window_attention between its qkv and proj Linears.  qkv [B][H][W][3C] = the qkv Linear's output with its bias, last axis
 * ordered [3][heads][32]; qkv_bias [3C]; table [169][heads] (relative_position_bias_table); out [B][H][W][C].  The zero padding of H
 * and W up to multiples of the window, the roll by -shift, the window partition, the bias lookup
 * table[(dy + 6) * 13 + (dx + 6)][head], the additive -100 mask between the regions of the rolled frame and the inverses are index
 * arithmetic: a token outside H x W is a key / value equal to qkv_bias.  The shift of an axis whose padded size is one window is
 * ignored.  Specialised to window == 7 and C == 32 * heads: anything else returns -22. */
int adm_swin_attn_fwd(const float* qkv, const float* qkv_bias, const float* table, float* out, int B, int H, int W, int C,
                      int heads, int window, int shift_h, int shift_w, hipStream_t stream);
/* nn.LayerNorm(C) with weight and bias over the rows of x [M][C]; 32 <= C <= 2048, C % 4 == 0.  Two passes over the row in
 * registers (mean, then squared deviations). */
int adm_ln_affine_fwd(const float* x, const float* w, const float* b, float* y, long M, int C, float eps, hipStream_t stream);
/* The register form the LayerNorm kernels (plain and merged, forward and backward) take for a row of C floats (merged: C = 4 Cin):
 * out[0] = NQ, the float4 slots per lane (1, 2, 4 or 8; the row uses ceil(C / 256) of them), out[1] = the float4 of the row in its
 * last used trip over the 64 lanes (64: the trip is whole; fewer: lanes past the row's end).  The function the launches choose
 * through.  -22 for a C they refuse. */
int adm_ln_form(int C, int* out);
/* PatchMerging's gather fused with its LayerNorm(4C): x [B][H][W][C] -> y [B][ceil(H/2)][ceil(W/2)][4C], the 2x2 cell's pixels in
 * the order (0,0), (1,0), (0,1), (1,1) as (dy, dx), zeros past an odd edge; w, b [4C]; C % 4 == 0, 8 <= C <= 512. */
int adm_swin_merge_ln_fwd(const float* x, const float* w, const float* b, float* y, int B, int H, int W, int C, float eps,
                          hipStream_t stream);

/* ================================================================================================
 * Backward of the Swin condition encoder (csrc/swin.hip).  No float atomics: every sum over units / rows goes through partials in
 * the caller's workspace and a second kernel that adds them in a fixed order, so the results are the same bits every run.
 * ================================================================================================ */

/* Gradient of adm_swin_attn_fwd (same geometry arguments; scores and softmax are recomputed, nothing is saved by the forward).
 * d_out [B][H][W][C] -> d_qkv [B][H][W][3C] (every element written), d_table [169][heads], d_qkv_bias [3C].  A padding token is a
 * key / value equal to qkv_bias, so its dK and dV go to the K and V thirds of d_qkv_bias (the Q third is zero); the share of the
 * real tokens reaches the bias through the qkv Linear's own backward.  acc_table / acc_bias != 0: add to what d_table / d_qkv_bias
 * hold.  ws: adm_swin_attn_bwd_ws_floats(B, H, W, heads) floats (need not be cleared). */
long adm_swin_attn_bwd_ws_floats(int B, int H, int W, int heads);
int adm_swin_attn_bwd(const float* qkv, const float* qkv_bias, const float* table, const float* d_out, float* d_qkv, float* d_table,
                      float* d_qkv_bias, float* ws, int B, int H, int W, int C, int heads, int window, int shift_h, int shift_w,
                      int acc_table, int acc_bias, hipStream_t stream);
/* Gradients of adm_ln_affine_fwd: dx [M][C], dw [C], db [C] from x, w and dy; the row statistics are recomputed in the forward's
 * shifted two-pass form.  accumulate != 0: add to what dw / db hold.  ws: adm_ln_bwd_ws_floats(M, C) floats. */
long adm_ln_bwd_ws_floats(long M, int C);
int adm_ln_affine_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, float* ws, long M, int C,
                      float eps, int accumulate, hipStream_t stream);
/* Gradients of adm_swin_merge_ln_fwd: dy [B][ceil(H/2)][ceil(W/2)][4C] -> dx [B][H][W][C] (scattered back through the 2x2 gather:
 * every pixel has one destination, positions past an odd edge are dropped), dw, db [4C].
 * ws: adm_ln_bwd_ws_floats(B * ceil(H/2) * ceil(W/2), 4C) floats. */
int adm_swin_merge_ln_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, float* ws, int B, int H,
                          int W, int C, float eps, int accumulate, hipStream_t stream);
/* Stochastic depth in "row" mode: y[b][i] = x[b][i] + s[b] * r[b][i] for B samples of n elements (n % 4 == 0), s[b] = keep_b /
 * (1 - p).  x == NULL: y = s[b] * r (the gradient of the branch).  A row with s[b] == 0 copies x bit for bit. */
int adm_rowscale_add(const float* x, const float* r, const float* s, float* y, int B, long n, hipStream_t stream);

/* Patch embedding of a ONE-channel image fused with its LayerNorm (the stem of the single-channel condition encoder): x [B][1][H][W]
 * f32 -> conv 4x4, stride 4, no padding with w [E][1][4][4] and bias cb [E] -> LayerNorm over E with gamma, beta [E] ->
 * y [B][H/4][W/4][E] (floor division: trailing rows / columns of x are never read).  One launch; neither a channel-padded copy of x
 * nor the pre-norm tensor exists in memory.  The statistics are two passes over registers (the mean, then the squared deviations
 * from it).  E % 32 == 0 and 32 <= E <= 512; anything else, H < 4 or W < 4 returns -22.  w, cb, gamma, beta and y 16-byte aligned;
 * x is read in 16-byte pieces when it is aligned and W % 4 == 0, else by element. */
int adm_patch_embed_ln_fwd(const float* x, const float* w, const float* cb, const float* gamma, const float* beta, float* y, int B,
                           int H, int W, int E, float eps, hipStream_t stream);
/* The lane layout the stem kernels (forward and backward) take for a width E: out = (G lanes per token, Q float4 per lane, E / 4
 * float4 per token); G Q > E / 4 means lanes past the row.  The function the launches choose through.  -22 for an E they refuse. */
int adm_patch_embed_form(int E, int* out);
/* Parameter gradients of adm_patch_embed_ln_fwd from x and dy [B][H/4][W/4][E]: dW [E][16], db, dgamma, dbeta [E].  There is no dX.
 * The conv outputs and the token statistics are recomputed from x (the forward saves nothing).  The sums over tokens go through one
 * partial per workgroup in ws and a second kernel that adds them in workgroup order: no float atomics, the same bits every run.
 * accumulate: bit 0 dW, bit 1 db, bit 2 dgamma, bit 3 dbeta -- add to what the destination holds.
 * ws: adm_patch_embed_ln_bwd_ws_floats(B, H, W, E) floats (need not be cleared; 0 for an unsupported shape). */
long adm_patch_embed_ln_bwd_ws_floats(int B, int H, int W, int E);
int adm_patch_embed_ln_bwd(const float* x, const float* w, const float* cb, const float* gamma, const float* dy, float* dW, float* db,
                           float* dgamma, float* dbeta, float* ws, int B, int H, int W, int E, float eps, int accumulate,
                           hipStream_t stream);

/* ================================================================================================
 * InceptionV3 feature extractor and feature statistics behind FID / Inception score (csrc/inception.hip).  Forward only, NHWC f32,
 * channels padded to 32.  These entry points do not look at any compute-mode switch: the math is the exact f32 MFMA.
 * ================================================================================================ */

/* y[.., yoff : yoff + N] = act(conv(x, w) + bias) for a kh x kw filter (each side 1, 3, 5 or 7), stride 1 or 2, zero padding pad_h /
 * pad_w (each at most half its side).  x [B][Hin][Win][ldx] with Cin % 32 == 0 channels read (x may itself be a slice of a wider
 * buffer); wp [N][kh*kw*Cin] with k = (dy*kw + dx)*Cin + c; bias [N] or NULL; N % 32 == 0 -- rows of wp and bias past the real
 * output channels are zero, so the padded lanes are written as zero.  y has row stride ldy, yoff % 32 == 0, and only columns
 * yoff .. yoff+N-1 are written; Ho = (Hin + 2 pad_h - kh) / stride + 1, likewise Wo.  act: 1 = ReLU, 0 = none (the fc layer).
 * tile: -1 = chosen by the launcher, 0..3 = 128x128 / 128x96 / 64x64 / 128x32.  x and wp 16-byte aligned. */
int adm_conv_rect_relu_fwd(const float* x, const float* wp, const float* bias, float* y, int B, int Hin, int Win, int Cin, int ldx,
                           int N, int ldy, int yoff, int kh, int kw, int stride, int pad_h, int pad_w, int act, int tile,
                           hipStream_t stream);
/* 3x3 pooling of x [B][H][W][ldx] (C % 4 == 0 channels) into y[.., yoff : yoff + C] with row stride ldy.  mode 0: max, stride 2, no
 * padding (Ho = (H-3)/2 + 1); 1: max, stride 1, pad 1, padding = -inf; 2: average, stride 1, pad 1, divided by the number of taps
 * inside the image (count_include_pad = False). */
int adm_pool3x3_fwd(const float* x, float* y, int B, int H, int W, int C, int ldx, int ldy, int yoff, int mode, hipStream_t stream);
/* x [B][H][W][ldx] -> y [B][C]: spatial mean, summed in float64 in a fixed order. */
int adm_global_avgpool_fwd(const float* x, float* y, int B, int H, int W, int C, int ldx, hipStream_t stream);
/* img uint8 [B][3][H][W] -> y [B][299][299][32] f32 (channels 3..31 zero): TensorFlow-1 bilinear resize (align_corners = False; grid =
 * float(i) * float32(in / out), truncated; hi = min(lo + 1, n - 1); a + (b - a) * d along x, then y; no fma) followed by
 * (v - 128) / 128.  Equal bit for bit to the same float32 operations on the host. */
int adm_tf1_resize_norm_u8(const unsigned char* img, float* y, int B, int H, int W, hipStream_t stream);
/* Streaming first and second moments of feature rows x [n][D] in float64: sum[D] += sum_r (x[r] - shift), outer[D][D] +=
 * sum_r (x[r] - shift)(x[r] - shift)^T.  first != 0: shift[D] is set to this batch's column mean before anything is added (the
 * caller clears sum and outer); later calls reuse it.  One thread owns each output element and adds the rows in order: no atomics,
 * the same bits every run.  The host forms mu = shift + sum / N and sigma = (outer - sum sum^T / N) / (N - 1). */
int adm_feat_stats_accum(const float* x, int n, int D, double* shift, double* sum, double* outer, int first, hipStream_t stream);

/* ================================================================================================
 * Depth estimation (csrc/depth_data.hip): the batches of ddm.data.NYUDv2DepthDataset (ddm/data.py:869-887) and the depth score.
 * ================================================================================================ */

/* One launch makes a batch from a uint8 HWC photo pool (adm_sr_batch's layout) and a 16-BIT depth pool: little-endian, two bytes
 * per pixel, 2-byte aligned, depth_bytes even, every depth_off[n] even.  Image n of either pool starts at byte *_off[n] and is
 * *_hw[2n] x *_hw[2n+1] pixels.  Sample b is image n = idx[b] (clamped to [0, n_images)); output pixel (y, x) is the source pixel
 *   (box_top + top[b] + y,  box_left + left[b] + (flip[b] ? W - 1 - x : x))
 * of both planes, top / left clamped to [0, box height - H] / [0, box width - W]; the box is PIL's (left, upper, right, lower).
 *   image [B][1][H][W] = (u16 / 10000) * 2 - 1 (no clipping), cond [B][3][H][W] = (u8 / 255) * 2 - 1: IEEE float32 operations in
 *   that order, equal bit for bit to NumPy's.
 * `image` or `cond` may be NULL (not both); the pool of a NULL output is not read and may be NULL too.  idx / top / left / flip:
 * int32 [B], read on the device.  With W % 4 == 0 and 16-byte aligned outputs every thread writes 16 bytes per plane, otherwise one
 * pixel.  ADM_EINVAL, without launching: a missing pointer, an odd depth_bytes or depth pointer, B > 65535, a box smaller than
 * H x W or with a negative corner.  A source pixel outside its image or its pool reads as 0: wrong tables give wrong pixels, never an
 * access outside the pools. */
int adm_depth_batch(const uint8_t* rgb_pool, long rgb_bytes, const int64_t* rgb_off, const int* rgb_hw, const uint8_t* depth_pool,
                    long depth_bytes, const int64_t* depth_off, const int* depth_hw, int n_images, int box_left, int box_top,
                    int box_right, int box_bottom, const int* idx, const int* top, const int* left, const int* flip, float* image,
                    float* cond, int B, int H, int W, hipStream_t stream);

/* Per-image float64 sums of the depth score from pred / gt [B][hw] float32, depth as a FRACTION of 10 m (metres = 10 x): over the
 * pixels with min_depth < gt_m < max_depth, with pred_m clamped to [min_depth, max_depth],
 *   sums[b] = { n, S|p-g|/g, S(p-g)^2/g, S(p-g)^2, S(ln p - ln g)^2, S(ln p - ln g), S|log10 p - log10 g|,
 *               #[r < 1.25], #[r < 1.25^2], #[r < 1.25^3] },  r = max(p/g, g/p)          (ADM_DEPTH_SUMS doubles, counts as doubles)
 * One launch of adm_depth_metrics_blocks(hw) workgroups per image (one per ADM_DEPTH_CHUNK pixels, at most ADM_DEPTH_MAX_BLOCKS); each
 * writes its partial sums to partial [B][blocks][ADM_DEPTH_SUMS], and the last one of an image to finish (ticket[b], an integer
 * counter) adds them in index order: no float atomics, the same bits every run.  ticket: int32 [B], ZERO on entry and zero again on
 * return.  ADM_EINVAL: a null pointer, B > 65535, min_depth <= 0 or max_depth <= min_depth. */
#define ADM_DEPTH_SUMS 10
#define ADM_DEPTH_CHUNK 4096
#define ADM_DEPTH_MAX_BLOCKS 64
int adm_depth_metrics_blocks(long hw);
int adm_depth_metrics(const float* pred, const float* gt, double* sums, double* partial, int* ticket, int B, long hw,
                      double min_depth, double max_depth, hipStream_t stream);

/* ================================================================================================
 * Kernel Inception distance (csrc/kid.hip): the polynomial-kernel MMD sums of every subset, in one launch.
 * ================================================================================================ */

/* f1 [n1][D], f2 [n2][D] float32, rows contiguous (ld = D), 16-byte aligned; idx1, idx2 int32 [S][m], read on the device.  For
 * subset s with X = f1[idx1[s]], Y = f2[idx2[s]] and k(a, b) = (gamma <a, b> + coef0)^degree:
 *   sums[s] = { sum_{i != j} k(X_i, X_j), sum_{i != j} k(Y_i, Y_j), sum_{i, j} k(X_i, Y_j) }              (float64 [S][3])
 * i, j are subset POSITIONS: a feature row drawn twice into one subset counts as two rows.  The unbiased MMD^2 of the subset is
 * (sums[0] + sums[1]) / (m (m - 1)) - 2 sums[2] / m^2.
 * One launch of S * adm_kid_sums_blocks(m) workgroups covers all subsets and all three blocks: each gathers its rows through the
 * index tables, forms an ADM_KID_TILE-square tile of dot products on the exact f32 MFMA (an fmaf chain over k), and sums
 * (double(dot) * gamma + coef0)^degree (repeated multiplication) in float64 into partial [S][blocks]; no Gram matrix is written.  XX
 * and YY are computed as upper triangles, off-diagonal tiles counted twice.  A second small launch adds each subset's partials in
 * index order: no float atomics, the same bits every run.
 * adm_kid_sums_tile(which): the workgroup tile edge of form `which` (0 ..), 0 past the last form -- there is one, ADM_KID_TILE.
 * ADM_EINVAL, without launching: a null or misaligned pointer, D % 4 != 0, m < 2, m > min(n1, n2), S < 1, degree outside 1..8, a
 * feature matrix of 2^31 bytes or more.  The caller checks 0 <= idx < n; an index outside reads as a zero row: wrong tables give
 * wrong sums, never an access outside the features. */
#define ADM_KID_TILE 128
int adm_kid_sums_tile(int which);
long adm_kid_sums_blocks(int m);
int adm_kid_sums(const float* f1, int n1, const float* f2, int n2, int D, const int* idx1, const int* idx2, int S, int m, int degree,
                 double gamma, double coef0, double* sums, double* partial, hipStream_t stream);

/* ================================================================================================
 * Saliency score (csrc/saliency_metrics.hip): the integer tables behind MAE, F-, E- and S-measure, in one launch.
 * ================================================================================================ */

/* pred [B][H][W] uint8, or float32 with pred_is_f32 != 0 (quantised as rintf(fminf(fmaxf(p, 0), 1) * 255), ties to even, NaN -> 0:
 * the bytes of the samplers' 8-bit PNGs); map [B][H][W] uint8, foreground g = [map > 128].  Per image:
 *   head   [B][5]         int64 = { nF, sum x g, sum y g, cx, cy }, x / y 0-based; cx = X + 1 with X = (2 sum x g + nF) / (2 nF) in
 *                                 integers (round half up), X = W / 2 when nF = 0; cy likewise from y and H: 1 <= cx <= W, 1 <= cy <= H
 *   tables [B][4][2][256] int64 = the number of pixels with prediction byte v and class c = g in quadrant q = 2 [y >= cy] + [x >= cx]
 * One workgroup per image: an integer reduction over the map, then a 4 x 2 x 256 uint32 histogram in LDS (LDS integer atomics, one per
 * run of equal keys), stored widened.  Nothing passes between workgroups and no float is added: the same integers every run, equal to
 * a bincount.  Both outputs are overwritten whole.  Images need no alignment (image k starts at byte k H W); 16-byte loads are used
 * where the addresses allow.  ADM_EINVAL, without launching: a null pointer, B outside 1 .. 65535, H or W < 1, H W >
 * ADM_SALIENCY_MAX_PIXELS, a float32 pred off a 4-byte or an output off an 8-byte boundary. */
#define ADM_SALIENCY_BINS 2048
#define ADM_SALIENCY_MAX_PIXELS (1L << 24)
int adm_saliency_tables(const void* pred, int pred_is_f32, const uint8_t* map, int64_t* tables, int64_t* head, int B, int H, int W,
                        hipStream_t stream);

/* ================================================================================================
 * Restoration score (csrc/restoration_metrics.hip): the sums behind PSNR and SSIM, on RGB and on Y, in one launch.
 * ================================================================================================ */

/* pred / target [B][C][H][W], C = 1 or 3, each uint8 or -- with its own *_is_f32 != 0 -- float32 (quantised as
 * rintf(fminf(fmaxf(v, 0), 1) * 255), ties to even, NaN -> 0: the bytes of the samplers' 8-bit PNGs).  crop_border = s >= 0 pixels are
 * skipped on every side by addressing: the scored area is H' x W' = (H - 2s) x (W - 2s).  Planes P: for C = 3 four -- R, G, B and
 * Y = 16 + N / 255000 with the integer N = 65481 R + 128553 G + 24966 B --, for C = 1 one.  Per image and plane:
 *   sse  [B][P][2] int64  = {lo, hi}, hi 2^32 + lo = the sum over the area of d^2 as an exact integer, 0 <= lo < 2^32; d = p - g on a
 *                           byte plane, N_p - N_g on Y (the caller scales by 255000^-2)
 *   ssim [B][P]    double = the SUM over the (H' - 10) x (W' - 10) valid positions of the SSIM value under the 11 x 11 Gaussian
 *                           window (sigma 1.5, normalised, separable), C1 = 6.5025, C2 = 58.5225; filtered in float64
 * One workgroup per ADM_RESTORATION_TILE^2 tile of valid positions and image: adm_restoration_blocks(H', W') of them per image
 * (ADM_EINVAL below 11 x 11).  Each writes its sums to partial [B][blocks][P][2] int64, and the last one of an image to finish
 * (ticket[b], an integer counter) adds them in index order: no float atomics, the same bits every run.  ticket: int32 [B], ZERO on
 * entry and zero again on return.  Both outputs are overwritten whole.  Images need no alignment (image k starts at element
 * k C H W); 4- and 16-byte loads are used where the addresses allow.  ADM_EINVAL, without launching: a null pointer, B outside
 * 1 .. 65535, C not 1 or 3, crop_border < 0, H' or W' < 11, H W > ADM_RESTORATION_MAX_PIXELS, a float32 input off a 4-byte, an output
 * or partial off an 8-byte or ticket off a 4-byte boundary. */
#define ADM_RESTORATION_TILE 32
#define ADM_RESTORATION_WINDOW 11
#define ADM_RESTORATION_MAX_PIXELS (1L << 24)
int adm_restoration_blocks(int Hs, int Ws);
int adm_restoration_sums(const void* pred, int pred_is_f32, const void* target, int target_is_f32, int64_t* sse, double* ssim,
                         int64_t* partial, int* ticket, int B, int C, int H, int W, int crop_border, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADM_HIP_H */

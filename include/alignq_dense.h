/* alignq_dense.h - DenseNet's evaluation pass without concatenations (csrc/dense_eval_kernels.hip; Python: alignq_amd/fused.py
 * dense_layer_eval / avgpool2_into, alignq_amd/densenet.py DenseNet._forward_eval).  The entry points link into the same
 * libalignq_hip.so as those of alignq.h and use its error codes and formula constants; the clamps are those of alignq_mobile.h.
 *
 * Why a fifth header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h,
 * alignq_pointwise.h and alignq_k3conv.h are fixed sets too.  This extension only ADDS entry points, so it is declared next to them
 * and read by alignq_amd/_lib.py into a table of its own (DENSE_SIGNATURES, bound last); nothing declared here appears in any other
 * header.  The header is plain C in the vocabulary alignq_amd/_header.py reads: prototypes over pointers and scalars, one POD record.
 *
 * A dense layer of the reference (cdf_alignment/dense-cifar-10/model/densenet.py:17-41) is bn1 -> act_q0 -> ReLU -> 3x3 convolution
 * (CIN -> growthRate), its output concatenated behind its input.  In evaluation the site is per channel and elementwise, so it is
 * applied while the convolution stages its input tile, and the convolution writes its channels straight behind its input into ONE
 * buffer per dense block: pixel p of a tensor starts at base + p * pitch (floats), its channels contiguous from there.
 *
 * alignq_dense_layer_eval_fwd:   y[p][0..COUT) = conv3x3( clamp(q(a_c * x[p][c] + b_c)), W_q )
 *   * x: B * H * W pixels at pitch ldx, of which the first CIN floats are read and nothing beyond them; y: the same pixels at pitch
 *     ldy, of which the first COUT floats are written and nothing else.  The floats read and the floats written must be disjoint;
 *     the SAME buffer with disjoint channel ranges is allowed and is the main use:  y = x + CIN, ldy = ldx.
 *   * the site (alignq_dense_site; fields and NULL rules of alignq_eval_site, alignq_mobile.h, without its z) is exactly
 *     alignq_site_eval_fwd's:  s_c = sqrt(running_var_c + bn_eps), a_c = gamma_c / s_c (square root and quotient formed in double and
 *     rounded once), b_c = beta_c - (a_c * running_mean_c), v = (a_c * x) + b_c, every fp32 operation rounded on its own; q = the
 *     quantiser of alignq_act_quant_fwd (formula, act_range; k == 32: none); then the clamp (NaN and -0 give +0 under RELU / RELU6).
 *     The coefficients are formed inside the launch from the batch-norm vectors, which are only READ: there is no preparing launch,
 *     and a captured graph stays valid when the running statistics change;
 *   * the convolution is exactly alignq_k3conv_fwd's (alignq_k3conv.h): w_bins = the filter's bf16 bins [COUT][3][3][CIN]; the site's
 *     output is split into three bf16 terms once per element and chunk; 32-channel chunks in ascending order, inside a chunk the nine
 *     taps in ascending order of the pixel read, inside a tap lo, mid, hi; one division by n = 2^w_bit - 1;
 *   * the padding, the tile pixels outside the image and the channel tail of the last chunk are zeros AFTER the site: 0, not q(b_c);
 *   * the result is bit-identical to alignq_site_eval_fwd into a contiguous temporary followed by alignq_k3conv_fwd; the quantised
 *     input is never written;
 *   * supported set: CIN, COUT multiples of 4 in [4, 512]; ldx >= CIN, ldy >= COUT, both multiples of 4; B, H, W >= 1 with
 *     B * H * W * max(ldx, ldy) <= 2^31 - 1; 1 <= w_bit <= 8; k in 1..16, or 32; x, y and w_bins 16-byte aligned;
 *   * ALIGNQ_EINVAL: a NULL x, y, w_bins, record, running_mean or running_var; a misaligned x, y or w_bins; a w_bit outside 1..8; a
 *     k outside 1..16 and != 32; a formula neither ALIGNQ_FORMULA_ADMM nor ALIGNQ_FORMULA_CDF; a clamp outside ALIGNQ_CLAMP_*; a
 *     pitch that is no multiple of 4 or is below its width.  ALIGNQ_EUNSUPPORTED: any other shape.  A bad argument is named before an
 *     unsupported shape, and both before anything is launched;
 *   * the tile width follows alignq_k3conv_form(ALIGNQ_K3_FWD, ...) (16 / 32 / 64 output channels); at most 2048 spatial tiles are in
 *     the grid, the rest go by grid stride; an output of 1 MiB to 64 MiB (B * H * W * COUT * 4 bytes written) is stored write-through
 *     (csrc/store_forms.h); same values, same addresses.
 *
 * alignq_avgpool2_nhwc_fwd: a transition's 2 x 2 / stride 2 average pool, written at a pitch so that it lands in the next block's
 *   buffer.  x: [B][H][W][C] contiguous; y: [B][H / 2][W / 2] pixels at pitch ldy, C floats of each written.
 *       y = (((x[2h][2w] + x[2h][2w+1]) + x[2h+1][2w]) + x[2h+1][2w+1]) * 0.25f        every operation its own fp32 operation
 *   An odd trailing row or column is dropped, as F.avg_pool2d does.  H, W >= 2; C % 4 == 0 in [4, 2048]; ldy >= C, a multiple of 4;
 *   B >= 1 with B * H * W * C and B * (H / 2) * (W / 2) * ldy <= 2^31 - 1.  ALIGNQ_EINVAL: a NULL or misaligned pointer, a pitch that
 *   is no multiple of 4 or is below C; ALIGNQ_EUNSUPPORTED: any other shape.  x and the floats written must be disjoint.
 *
 * Both entry points only enqueue on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable; two launches
 * on the same inputs give the same bits.                                                                                        */
#ifndef ALIGNQ_DENSE_H
#define ALIGNQ_DENSE_H

#include <stddef.h>
#include <stdint.h>

#include "alignq_mobile.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct alignq_dense_site {
  const float* gamma;        /* [CIN] or NULL = 1 */
  const float* beta;         /* [CIN] or NULL = 0 */
  const float* running_mean; /* [CIN] */
  const float* running_var;  /* [CIN] */
  float bn_eps;
  int k;                     /* 1..16, or 32: no quantiser */
  int clamp;                 /* ALIGNQ_CLAMP_* (alignq_mobile.h) */
} alignq_dense_site;

int alignq_dense_layer_eval_fwd(const float* x, int ldx, float* y, int ldy, const alignq_dense_site* site, const void* w_bins, int B,
                                int H, int W, int CIN, int COUT, int w_bit, float act_range, int formula, void* stream);

int alignq_avgpool2_nhwc_fwd(const float* x, float* y, int ldy, int B, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_DENSE_H */

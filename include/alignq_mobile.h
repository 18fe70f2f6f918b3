/* alignq_mobile.h - the folded evaluation sites of MobileNet-V2 (csrc/mobile_eval_kernels.hip; Python: alignq_amd/fused.py
 * site_eval_any / site_eval_twin / dw_site_eval, alignq_amd/mobilenet.py).  The entry points link into the same libalignq_hip.so
 * as those of alignq.h and use its error codes and formula constants.
 *
 * Why a second header: alignq.h is the core C ABI.  Its set of entry points and ALIGNQ_ABI_VERSION are fixed and checked against
 * the binding one by one; an extension that only ADDS entry points for one model family lives next to it instead of moving it.
 * alignq_amd/_lib.py reads this header into its own table (MOBILE_SIGNATURES); nothing declared here appears in alignq.h.
 * The header is plain C in the vocabulary alignq_amd/_header.py reads: prototypes over pointers and scalars, one POD record,
 * integer #defines.
 *
 * Common to the three entry points
 *   fp32, channels-last [P][C] tensors (P = B * H * W pixels, channels fastest), every pointer 16-byte aligned, C % 4 == 0 and
 *   4 <= C <= 2048.  They only enqueue on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable.
 *   One site (alignq_eval_site): the eval-mode batch-norm's [C] vectors (gamma / beta may be NULL = 1 / 0; running_mean and
 *   running_var are required; all are only READ), its eps, the quantiser's bit width k (1..16, or 32 = NO quantiser) and the clamp
 *   applied last.  Arithmetic: exactly alignq_bnq_eval_fwd's (alignq.h), fp32, every operation rounded on its own, no fused
 *   multiply-add; the square root and the quotient are formed in double and rounded once:
 *       s_c = sqrt(running_var_c + bn_eps);   a_c = gamma_c / s_c;   b_c = beta_c - (a_c * running_mean_c);   x = (a_c * z) + b_c
 *   then q(x) = the quantiser of alignq_act_quant_fwd (formula, act_range; k == 32: q(x) = x), then the sum where there is one, then
 *   the clamp:
 *       ALIGNQ_CLAMP_NONE   v
 *       ALIGNQ_CLAMP_RELU   v > 0 ? v : +0
 *       ALIGNQ_CLAMP_RELU6  v > 0 ? (v < 6 ? v : 6) : +0
 *   NaN and -0 give +0 under both clamps, the convention of oracle/alignq_oracle.c for relu.  torch.nn.ReLU6 (hardtanh) differs
 *   there: it propagates NaN and keeps -0; on every other input the values are equal.
 *   Checks, all before anything is launched.  ALIGNQ_EINVAL: a NULL record, z, running_mean, running_var or y; a pointer that is
 *   not 16-byte aligned; k outside 1..16 and != 32; formula neither ALIGNQ_FORMULA_ADMM nor ALIGNQ_FORMULA_CDF; a clamp outside
 *   the three above; P < 1 (B, H_in or W_in < 1).  ALIGNQ_EUNSUPPORTED: a C outside the set above (and, for the depthwise form, a
 *   stride other than 1 or 2 or a shape alignq_dwconv3x3_supported refuses).
 *   Outputs of 1 MiB to 64 MiB are stored write-through (csrc/store_forms.h); same values, same addresses.                    */
#ifndef ALIGNQ_MOBILE_H
#define ALIGNQ_MOBILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNQ_CLAMP_NONE 0
#define ALIGNQ_CLAMP_RELU 1
#define ALIGNQ_CLAMP_RELU6 2

typedef struct alignq_eval_site {
  const float* z;            /* [P][C]: the convolution's output (alignq_dwconv3x3_site_eval_fwd forms it itself: ignored there) */
  const float* gamma;        /* [C] or NULL = 1 */
  const float* beta;         /* [C] or NULL = 0 */
  const float* running_mean; /* [C] */
  const float* running_var;  /* [C] */
  float bn_eps;
  int k;                     /* 1..16, or 32: no quantiser */
  int clamp;                 /* ALIGNQ_CLAMP_* */
} alignq_eval_site;

/* y = clamp( q(a_c z + b_c) [+ residual] ): alignq_bnq_eval_fwd's form at any C % 4 == 0, with ReLU6 among the clamps and without a
 * packed-index output.  residual: [P][C] or NULL.  At a power-of-two C, clamp NONE / RELU gives the bits of alignq_bnq_eval_fwd
 * with relu = 0 / 1.                                                                                                             */
int alignq_site_eval_fwd(const alignq_eval_site* site, int64_t P, int C, float act_range, int formula, const float* residual,
                         float* y, void* stream);

/* The stride-1 block's tail in one pass:  y = q_A(a_A z_A + b_A) + clamp_B( q_B(a_B z_B + b_B) ).  Both operands [P][C]; each has its
 * own batch-norm vectors, eps and k; formula and act_range are shared.  a->clamp must be ALIGNQ_CLAMP_NONE (else ALIGNQ_EINVAL): nothing
 * follows the sum.  The output is bit-identical to two launches of alignq_site_eval_fwd: site b into a temporary, then site a with
 * that temporary as `residual`.                                                                                                  */
int alignq_site_eval_twin_fwd(const alignq_eval_site* a, const alignq_eval_site* b, int64_t P, int C, float act_range, int formula,
                              float* y, void* stream);

/* The depthwise convolution with the site as its epilogue:  y = clamp( q(a_c * dw(x, wq) + b_c) ),  dw = the accumulation of
 * alignq_dwconv3x3_nhwc_fwd (alignq.h: acc = +0, taps in row-major order, taps in the padding skipped, every product and every sum
 * its own fp32 operation), padding 1, stride 1 or 2, wq [C][1][3][3].  x: [B][H_in][W_in][C]; y: [B][H_out][W_out][C] with
 * H_out = (H_in - 1) / stride + 1.  site->z is ignored.  The output is bit-identical to alignq_dwconv3x3_nhwc_fwd followed by
 * alignq_site_eval_fwd; the convolution's output is never written.                                                              */
int alignq_dwconv3x3_site_eval_fwd(const float* x, const float* wq, const alignq_eval_site* site, int B, int H_in, int W_in, int C,
                                   int stride, float act_range, int formula, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_MOBILE_H */

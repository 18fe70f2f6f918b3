/* alignq_pointwise.h - the pointwise (1x1) Conv2d_Q convolutions at MobileNet-V2's widths (csrc/pointwise_kernels.hip; Python:
 * alignq_amd/ops.py QConvPwFn, alignq_amd/mobilenet.py use_hip_convs(model, pointwise=True)).  The entry points link into the same
 * libalignq_hip.so as those of alignq.h and use its error codes.
 *
 * Why a third header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h is the
 * fixed set of the folded evaluation sites.  This extension only ADDS entry points, so it is declared next to them and read by
 * alignq_amd/_lib.py into a table of its own (POINTWISE_SIGNATURES); nothing declared here appears in either other header.
 * alignq_qconv_* (alignq.h) keeps its supported set: channel counts that are multiples of 64.
 *
 * The operation:  F.conv2d(x, W_q) for a (COUT, CIN, 1, 1) filter, stride 1, padding 0, dilation 1, groups 1, no bias, as a GEMM
 * over the M = B * H * W pixels of channels-last fp32 tensors:
 *     forward          y[m][co]   = sum_ci x[m][ci]  * W_q[co][ci]              x: [M][CIN],   y:  [M][COUT]
 *     data gradient    dx[m][ci]  = sum_co dy[m][co] * W_q[co][ci]              dy: [M][COUT], dx: [M][CIN]
 *     filter gradient  dW[co][ci] = sum_m  dy[m][co] * x[m][ci]                 dW: [COUT][CIN]
 *
 * Supported set:  CIN and COUT multiples of 8 in [8, 2048];  M >= 1 with M * max(CIN, COUT) <= 2^31 - 1;  1 <= w_bit <= 8;  every
 * pointer 16-byte aligned.  ALIGNQ_EINVAL: a NULL or misaligned pointer, a w_bit outside 1..8.  ALIGNQ_EUNSUPPORTED: any other
 * shape.  A bad argument is named before an unsupported shape, and both before anything is launched.
 *
 * Arithmetic contract (that of alignq_qconv_* with a general fp32 operand):
 *   * the filter operand is the integer bin b = rint(W_q * n), n = 2^w_bit - 1, |b| <= n <= 255, as bf16 bit patterns in the filter's
 *     own [COUT][CIN] layout: the first output of alignq_qconv_pack_weights (alignq.h), which takes any numel % 4 == 0;
 *   * the fp32 activation (forward) or gradient (data gradient) is split exactly into three bf16 terms v = hi + mid + lo
 *     (hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), round to nearest even); every product bin x term is exact in
 *     fp32 and goes through v_mfma_f32_16x16x32_bf16 with fp32 accumulation: per 32-deep k step the terms lo, mid, hi in that order,
 *     k steps in ascending order, the tail of the last step zero on both operands.  The order is a function of the shape alone;
 *   * the epilogue is ONE fp32 division of the sum by n;
 *   * filter gradient: dy and x are each split into three terms (d0 + d1 + d2, x0 + x1 + x2, leading term first); the SIX leading
 *     pairs are taken, per 32-pixel step in the order (x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0); the pairs (x1,d2), (x2,d1)
 *     and (x2,d2) - below 2^-24 of the leading product - are dropped.  No division (W_q's scale is not part of dW).  The pixels
 *     are cut into n_slabs slabs of whole 32-pixel steps; every slab's sum is stored to `ws` (no atomics, no zero-fill pass) and
 *     the slabs are added in a fixed order by the slab reduction of the other convolutions (csrc/wgrad_reduce_body.h);
 *   * two launches on the same inputs give the same bits, for all three operations.
 * Outputs of 1 MiB to 64 MiB are stored write-through (csrc/store_forms.h); same values, same addresses.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable.           */
#ifndef ALIGNQ_POINTWISE_H
#define ALIGNQ_POINTWISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNQ_PW_FWD 0
#define ALIGNQ_PW_DGRAD 1
#define ALIGNQ_PW_WGRAD 2

/* forward / data gradient: the output-channel width of a workgroup's tile (64 pixels x 16, 32 or 64 channels) */
#define ALIGNQ_PW_FORM_N16 0
#define ALIGNQ_PW_FORM_N32 1
#define ALIGNQ_PW_FORM_N64 2
/* filter gradient: the (CIN x COUT) tile of a workgroup */
#define ALIGNQ_PW_FORM_W32X32 0
#define ALIGNQ_PW_FORM_W64X32 1
#define ALIGNQ_PW_FORM_W32X64 2
#define ALIGNQ_PW_FORM_W64X64 3

/* 1 if (M, CIN, COUT) is in the supported set, else 0 */
int alignq_pwconv_supported(int64_t M, int CIN, int COUT);

/* The launch form the launcher chooses for `op` (ALIGNQ_PW_*) at this shape; -1 for an unknown op or an unsupported shape.
 *   forward / data gradient (N = COUT / CIN, the output width): the widest of the 64-, 32- and 16-channel tiles that pads N by no more
 *   than rounding it up to 16 does - ALIGNQ_PW_FORM_N64 / N32 / N16;
 *   filter gradient: 32 input channels per tile for CIN <= 32, else 64; 32 output channels for COUT <= 32, else 64 -
 *   ALIGNQ_PW_FORM_W{32,64}X{32,64}.                                                                                          */
int alignq_pwconv_form(int op, int64_t M, int CIN, int COUT);

/* y = conv(x, W_q).  w_bins: the filter's bf16 bins [COUT][CIN]. */
int alignq_pwconv_fwd(const float* x, const void* w_bins, float* y, int64_t M, int CIN, int COUT, int w_bit, void* stream);

/* dx = the data gradient; writes exactly M * CIN elements.  w_bins as for the forward (read transposed). */
int alignq_pwconv_dgrad(const float* dy, const void* w_bins, float* dx, int64_t M, int CIN, int COUT, int w_bit, void* stream);

/* bytes of `ws` alignq_pwconv_wgrad needs: n_slabs * COUT * CIN floats (0 for an unsupported shape) */
size_t alignq_pwconv_wgrad_ws_bytes(int64_t M, int CIN, int COUT);

/* dW = the filter gradient.  n_slabs_out == NULL: the slabs are reduced into dw by a second launch.  n_slabs_out != NULL: only the
 * slabs are written, their count is stored there and dw may be NULL: the caller reduces them (alignq_conv3x3_wgrad_reduce_multi,
 * alignq.h), the same sums in the same order.                                                                                  */
int alignq_pwconv_wgrad(const float* x, const float* dy, float* dw, void* ws, int64_t M, int CIN, int COUT, int* n_slabs_out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_POINTWISE_H */

/* alignq_digit.h - the digit-domain DANN's evaluation pass (csrc/digit_eval_kernels.hip; Python: alignq_amd/fused.py
 * k5_site_pool_eval, alignq_amd/digit.py MNISTmodel_quant._forward_eval).  The entry points link into the same libalignq_hip.so as those
 * of alignq.h and use its error codes and formula constants; the site record is alignq_dense_site (alignq_dense.h), the clamp one of
 * alignq_mobile.h's.
 *
 * Why a seventh header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h,
 * alignq_pointwise.h, alignq_k3conv.h, alignq_dense.h and alignq_k5conv.h are fixed sets too.  This extension only ADDS entry points,
 * so it is declared next to them and read by alignq_amd/_lib.py into a table of its own (DIGIT_SIGNATURES, bound last); nothing
 * declared here appears in any other header.
 *
 * In evaluation each half of the reference's `feature` (cdf_alignment/dann_digit/model/dann.py:143-155) is conv 5x5 + bias ->
 * eval-mode batch-norm -> act_q -> (Dropout2d: the identity) -> ReLU -> MaxPool2d(2).  All of it is per channel and elementwise up to
 * the pool, and the forward's 8 x 8 output tile holds every 2 x 2 window whole, so it is the convolution's epilogue:
 *
 * alignq_k5conv_site_pool_eval_fwd:   y = maxpool2( relu( q( a_c * (conv5x5(x, W_q) + bias_c) + b_c ) ) )         ONE launch
 *   * x: [B][H][W][CIN] channels-last fp32 (x_channels == CIN), or - image form only, CIN == 3 - x_channels == 1: a one-channel image
 *     [B][H][W] whose value is used for all three input channels (the reference's `expand`; the expanded copy is never made);
 *   * the convolution is exactly alignq_k5conv_fwd's (alignq_k5conv.h): the same two forms by CIN, w_bins and bias as there, the same
 *     staging, accumulation and term order, ONE division by n = 2^w_bit - 1, then ONE add of the bias; the kernels run the same
 *     main loop (csrc/k5_fwd_body.h);
 *   * the site is exactly alignq_site_eval_fwd's (alignq_mobile.h) with ALIGNQ_CLAMP_RELU over the COUT channels: a_c, b_c formed
 *     inside the launch from the batch-norm vectors of `site` (only READ: no preparing launch, a captured graph stays valid when the
 *     running statistics change), v = (a_c * z) + b_c, the quantiser of alignq_act_quant_fwd (formula, act_range; k == 32: none), the
 *     clamp (NaN and -0 give +0).  site->clamp must be ALIGNQ_CLAMP_RELU: the pool relies on values >= +0;
 *   * the pool is F.max_pool2d(., 2): PH = (H - 4) / 2, PW = (W - 4) / 2 (floor); an odd trailing row or column is dropped.  A lane of
 *     the tile holds pixel (2 wv + (fr >> 3), fr & 7) (fr = lane & 15, wv the wave), so a window is lanes fr, fr ^ 1, fr ^ 8, fr ^ 9 of
 *     one 16-lane row: two DPP exchanges, no LDS; the lane with (fr & 9) == 0 stores;
 *   * out_layout ALIGNQ_DIGIT_OUT_NHWC: y is [B][PH][PW][COUT] (a channels-last (B, COUT, PH, PW) tensor); ALIGNQ_DIGIT_OUT_FLAT_CHW:
 *     y is [B][COUT * PH * PW] in (c, h, w) order, what the reference's view(-1, 768) reads.  Exactly B * PH * PW * COUT floats are
 *     written, the same values in both;
 *   * the result is bit-identical to alignq_k5conv_fwd into a temporary, alignq_site_eval_fwd (ALIGNQ_CLAMP_RELU) and
 *     F.max_pool2d(., 2); the un-pooled tensor is never written;
 *   * supported set: alignq_k5conv_fwd's, and H, W >= 6 (one window); k in 1..16, or 32; 1 <= w_bit <= 8;
 *   * ALIGNQ_EINVAL: a NULL x, w_bins, y, record, running_mean or running_var; x, w_bins or y not 16-byte aligned, bias not 4-byte
 *     aligned; a w_bit outside 1..8; a k outside 1..16 and != 32; a formula neither ALIGNQ_FORMULA_ADMM nor ALIGNQ_FORMULA_CDF; a
 *     clamp other than ALIGNQ_CLAMP_RELU; an unknown out_layout; an x_channels that is neither CIN nor (CIN == 3) 1.
 *     ALIGNQ_EUNSUPPORTED: any other shape.  A bad argument is named before an unsupported shape, both before anything is launched;
 *   * the tile width follows alignq_k5conv_form(ALIGNQ_K5_FWD, ...); at most 2048 spatial tiles are in the grid, the rest go by grid
 *     stride; an output of 1 MiB to 64 MiB (the POOLED bytes) is stored write-through (csrc/store_forms.h);
 *   * only enqueues on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable; two launches on the same
 *     inputs give the same bits.                                                                                                 */
#ifndef ALIGNQ_DIGIT_H
#define ALIGNQ_DIGIT_H

#include <stddef.h>
#include <stdint.h>

#include "alignq_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNQ_DIGIT_OUT_NHWC 0
#define ALIGNQ_DIGIT_OUT_FLAT_CHW 1

/* 1 if (B, H, W, CIN, COUT) - H, W the INPUT's - is in the supported set, else 0 */
int alignq_k5conv_site_pool_eval_supported(int B, int H, int W, int CIN, int COUT);

int alignq_k5conv_site_pool_eval_fwd(const float* x, int x_channels, const void* w_bins, const float* bias, const alignq_dense_site* site,
                                     float* y, int out_layout, int B, int H, int W, int CIN, int COUT, int w_bit, float act_range,
                                     int formula, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_DIGIT_H */

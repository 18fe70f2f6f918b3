/* alignq_k5conv.h - the 5x5 / stride 1 / padding 0 Conv2d_Q convolutions with an optional bias (csrc/k5conv_kernels.hip; Python:
 * alignq_amd/ops.py QConvK5Fn, alignq_amd/digit.py use_hip_convs).  The digit-domain DANN (MNISTmodel_quant: 3 -> 32 at 28 x 28 and
 * 32 -> 48 at 12 x 12) is the first user.  The entry points link into the same libalignq_hip.so as those of alignq.h and use its error
 * codes.
 *
 * Why a sixth header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h,
 * alignq_pointwise.h, alignq_k3conv.h and alignq_dense.h are fixed sets too.  This extension only ADDS entry points, so it is declared
 * next to them and read by alignq_amd/_lib.py into a table of its own (K5CONV_SIGNATURES); nothing declared here appears in any other
 * header.
 *
 * The operation:  F.conv2d(x, W_q, bias, 1, 0) for a (COUT, CIN, 5, 5) filter on channels-last fp32 tensors, the filter channels-last
 * too ([COUT][5][5][CIN] in memory).  H, W are the INPUT's height and width; the output is (H - 4) x (W - 4):
 *     forward          y[b][h][w][co]     = bias[co] + sum_{ky,kx,ci} x[b][h+ky][w+kx][ci]  * W_q[co][ky][kx][ci]
 *     data gradient    dx[b][h][w][ci]    = sum_{ky,kx,co} dy[b][h-ky][w-kx][co] * W_q[co][ky][kx][ci]     (dy zero outside its extent)
 *     filter gradient  dW[co][ky][kx][ci] = sum_{b,h,w}   dy[b][h][w][co] * x[b][h+ky][w+kx][ci]
 * x, dx: [B][H][W][CIN];  y, dy: [B][H-4][W-4][COUT];  dW: [COUT][5][5][CIN];  bias: [COUT] or NULL.  The bias gradient is the
 * caller's (dy summed over b, h, w).
 *
 * Supported set, two forms chosen by CIN:
 *   body form   CIN and COUT multiples of 4 in [4, 512]: all three operations;
 *   image form  CIN == 3, COUT a multiple of 4 in [4, 512]: forward and filter gradient only (a network's first layer; its input
 *               needs no gradient) - alignq_k5conv_dgrad returns ALIGNQ_EUNSUPPORTED;
 *   both        B >= 1, H, W >= 5 with B * H * W * max(CIN, COUT) <= 2^31 - 1;  1 <= w_bit <= 8;  x, y, dy, dx, dW, w_bins, ws 16-byte
 *               aligned, bias 4-byte aligned.
 * ALIGNQ_EINVAL: a NULL (bias excepted) or misaligned pointer, a w_bit outside 1..8.  ALIGNQ_EUNSUPPORTED: any other shape.  A bad
 * argument is named before an unsupported shape, and both before anything is launched.
 *
 * Arithmetic contract (that of alignq_k3conv_*, restated for 25 taps):
 *   * the filter operand is the integer bin b = rint(W_q * n), n = 2^w_bit - 1, |b| <= n <= 255, as bf16 bit patterns in the filter's
 *     own [COUT][5][5][CIN] layout: the first output of alignq_qconv_pack_weights (alignq.h).  The data gradient reads the SAME
 *     bins, flipped and transposed while they are staged; there is no second packed copy;
 *   * the fp32 activation (forward) or gradient (data gradient) is split exactly into three bf16 terms v = hi + mid + lo
 *     (hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), round to nearest even), once per element and channel chunk; every
 *     product bin x term is exact in fp32 and goes through v_mfma_f32_16x16x32_bf16 with fp32 accumulation, in this order:
 *       body form   channel chunks of 32 (of CIN for the forward, of COUT for the data gradient) in ascending order; inside a chunk the
 *                   25 taps in ascending order of the pixel they READ (the forward's (ky, kx) row-major; the data gradient's
 *                   (4 - ky, 4 - kx) row-major, reading dy at (h - 4 + ty, w - 4 + tx)); inside a tap the terms lo, mid, hi;
 *       image form  taps and channels fold into one K: k = ky * 15 + kx * 3 + ci (the filter row's own order), 75 values zero-tailed
 *                   to 96; the three k steps of 32 in ascending order, inside a step the terms lo, mid, hi.
 *     The tail of the last chunk, pixels outside the operand and the rows of a tile beyond the output are zeros.  The order is a
 *     function of the shape alone;
 *   * the epilogue is ONE fp32 division of the sum by n, then ONE fp32 add of bias[co] (forward, bias != NULL);
 *   * filter gradient: dy and x are each split into three terms (d0 + d1 + d2, x0 + x1 + x2, leading term first); the SIX leading
 *     pairs are taken, per 32-pixel step and tap (image form: per step) in the order (x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0);
 *     the pairs (x1,d2), (x2,d1) and (x2,d2) are dropped.  No division.  A step is a spatial tile of 4 rows x 8 columns of OUTPUT
 *     pixels of one image (pixels beyond the output are zeros); the tiles, numbered image by image, row-major, are cut into n_slabs
 *     slabs of whole tiles; every slab's sum is stored to `ws` (no atomics, no zero-fill pass) and the slabs are added in a fixed
 *     order by the slab reduction of the other convolutions (csrc/wgrad_reduce_body.h);
 *   * two launches on the same inputs give the same bits, for all three operations.
 * A footprint is read with the operand's own bounds: never from the neighbouring image or row.
 * Outputs of 1 MiB to 64 MiB are stored write-through (csrc/store_forms.h); same values, same addresses.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable.           */
#ifndef ALIGNQ_K5CONV_H
#define ALIGNQ_K5CONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNQ_K5_FWD 0
#define ALIGNQ_K5_DGRAD 1
#define ALIGNQ_K5_WGRAD 2

/* forward / data gradient, both forms: the output-channel width of a workgroup's tile (8 x 8 pixels x 16, 32 or 64 channels) */
#define ALIGNQ_K5_FORM_N16 0
#define ALIGNQ_K5_FORM_N32 1
#define ALIGNQ_K5_FORM_N64 2
/* filter gradient: the (CIN x COUT) tile of a workgroup; image form: 64 output channels x the 75 folded k */
#define ALIGNQ_K5_FORM_W64X16 0
#define ALIGNQ_K5_FORM_W16X64 1
#define ALIGNQ_K5_FORM_WIMAGE 2

/* 1 if `op` (ALIGNQ_K5_*) at (B, H, W, CIN, COUT) is in the supported set, else 0 (the data gradient of the image form: 0) */
int alignq_k5conv_supported(int op, int B, int H, int W, int CIN, int COUT);

/* The launch form the launcher chooses for `op` at this shape; -1 for an unknown op or an unsupported shape.
 *   forward / data gradient (N = COUT / CIN, the output width): the widest of the 64-, 32- and 16-channel tiles that pads N by no more
 *   than rounding it up to 16 does - ALIGNQ_K5_FORM_N64 / N32 / N16;
 *   filter gradient: CIN == 3: ALIGNQ_K5_FORM_WIMAGE; else 64 input x 16 output channels per workgroup where CIN >= COUT, else
 *   16 x 64 - ALIGNQ_K5_FORM_W64X16 / W16X64. */
int alignq_k5conv_form(int op, int B, int H, int W, int CIN, int COUT);

/* y = conv(x, W_q) + bias.  w_bins: the filter's bf16 bins [COUT][5][5][CIN]; bias: [COUT] or NULL. */
int alignq_k5conv_fwd(const float* x, const void* w_bins, const float* bias, float* y, int B, int H, int W, int CIN, int COUT, int w_bit,
                      void* stream);

/* dx = the data gradient (body form only); writes exactly B * H * W * CIN elements.  w_bins as for the forward. */
int alignq_k5conv_dgrad(const float* dy, const void* w_bins, float* dx, int B, int H, int W, int CIN, int COUT, int w_bit,
                        void* stream);

/* bytes of `ws` alignq_k5conv_wgrad needs: n_slabs * COUT * 25 * CIN floats (0 for an unsupported shape).  With
 * T = B * ceil((H - 4) / 4) * ceil((W - 4) / 8) spatial tiles and C = ceil(CIN / 64) ceil(COUT / 16) (or ceil(CIN / 16) ceil(COUT / 64);
 * image form: ceil(COUT / 64)) channel tiles:  s = max(1, min(ceil(512 / C), ceil(T / 2), 1024)),  per = ceil(T / s),
 * n_slabs = ceil(T / per): no slab is empty. */
size_t alignq_k5conv_wgrad_ws_bytes(int B, int H, int W, int CIN, int COUT);

/* dW = the filter gradient.  n_slabs_out == NULL: the slabs are reduced into dw by a second launch.  n_slabs_out != NULL: only the
 * slabs are written, their count is stored there and dw may be NULL: the caller reduces them (alignq_conv3x3_wgrad_reduce_multi,
 * alignq.h), the same sums in the same order.                                                                                  */
int alignq_k5conv_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H, int W, int CIN, int COUT,
                        int* n_slabs_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_K5CONV_H */

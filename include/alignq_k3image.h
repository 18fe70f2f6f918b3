/* alignq_k3image.h - the 3x3 / stride 1 / padding 1 Conv2d_Q convolution of a 3-channel image (csrc/k3image_kernels.hip; Python:
 * alignq_amd/ops.py QConvK3ImageFn, alignq_amd/fused.py stem_eval_into, alignq_amd/densenet.py use_hip_convs(stem=True)).  The stems
 * of DenseNet-40 (3 -> 24 at 32 x 32) and MobileNet-V2 (3 -> 32) are its shapes.  The entry points link into the same
 * libalignq_hip.so as those of alignq.h and use its error codes.
 *
 * Why an eighth header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h,
 * alignq_pointwise.h, alignq_k3conv.h, alignq_dense.h, alignq_k5conv.h and alignq_digit.h are fixed sets too.  This extension only
 * ADDS entry points, so it is declared next to them and read by alignq_amd/_lib.py into a table of its own (K3IMAGE_SIGNATURES);
 * nothing declared here appears in any other header.
 *
 * The operation:  F.conv2d(x, W_q, None, 1, 1) for a (COUT, 3, 3, 3) filter on channels-last fp32 tensors, the filter channels-last
 * too ([COUT][3][3][3] in memory):
 *     forward          y[b][h][w][co]     = sum_{ky,kx,ci} x[b][h+ky-1][w+kx-1][ci] * W_q[co][ky][kx][ci]      (x zero outside the image)
 *     filter gradient  dW[co][ky][kx][ci] = sum_{b,h,w}   dy[b][h][w][co] * x[b][h+ky-1][w+kx-1][ci]
 * x: [B][H][W][3];  y: y[((b * H + h) * W + w) * ldy + co], the plain channels-last tensor where ldy == COUT, else the first COUT
 * channels of a wider one (a dense block's buffer), whose other channels are not touched;  dy: [B][H][W][COUT], dense;
 * dW: [COUT][3][3][3].  There is no data gradient: the input is the image.
 *
 * Supported set:  COUT a multiple of 4 in [4, 512];  B, H, W >= 1;  ldy a multiple of 4, ldy >= COUT;  B * H * W * ldy <= 2^31 - 1
 * (the filter gradient: B * H * W * COUT);  1 <= w_bit <= 8;  x, y, dy, dW, w_bins, ws 16-byte aligned.
 * ALIGNQ_EINVAL: a NULL or misaligned pointer, a w_bit outside 1..8.  ALIGNQ_EUNSUPPORTED: any other shape or pitch.  A bad argument
 * is named before an unsupported shape, and both before anything is launched.
 *
 * Arithmetic contract (that of alignq_k5conv_*'s image form, restated for nine taps):
 *   * the filter operand is the integer bin b = rint(W_q * n), n = 2^w_bit - 1, |b| <= n <= 255, as bf16 bit patterns in the filter's
 *     own [COUT][3][3][3] layout: the first output of alignq_qconv_pack_weights (alignq.h);
 *   * the fp32 image value is split exactly into three bf16 terms v = hi + mid + lo (hi = bf16(v), mid = bf16(v - hi),
 *     lo = bf16(v - hi - mid), round to nearest even), once per staged element; every product bin x term is exact in fp32 and goes
 *     through v_mfma_f32_16x16x32_bf16 with fp32 accumulation;
 *   * taps and channels fold into one K: k = ky * 9 + kx * 3 + ci (the filter row's own order), 27 values zero-tailed to 32: ONE k
 *     step; inside the step the terms lo, mid, hi.  Padding pixels and the rows and columns of a tile beyond the image are zeros
 *     on the activation operand and are never read from memory: not from the neighbouring image, not from the neighbouring row.
 *     The order is a function of the shape alone; which workgroup computes a tile changes no value;
 *   * the epilogue is ONE fp32 division of the sum by n;
 *   * filter gradient: dy and x are each split into three terms (d0 + d1 + d2, x0 + x1 + x2, leading term first); the SIX leading
 *     pairs are taken per 32-pixel step in the order (x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0); the pairs (x1,d2), (x2,d1) and
 *     (x2,d2) are dropped.  No division.  A step is a spatial tile of 4 rows x 8 columns of pixels of one image (pixels beyond the
 *     image are zeros); the tiles, numbered image by image, row-major, are cut into n_slabs slabs of whole tiles; every slab's sum
 *     is stored to `ws` (no atomics, no zero-fill pass) and the slabs are added in a fixed order by the slab reduction of the other
 *     convolutions (csrc/wgrad_reduce_body.h);
 *   * two launches on the same inputs give the same bits.
 * Outputs of 1 MiB to 64 MiB are stored write-through (csrc/store_forms.h); same values, same addresses.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable.           */
#ifndef ALIGNQ_K3IMAGE_H
#define ALIGNQ_K3IMAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNQ_K3I_FWD 0
#define ALIGNQ_K3I_WGRAD 1

/* forward: the output-channel width of a workgroup's tile (8 x 8 pixels x 16, 32 or 64 channels) */
#define ALIGNQ_K3I_FORM_N16 0
#define ALIGNQ_K3I_FORM_N32 1
#define ALIGNQ_K3I_FORM_N64 2
/* filter gradient: 64 output channels x the 27 folded k per workgroup */
#define ALIGNQ_K3I_FORM_WIMAGE 3

/* 1 if `op` (ALIGNQ_K3I_*) at (B, H, W, COUT) is in the supported set (with ldy == COUT), else 0 */
int alignq_k3image_supported(int op, int B, int H, int W, int COUT);

/* The launch form the launcher chooses for `op` at this shape; -1 for an unknown op or an unsupported shape.
 *   forward: the widest of the 64-, 32- and 16-channel tiles that pads COUT by no more than rounding it up to 16 does -
 *   ALIGNQ_K3I_FORM_N64 / N32 / N16;  filter gradient: ALIGNQ_K3I_FORM_WIMAGE. */
int alignq_k3image_form(int op, int B, int H, int W, int COUT);

/* y = conv(x, W_q) at the pitch ldy.  w_bins: the filter's bf16 bins [COUT][3][3][3]. */
int alignq_k3image_fwd(const float* x, const void* w_bins, float* y, int B, int H, int W, int COUT, int ldy, int w_bit, void* stream);

/* bytes of `ws` alignq_k3image_wgrad needs: n_slabs * COUT * 27 floats (0 for an unsupported shape).  With
 * T = B * ceil(H / 4) * ceil(W / 8) spatial tiles and C = ceil(COUT / 64) channel tiles:
 * s = max(1, min(ceil(512 / C), ceil(T / 2), 1024)),  per = ceil(T / s),  n_slabs = ceil(T / per): no slab is empty. */
size_t alignq_k3image_wgrad_ws_bytes(int B, int H, int W, int COUT);

/* dW = the filter gradient.  n_slabs_out == NULL: the slabs are reduced into dw by a second launch.  n_slabs_out != NULL: only the
 * slabs are written, their count is stored there and dw may be NULL: the caller reduces them (alignq_conv3x3_wgrad_reduce_multi,
 * alignq.h), the same sums in the same order.                                                                                  */
int alignq_k3image_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H, int W, int COUT, int* n_slabs_out,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_K3IMAGE_H */

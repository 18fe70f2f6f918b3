/* alignq_k3conv.h - the 3x3 / stride 1 / padding 1 Conv2d_Q convolutions at ANY channel count that is a multiple of 4
 * (csrc/k3conv_kernels.hip; Python: alignq_amd/ops.py QConvK3Fn, alignq_amd/densenet.py use_hip_convs).  DenseNet-40's dense layers
 * (CIN = 24, 36, ..., 444 -> COUT = 12) are the first user.  The entry points link into the same libalignq_hip.so as those of
 * alignq.h and use its error codes.
 *
 * Why a fourth header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h and
 * alignq_pointwise.h are fixed sets too.  This extension only ADDS entry points, so it is declared next to them and read by
 * alignq_amd/_lib.py into a table of its own (K3CONV_SIGNATURES); nothing declared here appears in any other header.
 * alignq_conv3x3_nhwc keeps its set (16, 32, 64 channels at widths 32, 16, 8), alignq_qconv_* its own (multiples of 64).
 *
 * The operation:  F.conv2d(x, W_q, None, 1, 1) for a (COUT, CIN, 3, 3) filter on channels-last fp32 tensors, the filter
 * channels-last too ([COUT][3][3][CIN] in memory); tap (ky, kx) reads the input pixel (h + ky - 1, w + kx - 1), zero outside the image:
 *     forward          y[b][h][w][co]    = sum_{ky,kx,ci} x[b][h+ky-1][w+kx-1][ci]  * W_q[co][ky][kx][ci]
 *     data gradient    dx[b][h][w][ci]   = sum_{ky,kx,co} dy[b][h-ky+1][w-kx+1][co] * W_q[co][ky][kx][ci]
 *     filter gradient  dW[co][ky][kx][ci] = sum_{b,h,w}   dy[b][h][w][co] * x[b][h+ky-1][w+kx-1][ci]
 * x, dx: [B][H][W][CIN];  y, dy: [B][H][W][COUT];  dW: [COUT][3][3][CIN].
 *
 * Supported set:  CIN and COUT multiples of 4 in [4, 512];  B, H, W >= 1 with B * H * W * max(CIN, COUT) <= 2^31 - 1;
 * 1 <= w_bit <= 8;  every pointer 16-byte aligned.  ALIGNQ_EINVAL: a NULL or misaligned pointer, a w_bit outside 1..8.
 * ALIGNQ_EUNSUPPORTED: any other shape.  A bad argument is named before an unsupported shape, and both before anything is launched.
 *
 * Arithmetic contract (that of alignq_pwconv_*, restated for nine taps):
 *   * the filter operand is the integer bin b = rint(W_q * n), n = 2^w_bit - 1, |b| <= n <= 255, as bf16 bit patterns in the filter's
 *     own [COUT][3][3][CIN] layout: the first output of alignq_qconv_pack_weights (alignq.h).  The data gradient reads the SAME
 *     bins, flipped and transposed while they are staged; there is no second packed copy;
 *   * the fp32 activation (forward) or gradient (data gradient) is split exactly into three bf16 terms v = hi + mid + lo
 *     (hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), round to nearest even), once per element and channel chunk; every
 *     product bin x term is exact in fp32 and goes through v_mfma_f32_16x16x32_bf16 with fp32 accumulation, in this order:
 *         channel chunks of 32 (of CIN for the forward, of COUT for the data gradient) in ascending order;
 *         inside a chunk the nine taps in ascending order of the pixel they READ: (-1,-1), (-1,0), (-1,+1), (0,-1) ... (+1,+1)
 *         (the forward's (ky, kx) row-major; the data gradient's (2 - ky, 2 - kx) row-major);
 *         inside a tap the terms lo, mid, hi.
 *     The tail of the last chunk, the pixels outside the image (the padding) and the rows of a tile beyond the image are zeros on
 *     both operands.  The order is a function of the shape alone;
 *   * the epilogue is ONE fp32 division of the sum by n;
 *   * filter gradient: dy and x are each split into three terms (d0 + d1 + d2, x0 + x1 + x2, leading term first); the SIX leading
 *     pairs are taken, per 32-pixel step and tap in the order (x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0); the pairs (x1,d2),
 *     (x2,d1) and (x2,d2) - below 2^-24 of the leading product - are dropped.  No division (W_q's scale is not part of dW).  A step
 *     is a spatial tile of 4 rows x 8 columns of one image (pixels beyond the image are zeros); the tiles, numbered image by image,
 *     row-major, are cut into n_slabs slabs of whole tiles; every slab's sum is stored to `ws` (no atomics, no zero-fill pass) and
 *     the slabs are added in a fixed order by the slab reduction of the other convolutions (csrc/wgrad_reduce_body.h);
 *   * two launches on the same inputs give the same bits, for all three operations.
 * A halo is read with the image's own bounds: never from the neighbouring image or row.
 * Outputs of 1 MiB to 64 MiB are stored write-through (csrc/store_forms.h); same values, same addresses.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state, hipGraph-capturable.           */
#ifndef ALIGNQ_K3CONV_H
#define ALIGNQ_K3CONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNQ_K3_FWD 0
#define ALIGNQ_K3_DGRAD 1
#define ALIGNQ_K3_WGRAD 2

/* forward / data gradient: the output-channel width of a workgroup's tile (8 x 8 pixels x 16, 32 or 64 channels) */
#define ALIGNQ_K3_FORM_N16 0
#define ALIGNQ_K3_FORM_N32 1
#define ALIGNQ_K3_FORM_N64 2
/* filter gradient: the (CIN x COUT) tile of a workgroup */
#define ALIGNQ_K3_FORM_W64X16 0
#define ALIGNQ_K3_FORM_W16X64 1

/* 1 if (B, H, W, CIN, COUT) is in the supported set, else 0 */
int alignq_k3conv_supported(int B, int H, int W, int CIN, int COUT);

/* The launch form the launcher chooses for `op` (ALIGNQ_K3_*) at this shape; -1 for an unknown op or an unsupported shape.
 *   forward / data gradient (N = COUT / CIN, the output width): the widest of the 64-, 32- and 16-channel tiles that pads N by no more
 *   than rounding it up to 16 does - ALIGNQ_K3_FORM_N64 / N32 / N16 (N = 12: a 16-wide tile, one quarter of it idle);
 *   filter gradient: 64 input x 16 output channels per workgroup where CIN >= COUT, else 16 x 64 - ALIGNQ_K3_FORM_W64X16 / W16X64. */
int alignq_k3conv_form(int op, int B, int H, int W, int CIN, int COUT);

/* y = conv(x, W_q).  w_bins: the filter's bf16 bins [COUT][3][3][CIN]. */
int alignq_k3conv_fwd(const float* x, const void* w_bins, float* y, int B, int H, int W, int CIN, int COUT, int w_bit, void* stream);

/* dx = the data gradient; writes exactly B * H * W * CIN elements.  w_bins as for the forward (read flipped and transposed). */
int alignq_k3conv_dgrad(const float* dy, const void* w_bins, float* dx, int B, int H, int W, int CIN, int COUT, int w_bit,
                        void* stream);

/* bytes of `ws` alignq_k3conv_wgrad needs: n_slabs * COUT * 9 * CIN floats (0 for an unsupported shape).  With
 * T = B * ceil(H / 4) * ceil(W / 8) spatial tiles and C = ceil(CIN / 64) ceil(COUT / 16) (or ceil(CIN / 16) ceil(COUT / 64)) channel
 * tiles:  s = max(1, min(ceil(512 / C), ceil(T / 2), 1024)),  per = ceil(T / s),  n_slabs = ceil(T / per): no slab is empty. */
size_t alignq_k3conv_wgrad_ws_bytes(int B, int H, int W, int CIN, int COUT);

/* dW = the filter gradient.  n_slabs_out == NULL: the slabs are reduced into dw by a second launch.  n_slabs_out != NULL: only the
 * slabs are written, their count is stored there and dw may be NULL: the caller reduces them (alignq_conv3x3_wgrad_reduce_multi,
 * alignq.h), the same sums in the same order.                                                                                  */
int alignq_k3conv_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H, int W, int CIN, int COUT,
                        int* n_slabs_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_K3CONV_H */

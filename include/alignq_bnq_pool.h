/* alignq_bnq_pool.h - training-mode batch-norm folded into the plain quantiser, a ReLU and a 2 x 2 max-pool: the two sites of the
 * digit-domain DANN in training (csrc/bnq_pool_kernels.hip; Python: alignq_amd/fused.py BNQuantPoolFn / bn_act_pool, alignq_amd/digit.py
 * with the `fuse_train_sites` flag).  The entry points link into the same libalignq_hip.so as those of alignq.h and use its error
 * codes and formula constants.
 *
 * Why a tenth header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h,
 * alignq_pointwise.h, alignq_k3conv.h, alignq_dense.h, alignq_k5conv.h, alignq_digit.h, alignq_k3image.h and alignq_bnq_any.h are fixed
 * sets too.  This extension only ADDS entry points, so it is declared next to them and read by alignq_amd/_lib.py into a table of its
 * own (BNQPOOL_SIGNATURES); nothing declared here appears in any other header.
 *
 * The operation, on one channels-last fp32 tensor z[B][H][W][C] with H and W even:
 *     y[B][H/2][W/2][C] = maxpool2x2( relu( q( BatchNorm2d.train()(z) ) ) )
 * the chain the reference writes as modules 1-4 and 6-10 of the `feature` Sequential in cdf_alignment/dann_digit/model/dann.py
 * (MNISTmodel_quant: BatchNorm2d -> act_q -> [Dropout2d ->] ReLU -> MaxPool2d(2); Dropout2d is NOT part of this operation: the caller
 * applies it to the pooled y, which gives the same values, alignq_amd/digit.py).  alignq_bnq_any_fwd / _bwd (alignq_bnq_any.h) with
 * ALIGNQ_CLAMP_RELU are the chain without the pool; their y is un-pooled and their mask has no pool selection.  Here the un-pooled
 * y and the un-pooled gradient never exist.
 *
 * Supported set:  C % 4 == 0, 4 <= C <= 1024;  H, W even and >= 2;  2 <= P = B * H * W <= 2^40.  ALIGNQ_EINVAL: a NULL or not 16-byte
 * aligned z, y, g, dz, code or ws; a NULL ab or save; B, H or W < 1 or P < 2; k outside 1..16 and != 32; an unknown formula.
 * ALIGNQ_EUNSUPPORTED: a C outside the set, an odd H or W, or P > 2^40 (the checks run in this order: a bad argument is named
 * before an unsupported shape).  A refusal is returned before anything is launched: nothing is written.
 *
 * Arithmetic (every operation rounded on its own unless written as fma):
 *   statistics, finalisation   those of alignq_bnq_any_fwd over the P un-pooled pixels (alignq_bnq_any.h, "Arithmetic" and "Order": the
 *                same kernels, csrc/bnq_any_body.h): ab, save, running_mean, running_var and num_batches_tracked are bit-equal to
 *                what alignq_bnq_any_fwd writes for the same z
 *   forward      at each of a window's four positions  x = fma(a, z, b);  v = the quantiser of alignq_act_quant_fwd (k, act_range,
 *                formula) on x;  u = v > 0 ? v : +0  (alignq_bnq_any_fwd with ALIGNQ_CLAMP_RELU);  y = the FIRST maximum of the four
 *                u in the order (0,0), (0,1), (1,0), (1,1) (a later position wins only if it is strictly greater): the element
 *                F.max_pool2d's backward routes to
 *   backward     at the selected position  x as above;  dx = gm * ((r * 2/sqrt(2 pi)) * __expf((-0.5f * x) * x)),  gm = g where the pass
 *                bit is set, else 0;  at the other three positions dx = +0;  zhat = (z - mean) * invstd;
 *                k0 = f32(sum dx / P), k1 = f32(sum dx * zhat / P): sums in double over the POOLED elements only (the other three
 *                quarters of the window add exact zeros), divided by the full P;  dbeta = f32(sum dx);  dgamma = f32(sum dx * zhat);
 *                dz = a * ((dx - k0) - zhat * k1) at all four positions
 * The backward reads g, z and the code, never y.
 *
 * The code: one byte per pooled element, laid out like y (code[B][H/2][W/2][C], byte index == element index of y):
 *     bits 0-1  the window position of the first maximum, 2 * dy + dx   (0: (0,0), 1: (0,1), 2: (1,0), 3: (1,1))
 *     bit  2    "the gradient passes": y > 0
 *     bits 3-7  0
 *
 * Order: three launches each way and no atomics.
 *   forward   the two statistics launches of alignq_bnq_any_fwd with P = B * H * W, then one launch in which a thread owns one channel
 *             quad of one pooled pixel
 *   backward  with PP = P / 4 pooled pixels, lanes per pixel L = C / 4, the block size NT and slots = floor(NT / L) of alignq_bnq_any.h,
 *                 n = clamp(floor(PP / (4 * slots)), 1, min(256, floor(4 MiB / (16 C))));  per = ceil(PP / n);  parts = ceil(PP / per)
 *             workgroup w sums pooled pixels [w * per, min((w + 1) * per, PP)) in the order b, h/2, w/2: slot t takes pixels t,
 *             t + slots, ... of the range in ascending order, the slots are added in slot order, and one thread per channel adds
 *             the partials in index order; then one launch in which a thread owns one channel quad of one window.
 * All of it is a function of (B, H, W, C) alone, so two launches on the same inputs give the same bits.
 * A y or dz of 1 MiB to 64 MiB is stored write-through (csrc/store_forms.h); same values, same addresses.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state.                                 */
#ifndef ALIGNQ_BNQ_POOL_H
#define ALIGNQ_BNQ_POOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if (B, H, W, C) is in the supported set, else 0 */
int alignq_bnq_pool_supported(int64_t B, int H, int W, int C);

/* bytes of `ws` both directions need: max(forward partials, backward partials) * C * 2 doubles + 2 * C floats (k0 | k1); 0 for an
 * unsupported shape */
size_t alignq_bnq_pool_ws_bytes(int64_t B, int H, int W, int C);

/* bytes of the code: B * (H / 2) * (W / 2) * C; 0 for an unsupported shape */
size_t alignq_bnq_pool_code_bytes(int64_t B, int H, int W, int C);

/* gamma / beta: [C] or NULL = 1 / 0.  running_mean, running_var, num_batches_tracked: updated in place; any of the three may be
 * NULL.  ab, save: [2][C] outputs the backward takes.  y: [B][H/2][W/2][C].  code: alignq_bnq_pool_code_bytes bytes. */
int alignq_bnq_pool_fwd(const float* z, int64_t B, int H, int W, int C, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, float momentum, float bn_eps, int k, float act_range,
                        int formula, float* ab, float* save, float* y, void* code, void* ws, void* stream);

/* g: the gradient of y, [B][H/2][W/2][C].  dz: [B][H][W][C].  dgamma / dbeta: [C] or NULL.  dz must not alias g or z. */
int alignq_bnq_pool_bwd(const float* g, const float* z, const void* code, const float* ab, const float* save, int64_t B, int H, int W,
                        int C, float act_range, float* dz, float* dgamma, float* dbeta, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_BNQ_POOL_H */

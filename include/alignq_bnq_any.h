/* alignq_bnq_any.h - training-mode batch-norm folded into the plain quantiser and a clamp at ANY channel count C % 4 == 0
 * (csrc/bnq_any_kernels.hip; Python: alignq_amd/fused.py BNQuantAnyFn / bn_act_any, alignq_amd/densenet.py with the
 * `fuse_train_sites` flag).  The entry points link into the same libalignq_hip.so as those of alignq.h and use its error codes and
 * formula constants; the clamps are alignq_mobile.h's ALIGNQ_CLAMP_NONE / _RELU / _RELU6.
 *
 * Why a ninth header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION; alignq_mobile.h,
 * alignq_pointwise.h, alignq_k3conv.h, alignq_dense.h, alignq_k5conv.h, alignq_digit.h and alignq_k3image.h are fixed sets too.  This
 * extension only ADDS entry points, so it is declared next to them and read by alignq_amd/_lib.py into a table of its own
 * (BNQANY_SIGNATURES); nothing declared here appears in any other header.
 *
 * The operation, on one channels-last fp32 tensor viewed as z[P][C] (P = B * H * W pixels, channels fastest):
 *     y = clamp( q( BatchNorm2d.train()(z) ) )
 * the site the reference writes as three modules: cdf_alignment/mobilenet-v2-svhn/model/mobilenetV2.py:55-69 (a block's bn -> act_q ->
 * ReLU6, its bn3 -> act_q3 and the shortcut's bn -> act_skip -> ReLU) and :114-125 (stem and head), and
 * cdf_alignment/dense-cifar-10/model/densenet.py:31-34, :56-59, :148-150 (bn1 -> act_q0 -> relu of a dense layer, a transition, the head).
 * alignq_bnq_fwd / _bwd (alignq.h) are the same chain at C = 4 * 2^j; at such a C with ALIGNQ_CLAMP_RELU both families give the same bits.
 *
 * Supported set:  C % 4 == 0, 4 <= C <= 2048;  2 <= P <= 2^40.  No groups, no residual operand, no level-index output, no
 * statistics handed in.  ALIGNQ_EINVAL: a NULL or not 16-byte aligned z, y, g, dz or ws; a NULL ab or save; P < 2; k outside 1..16
 * and != 32; an unknown formula or clamp; a mask given with ALIGNQ_CLAMP_NONE or missing with a clamp.  ALIGNQ_EUNSUPPORTED: a C
 * outside the set, or P > 2^40 (P < 2 is ALIGNQ_EINVAL, above; the checks run in this order).  A refusal is returned before anything is launched: nothing is written.
 *
 * Arithmetic (that of alignq_bnq_fwd / _bwd, operation for operation; every operation rounded on its own unless written as fma):
 *   statistics   s = sum z, q = sum z^2 over the pixels, in double, in a fixed order (see "Order" below)
 *   finalisation mean = s / P;  var = max(q / P - mean * mean, 0);  invstd = f32(1 / sqrt(var + f64(bn_eps)))          (double)
 *                a = gamma * invstd;  b = beta - f32(mean) * a                                                         (float)
 *                running_mean = (1 - m) * running_mean + m * f32(mean);  running_var = (1 - m) * running_var + m * f32(var * P / (P - 1))
 *                num_batches_tracked += 1;  ab = [a | b], save = [f32(mean) | invstd], both [2][C]
 *   forward      x = fma(a, z, b);  v = the quantiser of alignq_act_quant_fwd (k, act_range, formula) on x;
 *                y = v (NONE);  v > 0 ? v : +0 (RELU);  v > 0 ? (v < 6 ? v : 6) : +0 (RELU6)
 *                mask bit = "the gradient passes":  y > 0 (RELU),  0 < y < 6 (RELU6)
 *   backward     x as above;  dx = gm * ((r * 2/sqrt(2 pi)) * __expf((-0.5f * x) * x)),  gm = g where the mask bit is set (or there is
 *                no clamp), else 0;  zhat = (z - mean) * invstd;  k0 = f32(sum dx / P), k1 = f32(sum dx * zhat / P), sums in double;
 *                dz = a * ((dx - k0) - zhat * k1);  dbeta = f32(sum dx);  dgamma = f32(sum dx * zhat)
 * The backward reads g, z and the mask, never y.
 *
 * The mask (alignq_bnq_fwd's layout): with i the index of a float4 of the flat tensor, every chunk of 64 consecutive float4 has four
 * 64-bit words, one per float4 component; bit (i & 63) of word 4 * (i >> 6) + component.  Bits beyond the tensor are 0.
 *
 * Order: three launches each way and no atomics.  Lanes per pixel L = C / 4 (C <= 1024) or ceil(C / 8) (above: a thread owns two
 * channel quads); the reduction's block size NT is the first of 256, 192, 128, 320, 384, 448, 512 with the largest floor(NT / L) * L / NT,
 * slots = floor(NT / L).  The number of partials is
 *     n = clamp(floor(P / (8 * slots)), 1, min(256, floor(4 MiB / (16 C))));  per = ceil(P / n);  parts = ceil(P / per)
 * workgroup w sums pixels [w * per, min((w + 1) * per, P)): slot t takes pixels t, t + slots, ... of the range in ascending order, the
 * slots are added in slot order, and one thread per channel adds the partials in index order.  All of it is a function of (P, C)
 * alone, so two launches on the same inputs give the same bits.
 * Outputs of 1 MiB to 64 MiB are stored write-through (csrc/store_forms.h); same values, same addresses.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state.                                 */
#ifndef ALIGNQ_BNQ_ANY_H
#define ALIGNQ_BNQ_ANY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if (P, C) is in the supported set, else 0 */
int alignq_bnq_any_supported(int64_t P, int C);

/* bytes of `ws` both directions need: parts * C * 2 doubles (the partials) + 2 * C floats (k0 | k1); 0 for an unsupported (P, C) */
size_t alignq_bnq_any_ws_bytes(int64_t P, int C);

/* bytes of the mask: 32 * ceil(P * C / 256); 0 for an unsupported (P, C) */
size_t alignq_bnq_any_mask_bytes(int64_t P, int C);

/* gamma / beta: [C] or NULL = 1 / 0.  running_mean, running_var, num_batches_tracked: updated in place; any of the three may be
 * NULL.  ab, save: [2][C] outputs the backward takes.  mask: alignq_bnq_any_mask_bytes bytes, NULL exactly with ALIGNQ_CLAMP_NONE. */
int alignq_bnq_any_fwd(const float* z, int64_t P, int C, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, float momentum, float bn_eps, int k, float act_range,
                       int formula, int clamp, float* ab, float* save, float* y, void* mask, void* ws, void* stream);

/* g: the gradient of y.  dgamma / dbeta: [C] or NULL.  dz must not alias g or z. */
int alignq_bnq_any_bwd(const float* g, const float* z, const void* mask, const float* ab, const float* save, int64_t P, int C,
                       float act_range, int clamp, float* dz, float* dgamma, float* dbeta, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_BNQ_ANY_H */

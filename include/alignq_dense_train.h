/* alignq_dense_train.h - DenseNet's dense blocks in TRAINING without concatenations (csrc/dense_train_kernels.hip; Python:
 * alignq_amd/fused.py DenseBlockFn, alignq_amd/densenet.py with the `fuse_dense_train` flag).  The entry points link into the same
 * libalignq_hip.so as those of alignq.h and use its error codes and formula constants.
 *
 * Why an eleventh header: alignq.h is the core C ABI with a fixed set of entry points and ALIGNQ_ABI_VERSION, and the nine headers
 * added since are fixed sets too.  This extension only ADDS entry points, so it is declared next to them and read by
 * alignq_amd/_lib.py into a table of its own (DENSETRAIN_SIGNATURES); nothing declared here appears in any other header.
 *
 * The memory-efficient dense block: ONE channels-last fp32 buffer [B][H][W][C_end] per block and one gradient buffer G of the same
 * shape.  Pixel p of an operand "at a pitch ld" lies at base + p * ld floats.  Layer i (bn1 -> act_q0 -> ReLU -> 3x3 Conv2d_Q,
 * cdf_alignment/dense-cifar-10/model/densenet.py:31-41) reads the first CIN channels of every pixel and writes its COUT channels
 * right behind them; the quantised activation y and the ReLU mask are never written: the backward forms them again from the buffer,
 * which still holds every layer's z.  Every entry point reproduces an existing launch BIT FOR BIT on a contiguous copy:
 *
 *   alignq_dense_train_stats      the statistics and finalisation launches of alignq_bnq_any_fwd (alignq_bnq_any.h, "Arithmetic" and
 *                                 "Order": same partition, block size, slot order and partial count for (P, C)): ab, save, the running
 *                                 statistics and the counter.  No y, no mask.
 *   alignq_dense_train_layer_fwd  alignq_bnq_any_fwd(.., ALIGNQ_CLAMP_RELU) into a temporary + alignq_k3conv_fwd, as ONE launch: the
 *                                 kernel of alignq_dense_layer_eval_fwd (alignq_dense.h) with the [2][CIN] table read from `ab` and
 *                                 the site's training statement x = fma(a, z, b).  Padding, tile tail and chunk tail are zeros stored
 *                                 BEHIND the site.  x and y may lie in one buffer on disjoint channel ranges.
 *   alignq_dense_train_dgrad      alignq_k3conv_dgrad with dy read at a pitch; gy is dense [P][CIN].
 *   alignq_dense_train_wgrad      alignq_k3conv_wgrad(y, dy, ..) with y = relu(q(fma(a, z, b))) formed while the 6 x 10 halo tile is
 *                                 staged, z and dy at a pitch: the same six term pairs in the same order, the slab geometry of
 *                                 alignq_k3conv_wgrad_ws_bytes, the same slab reduction (or, with n_slabs_out, deferred to the caller).
 *   alignq_dense_train_site_bwd   the three launches of alignq_bnq_any_bwd (sums, finalisation, apply) with gy dense, z at a pitch
 *                                 and the gate relu(q(fma(a, z, b))) > 0 formed again instead of read from a mask; the apply pass
 *                                 ACCUMULATES: G[p][c] = G[p][c] + dz[p][c] for c < C, one fp32 add per element, G at a pitch.
 *                                 dgamma, dbeta and dz have alignq_bnq_any_bwd's bits.
 *
 * Supported set: CIN, COUT (C) % 4 == 0 in [4, 512]; pitches % 4 == 0 and no smaller than the width read or written; pixels * the
 * largest pitch of the call <= 2^31 - 1; w_bit 1..8; k 1..16; both formulas; the ReLU clamp only.
 * ALIGNQ_EINVAL: a NULL or not 16-byte aligned tensor operand or ws; a NULL ab or save; a bad pitch, w_bit, k or formula; P < 2
 * (stats, site_bwd); dw and n_slabs_out both NULL.  ALIGNQ_EUNSUPPORTED: a shape outside the set.  ALIGNQ_EINVAL is named first,
 * and a refusal is returned before anything is launched: nothing is written.
 * The entry points only enqueue on `stream`: no allocation, no synchronisation, no global state, no atomics; two launches on the
 * same inputs give the same bits.                                                                                                  */
#ifndef ALIGNQ_DENSE_TRAIN_H
#define ALIGNQ_DENSE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if a layer (B, H, W, CIN -> COUT) in a buffer of pitch ld is in the supported set, else 0 */
int alignq_dense_train_supported(int B, int H, int W, int CIN, int COUT, int ld);

/* bytes of `ws` of _stats and _site_bwd: alignq_bnq_any_ws_bytes(P, C); 0 for an unsupported (P, C) */
size_t alignq_dense_train_site_ws_bytes(int64_t P, int C);

/* bytes of `ws` of _wgrad: alignq_k3conv_wgrad_ws_bytes(B, H, W, CIN, COUT); 0 for an unsupported shape */
size_t alignq_dense_train_wgrad_ws_bytes(int B, int H, int W, int CIN, int COUT);

/* z: the first C channels of P pixels at pitch ld.  gamma / beta: [C] or NULL = 1 / 0.  running_mean, running_var,
 * num_batches_tracked: updated in place; any of the three may be NULL.  ab, save: [2][C] outputs. */
int alignq_dense_train_stats(const float* z, int ld, int64_t P, int C, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, int64_t* num_batches_tracked, float momentum, float bn_eps, float* ab, float* save,
                             void* ws, void* stream);

/* y[p][0..COUT) = conv3x3(relu(q(fma(a, x, b))))[p], x at pitch ldx (CIN channels), y at pitch ldy; ab: [2][CIN] of _stats;
 * w_bins: the filter's bf16 bins [COUT][3][3][CIN] (alignq_qconv_pack_weights) */
int alignq_dense_train_layer_fwd(const float* x, int ldx, float* y, int ldy, const float* ab, const void* w_bins, int B, int H, int W,
                                 int CIN, int COUT, int w_bit, int k, float act_range, int formula, void* stream);

/* gy: dense [P][CIN]; dy: COUT channels at pitch lddy */
int alignq_dense_train_dgrad(const float* dy, int lddy, const void* w_bins, float* gy, int B, int H, int W, int CIN, int COUT,
                             int w_bit, void* stream);

/* dw: [COUT][3][3][CIN] or NULL with n_slabs_out (the caller reduces the slabs in ws: alignq_conv3x3_wgrad_reduce_multi) */
int alignq_dense_train_wgrad(const float* z, int ldz, const float* ab, const float* dy, int lddy, float* dw, void* ws, int B, int H,
                             int W, int CIN, int COUT, int k, float act_range, int formula, int* n_slabs_out, void* stream);

/* gy: dense [P][C], the gradient of the layer's quantised activation.  G: the block's gradient buffer at pitch ldg, its first C
 * channels updated in place; must not alias gy or z.  dgamma / dbeta: [C] or NULL. */
int alignq_dense_train_site_bwd(const float* gy, const float* z, int ldz, const float* ab, const float* save, float* G, int ldg,
                                int64_t P, int C, int k, float act_range, int formula, float* dgamma, float* dbeta, void* ws,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNQ_DENSE_TRAIN_H */

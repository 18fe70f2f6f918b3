// filter_image.h — the scatter of one quantised filter element into its two pre-packed bf16 filter images (include/alignq.h,
// alignq_weight_quant_fwd_multi_img; DESIGN.md, "Filter images"), shared by every launch that forms W_q: the weight quantiser
// (multi_tensor_kernels.hip) and the unpacking of k-bit weight codes (pack_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/alignq.h"

namespace alignq {

// Pre-packed bf16 filter images for the convolutions of conv_kernels.hip: the integer bins b = (__bf16) rintf(W_q * (2^k - 1)) of a
// channels-last filter [CO][KK][CI], laid out so that a wave's A fragment of one k step is one contiguous 1 KB (16 bytes per lane).
// Two images back to back: F[CO/16][NSF][64][8] (forward: k = (tap, ci)) and D[CI/16][NSD][64][8] (data gradient: k = (tap', co),
// tap' = KK - 1 - tap when `flip`).  Written by the launch that forms W_q, from the register that is stored to q; the padding slots
// (k steps past the last tap) are written as +0 by the threads that hold the last tap, so nothing depends on what the buffer held
// before.
constexpr int kImgMaxC = 1023, kImgMaxKK = 255;

__device__ __forceinline__ long img_slot(int row, int kk, int ns) {
  return ((((long)(row >> 4) * ns + (kk >> 5)) * 64 + ((kk >> 3) & 3) * 16 + (row & 15)) << 3) + (kk & 7);
}

// geo: CO | CI << 10 | KK << 20 | flip << 28 (img_geo_word)
__device__ __forceinline__ void img_store(unsigned short* __restrict__ img, unsigned geo, long i, float qv, float nlev) {
  const int CO = geo & 1023, CI = (geo >> 10) & 1023, KK = (geo >> 20) & 255;
  const bool flip = (geo >> 28) & 1;
  const int ci = (int)(i % CI), r = (int)(i / CI), t = r % KK, co = r / KK;
  const unsigned short b = __builtin_bit_cast(unsigned short, (__bf16)rintf(qv * nlev));
  const int nsf = (KK * CI + 31) >> 5, nsd = (KK * CO + 31) >> 5;
  img[img_slot(co, t * CI + ci, nsf)] = b;
  if (t == KK - 1 && ci < 32 * nsf - KK * CI) img[img_slot(co, KK * CI + ci, nsf)] = 0;
  unsigned short* __restrict__ D = img + (long)(CO >> 4) * nsf * 512;
  const int td = flip ? KK - 1 - t : t;
  D[img_slot(ci, td * CO + co, nsd)] = b;
  if (td == KK - 1 && co < 32 * nsd - KK * CO) D[img_slot(ci, KK * CO + co, nsd)] = 0;
}

// host: the packed geometry word of a geom row {CO, KK, CI, flip} for a filter of n elements; 0 when the geometry has no images
// (alignq_filter_image_bytes) or does not match n
inline unsigned img_geo_word(const int32_t* g4, long n) {
  const int CO = g4[0], KK = g4[1], CI = g4[2];
  if (!alignq_filter_image_bytes(CO, KK, CI) || (long)CO * KK * CI != n) return 0u;
  return (unsigned)CO | (unsigned)CI << 10 | (unsigned)KK << 20 | (g4[3] ? 1u << 28 : 0u);
}

}  // namespace alignq

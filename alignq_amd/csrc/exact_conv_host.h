// exact_conv_host.h - the launchers' shared rules of the exact-product convolutions (pointwise_kernels.hip, k3conv_kernels.hip,
// dense_eval_kernels.hip): what they refuse and how they choose a tile and a store form.
#pragma once
#include <stdint.h>

namespace alignq_xmma {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// B * H * W * ld <= 2^31 - 1, without overflow
inline bool fits31(int B, int H, int W, int ld) {
  const int64_t lim = INT32_MAX;
  int64_t m = (int64_t)B * H;
  if (m > lim) return false;
  m *= W;
  if (m > lim) return false;
  return m * ld <= lim;
}

// channels per output tile, 16, 32 or 64: the widest tile that pads N by no more than rounding it up to 16 does
inline int n_tile_width(int N) {
  const int r16 = (N + 15) / 16 * 16;
  if ((N + 63) / 64 * 64 == r16) return 64;
  if ((N + 31) / 32 * 32 == r16) return 32;
  return 16;
}

// the write-through window (store_forms.h): outputs of 1 MiB to 64 MiB are stored through to memory
inline bool write_through(int64_t out_bytes) { return out_bytes >= ((int64_t)1 << 20) && out_bytes <= ((int64_t)64 << 20); }

}  // namespace alignq_xmma

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

// The 3x3 filter gradient's launch geometry (k3conv_kernels.hip; dense_train_kernels.hip runs the same slabs): a step is one
// 4 x 8 pixel tile, the four waves lie along CIN (64 x 16) or along COUT (16 x 64), and split-K runs over slabs of spatial tiles:
// enough workgroups for the chip, at least two steps per slab, no empty slab.
constexpr int kK3WgradTileH = 4, kK3WgradTileW = 8;
struct K3WgradGeom { int cb, ob, th, tw, s_tiles, c_tiles, o_tiles, per, splits; };
inline K3WgradGeom k3_wgrad_geometry(int B, int H, int W, int CIN, int COUT) {
  K3WgradGeom g{};
  g.cb = CIN >= COUT ? 64 : 16; g.ob = CIN >= COUT ? 16 : 64;
  g.th = (H + kK3WgradTileH - 1) / kK3WgradTileH; g.tw = (W + kK3WgradTileW - 1) / kK3WgradTileW;
  g.s_tiles = B * g.th * g.tw;
  g.c_tiles = (CIN + g.cb - 1) / g.cb; g.o_tiles = (COUT + g.ob - 1) / g.ob;
  const int tiles = g.c_tiles * g.o_tiles;
  int s = (512 + tiles - 1) / tiles;
  const int max_s = (g.s_tiles + 1) / 2;
  if (s > max_s) s = max_s;
  if (s > 1024) s = 1024;
  if (s < 1) s = 1;
  g.per = (g.s_tiles + s - 1) / s;
  g.splits = (g.s_tiles + g.per - 1) / g.per;
  return g;
}

}  // namespace alignq_xmma

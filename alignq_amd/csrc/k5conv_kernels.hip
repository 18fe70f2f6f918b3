// k5conv_kernels.hip — Conv2d_Q's 5x5 / stride 1 / padding 0 convolutions with a bias (reference: cdf_alignment/dann_digit/model/
// dann.py:125-230, MNISTmodel_quant's two layers: 3 -> 32 at 28 x 28 and 32 -> 48 at 12 x 12).  Forward, data gradient and filter
// gradient with the arithmetic of k3conv_kernels.hip: the filter's integer bins as bf16, the fp32 operand in three exact bf16 terms,
// v_mfma_f32_16x16x32_bf16, fp32 accumulation in an order the shape fixes, one division, one add of the bias (the primitives:
// exact_mma.h; the launchers' shared rules: exact_conv_host.h).  include/alignq_k5conv.h states the contract.  The tile loops of the
// forward / data gradient (both forms) are in k5_fwd_body.h, shared with digit_eval_kernels.hip.  Two forms, by CIN:
//
// BODY (CIN a multiple of 4)
//   forward / data gradient  one workgroup = 256 threads = 4 waves = an 8 x 8 tile of OUTPUT pixels of ONE image x 16, 32 or 64 output
//           channels.  Per 32-deep channel chunk the tile's 12 x 12 footprint is staged in LDS once, already split into the three term
//           planes; the 25 taps read it at shifted rows.  Footprint pixels outside the operand are zeros and are never read from
//           memory: the forward's footprint ends with the image, the data gradient's (dy at (h - 4 + ty, w - 4 + tx)) begins four
//           pixels before it.  The chunk's filter is staged ONE TAP ROW (five taps) at a time, [tap][n][k]: all 25 taps of a
//           64-channel tile would be 128 KB.  The data gradient reads the same bins flipped (tap 24 - t) and transposed while staging.
//   filter gradient  a 32-pixel k step = a 4 x 8 tile of output pixels of one image; x is staged with its footprint (8 x 12 pixels), dy
//           without, both [pixel][channel] in three term planes and read through ds_read_b64_tr_b16; every tap reads x at its own
//           shifted rows.  A wave owns 16 input x 16 output channels x 25 taps (100 accumulator registers); the four waves lie along
//           CIN or along COUT.
// IMAGE (CIN == 3: the first layer; its input needs no gradient)
//   Taps and channels fold into the GEMM's K: k = ky * 15 + kx * 3 + ci, 75 values, zero-tailed to 96 = three MFMA k steps.  The
//   filter's own channels-last row [ky][kx][ci] IS that order; rows are 150 B, so they are staged in 4-byte words of the whole
//   contiguous tile and scattered halfword by halfword.
//   forward  the 12 x 12 x 3 patch of an 8 x 8 output tile is staged once as three term planes; the [64 pixels][96] term images are built
//           from it in LDS (pixel (py, px), tap row ky: 15 consecutive patch values from ((py + ky) * 12 + px) * 3); the fragments are
//           read as in the body form.  The filter tile does not depend on the spatial tile: its fragments stay in registers.
//   filter gradient  the same im2col image ([32 pixels][80] per 4 x 8 step) against dy: rows of D are output channels (a wave owns 16),
//           columns the 75 live k in five 16-wide blocks.
// MFMA roles as in k3conv_kernels.hip: A operand = rows of D (4 consecutive per lane), B operand = columns of D.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_k5conv.h"
#include "exact_conv_host.h"
#include "exact_mma.h"
#include "k5_fwd_body.h"
#include "wgrad_reduce_body.h"

using namespace alignq_xmma;
using namespace alignq_k5;          // the geometry constants, K5 / K5I and the two forward tile loops (shared with digit_eval_kernels.hip)

namespace {

// Body form, forward and data gradient, and image form, forward: the tile loops of k5_fwd_body.h with the plain store
template <int TN, bool WTR>
__global__ __launch_bounds__(256, 2) void k5_gemm_kernel(const K5 p) {
  k5_gemm_body<TN, WTR>(p, K5Store{p.out, p.bias, p.OH, p.OW, p.N, p.nlev, p.wt});
}

template <int TN>
__global__ __launch_bounds__(256, 2) void k5_image_fwd_kernel(const K5I p) {
  k5_image_fwd_body<TN, false>(p, K5Store{p.y, p.bias, p.OH, p.OW, p.N, p.nlev, p.wt});
}

// ---------------------------------------------------------------------------------------------------------------------------
// Body form, filter gradient:  slab[split][co][t][ci] = sum over the split's spatial tiles of dy[pixel][co] * x[pixel + t][ci]
// A step is one 4 x 8 tile of OUTPUT pixels (k = 8 row + column).  Lane group g takes pixels {4g .. 4g+3} and {16 + 4g .. 16 + 4g + 3} of
// the step on both operands: tile rows g >> 1 and 2 + (g >> 1).  Channels beyond CIN / COUT are staged as zeros and never stored.
constexpr int WTH = 4, WTW = 8, WK = WTH * WTW;
constexpr int WFW = WTW + KS - 1, WFP = (WTH + KS - 1) * WFW;          // x with its footprint: 8 x 12 pixels
struct K5W {
  const float* x; const float* dy; float* slabs;
  int H, W, OH, OW, CIN, COUT;
  int th, tw, s_tiles, per;        // tiles along OH and OW, spatial tiles in all, spatial tiles per split
  int c_tiles, o_tiles;
};

template <int CB, int OB>
__global__ __launch_bounds__(256, 2) void k5_wgrad_kernel(const K5W a) {
  static_assert((CB == 64 && OB == 16) || (CB == 16 && OB == 64), "four waves along CIN or along COUT");
  constexpr int LDC = CB + 16, LDO = OB + 16;
  constexpr int XPL = WFP * LDC, DPL = WK * LDO;
  constexpr int NXP = WFP * CB / 4, NX = (NXP + 255) / 256;
  constexpr int NDP = WK * OB / 4, ND = (NDP + 255) / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + 3 * DPL];
  u16* const Xs = lds;
  u16* const Ds = lds + 3 * XPL;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wc = CB == 64 ? wv : 0, wo = OB == 64 ? wv : 0;
  const int tiles = a.c_tiles * a.o_tiles;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = pid / tiles, tile = pid % tiles;
  const int ct = tile % a.c_tiles, ot = tile / a.c_tiles;
  const int c0 = ct * CB, o0 = ot * OB;
  const int t_begin = split * a.per, t_end = (t_begin + a.per < a.s_tiles) ? t_begin + a.per : a.s_tiles;
  const int per_img = a.th * a.tw;

  f32x4 rx[NX], rd[ND];
  auto fetch = [&](int st) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / a.tw) * WTH, w0 = (r % a.tw) * WTW;
    const int64_t img_x = (int64_t)b * a.H * a.W, img_d = (int64_t)b * a.OH * a.OW;
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i, fp = idx / (CB / 4), q4 = idx % (CB / 4);
      const int hy = fp / WFW, hx = fp - hy * WFW;
      const int h = h0 + hy, w = w0 + hx, c = c0 + 4 * q4;
      const bool ok = idx < NXP && h < a.H && w < a.W && c < a.CIN;
      rx[i] = *reinterpret_cast<const f32x4*>(a.x + (ok ? (img_x + (int64_t)h * a.W + w) * a.CIN + c : 0));
      if (!ok) rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (OB / 4), q4 = idx % (OB / 4);
      const int h = h0 + (kr >> 3), w = w0 + (kr & 7), o = o0 + 4 * q4;
      const bool ok = idx < NDP && h < a.OH && w < a.OW && o < a.COUT;
      rd[i] = *reinterpret_cast<const f32x4*>(a.dy + (ok ? (img_d + (int64_t)h * a.OW + w) * a.COUT + o : 0));
      if (!ok) rd[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i;
      if (idx >= NXP) continue;
      const int o = (idx / (CB / 4)) * LDC + 4 * (idx % (CB / 4));
      s16x4 h, m, l;
      split3(rx[i], h, m, l);
      *reinterpret_cast<s16x4*>(Xs + o) = h;
      *reinterpret_cast<s16x4*>(Xs + XPL + o) = m;
      *reinterpret_cast<s16x4*>(Xs + 2 * XPL + o) = l;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i;
      if (idx >= NDP) continue;
      const int o = (idx / (OB / 4)) * LDO + 4 * (idx % (OB / 4));
      s16x4 h, m, l;
      split3(rd[i], h, m, l);
      *reinterpret_cast<s16x4*>(Ds + o) = h;
      *reinterpret_cast<s16x4*>(Ds + DPL + o) = m;
      *reinterpret_cast<s16x4*>(Ds + 2 * DPL + o) = l;
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fc = 4 * (lane & 3);
  const int krow = 4 * fg + fq;                       // first pixel of this lane's block (second: + 16 = two tile rows down)
  const int ky = krow >> 3, kx = krow & 7;
  if (t_begin < t_end) fetch(t_begin);
  for (int st = t_begin; st < t_end; st++) {          // every lane of the workgroup takes the same trips (ds_read_tr needs EXEC full)
    __syncthreads();
    park();
    __syncthreads();
    if (st + 1 < t_end) fetch(st + 1);
    s16x8 df[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const u16* p = Ds + s * DPL + krow * LDO + wo * 16 + fc;
      df[s] = join8(tr_read(p), tr_read(p + 16 * LDO));
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
      s16x8 xf[3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
        const u16* p = Xs + s * XPL + ((ky + t / KS) * WFW + kx + t % KS) * LDC + wc * 16 + fc;
        xf[s] = join8(tr_read(p), tr_read(p + 2 * WFW * LDC));
      }
      f32x4 v = acc[t];                      // the six leading pairs, smallest first
      v = mfma16(xf[1], df[1], v);
      v = mfma16(xf[0], df[2], v);
      v = mfma16(xf[2], df[0], v);
      v = mfma16(xf[0], df[1], v);
      v = mfma16(xf[1], df[0], v);
      v = mfma16(xf[0], df[0], v);
      acc[t] = v;
    }
  }
  // D: column = output channel (lane & 15), rows = input channels 4 * (lane >> 4) + e
  float* slab = a.slabs + (int64_t)split * a.COUT * NT * a.CIN;
  const int o = o0 + wo * 16 + (lane & 15), c = c0 + wc * 16 + 4 * fg;
  if (o < a.COUT && c < a.CIN) {
#pragma unroll
    for (int t = 0; t < NT; t++)
      __builtin_nontemporal_store(acc[t], reinterpret_cast<f32x4*>(slab + ((int64_t)o * NT + t) * a.CIN + c));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------------------------------------------
// Image form, filter gradient:  slab[split][co][k] = sum over the split's 4 x 8 steps of dy[pixel][co] * im[pixel][k]
// A workgroup owns 64 output channels (a wave 16) x the five 16-wide k blocks; the pixel mapping of a lane is the body form's.
constexpr int IWB = 5;                 // k blocks of 16: 80 >= 75
constexpr int IWP = WFP * 3;           // floats of the 8 x 12 x 3 patch
struct K5IW {
  const float* x; const float* dy; float* slabs;
  int H, W, OH, OW, COUT;
  int th, tw, s_tiles, per, o_tiles;
};

__global__ __launch_bounds__(256, 2) void k5_image_wgrad_kernel(const K5IW a) {
  constexpr int OB = 64, LDO = OB + 16, DPL = WK * LDO;
  constexpr int LDI = 16 * IWB + 16, IPL = WK * LDI;
  constexpr int NP = (IWP + 255) / 256;
  constexpr int NDP = WK * OB / 4, ND = NDP / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * IPL + 3 * DPL + 3 * IWP];
  u16* const Is = lds;
  u16* const Ds = lds + 3 * IPL;
  u16* const Ps = Ds + 3 * DPL;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = pid / a.o_tiles, ot = pid % a.o_tiles;
  const int o0 = ot * OB;
  const int t_begin = split * a.per, t_end = (t_begin + a.per < a.s_tiles) ? t_begin + a.per : a.s_tiles;
  const int per_img = a.th * a.tw;

  float rp[NP];
  f32x4 rd[ND];
  auto fetch = [&](int st) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / a.tw) * WTH, w0 = (r % a.tw) * WTW;
    const int64_t img_x = (int64_t)b * a.H * a.W, img_d = (int64_t)b * a.OH * a.OW;
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const int idx = tid + 256 * i, fp = idx / 3, ci = idx - 3 * fp;
      const int hy = fp / WFW, hx = fp - hy * WFW;
      const int h = h0 + hy, w = w0 + hx;
      const bool ok = idx < IWP && h < a.H && w < a.W;
      rp[i] = ok ? a.x[(img_x + (int64_t)h * a.W + w) * 3 + ci] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (OB / 4), q4 = idx % (OB / 4);
      const int h = h0 + (kr >> 3), w = w0 + (kr & 7), o = o0 + 4 * q4;
      const bool ok = h < a.OH && w < a.OW && o < a.COUT;
      rd[i] = *reinterpret_cast<const f32x4*>(a.dy + (ok ? (img_d + (int64_t)h * a.OW + w) * a.COUT + o : 0));
      if (!ok) rd[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x4 acc[IWB];
#pragma unroll
  for (int j = 0; j < IWB; j++) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fc = 4 * (lane & 3);
  const int krow = 4 * fg + fq;
  if (t_begin < t_end) fetch(t_begin);
  for (int st = t_begin; st < t_end; st++) {          // every lane of the workgroup takes the same trips (ds_read_tr needs EXEC full)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const int idx = tid + 256 * i;
      if (idx >= IWP) continue;
      split3_one(rp[i], Ps[idx], Ps[IWP + idx], Ps[2 * IWP + idx]);
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i;
      const int o = (idx / (OB / 4)) * LDO + 4 * (idx % (OB / 4));
      s16x4 h, m, l;
      split3(rd[i], h, m, l);
      *reinterpret_cast<s16x4*>(Ds + o) = h;
      *reinterpret_cast<s16x4*>(Ds + DPL + o) = m;
      *reinterpret_cast<s16x4*>(Ds + 2 * DPL + o) = l;
    }
    __syncthreads();
    if (st + 1 < t_end) fetch(st + 1);
    for (int j = tid; j < WK * 16 * IWB; j += 256) {          // the term images: [pixel][k], zeros beyond k = 74
      const int pix = j / (16 * IWB), k = j - pix * (16 * IWB);
      const bool live = k < IK;
      const int ky = k / 15, src = live ? (((pix >> 3) + ky) * WFW + (pix & 7)) * 3 + (k - 15 * ky) : 0;
#pragma unroll
      for (int q = 0; q < 3; q++) Is[q * IPL + pix * LDI + k] = live ? Ps[q * IWP + src] : (u16)0;
    }
    __syncthreads();
    s16x8 df[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const u16* p = Ds + s * DPL + krow * LDO + wv * 16 + fc;
      df[s] = join8(tr_read(p), tr_read(p + 16 * LDO));
    }
#pragma unroll
    for (int j = 0; j < IWB; j++) {
      s16x8 xf[3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
        const u16* p = Is + s * IPL + krow * LDI + 16 * j + fc;
        xf[s] = join8(tr_read(p), tr_read(p + 16 * LDI));
      }
      f32x4 v = acc[j];                      // the six leading pairs, smallest first; rows of D = dy's channels
      v = mfma16(df[1], xf[1], v);
      v = mfma16(df[2], xf[0], v);
      v = mfma16(df[0], xf[2], v);
      v = mfma16(df[1], xf[0], v);
      v = mfma16(df[0], xf[1], v);
      v = mfma16(df[0], xf[0], v);
      acc[j] = v;
    }
  }
  // D: rows = output channels 4 * (lane >> 4) + e of the wave's 16, column = k (lane & 15) of the block
  float* slab = a.slabs + (int64_t)split * a.COUT * IK;
#pragma unroll
  for (int j = 0; j < IWB; j++) {
    const int k = 16 * j + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int o = o0 + wv * 16 + 4 * fg + e;
      if (o < a.COUT && k < IK) __builtin_nontemporal_store(acc[j][e], slab + (int64_t)o * IK + k);
    }
  }
}

// The slab reduction of wgrad_reduce_body.h at 256 threads (k3conv_kernels.hip: same groups, same order, same bits as the
// 1024-thread alignq_conv3x3_wgrad_reduce_multi).
constexpr int kRedThreads = 256;
__global__ __launch_bounds__(kRedThreads) void k5_slab_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int n_elem,
                                                                     float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float part[4 * kRedThreads];
  alignq_wgr::wgrad_reduce_body<kRedThreads>(slabs, n_slabs, n_elem, dw, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------------------
inline bool chan_ok(int C) { return C >= kMinC && C <= kMaxC && !(C & 3); }
inline bool shape_ok(int op, int B, int H, int W, int CIN, int COUT) {
  if (op != ALIGNQ_K5_FWD && op != ALIGNQ_K5_DGRAD && op != ALIGNQ_K5_WGRAD) return false;
  const bool image = CIN == 3 && op != ALIGNQ_K5_DGRAD;
  if (!(image || chan_ok(CIN)) || !chan_ok(COUT) || B < 1 || H < KS || W < KS) return false;
  return fits31(B, H, W, CIN > COUT ? CIN : COUT);
}

inline int gemm_form(int N) {
  const int bn = n_tile_width(N);
  return bn == 64 ? ALIGNQ_K5_FORM_N64 : (bn == 32 ? ALIGNQ_K5_FORM_N32 : ALIGNQ_K5_FORM_N16);
}
inline int wgrad_form(int CIN, int COUT) {
  return CIN == 3 ? ALIGNQ_K5_FORM_WIMAGE : (CIN >= COUT ? ALIGNQ_K5_FORM_W64X16 : ALIGNQ_K5_FORM_W16X64);
}

inline int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// forward (dgrad = false: a = x, K = CIN, N = COUT) or data gradient (a = dy, K = COUT, N = CIN) of the body form
template <bool WTR>
int launch_gemm(const float* a, const void* w, const float* bias, float* out, int B, int H, int W, int K, int N, int w_bit,
                hipStream_t st) {
  K5 p{};
  p.a = a; p.w = (const u16*)w; p.bias = bias; p.out = out;
  p.AH = WTR ? H - (KS - 1) : H; p.AW = WTR ? W - (KS - 1) : W;
  p.OH = WTR ? H : H - (KS - 1); p.OW = WTR ? W : W - (KS - 1);
  p.K = K; p.N = N; p.off = WTR ? -(KS - 1) : 0;
  p.th = (p.OH + TS - 1) / TS; p.tw = (p.OW + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;                       // <= B * H * W
  p.s_blocks = p.s_tiles < kMaxTileBlocks ? p.s_tiles : kMaxTileBlocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.wt = write_through((int64_t)B * p.OH * p.OW * N * (int64_t)sizeof(float));
  const int bn = n_tile_width(N);
  p.n_tiles = (N + bn - 1) / bn;
  const dim3 grid(p.s_blocks * p.n_tiles), blk(256);
  if (bn == 64) hipLaunchKernelGGL((k5_gemm_kernel<4, WTR>), grid, blk, 0, st, p);
  else if (bn == 32) hipLaunchKernelGGL((k5_gemm_kernel<2, WTR>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((k5_gemm_kernel<1, WTR>), grid, blk, 0, st, p);
  return last_error();
}

int launch_image_fwd(const float* x, const void* w, const float* bias, float* y, int B, int H, int W, int N, int w_bit, hipStream_t st) {
  K5I p{};
  p.x = x; p.w = (const u16*)w; p.bias = bias; p.y = y;
  p.H = H; p.W = W; p.OH = H - (KS - 1); p.OW = W - (KS - 1); p.N = N;
  p.th = (p.OH + TS - 1) / TS; p.tw = (p.OW + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;
  p.s_blocks = p.s_tiles < kMaxTileBlocks ? p.s_tiles : kMaxTileBlocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.wt = write_through((int64_t)B * p.OH * p.OW * N * (int64_t)sizeof(float));
  const int bn = n_tile_width(N);
  p.n_tiles = (N + bn - 1) / bn;
  const dim3 grid(p.s_blocks * p.n_tiles), blk(256);
  if (bn == 64) hipLaunchKernelGGL((k5_image_fwd_kernel<4>), grid, blk, 0, st, p);
  else if (bn == 32) hipLaunchKernelGGL((k5_image_fwd_kernel<2>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((k5_image_fwd_kernel<1>), grid, blk, 0, st, p);
  return last_error();
}

// split-K over slabs of spatial tiles (k3conv_kernels.hip's rule): enough workgroups for the chip, at least two steps per slab, no
// empty slab
struct WGeom { int form, th, tw, s_tiles, c_tiles, o_tiles, per, splits; };
inline WGeom wgrad_geometry(int B, int H, int W, int CIN, int COUT) {
  WGeom g{};
  g.form = wgrad_form(CIN, COUT);
  const int cb = g.form == ALIGNQ_K5_FORM_W64X16 ? 64 : 16, ob = g.form == ALIGNQ_K5_FORM_W64X16 ? 16 : 64;
  g.th = (H - (KS - 1) + WTH - 1) / WTH; g.tw = (W - (KS - 1) + WTW - 1) / WTW;
  g.s_tiles = B * g.th * g.tw;
  g.c_tiles = g.form == ALIGNQ_K5_FORM_WIMAGE ? 1 : (CIN + cb - 1) / cb;
  g.o_tiles = (COUT + ob - 1) / ob;
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

}  // namespace

extern "C" {

int alignq_k5conv_supported(int op, int B, int H, int W, int CIN, int COUT) { return shape_ok(op, B, H, W, CIN, COUT) ? 1 : 0; }

int alignq_k5conv_form(int op, int B, int H, int W, int CIN, int COUT) {
  if (!shape_ok(op, B, H, W, CIN, COUT)) return -1;
  if (op == ALIGNQ_K5_FWD) return gemm_form(COUT);
  if (op == ALIGNQ_K5_DGRAD) return gemm_form(CIN);
  return wgrad_form(CIN, COUT);
}

int alignq_k5conv_fwd(const float* x, const void* w_bins, const float* bias, float* y, int B, int H, int W, int CIN, int COUT, int w_bit,
                      void* stream) {
  if (!x || !w_bins || !y || !aligned16(x) || !aligned16(w_bins) || !aligned16(y) || ((uintptr_t)bias & 3) || w_bit < 1 || w_bit > 8)
    return ALIGNQ_EINVAL;
  if (!shape_ok(ALIGNQ_K5_FWD, B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  if (CIN == 3) return launch_image_fwd(x, w_bins, bias, y, B, H, W, COUT, w_bit, (hipStream_t)stream);
  return launch_gemm<false>(x, w_bins, bias, y, B, H, W, CIN, COUT, w_bit, (hipStream_t)stream);
}

int alignq_k5conv_dgrad(const float* dy, const void* w_bins, float* dx, int B, int H, int W, int CIN, int COUT, int w_bit,
                        void* stream) {
  if (!dy || !w_bins || !dx || !aligned16(dy) || !aligned16(w_bins) || !aligned16(dx) || w_bit < 1 || w_bit > 8) return ALIGNQ_EINVAL;
  if (!shape_ok(ALIGNQ_K5_DGRAD, B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  return launch_gemm<true>(dy, w_bins, nullptr, dx, B, H, W, COUT, CIN, w_bit, (hipStream_t)stream);
}

size_t alignq_k5conv_wgrad_ws_bytes(int B, int H, int W, int CIN, int COUT) {
  if (!shape_ok(ALIGNQ_K5_WGRAD, B, H, W, CIN, COUT)) return 0;
  const WGeom g = wgrad_geometry(B, H, W, CIN, COUT);
  return (size_t)g.splits * (size_t)COUT * NT * CIN * sizeof(float);
}

int alignq_k5conv_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H, int W, int CIN, int COUT,
                        int* n_slabs_out, void* stream) {
  if (!x || !dy || !ws || (!dw && !n_slabs_out) || !aligned16(x) || !aligned16(dy) || !aligned16(ws) || !aligned16(dw))
    return ALIGNQ_EINVAL;
  if (!shape_ok(ALIGNQ_K5_WGRAD, B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  const WGeom g = wgrad_geometry(B, H, W, CIN, COUT);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.c_tiles * g.o_tiles * g.splits), blk(256);
  if (g.form == ALIGNQ_K5_FORM_WIMAGE) {
    K5IW a{};
    a.x = x; a.dy = dy; a.slabs = (float*)ws;
    a.H = H; a.W = W; a.OH = H - (KS - 1); a.OW = W - (KS - 1); a.COUT = COUT;
    a.th = g.th; a.tw = g.tw; a.s_tiles = g.s_tiles; a.per = g.per; a.o_tiles = g.o_tiles;
    hipLaunchKernelGGL(k5_image_wgrad_kernel, grid, blk, 0, st, a);
  } else {
    K5W a{};
    a.x = x; a.dy = dy; a.slabs = (float*)ws;
    a.H = H; a.W = W; a.OH = H - (KS - 1); a.OW = W - (KS - 1); a.CIN = CIN; a.COUT = COUT;
    a.th = g.th; a.tw = g.tw; a.s_tiles = g.s_tiles; a.per = g.per;
    a.c_tiles = g.c_tiles; a.o_tiles = g.o_tiles;
    if (g.form == ALIGNQ_K5_FORM_W64X16) hipLaunchKernelGGL((k5_wgrad_kernel<64, 16>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k5_wgrad_kernel<16, 64>), grid, blk, 0, st, a);
  }
  int e = last_error();
  if (e) return e;
  if (n_slabs_out) { *n_slabs_out = g.splits; return 0; }      // deferred: the caller reduces (alignq_conv3x3_wgrad_reduce_multi)
  const int n_elem = COUT * NT * CIN;
  hipLaunchKernelGGL(k5_slab_reduce_kernel, dim3(alignq_wgr::wgrad_reduce_blocks(g.splits, n_elem, kRedThreads)), dim3(kRedThreads), 0,
                     st, (const float*)ws, g.splits, n_elem, dw);
  return last_error();
}

}  // extern "C"

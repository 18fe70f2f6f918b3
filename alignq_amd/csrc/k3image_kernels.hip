// k3image_kernels.hip — Conv2d_Q's 3x3 / stride 1 / padding 1 convolution of a 3-channel image (reference: cdf_alignment/dense-cifar-10/
// model/densenet.py, DenseNet's conv1, 3 -> 24 at 32 x 32; MobileNet-V2's conv1, 3 -> 32).  Forward and filter gradient with the
// arithmetic of k5conv_kernels.hip's image form: the filter's integer bins as bf16, the fp32 image in three exact bf16 terms,
// v_mfma_f32_16x16x32_bf16, fp32 accumulation in an order the shape fixes, one division (the primitives: exact_mma.h; the launchers'
// shared rules: exact_conv_host.h).  include/alignq_k3image.h states the contract.
//
// Taps and channels fold into the GEMM's K: k = ky * 9 + kx * 3 + ci, 27 values, zero-tailed to 32 = ONE MFMA k step.  The filter's
// own channels-last row [ky][kx][ci] IS that order; rows are 54 B, so they are staged in 4-byte words of the whole contiguous tile and
// scattered halfword by halfword.
//
// forward  one workgroup = 256 threads = 4 waves = an 8 x 8 tile of output pixels of ONE image x 16, 32 or 64 output channels, and it
//         is PERSISTENT over spatial tiles: the grid is sized from the CU count, a workgroup walks its tiles by grid stride.  The
//         filter tile does not depend on the spatial tile: every wave reads its A fragments (TN x 8 halfwords per lane) once and keeps
//         them in registers for the whole launch.  Per tile the 10 x 10 x 3 patch (one pixel of padding all round; pixels outside the
//         image are zeros and are never read) is staged once in LDS as three term planes of 300 halfwords.  A lane's B fragment - its
//         pixel (py, px), k = 8 g .. 8 g + 7 - is built DIRECTLY into registers from the planes: tap row ky is the 9 consecutive
//         patch values from ((py + ky) * 10 + px) * 3, so the eight offsets are lane constants and the dead k (27 .. 31) point at a
//         zero halfword behind each plane.  There is no [64 pixels][32] term image: it would cost 24 LDS writes, 24 reads and one
//         barrier more per thread and tile than the 24 reads of the direct build.  Three MFMAs per 16 x 16 output block (lo, mid,
//         hi).  The next tile's patch loads are issued before the current tile's fragment reads and MFMAs: the kernel is bound by
//         its output stores (8 KB per tile and 32 channels against 1.2 KB read).
// filter gradient  a 32-pixel k step = a 4 x 8 tile of pixels of one image.  Rows of D are output channels (a workgroup owns 64, a
//         wave 16), columns the 27 live k in two 16-wide blocks, the contraction the 32 pixels.  The im2col term image [32 pixels][32]
//         is built in LDS from the staged 6 x 10 x 3 patch; dy is staged [pixel][channel] in three term planes; both are read through
//         ds_read_b64_tr_b16.  Slabs of whole steps, reduced by wgrad_reduce_body.h.
// MFMA roles as in k3conv_kernels.hip: A operand = rows of D (4 consecutive per lane), B operand = columns of D.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_k3image.h"
#include "exact_conv_host.h"
#include "exact_mma.h"
#include "wgrad_reduce_body.h"

using namespace alignq_xmma;

namespace {

constexpr int IK = 27;                 // the live k: 3 x 3 taps x 3 channels
constexpr int kMinC = 4, kMaxC = 512;

// one float of a patch in its three terms (split3 on a padded quad: the same bits as every other split of the family)
__device__ __forceinline__ void split3_one(const float v, u16& h, u16& m, u16& l) {
  s16x4 hh, mm, ll;
  split3((f32x4){v, 0.f, 0.f, 0.f}, hh, mm, ll);
  h = (u16)hh[0]; m = (u16)mm[0]; l = (u16)ll[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Forward:  y[b][h][w][n] = (1 / nlev) * sum_{k < 27} im[b][h][w][k] * w[n][k],  im[b][h][w][ky * 9 + kx * 3 + ci] = x[b][h+ky-1][w+kx-1][ci]
constexpr int TS = 8;                  // the spatial tile is TS x TS output pixels
constexpr int FS = TS + 2;             // its patch: 10 x 10 pixels
constexpr int IPP = FS * FS * 3;       // floats of the patch
constexpr int PPL = IPP + 4;           // halfwords per term plane: the patch, then the zero the dead k read
constexpr int LDW = 40;                // halfwords per filter row in LDS: 80 B rows, 16 lanes' ds_read_b128 on 16 distinct 16-byte slots
constexpr int kTilesPerCu = 4;         // resident workgroups per CU the grid is sized for

struct K3I {
  const float* x; const u16* w; float* y;
  int H, W, N, ldy;
  int th, tw, s_tiles, s_blocks, n_tiles;      // tiles along H and W, spatial tiles, workgroups per channel tile (their stride), channel tiles
  float nlev;
  int wt;                                      // write-through output stores
};

template <int TN>
__global__ __launch_bounds__(256, 2) void k3i_fwd_kernel(const K3I p) {
  constexpr int BN = 16 * TN;
  constexpr int NP = (IPP + 255) / 256;               // patch floats per thread
  __shared__ __attribute__((aligned(16))) u16 lds[3 * PPL + BN * LDW];
  u16* const Ps = lds;
  u16* const Ws = lds + 3 * PPL;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = pid % p.n_tiles, sb = pid / p.n_tiles;
  const int n0 = nt * BN;
  const int fr = lane & 15, fg = lane >> 4;
  const int pl = wv * 16 + fr, py = pl >> 3, px = pl & 7;          // this lane's pixel of the tile (B operand column)
  const int per_img = p.th * p.tw;

  // the filter tile, once per workgroup: its live rows are ONE contiguous run of rows * 27 halfwords (an even count, 4-byte aligned: n0
  // is a multiple of 16 and N of 4), read in 4-byte words and scattered into [row][LDW]; the k tail and the rows beyond N are zeros
  for (int j = tid; j < BN * LDW / 2; j += 256) reinterpret_cast<uint32_t*>(Ws)[j] = 0u;
  if (tid < 12) Ps[(tid >> 2) * PPL + IPP + (tid & 3)] = 0;
  __syncthreads();
  {
    const int rows = p.N - n0 < BN ? p.N - n0 : BN;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.w + (int64_t)n0 * IK);
    for (int j = tid; 2 * j < rows * IK; j += 256) {
      const uint32_t v = src[j];
      const int e0 = 2 * j, e1 = e0 + 1;
      Ws[(e0 / IK) * LDW + e0 % IK] = (u16)(v & 0xffffu);
      Ws[(e1 / IK) * LDW + e1 % IK] = (u16)(v >> 16);
    }
  }
  __syncthreads();
  s16x8 wf[TN];
#pragma unroll
  for (int tn = 0; tn < TN; tn++) wf[tn] = *reinterpret_cast<const s16x8*>(Ws + (tn * 16 + fr) * LDW + 8 * fg);

  // where this lane's eight k lie in a term plane (the same for every tile)
  int off[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int k = 8 * fg + e, ky = k / 9;
    off[e] = k < IK ? ((py + ky) * FS + px) * 3 + (k - 9 * ky) : IPP;
  }

  float rp[NP];
  auto fetch = [&](int st) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / p.tw) * TS - 1, w0 = (r % p.tw) * TS - 1;
    const int64_t img = (int64_t)b * p.H * p.W;
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const int idx = tid + 256 * i, fp = idx / 3, ci = idx - 3 * fp;
      const int hy = fp / FS, hx = fp - hy * FS;
      const int h = h0 + hy, w = w0 + hx;
      const bool ok = idx < IPP && h >= 0 && h < p.H && w >= 0 && w < p.W;
      rp[i] = ok ? p.x[(img + (int64_t)h * p.W + w) * 3 + ci] : 0.f;
    }
  };

  if (sb < p.s_tiles) fetch(sb);
  for (int st = sb; st < p.s_tiles; st += p.s_blocks) {
    const int b = st / per_img, r = st - b * per_img;
    const int h = (r / p.tw) * TS + py, w = (r % p.tw) * TS + px;
    __syncthreads();                           // the previous tile's fragment reads are done
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const int idx = tid + 256 * i;
      if (idx >= IPP) continue;
      split3_one(rp[i], Ps[idx], Ps[PPL + idx], Ps[2 * PPL + idx]);
    }
    __syncthreads();
    if (st + p.s_blocks < p.s_tiles) fetch(st + p.s_blocks);          // in flight under this tile's MFMAs and stores
    s16x8 xf[3];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int e = 0; e < 8; e++) xf[q][e] = (short)Ps[q * PPL + off[e]];
    f32x4 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 2; q >= 0; q--) {             // smallest term first
#pragma unroll
      for (int tn = 0; tn < TN; tn++) acc[tn] = mfma16(wf[tn], xf[q], acc[tn]);
    }
    // epilogue: lane = pixel (lane & 15) of the wave's 16, 4 consecutive channels 4 * (lane >> 4) + e of every 16-channel block
    if (h < p.H && w < p.W) {
      float* const row = p.y + (((int64_t)b * p.H + h) * p.W + w) * p.ldy;
#pragma unroll
      for (int tn = 0; tn < TN; tn++) {
        const int n = n0 + tn * 16 + 4 * fg;
        if (n < p.N) {
          const f32x4 v = acc[tn];
          st_out(row + n, (f32x4){v[0] / p.nlev, v[1] / p.nlev, v[2] / p.nlev, v[3] / p.nlev}, p.wt);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Filter gradient:  slab[split][co][k] = sum over the split's 4 x 8 steps of dy[pixel][co] * im[pixel][k]
// Lane group g takes pixels {4g .. 4g+3} and {16 + 4g .. 16 + 4g + 3} of the step on both operands: tile rows g >> 1 and 2 + (g >> 1).
// Channels beyond COUT and pixels beyond the image are staged as zeros and never stored.
constexpr int WTH = 4, WTW = 8, WK = WTH * WTW;
constexpr int WFW = WTW + 2, WFP = (WTH + 2) * WFW;          // x with its padding: 6 x 10 pixels
constexpr int IWB = 2;                 // k blocks of 16: 32 >= 27
constexpr int IWP = WFP * 3;           // floats of the 6 x 10 x 3 patch
struct K3IW {
  const float* x; const float* dy; float* slabs;
  int H, W, COUT;
  int th, tw, s_tiles, per, o_tiles;
};

__global__ __launch_bounds__(256, 2) void k3i_wgrad_kernel(const K3IW a) {
  constexpr int OB = 64, LDO = OB + 16, DPL = WK * LDO;
  constexpr int LDI = 16 * IWB + 16, IPL = WK * LDI;
  constexpr int NDP = WK * OB / 4, ND = NDP / 256;
  static_assert(IWP <= 256, "one patch float per thread");
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

  float rp;
  f32x4 rd[ND];
  auto fetch = [&](int st) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / a.tw) * WTH, w0 = (r % a.tw) * WTW;
    const int64_t img = (int64_t)b * a.H * a.W;
    {
      const int fp = tid / 3, ci = tid - 3 * fp;
      const int hy = fp / WFW, hx = fp - hy * WFW;
      const int h = h0 - 1 + hy, w = w0 - 1 + hx;
      const bool ok = tid < IWP && h >= 0 && h < a.H && w >= 0 && w < a.W;
      rp = ok ? a.x[(img + (int64_t)h * a.W + w) * 3 + ci] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (OB / 4), q4 = idx % (OB / 4);
      const int h = h0 + (kr >> 3), w = w0 + (kr & 7), o = o0 + 4 * q4;
      const bool ok = h < a.H && w < a.W && o < a.COUT;
      rd[i] = *reinterpret_cast<const f32x4*>(a.dy + (ok ? (img + (int64_t)h * a.W + w) * a.COUT + o : 0));
      if (!ok) rd[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x4 acc[IWB];
#pragma unroll
  for (int j = 0; j < IWB; j++) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fc = 4 * (lane & 3);
  const int krow = 4 * fg + fq;                       // first pixel of this lane's block (second: + 16 = two tile rows down)
  if (t_begin < t_end) fetch(t_begin);
  for (int st = t_begin; st < t_end; st++) {          // every lane of the workgroup takes the same trips (ds_read_tr needs EXEC full)
    __syncthreads();
    if (tid < IWP) split3_one(rp, Ps[tid], Ps[IWP + tid], Ps[2 * IWP + tid]);
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
#pragma unroll
    for (int j = tid; j < WK * 16 * IWB; j += 256) {          // the term images: [pixel][k], zeros beyond k = 26
      const int pix = j / (16 * IWB), k = j - pix * (16 * IWB);
      const bool live = k < IK;
      const int ky = k / 9, src = live ? (((pix >> 3) + ky) * WFW + (pix & 7)) * 3 + (k - 9 * ky) : 0;
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
__global__ __launch_bounds__(kRedThreads) void k3i_slab_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int n_elem,
                                                                      float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float part[4 * kRedThreads];
  alignq_wgr::wgrad_reduce_body<kRedThreads>(slabs, n_slabs, n_elem, dw, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------------------
inline bool shape_ok(int op, int B, int H, int W, int COUT, int ld) {
  if (op != ALIGNQ_K3I_FWD && op != ALIGNQ_K3I_WGRAD) return false;
  if (COUT < kMinC || COUT > kMaxC || (COUT & 3) || B < 1 || H < 1 || W < 1 || ld < COUT || (ld & 3)) return false;
  return fits31(B, H, W, ld);
}

inline int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// the CUs of the current device (the persistent forward's grid); a query that fails leaves no error behind and answers the MI355X's
inline int cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return 256;
  }
  return n;
}

// split-K over slabs of spatial tiles (k3conv_kernels.hip's rule): enough workgroups for the chip, at least two steps per slab, no
// empty slab
struct WGeom { int th, tw, s_tiles, o_tiles, per, splits; };
inline WGeom wgrad_geometry(int B, int H, int W, int COUT) {
  WGeom g{};
  g.th = (H + WTH - 1) / WTH; g.tw = (W + WTW - 1) / WTW;
  g.s_tiles = B * g.th * g.tw;                       // <= B * H * W
  g.o_tiles = (COUT + 63) / 64;
  int s = (512 + g.o_tiles - 1) / g.o_tiles;
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

int alignq_k3image_supported(int op, int B, int H, int W, int COUT) { return shape_ok(op, B, H, W, COUT, COUT) ? 1 : 0; }

int alignq_k3image_form(int op, int B, int H, int W, int COUT) {
  if (!shape_ok(op, B, H, W, COUT, COUT)) return -1;
  if (op == ALIGNQ_K3I_WGRAD) return ALIGNQ_K3I_FORM_WIMAGE;
  const int bn = n_tile_width(COUT);
  return bn == 64 ? ALIGNQ_K3I_FORM_N64 : (bn == 32 ? ALIGNQ_K3I_FORM_N32 : ALIGNQ_K3I_FORM_N16);
}

int alignq_k3image_fwd(const float* x, const void* w_bins, float* y, int B, int H, int W, int COUT, int ldy, int w_bit, void* stream) {
  if (!x || !w_bins || !y || !aligned16(x) || !aligned16(w_bins) || !aligned16(y) || w_bit < 1 || w_bit > 8) return ALIGNQ_EINVAL;
  if (!shape_ok(ALIGNQ_K3I_FWD, B, H, W, COUT, ldy)) return ALIGNQ_EUNSUPPORTED;
  K3I p{};
  p.x = x; p.w = (const u16*)w_bins; p.y = y;
  p.H = H; p.W = W; p.N = COUT; p.ldy = ldy;
  p.th = (H + TS - 1) / TS; p.tw = (W + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;                       // <= B * H * W
  const int bn = n_tile_width(COUT);
  p.n_tiles = (COUT + bn - 1) / bn;
  int blocks = kTilesPerCu * cu_count() / p.n_tiles;
  if (blocks < 1) blocks = 1;
  p.s_blocks = p.s_tiles < blocks ? p.s_tiles : blocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.wt = write_through((int64_t)B * H * W * COUT * (int64_t)sizeof(float));
  const dim3 grid(p.s_blocks * p.n_tiles), blk(256);
  hipStream_t st = (hipStream_t)stream;
  if (bn == 64) hipLaunchKernelGGL((k3i_fwd_kernel<4>), grid, blk, 0, st, p);
  else if (bn == 32) hipLaunchKernelGGL((k3i_fwd_kernel<2>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((k3i_fwd_kernel<1>), grid, blk, 0, st, p);
  return last_error();
}

size_t alignq_k3image_wgrad_ws_bytes(int B, int H, int W, int COUT) {
  if (!shape_ok(ALIGNQ_K3I_WGRAD, B, H, W, COUT, COUT)) return 0;
  const WGeom g = wgrad_geometry(B, H, W, COUT);
  return (size_t)g.splits * (size_t)COUT * IK * sizeof(float);
}

int alignq_k3image_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H, int W, int COUT, int* n_slabs_out,
                         void* stream) {
  if (!x || !dy || !ws || (!dw && !n_slabs_out) || !aligned16(x) || !aligned16(dy) || !aligned16(ws) || !aligned16(dw))
    return ALIGNQ_EINVAL;
  if (!shape_ok(ALIGNQ_K3I_WGRAD, B, H, W, COUT, COUT)) return ALIGNQ_EUNSUPPORTED;
  const WGeom g = wgrad_geometry(B, H, W, COUT);
  hipStream_t st = (hipStream_t)stream;
  K3IW a{};
  a.x = x; a.dy = dy; a.slabs = (float*)ws;
  a.H = H; a.W = W; a.COUT = COUT;
  a.th = g.th; a.tw = g.tw; a.s_tiles = g.s_tiles; a.per = g.per; a.o_tiles = g.o_tiles;
  hipLaunchKernelGGL(k3i_wgrad_kernel, dim3(g.o_tiles * g.splits), dim3(256), 0, st, a);
  int e = last_error();
  if (e) return e;
  if (n_slabs_out) { *n_slabs_out = g.splits; return 0; }      // deferred: the caller reduces (alignq_conv3x3_wgrad_reduce_multi)
  const int n_elem = COUT * IK;
  hipLaunchKernelGGL(k3i_slab_reduce_kernel, dim3(alignq_wgr::wgrad_reduce_blocks(g.splits, n_elem, kRedThreads)), dim3(kRedThreads), 0,
                     st, (const float*)ws, g.splits, n_elem, dw);
  return last_error();
}

}  // extern "C"

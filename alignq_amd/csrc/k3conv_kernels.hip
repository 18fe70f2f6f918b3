// k3conv_kernels.hip — Conv2d_Q's 3x3 / stride 1 / padding 1 convolutions (reference: cdf_alignment/dense-cifar-10/model/
// quantization.py, F.conv2d(input, weight_q, ...)) at any channel count that is a multiple of 4: DenseNet-40's dense layers,
// CIN = 24, 36, ..., 444 -> COUT = 12.  Forward, data gradient and filter gradient with the arithmetic of pointwise_kernels.hip:
// the filter's integer bins as bf16, the fp32 operand in three exact bf16 terms, v_mfma_f32_16x16x32_bf16, fp32 accumulation in an
// order the shape fixes, one division (the primitives: exact_mma.h; the launchers' shared rules: exact_conv_host.h).  include/alignq_k3conv.h states the contract.  The geometry:
//   forward / data gradient  one workgroup = 256 threads = 4 waves = an 8 x 8 pixel tile of ONE image x 16, 32 or 64 output channels.
//           Per 32-deep channel chunk the tile WITH ITS HALO (10 x 10 pixels) is staged in LDS once, already split into the three
//           term images; the nine taps read it at shifted rows, so an element is split once, not nine times.  Halo pixels outside
//           the image, tile pixels beyond it and channels beyond K are zeros; a halo never reaches into a neighbouring image or row.
//           The chunk's filter taps are staged [tap][n][k]; the data gradient reads the same bins flipped (tap 8 - t) and transposed
//           ([k][tap][n] in memory) while staging, so both forms read one LDS image.
//   filter gradient  a 32-pixel k step = a 4 x 8 pixel tile of one image; x is staged with its halo (6 x 10 pixels), dy without, both
//           [pixel][channel] in three term planes and read through ds_read_b64_tr_b16; every tap reads x at its own shifted rows.
//           A wave owns 16 input x 16 output channels x 9 taps (36 accumulator registers); the four waves lie along CIN or along COUT.
// MFMA roles as in pointwise_kernels.hip: A operand = filter side (rows of D, 4 consecutive per lane -> one float4 store per lane),
// B operand = pixel side (columns of D).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_k3conv.h"
#include "exact_conv_host.h"
#include "exact_mma.h"
#include "wgrad_reduce_body.h"

using namespace alignq_xmma;

namespace {

constexpr int BK = 32;                 // channels per chunk (one MFMA k step)
constexpr int LDX = BK + 8;            // halfwords per LDS row: 80 B rows, 16 lanes' ds_read_b128 on 16 distinct 16-byte slots
constexpr int TS = 8;                  // forward / data gradient: the spatial tile is TS x TS pixels
constexpr int HS = TS + 2, HP = HS * HS;          // with its halo: 10 x 10
constexpr int kMaxTileBlocks = 2048;   // grid cap over spatial tiles; the rest by grid stride
constexpr int kMinC = 4, kMaxC = 512;

// ---------------------------------------------------------------------------------------------------------------------------
// Forward and data gradient:  out[b][h][w][n] = (1 / nlev) * sum_{t = (ty, tx)} sum_k a[b][h + ty - 1][w + tx - 1][k] * Wb(n, t, k)
//   forward (WTR = false): a = x, K = CIN, N = COUT, Wb(n, t, k) = w[n][t][k] - rows k-contiguous, 8-byte pieces of 4 k;
//   data gradient (WTR = true): a = dy, K = COUT, N = CIN, Wb(n, t, k) = w[k][8 - t][n]: 8-byte pieces of 4 n are read along the
//   filter's rows and staged transposed.
struct K3 {
  const float* a; const u16* w; float* out;
  int H, W, K, N;
  int th, tw;                         // tiles along H and W
  int s_tiles, s_blocks, n_tiles;     // spatial tiles, spatial tiles the grid holds (stride of the rest), channel tiles
  float nlev;
  int wt;                             // write-through output stores
};

template <int TN, bool WTR>
__global__ __launch_bounds__(256, 2) void k3_gemm_kernel(const K3 p) {
  constexpr int BN = 16 * TN;
  constexpr int XPL = HP * LDX;                       // halfwords per pixel-side term plane
  constexpr int WPL = BN * LDX;                       // halfwords per filter tap
  constexpr int NAP = HP * (BK / 4);                  // float4 of the halo tile
  constexpr int NA = (NAP + 255) / 256;
  constexpr int NBP = 9 * BN * (BK / 4);              // 8-byte pieces (4 bins) of the nine filter taps
  constexpr int NB = (NBP + 255) / 256;
  // The transposed filter staging of the data gradient is 2-byte LDS stores.  At 64 channels (18 pieces per thread) it walks only the
  // rows below K and zero-fills the rest in 8-byte pieces: 0.81 - 0.84x of the full walk's time at K = 12, in two runs.  At 16 and 32
  // channels (5 and 9 pieces per thread) the same walk, with its run-time divisor, measured no gain (1.05 - 1.09x of the full walk in
  // the run before it, 1.1x of the run after it), so they walk all 32 rows (NOTES.md, "3x3 Conv2d_Q at DenseNet-40's widths").
  constexpr bool LIVE = WTR && TN == 4;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + 9 * WPL];
  u16* const Xs = lds;
  u16* const Ws = lds + 3 * XPL;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = pid % p.n_tiles, sb = pid / p.n_tiles;
  const int n0 = nt * BN;
  const int fr = lane & 15, fg = lane >> 4;
  const int pl = wv * 16 + fr, py = pl >> 3, px = pl & 7;          // this lane's pixel of the tile (B operand column)
  const int nk = (p.K + BK - 1) / BK;
  const int per_img = p.th * p.tw;

  for (int st = sb; st < p.s_tiles; st += p.s_blocks) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / p.tw) * TS, w0 = (r % p.tw) * TS;
    const int64_t img = (int64_t)b * p.H * p.W;
    f32x4 ra[NA];
    s16x4 rw[NB];
    auto fetch = [&](int kt) {
      const int k0 = kt * BK;
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int idx = tid + 256 * i, hp = idx >> 3, c4 = idx & 7;
        const int hy = hp / HS, hx = hp - hy * HS;
        const int h = h0 + hy - 1, w = w0 + hx - 1, k = k0 + 4 * c4;
        const bool ok = idx < NAP && h >= 0 && h < p.H && w >= 0 && w < p.W && k < p.K;
        ra[i] = *reinterpret_cast<const f32x4*>(p.a + (ok ? (img + (int64_t)h * p.W + w) * p.K + k : 0));
        if (!ok) ra[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        int n, k, t;
        bool ok = idx < NBP;
        if (!WTR) { k = k0 + 4 * (idx & 7); n = n0 + (idx >> 3) % BN; t = (idx >> 3) / BN; }
        else {          // LIVE: only the chunk's kc live rows are walked (K = COUT = 12: 12 of 32); park() zero-fills the others
          const int kc = LIVE && p.K - k0 < BK ? p.K - k0 : BK, r = idx / (BN / 4);
          n = n0 + 4 * (idx % (BN / 4)); k = k0 + r % kc; t = 8 - r / kc;
          ok = r < 9 * kc;
        }
        ok = ok && n < p.N && k < p.K;
        const int64_t off = WTR ? ((int64_t)k * 9 + t) * p.N + n : ((int64_t)n * 9 + t) * p.K + k;
        rw[i] = *reinterpret_cast<const s16x4*>(p.w + (ok ? off : 0));
        if (!ok) rw[i] = (s16x4){0, 0, 0, 0};
      }
    };
    auto park = [&](int kt) {
      const int kc = LIVE && p.K - kt * BK < BK ? p.K - kt * BK : BK;          // rows of this chunk that are walked (a multiple of 4)
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int idx = tid + 256 * i;
        if (idx >= NAP) continue;
        const int o = (idx >> 3) * LDX + 4 * (idx & 7);
        s16x4 h, m, l;
        split3(ra[i], h, m, l);
        *reinterpret_cast<s16x4*>(Xs + o) = h;
        *reinterpret_cast<s16x4*>(Xs + XPL + o) = m;
        *reinterpret_cast<s16x4*>(Xs + 2 * XPL + o) = l;
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        if (idx >= NBP) continue;
        if (!WTR) {
          *reinterpret_cast<s16x4*>(Ws + ((idx >> 3) / BN) * WPL + ((idx >> 3) % BN) * LDX + 4 * (idx & 7)) = rw[i];
        } else {
          const int n4 = idx % (BN / 4), r = idx / (BN / 4);
          if (r >= 9 * kc) continue;
          const int kr = r % kc, t = r / kc;
#pragma unroll
          for (int j = 0; j < 4; j++) Ws[t * WPL + (4 * n4 + j) * LDX + kr] = (u16)rw[i][j];
        }
      }
      if (LIVE && kc < BK) {         // rows kc .. 31 of every (tap, n) line: zeros, in 8-byte pieces
        const int nz = (BK - kc) / 4;
        for (int j = tid; j < 9 * BN * nz; j += 256)
          *reinterpret_cast<s16x4*>(Ws + (j / nz) * LDX + kc + 4 * (j % nz)) = (s16x4){0, 0, 0, 0};
      }
    };

    f32x4 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int kt = 0; kt < nk; kt++) {
      __syncthreads();                         // the previous chunk's fragment reads are done
      park(kt);
      __syncthreads();
      if (kt + 1 < nk) fetch(kt + 1);          // in flight under this chunk's MFMAs
#pragma unroll 1
      for (int ty = 0; ty < 3; ty++) {         // taps in ascending order of the pixel read: rows (one row's fragments in registers) ...
#pragma unroll
        for (int tx = 0; tx < 3; tx++) {       // ... then columns
          const u16* pw = Ws + (3 * ty + tx) * WPL + fr * LDX + 8 * fg;
          s16x8 wf[TN];
#pragma unroll
          for (int tn = 0; tn < TN; tn++) wf[tn] = *reinterpret_cast<const s16x8*>(pw + tn * 16 * LDX);
          const u16* pxs = Xs + ((py + ty) * HS + px + tx) * LDX + 8 * fg;
#pragma unroll
          for (int s = 2; s >= 0; s--) {       // smallest term first
            const s16x8 xf = *reinterpret_cast<const s16x8*>(pxs + s * XPL);
#pragma unroll
            for (int tn = 0; tn < TN; tn++) acc[tn] = mfma16(wf[tn], xf, acc[tn]);
          }
        }
      }
    }
    // epilogue: lane = pixel (lane & 15) of the wave's 16, 4 consecutive channels 4 * (lane >> 4) + e of every 16-channel block
    const int h = h0 + py, w = w0 + px;
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      const int n = n0 + tn * 16 + 4 * fg;
      f32x4 v = acc[tn];
      v = (f32x4){v[0] / p.nlev, v[1] / p.nlev, v[2] / p.nlev, v[3] / p.nlev};
      if (h < p.H && w < p.W && n < p.N) st_out(p.out + (img + (int64_t)h * p.W + w) * p.N + n, v, p.wt);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Filter gradient:  slab[split][co][t][ci] = sum over the split's spatial tiles of dy[pixel][co] * x[pixel + t's offset][ci]
// A step is one 4 x 8 pixel tile (k = 8 row + column).  Lane group g takes pixels {4g .. 4g+3} and {16 + 4g .. 16 + 4g + 3} of the
// step on both operands: tile rows g >> 1 and 2 + (g >> 1).  Channels beyond CIN / COUT are staged as zeros and never stored.
constexpr int WTH = 4, WTW = 8, WK = WTH * WTW;
constexpr int WHW = WTW + 2, WHP = (WTH + 2) * WHW;          // x with its halo: 6 x 10 pixels
struct K3W {
  const float* x; const float* dy; float* slabs;
  int H, W, CIN, COUT;
  int th, tw, s_tiles, per;        // tiles along H and W, spatial tiles in all, spatial tiles per split
  int c_tiles, o_tiles;
};

template <int CB, int OB>
__global__ __launch_bounds__(256, 2) void k3_wgrad_kernel(const K3W a) {
  static_assert((CB == 64 && OB == 16) || (CB == 16 && OB == 64), "four waves along CIN or along COUT");
  constexpr int LDC = CB + 16, LDO = OB + 16;
  constexpr int XPL = WHP * LDC, DPL = WK * LDO;
  constexpr int NXP = WHP * CB / 4, NX = (NXP + 255) / 256;
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
    const int64_t img = (int64_t)b * a.H * a.W;
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i, hp = idx / (CB / 4), q4 = idx % (CB / 4);
      const int hy = hp / WHW, hx = hp - hy * WHW;
      const int h = h0 + hy - 1, w = w0 + hx - 1, c = c0 + 4 * q4;
      const bool ok = idx < NXP && h >= 0 && h < a.H && w >= 0 && w < a.W && c < a.CIN;
      rx[i] = *reinterpret_cast<const f32x4*>(a.x + (ok ? (img + (int64_t)h * a.W + w) * a.CIN + c : 0));
      if (!ok) rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (OB / 4), q4 = idx % (OB / 4);
      const int h = h0 + (kr >> 3), w = w0 + (kr & 7), o = o0 + 4 * q4;
      const bool ok = idx < NDP && h < a.H && w < a.W && o < a.COUT;
      rd[i] = *reinterpret_cast<const f32x4*>(a.dy + (ok ? (img + (int64_t)h * a.W + w) * a.COUT + o : 0));
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

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
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
    for (int t = 0; t < 9; t++) {
      s16x8 xf[3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
        const u16* p = Xs + s * XPL + ((ky + t / 3) * WHW + kx + t % 3) * LDC + wc * 16 + fc;
        xf[s] = join8(tr_read(p), tr_read(p + 2 * WHW * LDC));
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
  float* slab = a.slabs + (int64_t)split * a.COUT * 9 * a.CIN;
  const int o = o0 + wo * 16 + (lane & 15), c = c0 + wc * 16 + 4 * fg;
  if (o < a.COUT && c < a.CIN) {
#pragma unroll
    for (int t = 0; t < 9; t++)
      __builtin_nontemporal_store(acc[t], reinterpret_cast<f32x4*>(slab + ((int64_t)o * 9 + t) * a.CIN + c));
  }
}

// The slab reduction of wgrad_reduce_body.h at 256 threads (pointwise_kernels.hip: same groups, same order, same bits as the
// 1024-thread alignq_conv3x3_wgrad_reduce_multi).
constexpr int kRedThreads = 256;
__global__ __launch_bounds__(kRedThreads) void k3_slab_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int n_elem,
                                                                     float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float part[4 * kRedThreads];
  alignq_wgr::wgrad_reduce_body<kRedThreads>(slabs, n_slabs, n_elem, dw, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------------------
inline bool shape_ok(int B, int H, int W, int CIN, int COUT) {
  if (CIN < kMinC || CIN > kMaxC || (CIN & 3) || COUT < kMinC || COUT > kMaxC || (COUT & 3) || B < 1 || H < 1 || W < 1) return false;
  return fits31(B, H, W, CIN > COUT ? CIN : COUT);
}

inline int gemm_form(int N) {
  const int bn = n_tile_width(N);
  return bn == 64 ? ALIGNQ_K3_FORM_N64 : (bn == 32 ? ALIGNQ_K3_FORM_N32 : ALIGNQ_K3_FORM_N16);
}
inline int wgrad_form(int CIN, int COUT) { return CIN >= COUT ? ALIGNQ_K3_FORM_W64X16 : ALIGNQ_K3_FORM_W16X64; }

template <bool WTR>
int launch_gemm(const float* a, const void* w, float* out, int B, int H, int W, int K, int N, int w_bit, hipStream_t st) {
  K3 p{};
  p.a = a; p.w = (const u16*)w; p.out = out;
  p.H = H; p.W = W; p.K = K; p.N = N;
  p.th = (H + TS - 1) / TS; p.tw = (W + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;                       // <= B * H * W
  p.s_blocks = p.s_tiles < kMaxTileBlocks ? p.s_tiles : kMaxTileBlocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.wt = write_through((int64_t)B * H * W * N * (int64_t)sizeof(float));
  const int bn = n_tile_width(N);
  p.n_tiles = (N + bn - 1) / bn;
  const dim3 grid(p.s_blocks * p.n_tiles), blk(256);
  if (bn == 64) hipLaunchKernelGGL((k3_gemm_kernel<4, WTR>), grid, blk, 0, st, p);
  else if (bn == 32) hipLaunchKernelGGL((k3_gemm_kernel<2, WTR>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((k3_gemm_kernel<1, WTR>), grid, blk, 0, st, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// split-K over slabs of spatial tiles: enough workgroups for the chip, at least two steps per slab, no empty slab
struct WGeom { int form, th, tw, s_tiles, c_tiles, o_tiles, per, splits; };
inline WGeom wgrad_geometry(int B, int H, int W, int CIN, int COUT) {
  WGeom g{};
  g.form = wgrad_form(CIN, COUT);
  const int cb = g.form == ALIGNQ_K3_FORM_W64X16 ? 64 : 16, ob = g.form == ALIGNQ_K3_FORM_W64X16 ? 16 : 64;
  g.th = (H + WTH - 1) / WTH; g.tw = (W + WTW - 1) / WTW;
  g.s_tiles = B * g.th * g.tw;
  g.c_tiles = (CIN + cb - 1) / cb; g.o_tiles = (COUT + ob - 1) / ob;
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

int alignq_k3conv_supported(int B, int H, int W, int CIN, int COUT) { return shape_ok(B, H, W, CIN, COUT) ? 1 : 0; }

int alignq_k3conv_form(int op, int B, int H, int W, int CIN, int COUT) {
  if (!shape_ok(B, H, W, CIN, COUT)) return -1;
  if (op == ALIGNQ_K3_FWD) return gemm_form(COUT);
  if (op == ALIGNQ_K3_DGRAD) return gemm_form(CIN);
  if (op == ALIGNQ_K3_WGRAD) return wgrad_form(CIN, COUT);
  return -1;
}

int alignq_k3conv_fwd(const float* x, const void* w_bins, float* y, int B, int H, int W, int CIN, int COUT, int w_bit, void* stream) {
  if (!x || !w_bins || !y || !aligned16(x) || !aligned16(w_bins) || !aligned16(y) || w_bit < 1 || w_bit > 8) return ALIGNQ_EINVAL;
  if (!shape_ok(B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  return launch_gemm<false>(x, w_bins, y, B, H, W, CIN, COUT, w_bit, (hipStream_t)stream);
}

int alignq_k3conv_dgrad(const float* dy, const void* w_bins, float* dx, int B, int H, int W, int CIN, int COUT, int w_bit,
                        void* stream) {
  if (!dy || !w_bins || !dx || !aligned16(dy) || !aligned16(w_bins) || !aligned16(dx) || w_bit < 1 || w_bit > 8) return ALIGNQ_EINVAL;
  if (!shape_ok(B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  return launch_gemm<true>(dy, w_bins, dx, B, H, W, COUT, CIN, w_bit, (hipStream_t)stream);
}

size_t alignq_k3conv_wgrad_ws_bytes(int B, int H, int W, int CIN, int COUT) {
  if (!shape_ok(B, H, W, CIN, COUT)) return 0;
  const WGeom g = wgrad_geometry(B, H, W, CIN, COUT);
  return (size_t)g.splits * (size_t)COUT * 9 * CIN * sizeof(float);
}

int alignq_k3conv_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H, int W, int CIN, int COUT,
                        int* n_slabs_out, void* stream) {
  if (!x || !dy || !ws || (!dw && !n_slabs_out) || !aligned16(x) || !aligned16(dy) || !aligned16(ws) || !aligned16(dw))
    return ALIGNQ_EINVAL;
  if (!shape_ok(B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  const WGeom g = wgrad_geometry(B, H, W, CIN, COUT);
  K3W a{};
  a.x = x; a.dy = dy; a.slabs = (float*)ws;
  a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
  a.th = g.th; a.tw = g.tw; a.s_tiles = g.s_tiles; a.per = g.per;
  a.c_tiles = g.c_tiles; a.o_tiles = g.o_tiles;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.c_tiles * g.o_tiles * g.splits), blk(256);
  if (g.form == ALIGNQ_K3_FORM_W64X16) hipLaunchKernelGGL((k3_wgrad_kernel<64, 16>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((k3_wgrad_kernel<16, 64>), grid, blk, 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (n_slabs_out) { *n_slabs_out = g.splits; return 0; }      // deferred: the caller reduces (alignq_conv3x3_wgrad_reduce_multi)
  const int n_elem = COUT * 9 * CIN;
  hipLaunchKernelGGL(k3_slab_reduce_kernel, dim3(alignq_wgr::wgrad_reduce_blocks(g.splits, n_elem, kRedThreads)), dim3(kRedThreads), 0,
                     st, (const float*)ws, g.splits, n_elem, dw);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

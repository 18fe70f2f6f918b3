// k5_fwd_body.h - the main loops of the 5x5 forward / data-gradient kernels (include/alignq_k5conv.h), stated once: the body form's
// tile loop (k5conv_kernels.hip: k5_gemm_kernel) and the image form's (k5_image_fwd_kernel), with what happens to a lane's finished
// accumulator left to the caller.  k5conv_kernels.hip gives them the plain store (K5Store: one division, one add of the bias, one
// float4); digit_eval_kernels.hip the folded site and the 2 x 2 max-pool.  Staging, MFMA order and tile walk are this text for both,
// so the fused kernels give the bits of the launches they replace.
//
// The epilogue is a callable  epi(b, h, w, n, acc):  this lane's pixel (h, w) of image b - possibly beyond the output - and acc[tn],
// its four channels n + 16 tn .. n + 16 tn + 3 of the tile's TN 16-channel blocks - possibly beyond N.  It is called by EVERY lane of
// the workgroup, once per tile, outside any divergent branch, so it may exchange values between lanes; bounds are its own business.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_mma.h"

namespace alignq_k5 {

using namespace alignq_xmma;

constexpr int BK = 32;                 // channels per chunk (one MFMA k step)
constexpr int LDX = BK + 8;            // halfwords per LDS row: 80 B rows, 16 lanes' ds_read_b128 on 16 distinct 16-byte slots
constexpr int KS = 5, NT = KS * KS;    // taps per row, taps
constexpr int TS = 8;                  // forward / data gradient: the spatial tile is TS x TS output pixels
constexpr int FS = TS + KS - 1, FP = FS * FS;     // its footprint: 12 x 12
constexpr int kMaxTileBlocks = 2048;   // grid cap over spatial tiles; the rest by grid stride
constexpr int kMinC = 4, kMaxC = 512;
constexpr int IK = 3 * NT;             // image form: the live k (75)
constexpr int IKP = 96;                // ... zero-tailed to three k steps

// ---------------------------------------------------------------------------------------------------------------------------
// Body form, forward and data gradient:
//   out[b][h][w][n] = (1 / nlev) * sum_{t = (ty, tx)} sum_k a[b][h + off + ty][w + off + tx][k] * Wb(n, t, k)  (+ bias[n])
//   forward (WTR = false): a = x (H x W), out = y (H-4 x W-4), off = 0, K = CIN, N = COUT, Wb(n, t, k) = w[n][t][k];
//   data gradient (WTR = true): a = dy (H-4 x W-4), out = dx (H x W), off = -4, K = COUT, N = CIN, Wb(n, t, k) = w[k][24 - t][n]: 8-byte
//   pieces of 4 n are read along the filter's rows and staged transposed.
struct K5 {
  const float* a; const u16* w; const float* bias; float* out;
  int AH, AW, OH, OW, K, N;
  int off;
  int th, tw;                         // tiles along OH and OW
  int s_tiles, s_blocks, n_tiles;     // spatial tiles, spatial tiles the grid holds (stride of the rest), channel tiles
  float nlev;
  int wt;                             // write-through output stores
};

// the first output channel of this workgroup's tile (both forms: channel tiles vary fastest over the remapped workgroup id)
template <int TN>
__device__ __forceinline__ int tile_n0(const int n_tiles) {
  return (xcd_remap(blockIdx.x, gridDim.x) % n_tiles) * (16 * TN);
}

// the plain epilogue's store of one lane's four channels n .. n + 3 of one pixel: ONE division, then ONE add of the bias
__device__ __forceinline__ void store_out(float* o, f32x4 v, const float nlev, const float* bias, const int n, const int wt) {
  v = (f32x4){v[0] / nlev, v[1] / nlev, v[2] / nlev, v[3] / nlev};
  if (bias) v = (f32x4){v[0] + bias[n], v[1] + bias[n + 1], v[2] + bias[n + 2], v[3] + bias[n + 3]};
  st_out(o, v, wt);
}

// the plain epilogue: the pixels and channels inside out[B][OH][OW][N]
struct K5Store {
  float* out; const float* bias;
  int OH, OW, N;
  float nlev;
  int wt;
  template <int TN>
  __device__ __forceinline__ void operator()(const int b, const int h, const int w, const int n4, const f32x4 (&acc)[TN]) const {
    const int64_t img_o = (int64_t)b * OH * OW;
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      const int n = n4 + tn * 16;
      if (h < OH && w < OW && n < N) store_out(out + (img_o + (int64_t)h * OW + w) * N + n, acc[tn], nlev, bias, n, wt);
    }
  }
};

template <int TN, bool WTR, class Epi>
__device__ __forceinline__ void k5_gemm_body(const K5& p, const Epi& epi) {
  constexpr int BN = 16 * TN;
  constexpr int XPL = FP * LDX;                       // halfwords per pixel-side term plane
  constexpr int WPL = BN * LDX;                       // halfwords per filter tap
  constexpr int NAP = FP * (BK / 4);                  // float4 of the footprint
  constexpr int NA = (NAP + 255) / 256;
  constexpr int NBP = KS * BN * (BK / 4);             // 8-byte pieces (4 bins) of one tap row
  constexpr int NB = (NBP + 255) / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + KS * WPL];
  u16* const Xs = lds;
  u16* const Ws = lds + 3 * XPL;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = pid % p.n_tiles, sb = pid / p.n_tiles;
  const int n0 = nt * BN;
  const int fr = lane & 15, fg = lane >> 4;
  const int pl = wv * 16 + fr, py = pl >> 3, px = pl & 7;          // this lane's pixel of the tile (B operand column)
  const int nk = (p.K + BK - 1) / BK, steps = KS * nk;
  const int per_img = p.th * p.tw;

  for (int st = sb; st < p.s_tiles; st += p.s_blocks) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / p.tw) * TS, w0 = (r % p.tw) * TS;
    const int64_t img_a = (int64_t)b * p.AH * p.AW;
    f32x4 ra[NA];
    s16x4 rw[NB];
    auto fetch_x = [&](int kt) {
      const int k0 = kt * BK;
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int idx = tid + 256 * i, fp = idx >> 3, c4 = idx & 7;
        const int hy = fp / FS, hx = fp - hy * FS;
        const int h = h0 + p.off + hy, w = w0 + p.off + hx, k = k0 + 4 * c4;
        const bool ok = idx < NAP && h >= 0 && h < p.AH && w >= 0 && w < p.AW && k < p.K;
        ra[i] = *reinterpret_cast<const f32x4*>(p.a + (ok ? (img_a + (int64_t)h * p.AW + w) * p.K + k : 0));
        if (!ok) ra[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    };
    auto fetch_w = [&](int s) {                       // tap row s % 5 of chunk s / 5
      const int kt = s / KS, ty = s - kt * KS, k0 = kt * BK;
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        int n, k, t;
        if (!WTR) { k = k0 + 4 * (idx & 7); n = n0 + (idx >> 3) % BN; t = KS * ty + (idx >> 3) / BN; }
        else { n = n0 + 4 * (idx % (BN / 4)); const int q = idx / (BN / 4); k = k0 + (q & (BK - 1)); t = NT - 1 - (KS * ty + q / BK); }
        const bool ok = idx < NBP && n < p.N && k < p.K;
        const int64_t off = WTR ? ((int64_t)k * NT + t) * p.N + n : ((int64_t)n * NT + t) * p.K + k;
        rw[i] = *reinterpret_cast<const s16x4*>(p.w + (ok ? off : 0));
        if (!ok) rw[i] = (s16x4){0, 0, 0, 0};
      }
    };
    auto park_x = [&]() {
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
    };
    auto park_w = [&]() {
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        if (idx >= NBP) continue;
        if (!WTR) {
          *reinterpret_cast<s16x4*>(Ws + ((idx >> 3) / BN) * WPL + ((idx >> 3) % BN) * LDX + 4 * (idx & 7)) = rw[i];
        } else {
          const int n4 = idx % (BN / 4), q = idx / (BN / 4), kr = q & (BK - 1), tx = q / BK;
#pragma unroll
          for (int j = 0; j < 4; j++) Ws[tx * WPL + (4 * n4 + j) * LDX + kr] = (u16)rw[i][j];
        }
      }
    };

    f32x4 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    fetch_x(0);
    fetch_w(0);
#pragma unroll 1
    for (int s = 0; s < steps; s++) {          // chunks ascending; inside a chunk the tap rows in ascending order of the pixel read
      const int kt = s / KS, ty = s - kt * KS;
      __syncthreads();                         // the previous tap row's fragment reads are done
      if (ty == 0) park_x();
      park_w();
      __syncthreads();
      if (ty == 0 && kt + 1 < nk) fetch_x(kt + 1);          // in flight under this chunk's MFMAs
      if (s + 1 < steps) fetch_w(s + 1);                    // ... under this tap row's
#pragma unroll
      for (int tx = 0; tx < KS; tx++) {        // ... then the columns
        const u16* pw = Ws + tx * WPL + fr * LDX + 8 * fg;
        s16x8 wf[TN];
#pragma unroll
        for (int tn = 0; tn < TN; tn++) wf[tn] = *reinterpret_cast<const s16x8*>(pw + tn * 16 * LDX);
        const u16* pxs = Xs + ((py + ty) * FS + px + tx) * LDX + 8 * fg;
#pragma unroll
        for (int q = 2; q >= 0; q--) {         // smallest term first
          const s16x8 xf = *reinterpret_cast<const s16x8*>(pxs + q * XPL);
#pragma unroll
          for (int tn = 0; tn < TN; tn++) acc[tn] = mfma16(wf[tn], xf, acc[tn]);
        }
      }
    }
    // epilogue: lane = pixel (lane & 15) of the wave's 16, 4 consecutive channels 4 * (lane >> 4) + e of every 16-channel block
    epi(b, h0 + py, w0 + px, n0 + 4 * fg, acc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Image form, forward:  y[b][h][w][n] = (1 / nlev) * sum_{k < 75} im[b][h][w][k] * w[n][k] + bias[n],
//   im[b][h][w][ky * 15 + kx * 3 + ci] = x[b][h + ky][w + kx][ci];  k steps ascending, inside a step the terms lo, mid, hi.
constexpr int LDK = IKP + 8;           // halfwords per row of the term images and of the filter tile: 208 B, 13 16-byte slots
constexpr int IPP = FP * 3;            // floats of the 12 x 12 x 3 patch
struct K5I {
  const float* x; const u16* w; const float* bias; float* y;
  int H, W, OH, OW, N;
  int th, tw, s_tiles, s_blocks, n_tiles;
  float nlev;
  int wt;
};

// one float of a patch in its three terms (split3 on a padded quad: the same bits as every other split of the family)
__device__ __forceinline__ void split3_one(const float v, u16& h, u16& m, u16& l) {
  s16x4 hh, mm, ll;
  split3((f32x4){v, 0.f, 0.f, 0.f}, hh, mm, ll);
  h = (u16)hh[0]; m = (u16)mm[0]; l = (u16)ll[0];
}

// The filter tile's live rows are ONE contiguous run of `rows` * 75 halfwords (an even count, 4-byte aligned: n0 is a multiple of 16):
// read in 4-byte words, scattered halfword by halfword into [row][LDK]; the k tail and the rows beyond N were zero-filled before.
__device__ __forceinline__ void stage_image_filter(u16* Ws, const u16* w_tile, const int rows, const int tid) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(w_tile);
  for (int j = tid; 2 * j < rows * IK; j += 256) {
    const uint32_t v = src[j];
    const int e0 = 2 * j, e1 = e0 + 1;
    Ws[(e0 / IK) * LDK + e0 % IK] = (u16)(v & 0xffffu);
    Ws[(e1 / IK) * LDK + e1 % IK] = (u16)(v >> 16);
  }
}

// X1: x is a ONE-channel image [B][H][W] whose value stands for all three ci (the reference's `expand`); else [B][H][W][3]
template <int TN, bool X1, class Epi>
__device__ __forceinline__ void k5_image_fwd_body(const K5I& p, const Epi& epi) {
  constexpr int BN = 16 * TN;
  constexpr int IPL = TS * TS * LDK;                  // halfwords per term image
  constexpr int NP = (IPP + 255) / 256;               // patch floats per thread
  __shared__ __attribute__((aligned(16))) u16 lds[3 * IPL + 3 * IPP + BN * LDK];
  u16* const Is = lds;
  u16* const Ps = lds + 3 * IPL;
  u16* const Ws = Ps + 3 * IPP;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = pid % p.n_tiles, sb = pid / p.n_tiles;
  const int n0 = nt * BN;
  const int fr = lane & 15, fg = lane >> 4;
  const int pl = wv * 16 + fr, py = pl >> 3, px = pl & 7;
  const int per_img = p.th * p.tw;

  // the filter tile, once per workgroup
  for (int j = tid; j < BN * LDK / 2; j += 256) reinterpret_cast<uint32_t*>(Ws)[j] = 0u;
  __syncthreads();
  stage_image_filter(Ws, p.w + (int64_t)n0 * IK, p.N - n0 < BN ? p.N - n0 : BN, tid);
  __syncthreads();
  s16x8 wf[3][TN];
#pragma unroll
  for (int ks = 0; ks < 3; ks++)
#pragma unroll
    for (int tn = 0; tn < TN; tn++) wf[ks][tn] = *reinterpret_cast<const s16x8*>(Ws + (tn * 16 + fr) * LDK + BK * ks + 8 * fg);

  float rp[NP];
  auto fetch = [&](int st) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / p.tw) * TS, w0 = (r % p.tw) * TS;
    const int64_t img = (int64_t)b * p.H * p.W;
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const int idx = tid + 256 * i, fp = idx / 3, ci = idx - 3 * fp;
      const int hy = fp / FS, hx = fp - hy * FS;
      const int h = h0 + hy, w = w0 + hx;
      const bool ok = idx < IPP && h < p.H && w < p.W;
      if constexpr (X1) rp[i] = ok ? p.x[img + (int64_t)h * p.W + w] : 0.f;
      else rp[i] = ok ? p.x[(img + (int64_t)h * p.W + w) * 3 + ci] : 0.f;
    }
  };

  if (sb < p.s_tiles) fetch(sb);
  for (int st = sb; st < p.s_tiles; st += p.s_blocks) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / p.tw) * TS, w0 = (r % p.tw) * TS;
    __syncthreads();                           // the previous tile's fragment reads are done
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const int idx = tid + 256 * i;
      if (idx >= IPP) continue;
      split3_one(rp[i], Ps[idx], Ps[IPP + idx], Ps[2 * IPP + idx]);
    }
    __syncthreads();
    if (st + p.s_blocks < p.s_tiles) fetch(st + p.s_blocks);
    for (int j = tid; j < TS * TS * IKP; j += 256) {          // the term images: [pixel][k], zeros beyond k = 74
      const int pix = j / IKP, k = j - pix * IKP;
      const bool live = k < IK;
      const int ky = k / 15, src = live ? (((pix >> 3) + ky) * FS + (pix & 7)) * 3 + (k - 15 * ky) : 0;
#pragma unroll
      for (int q = 0; q < 3; q++) Is[q * IPL + pix * LDK + k] = live ? Ps[q * IPP + src] : (u16)0;
    }
    __syncthreads();
    f32x4 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 3; ks++) {
#pragma unroll
      for (int q = 2; q >= 0; q--) {           // smallest term first
        const s16x8 xf = *reinterpret_cast<const s16x8*>(Is + q * IPL + pl * LDK + BK * ks + 8 * fg);
#pragma unroll
        for (int tn = 0; tn < TN; tn++) acc[tn] = mfma16(wf[ks][tn], xf, acc[tn]);
      }
    }
    epi(b, h0 + py, w0 + px, n0 + 4 * fg, acc);
  }
}

// the launch geometry both forms share: tiles along the output, the grid cap, the channel tile (exact_conv_host.h: n_tile_width)
template <class P>
inline void tile_geometry(P& p, const int B, const int OH, const int OW, const int bn, const int N) {
  p.th = (OH + TS - 1) / TS; p.tw = (OW + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;                       // <= B * H * W
  p.s_blocks = p.s_tiles < kMaxTileBlocks ? p.s_tiles : kMaxTileBlocks;
  p.n_tiles = (N + bn - 1) / bn;
}

}  // namespace alignq_k5

// dense_train_kernels.hip — DenseNet's dense blocks in TRAINING without concatenations (the reference's train() on
// cdf_alignment/dense-cifar-10/model/densenet.py:17-41) for gfx950; include/alignq_dense_train.h states the contracts.  One buffer
// [B][H][W][C_end] per block and one gradient buffer of the same shape; a layer reads the first CIN channels of every pixel at the
// buffer's pitch and writes its COUT channels behind them.  The quantised activation and the ReLU mask are never written: every
// kernel that needs them forms relu(q(fma(a, z, b))) again from the buffer and the layer's [2][CIN] `ab`.  Each launch reproduces an
// existing one bit for bit, because it runs that launch's text with other addresses:
//   alignq_dense_train_stats      any_sums_kernel<0> at a pitch + any_finalize_fwd_kernel (bnq_any_body.h: alignq_bnq_any_fwd's)
//   alignq_dense_train_layer_fwd  dt_gemm_kernel<TN, false, FORMULA, BOUNDED>: k3conv_kernels.hip's k3_gemm_kernel (10 x 10 halo tile
//                                 of 32-channel chunks, nine taps, three terms smallest first) with pitches on both sides and the
//                                 training site (eval_site_body.h: site_q_fma) between a float4's load and its split3, as
//                                 dense_eval_kernels.hip applies the evaluation site; what is not loaded is stored as zeros BEHIND it
//   alignq_dense_train_dgrad      dt_gemm_kernel<TN, true, 2, false>: the same kernel without a site, filter flipped and transposed
//   alignq_dense_train_wgrad      dt_wgrad_kernel: k3_wgrad_kernel's 6 x 10 halo staging, six term pairs and slabs, the x operand
//                                 formed by the site while it is parked, dy at a pitch; then the slab reduction of wgrad_reduce_body.h
//   alignq_dense_train_site_bwd   dt_sums_bwd_kernel (any_sums_kernel<1>'s loop; the gate formed instead of read) ->
//                                 any_finalize_bwd_kernel -> dt_apply_bwd_kernel: G = G + a * ((dx - k0) - zhat * k1) at a pitch
// LDS: the erf table (1472 B) and the [2][CIN] table (4 KB at CIN = 512) lie beside the operand planes: 75.6 KB in the forward at 64
// output channels, 40.5 KB in the 64 x 16 filter gradient - two workgroups per CU (160 KB), the occupancy of the launches replaced.
// Every sum and product of the site is an individual fp32 operation except the fma written (-ffp-contract=off); built without packed
// fp32 arithmetic like the other code objects added since k5conv_kernels.hip (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_dense_train.h"
#include "alignq_math.h"
#include "eval_site_body.h"
#include "exact_conv_host.h"
#include "exact_mma.h"
#include "wgrad_reduce_body.h"
#include "bnq_any_body.h"              // the reductions, the finalisations and their geometry: alignq_bnq_any_fwd / _bwd's own

using namespace alignq;
using namespace alignq_evalsite;
using namespace alignq_xmma;

namespace {

// the geometry of k3conv_kernels.hip
constexpr int BK = 32;                 // channels per chunk (one MFMA k step)
constexpr int LDX = BK + 8;            // halfwords per LDS row
constexpr int TS = 8;                  // forward / data gradient: the spatial tile is TS x TS pixels
constexpr int HS = TS + 2, HP = HS * HS;          // with its halo: 10 x 10
constexpr int kMaxTileBlocks = 2048;   // grid cap over spatial tiles; the rest by grid stride
constexpr int kMinC = 4, kMaxC = 512;
constexpr int kTA = 256, kApplyBlocks = 2048;     // the accumulating apply pass: threads, grid cap (the rest by grid stride)

// relu(q(fma(a, z, b))) of one channel quad: alignq_bnq_any_fwd's y under ALIGNQ_CLAMP_RELU
template <int FORMULA, bool BOUNDED>
__device__ __forceinline__ f32x4 site_relu(const f32x4 v, const float* ab_s, int C, int cq, int k, const Levels& nlev, float r,
                                           const NerfTab tab) {
  const float4 q = clamp4(site_q_fma<FORMULA, BOUNDED>(make_float4(v[0], v[1], v[2], v[3]), ab_s, C, cq, k, nlev, r, tab),
                          ALIGNQ_CLAMP_RELU);
  return (f32x4){q.x, q.y, q.z, q.w};
}

// ---------------------------------------------------------------------------------------------------------------------------
// Forward and data gradient:  out[p][n] = (1 / nlev) * sum_{t = (ty, tx)} sum_k s(a[p + t's offset][k]) * Wb(n, t, k);
// pixel p of a at a + p * lda, of out at out + p * ldo.
//   forward (WTR = false, FORMULA 0 / 1): a = the buffer, s = the site of channel k, K = CIN, N = COUT, Wb(n, t, k) = w[n][t][k];
//   data gradient (WTR = true, FORMULA 2): a = the gradient buffer's COUT channels, s = identity, K = COUT, N = CIN,
//   Wb(n, t, k) = w[k][8 - t][n], staged transposed (k3conv_kernels.hip: LIVE walks only the rows below K at 64 channels).
struct DG {
  const float* a; const u16* w; float* out; const float* ab;
  int lda, ldo;
  int H, W, K, N;
  int th, tw;                         // tiles along H and W
  int s_tiles, s_blocks, n_tiles;     // spatial tiles, spatial tiles the grid holds (stride of the rest), channel tiles
  float nlev, r;
  int k;                              // the activation quantiser's bits
  int wt;                             // write-through output stores
};

template <int TN, bool WTR, int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(256, 2) void dt_gemm_kernel(const DG p) {
  constexpr bool SITE = FORMULA != 2;
  constexpr int BN = 16 * TN;
  constexpr int XPL = HP * LDX;                       // halfwords per pixel-side term plane
  constexpr int WPL = BN * LDX;                       // halfwords per filter tap
  constexpr int NAP = HP * (BK / 4);                  // float4 of the halo tile
  constexpr int NA = (NAP + 255) / 256;
  constexpr int NBP = 9 * BN * (BK / 4);              // 8-byte pieces (4 bins) of the nine filter taps
  constexpr int NB = (NBP + 255) / 256;
  constexpr bool LIVE = WTR && TN == 4;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + 9 * WPL];
  __shared__ __attribute__((aligned(16))) float tab_lds[SITE ? ALIGNQ_NERF_LDS_FLOATS : 4];
  __shared__ __attribute__((aligned(16))) float ab_s[SITE ? 2 * kMaxC : 4];      // [2][K]
  u16* const Xs = lds;
  u16* const Ws = lds + 3 * XPL;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (SITE) {                                 // (the first barrier of the chunk loop stands in front of the first read)
    nerf_tab_load(tab_lds);
    for (int i = tid; i < 2 * p.K; i += 256) ab_s[i] = p.ab[i];
  }
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev_q = make_levels(p.k, fabsf(p.r) <= 8.0f);

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
    unsigned live = 0;                         // bit i: ra[i] was loaded (else it is a zero that stays a zero behind the site)
    auto fetch = [&](int kt) {
      const int k0 = kt * BK;
      live = 0;
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int idx = tid + 256 * i, hp = idx >> 3, c4 = idx & 7;
        const int hy = hp / HS, hx = hp - hy * HS;
        const int h = h0 + hy - 1, w = w0 + hx - 1, k = k0 + 4 * c4;
        const bool ok = idx < NAP && h >= 0 && h < p.H && w >= 0 && w < p.W && k < p.K;
        ra[i] = *reinterpret_cast<const f32x4*>(p.a + (ok ? (img + (int64_t)h * p.W + w) * p.lda + k : 0));
        if (!ok) ra[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        live |= (ok ? 1u : 0u) << i;
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        int n, k, t;
        bool ok = idx < NBP;
        if (!WTR) { k = k0 + 4 * (idx & 7); n = n0 + (idx >> 3) % BN; t = (idx >> 3) / BN; }
        else {          // LIVE: only the chunk's kc live rows are walked; park() zero-fills the others
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
        f32x4 v = ra[i];
        if constexpr (SITE) {
          const bool ok = (live >> i) & 1u;
          const int cq = ok ? kt * (BK / 4) + (idx & 7) : 0;        // (a quad that was not loaded reads row 0 and is discarded)
          const f32x4 q = site_relu<FORMULA, BOUNDED>(v, ab_s, p.K, cq, p.k, nlev_q, p.r, tab);
          v = ok ? q : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        s16x4 h, m, l;
        split3(v, h, m, l);
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
      __syncthreads();                         // the previous chunk's fragment reads are done (first trip: the tables are written)
      park(kt);
      __syncthreads();
      if (kt + 1 < nk) fetch(kt + 1);          // in flight under this chunk's MFMAs
#pragma unroll 1
      for (int ty = 0; ty < 3; ty++) {         // taps in ascending order of the pixel read: rows ...
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
      if (h < p.H && w < p.W && n < p.N) st_out(p.out + (img + (int64_t)h * p.W + w) * p.ldo + n, v, p.wt);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Filter gradient:  slab[split][co][t][ci] = sum over the split's spatial tiles of dy[pixel][co] * s(z[pixel + t's offset][ci]),
// s = the training site with the ReLU.  k3_wgrad_kernel's steps (one 4 x 8 pixel tile; x with its 6 x 10 halo, dy without; both
// [pixel][channel] in three term planes read through ds_read_b64_tr_b16; 36 accumulator registers per wave) with the site applied
// to a float4 of the halo tile between its load and its split3, once per (input-channel tile, output-channel tile) workgroup.
constexpr int WTH = kK3WgradTileH, WTW = kK3WgradTileW, WK = WTH * WTW;
constexpr int WHW = WTW + 2, WHP = (WTH + 2) * WHW;          // x with its halo: 6 x 10 pixels
struct DW {
  const float* z; const float* dy; const float* ab; float* slabs;
  int ldz, lddy;
  int H, W, CIN, COUT;
  int th, tw, s_tiles, per;        // tiles along H and W, spatial tiles in all, spatial tiles per split
  int c_tiles, o_tiles;
  float r;
  int k;
};

template <int CB, int OB, int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(256, 2) void dt_wgrad_kernel(const DW a) {
  static_assert((CB == 64 && OB == 16) || (CB == 16 && OB == 64), "four waves along CIN or along COUT");
  constexpr int LDC = CB + 16, LDO = OB + 16;
  constexpr int XPL = WHP * LDC, DPL = WK * LDO;
  constexpr int NXP = WHP * CB / 4, NX = (NXP + 255) / 256;
  constexpr int NDP = WK * OB / 4, ND = (NDP + 255) / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + 3 * DPL];
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float ab_s[2 * kMaxC];        // [2][CIN]
  u16* const Xs = lds;
  u16* const Ds = lds + 3 * XPL;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  nerf_tab_load(tab_lds);                     // (the first barrier of the step loop stands in front of the first read)
  for (int i = tid; i < 2 * a.CIN; i += 256) ab_s[i] = a.ab[i];
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev_q = make_levels(a.k, fabsf(a.r) <= 8.0f);
  const int wc = CB == 64 ? wv : 0, wo = OB == 64 ? wv : 0;
  const int tiles = a.c_tiles * a.o_tiles;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = pid / tiles, tile = pid % tiles;
  const int ct = tile % a.c_tiles, ot = tile / a.c_tiles;
  const int c0 = ct * CB, o0 = ot * OB;
  const int t_begin = split * a.per, t_end = (t_begin + a.per < a.s_tiles) ? t_begin + a.per : a.s_tiles;
  const int per_img = a.th * a.tw;

  f32x4 rx[NX], rd[ND];
  unsigned live = 0;                           // bit i: rx[i] was loaded
  auto fetch = [&](int st) {
    const int b = st / per_img, r = st - b * per_img;
    const int h0 = (r / a.tw) * WTH, w0 = (r % a.tw) * WTW;
    const int64_t img = (int64_t)b * a.H * a.W;
    live = 0;
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i, hp = idx / (CB / 4), q4 = idx % (CB / 4);
      const int hy = hp / WHW, hx = hp - hy * WHW;
      const int h = h0 + hy - 1, w = w0 + hx - 1, c = c0 + 4 * q4;
      const bool ok = idx < NXP && h >= 0 && h < a.H && w >= 0 && w < a.W && c < a.CIN;
      rx[i] = *reinterpret_cast<const f32x4*>(a.z + (ok ? (img + (int64_t)h * a.W + w) * a.ldz + c : 0));
      if (!ok) rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      live |= (ok ? 1u : 0u) << i;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (OB / 4), q4 = idx % (OB / 4);
      const int h = h0 + (kr >> 3), w = w0 + (kr & 7), o = o0 + 4 * q4;
      const bool ok = idx < NDP && h < a.H && w < a.W && o < a.COUT;
      rd[i] = *reinterpret_cast<const f32x4*>(a.dy + (ok ? (img + (int64_t)h * a.W + w) * a.lddy + o : 0));
      if (!ok) rd[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i;
      if (idx >= NXP) continue;
      const int o = (idx / (CB / 4)) * LDC + 4 * (idx % (CB / 4));
      const bool ok = (live >> i) & 1u;
      const int cq = ok ? (c0 >> 2) + idx % (CB / 4) : 0;           // (a quad that was not loaded reads row 0 and is discarded)
      const f32x4 q = site_relu<FORMULA, BOUNDED>(rx[i], ab_s, a.CIN, cq, a.k, nlev_q, a.r, tab);
      s16x4 h, m, l;
      split3(ok ? q : (f32x4){0.f, 0.f, 0.f, 0.f}, h, m, l);
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

// the slab reduction of wgrad_reduce_body.h at 256 threads, as k3conv_kernels.hip instantiates it
constexpr int kRedThreads = 256;
__global__ __launch_bounds__(kRedThreads) void dt_slab_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int n_elem,
                                                                     float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float part[4 * kRedThreads];
  alignq_wgr::wgrad_reduce_body<kRedThreads>(slabs, n_slabs, n_elem, dw, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Site backward.  dx = gm * act_jac(fma(a, z, b)), gm = g where relu(q(fma(a, z, b))) > 0, else 0.
template <int FORMULA, bool BOUNDED>
__device__ __forceinline__ float site_dx(float g, float z, float a, float b, int k, const Levels& nlev, float r,
                                         const NerfTab tab) {
  const float x = __fmaf_rn(a, z, b);
  float t, bin;
  const bool pass = act_quant1<FORMULA, BOUNDED>(x, k, nlev, r, &t, &bin, tab) > 0.0f;
  return (pass ? g : 0.f) * act_jac(x, r);
}

// any_sums_kernel<1, 1>'s partition and loop (bnq_any_body.h: workgroup = a pixel range, thread = (slot, quad), U float4 per array in
// flight, double accumulators, slots added in slot order) with z at a pitch and the gate formed.  C <= 512: one quad per thread.
// part: [gridDim.x][C][2] doubles {sum dx, sum dx * zhat}.  blockDim.x = the Geo's NT.
template <int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(kMaxNT) void dt_sums_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z, int64_t ldq,
                                                             const float* __restrict__ ab, const float* __restrict__ save, int64_t P,
                                                             int C, int L, int slots, int64_t per, int k, float r,
                                                             double* __restrict__ part) {
  constexpr int U = 4;
  __shared__ double sm[kMaxNT * 4];
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  nerf_tab_load(tab_lds);
  __syncthreads();
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev = make_levels(k, fabsf(r) <= 8.0f);
  const int tid = threadIdx.x, C4 = C >> 2;
  const int slot = tid / L, l = tid - slot * L;
  const bool active = slot < slots;                          // the surplus lanes of the block idle
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < P ? p0 + per : P;
  float4 a4, b4, m4, i4;
  if (active) {
    a4 = ld4(ab + 4 * l); b4 = ld4(ab + C + 4 * l);
    m4 = ld4(save + 4 * l); i4 = ld4(save + C + 4 * l);
  }
  double s0[1][4], s1[1][4];
#pragma unroll
  for (int e = 0; e < 4; e++) { s0[0][e] = 0; s1[0][e] = 0; }
  if (active) {
    const float ae[4] = {a4.x, a4.y, a4.z, a4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
    const float me[4] = {m4.x, m4.y, m4.z, m4.w}, ie[4] = {i4.x, i4.y, i4.z, i4.w};
    for (int64_t base = p0 + slot; base < p1; base += (int64_t)slots * U) {
      float4 zv[U], gv[U];
#pragma unroll
      for (int u = 0; u < U; u++) {                          // clamped address, masked below
        const int64_t px = base + (int64_t)u * slots;
        const int64_t pc = px < p1 ? px : p1 - 1;
        zv[u] = ld4(z + 4 * (pc * ldq + l));
        gv[u] = ld4(g + 4 * (pc * C4 + l));
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (base + (int64_t)u * slots < p1) {
          const float ze[4] = {zv[u].x, zv[u].y, zv[u].z, zv[u].w}, ge[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float dx = site_dx<FORMULA, BOUNDED>(ge[e], ze[e], ae[e], be[e], k, nlev, r, tab);
            const float zh = (ze[e] - me[e]) * ie[e];
            s0[0][e] += (double)dx;
            s1[0][e] += (double)dx * (double)zh;
          }
        }
      }
    }
  }
  slot_reduce<1>(sm, s0, C, L, slots, 0, part);
  slot_reduce<1>(sm, s1, C, L, slots, 1, part);
}

// G[p][c] = G[p][c] + a * ((dx - k0) - zhat * k1) over the float4 index i = p * CQ + cq of the dense gy (nvec < 2^29: the pitch
// bound); z and G at their pitches in float4.  tab_s: [6][C] = a, b, mean, invstd, k0, k1.
template <int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(kTA) void dt_apply_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z, int64_t ldzq,
                                                           const float* __restrict__ ab, const float* __restrict__ save,
                                                           const float* __restrict__ ktot, int nvec, int C, int k, float r,
                                                           float* __restrict__ G, int64_t ldgq) {
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float tab_s[6 * kMaxC];
  nerf_tab_load(tab_lds);
  for (int i = threadIdx.x; i < 2 * C; i += kTA) {
    tab_s[i] = ab[i];
    tab_s[2 * C + i] = save[i];
    tab_s[4 * C + i] = ktot[i];
  }
  __syncthreads();
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev = make_levels(k, fabsf(r) <= 8.0f);
  const int CQ = C >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kTA + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * kTA) {
    const int p = (int)i / CQ, c = (int)i - p * CQ;
    const float4 gv = ld4_stream(g + 4 * i);                 // gy is read here for the last time; z and G are read again
    const float4 zv = ld4(z + 4 * (p * ldzq + c));
    float* const Gp = G + 4 * (p * ldgq + c);
    const float4 Gv = ld4(Gp);
    const float4 a4 = ld4(tab_s + 4 * c), b4 = ld4(tab_s + C + 4 * c), m4 = ld4(tab_s + 2 * C + 4 * c);
    const float4 i4 = ld4(tab_s + 3 * C + 4 * c), k0 = ld4(tab_s + 4 * C + 4 * c), k1 = ld4(tab_s + 5 * C + 4 * c);
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w}, ze[4] = {zv.x, zv.y, zv.z, zv.w}, Ge[4] = {Gv.x, Gv.y, Gv.z, Gv.w};
    const float ae[4] = {a4.x, a4.y, a4.z, a4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
    const float me[4] = {m4.x, m4.y, m4.z, m4.w}, ie[4] = {i4.x, i4.y, i4.z, i4.w};
    const float k0e[4] = {k0.x, k0.y, k0.z, k0.w}, k1e[4] = {k1.x, k1.y, k1.z, k1.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float dx = site_dx<FORMULA, BOUNDED>(ge[e], ze[e], ae[e], be[e], k, nlev, r, tab);
      const float zh = (ze[e] - me[e]) * ie[e];
      o[e] = Ge[e] + ae[e] * ((dx - k0e[e]) - zh * k1e[e]);
    }
    *reinterpret_cast<float4*>(Gp) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------ host ----------------------
inline bool bad_k(int k) { return k < 1 || k > 16; }
inline bool bad_formula(int f) { return f != ALIGNQ_FORMULA_ADMM && f != ALIGNQ_FORMULA_CDF; }
inline bool bad_pitch(int ld, int width) { return (ld & 3) != 0 || ld < width; }
inline bool bad_c(int C) { return C < kMinC || C > kMaxC || (C & 3) != 0; }

inline bool layer_shape_ok(int B, int H, int W, int CIN, int COUT, int ld) {
  if (bad_c(CIN) || bad_c(COUT) || B < 1 || H < 1 || W < 1) return false;
  const int m = CIN > COUT ? CIN : COUT;
  return fits31(B, H, W, ld > m ? ld : m);
}
// (P >= 2 is checked before: ALIGNQ_EINVAL)
inline bool site_shape_ok(int64_t P, int C, int ld) { return !bad_c(C) && P <= (int64_t)INT32_MAX / (ld > C ? ld : C); }

// the quantiser's variant: 2 * (formula == CDF) + the rounding form alignq_bnq_any_fwd's ALIGNQ_BOUNDED_SWITCH takes
inline int site_variant(int k, float act_range, int formula) {
  const bool bounded = make_levels(k, fabsf(act_range) <= 8.0f).yn != 0.0f;
  return (formula == ALIGNQ_FORMULA_CDF ? 2 : 0) + (bounded ? 1 : 0);
}
// runs the statements with the variant's (FORMULA, BOUNDED) as the constants kF, kB
#define DT_VARIANT_SWITCH(variant, ...)                                                        \
  switch (variant) {                                                                           \
    case 0: { constexpr int kF = 0; constexpr bool kB = false; __VA_ARGS__ } break;            \
    case 1: { constexpr int kF = 0; constexpr bool kB = true; __VA_ARGS__ } break;             \
    case 2: { constexpr int kF = 1; constexpr bool kB = false; __VA_ARGS__ } break;            \
    default: { constexpr int kF = 1; constexpr bool kB = true; __VA_ARGS__ } break;            \
  }

DG gemm_args(const float* a, int lda, const void* w, float* out, int ldo, int B, int H, int W, int K, int N, int w_bit) {
  DG p{};
  p.a = a; p.w = (const u16*)w; p.out = out;
  p.lda = lda; p.ldo = ldo;
  p.H = H; p.W = W; p.K = K; p.N = N;
  p.th = (H + TS - 1) / TS; p.tw = (W + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;                       // <= B * H * W
  p.s_blocks = p.s_tiles < kMaxTileBlocks ? p.s_tiles : kMaxTileBlocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.wt = write_through((int64_t)B * H * W * N * (int64_t)sizeof(float));
  const int bn = n_tile_width(N);
  p.n_tiles = (N + bn - 1) / bn;
  return p;
}

template <bool WTR, int FORMULA, bool BOUNDED>
void launch_gemm(const DG& p, hipStream_t st) {
  const int bn = n_tile_width(p.N);
  const dim3 grid(p.s_blocks * p.n_tiles), blk(256);
  if (bn == 64) hipLaunchKernelGGL((dt_gemm_kernel<4, WTR, FORMULA, BOUNDED>), grid, blk, 0, st, p);
  else if (bn == 32) hipLaunchKernelGGL((dt_gemm_kernel<2, WTR, FORMULA, BOUNDED>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((dt_gemm_kernel<1, WTR, FORMULA, BOUNDED>), grid, blk, 0, st, p);
}

inline int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int alignq_dense_train_supported(int B, int H, int W, int CIN, int COUT, int ld) {
  if (bad_pitch(ld, CIN) || bad_pitch(ld, COUT)) return 0;
  return layer_shape_ok(B, H, W, CIN, COUT, ld) ? 1 : 0;
}

size_t alignq_dense_train_site_ws_bytes(int64_t P, int C) {
  if (P < 2 || !site_shape_ok(P, C, C)) return 0;
  return (size_t)parts_for(P, C, nullptr) * C * 2 * sizeof(double) + (size_t)2 * C * sizeof(float);
}

size_t alignq_dense_train_wgrad_ws_bytes(int B, int H, int W, int CIN, int COUT) {
  if (!layer_shape_ok(B, H, W, CIN, COUT, 0)) return 0;
  return (size_t)k3_wgrad_geometry(B, H, W, CIN, COUT).splits * (size_t)COUT * 9 * CIN * sizeof(float);
}

int alignq_dense_train_stats(const float* z, int ld, int64_t P, int C, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, int64_t* num_batches_tracked, float momentum, float bn_eps, float* ab, float* save,
                             void* ws, void* stream) {
  if (!z || !ab || !save || !ws || P < 2 || misaligned(z) || misaligned(ws) || bad_pitch(ld, C)) return ALIGNQ_EINVAL;
  if (!site_shape_ok(P, C, ld)) return ALIGNQ_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const Geo ge = geo_for(C);                                           // C <= 512: one quad per thread
  int64_t per;
  const int np = parts_for(P, C, &per);
  hipLaunchKernelGGL((any_sums_kernel<0, 1>), dim3(np), dim3(ge.NT), 0, st, z, (const float*)nullptr,
                     (const unsigned long long*)nullptr, (const float*)nullptr, (const float*)nullptr, P, C, (int64_t)(ld >> 2), ge.L,
                     ge.slots, per, 0.0f, part);
  hipLaunchKernelGGL(any_finalize_fwd_kernel, dim3((C + kFinT - 1) / kFinT), dim3(kFinT), 0, st, (const double*)part, np, P, C, gamma,
                     beta, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, bn_eps, ab, save);
  return hipGetLastError() == hipSuccess ? 0 : ALIGNQ_EINVAL;
}

int alignq_dense_train_layer_fwd(const float* x, int ldx, float* y, int ldy, const float* ab, const void* w_bins, int B, int H, int W,
                                 int CIN, int COUT, int w_bit, int k, float act_range, int formula, void* stream) {
  if (!x || !y || !ab || !w_bins || !aligned16(x) || !aligned16(y) || !aligned16(w_bins)) return ALIGNQ_EINVAL;
  if (w_bit < 1 || w_bit > 8 || bad_k(k) || bad_formula(formula) || bad_pitch(ldx, CIN) || bad_pitch(ldy, COUT)) return ALIGNQ_EINVAL;
  if (!layer_shape_ok(B, H, W, CIN, COUT, ldx > ldy ? ldx : ldy)) return ALIGNQ_EUNSUPPORTED;
  DG p = gemm_args(x, ldx, w_bins, y, ldy, B, H, W, CIN, COUT, w_bit);
  p.ab = ab; p.k = k; p.r = act_range;
  DT_VARIANT_SWITCH(site_variant(k, act_range, formula), launch_gemm<false, kF, kB>(p, (hipStream_t)stream);)
  return last_error();
}

int alignq_dense_train_dgrad(const float* dy, int lddy, const void* w_bins, float* gy, int B, int H, int W, int CIN, int COUT,
                             int w_bit, void* stream) {
  if (!dy || !w_bins || !gy || !aligned16(dy) || !aligned16(w_bins) || !aligned16(gy) || w_bit < 1 || w_bit > 8 || bad_pitch(lddy, COUT))
    return ALIGNQ_EINVAL;
  if (!layer_shape_ok(B, H, W, CIN, COUT, lddy)) return ALIGNQ_EUNSUPPORTED;
  const DG p = gemm_args(dy, lddy, w_bins, gy, CIN, B, H, W, COUT, CIN, w_bit);
  launch_gemm<true, 2, false>(p, (hipStream_t)stream);
  return last_error();
}

int alignq_dense_train_wgrad(const float* z, int ldz, const float* ab, const float* dy, int lddy, float* dw, void* ws, int B, int H,
                             int W, int CIN, int COUT, int k, float act_range, int formula, int* n_slabs_out, void* stream) {
  if (!z || !ab || !dy || !ws || (!dw && !n_slabs_out) || !aligned16(z) || !aligned16(dy) || !aligned16(ws) || !aligned16(dw))
    return ALIGNQ_EINVAL;
  if (bad_k(k) || bad_formula(formula) || bad_pitch(ldz, CIN) || bad_pitch(lddy, COUT)) return ALIGNQ_EINVAL;
  if (!layer_shape_ok(B, H, W, CIN, COUT, ldz > lddy ? ldz : lddy)) return ALIGNQ_EUNSUPPORTED;
  const K3WgradGeom g = k3_wgrad_geometry(B, H, W, CIN, COUT);
  DW a{};
  a.z = z; a.dy = dy; a.ab = ab; a.slabs = (float*)ws;
  a.ldz = ldz; a.lddy = lddy;
  a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
  a.th = g.th; a.tw = g.tw; a.s_tiles = g.s_tiles; a.per = g.per;
  a.c_tiles = g.c_tiles; a.o_tiles = g.o_tiles;
  a.r = act_range; a.k = k;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.c_tiles * g.o_tiles * g.splits), blk(256);
  DT_VARIANT_SWITCH(site_variant(k, act_range, formula),
    if (g.cb == 64) hipLaunchKernelGGL((dt_wgrad_kernel<64, 16, kF, kB>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((dt_wgrad_kernel<16, 64, kF, kB>), grid, blk, 0, st, a);)
  int e = last_error();
  if (e) return e;
  if (n_slabs_out) { *n_slabs_out = g.splits; return 0; }      // deferred: the caller reduces (alignq_conv3x3_wgrad_reduce_multi)
  const int n_elem = COUT * 9 * CIN;
  hipLaunchKernelGGL(dt_slab_reduce_kernel, dim3(alignq_wgr::wgrad_reduce_blocks(g.splits, n_elem, kRedThreads)), dim3(kRedThreads), 0,
                     st, (const float*)ws, g.splits, n_elem, dw);
  return last_error();
}

int alignq_dense_train_site_bwd(const float* gy, const float* z, int ldz, const float* ab, const float* save, float* G, int ldg,
                                int64_t P, int C, int k, float act_range, int formula, float* dgamma, float* dbeta, void* ws,
                                void* stream) {
  if (!gy || !z || !ab || !save || !G || !ws || P < 2 || misaligned(gy) || misaligned(z) || misaligned(G) || misaligned(ws))
    return ALIGNQ_EINVAL;
  if (bad_k(k) || bad_formula(formula) || bad_pitch(ldz, C) || bad_pitch(ldg, C)) return ALIGNQ_EINVAL;
  if (!site_shape_ok(P, C, ldz > ldg ? ldz : ldg)) return ALIGNQ_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const Geo ge = geo_for(C);
  int64_t per;
  const int np = parts_for(P, C, &per);
  float* ktot = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + (size_t)np * C * 2 * sizeof(double));
  const int nvec = (int)(P * (C >> 2));
  const int64_t blocks = ((int64_t)nvec + kTA - 1) / kTA;
  const int grid = (int)(blocks > kApplyBlocks ? kApplyBlocks : blocks);
  DT_VARIANT_SWITCH(site_variant(k, act_range, formula),
    hipLaunchKernelGGL((dt_sums_bwd_kernel<kF, kB>), dim3(np), dim3(ge.NT), 0, st, gy, z, (int64_t)(ldz >> 2), ab, save, P, C, ge.L,
                       ge.slots, per, k, act_range, part);
    hipLaunchKernelGGL(any_finalize_bwd_kernel, dim3((C + kFinT - 1) / kFinT), dim3(kFinT), 0, st, (const double*)part, np, P, C, ktot,
                       dgamma, dbeta);
    hipLaunchKernelGGL((dt_apply_bwd_kernel<kF, kB>), dim3(grid), dim3(kTA), 0, st, gy, z, (int64_t)(ldz >> 2), ab, save,
                       (const float*)ktot, nvec, C, k, act_range, G, (int64_t)(ldg >> 2));)
  return hipGetLastError() == hipSuccess ? 0 : ALIGNQ_EINVAL;
}

}  // extern "C"

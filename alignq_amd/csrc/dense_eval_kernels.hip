// dense_eval_kernels.hip — DenseNet's evaluation pass without concatenations (the reference's test() on cdf_alignment/dense-cifar-10/
// model/densenet.py:17-41) for gfx950; include/alignq_dense.h states the contracts.
//
//   alignq_dense_layer_eval_fwd : one dense layer, bn1 -> act_q0 -> ReLU -> 3x3 Conv2d_Q, as ONE launch.  The kernel is
//                               k3_gemm_kernel<TN, false> of k3conv_kernels.hip (same tile, same staging, same MFMA order, same
//                               epilogue, the primitives of exact_mma.h) with two changes: pixels are addressed through a pitch on both sides, so that the layer
//                               reads the first CIN channels of its block's buffer and writes its COUT channels right behind them;
//                               and the site (eval_site_body.h: the statement mobile_eval_kernels.hip uses) is applied to a float4 of
//                               the halo tile between its load and its split into three bf16 terms.  What is not loaded - the padding,
//                               tile pixels outside the image, the channel tail of the last chunk - is stored as zeros AFTER the site.
//                               Every workgroup forms the [2][CIN] coefficient table itself from the batch-norm vectors.
//                               The site runs on 10 x 10 halo pixels per 8 x 8 tile and once per output-channel tile.
//   alignq_avgpool2_nhwc_fwd    : the transition's 2 x 2 average pool, one float4 of the output per item, written at a pitch.
//
// Every sum and product of the site and of the pool is an individual fp32 operation (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_dense.h"
#include "alignq_math.h"
#include "eval_site_body.h"
#include "exact_conv_host.h"
#include "exact_mma.h"

using namespace alignq;
using namespace alignq_evalsite;
using namespace alignq_xmma;

namespace {

// the geometry of k3conv_kernels.hip's forward
constexpr int BK = 32;                 // channels per chunk (one MFMA k step)
constexpr int LDX = BK + 8;            // halfwords per LDS row
constexpr int TS = 8;                  // the spatial tile is TS x TS pixels
constexpr int HS = TS + 2, HP = HS * HS;          // with its halo: 10 x 10
constexpr int kMaxTileBlocks = 2048;   // grid cap over spatial tiles; the rest by grid stride
constexpr int kMinC = 4, kMaxC = 512;
constexpr int kPoolMaxC = 2048, kPoolMaxGrid = 2048, kPoolThreads = 256;

// ---------------------------------------------------------------------------------------------------------------------------
// y[b][h][w][n] = (1 / nlev) * sum_{t = (ty, tx)} sum_k s(x[b][h + ty - 1][w + tx - 1][k]) * w[n][t][k],  s = the site of channel k;
// pixel p of x at x + p * ldx, of y at y + p * ldy.
struct DL {
  const float* x; const u16* w; float* y;
  SiteDev s;                          // (z unused)
  int ldx, ldy;
  int H, W, K, N;
  int th, tw;                         // tiles along H and W
  int s_tiles, s_blocks, n_tiles;     // spatial tiles, spatial tiles the grid holds (stride of the rest), channel tiles
  float nlev, r;
  int wt;                             // write-through output stores
};

// FORMULA: 0 = ALIGNQ_FORMULA_ADMM, 1 = ALIGNQ_FORMULA_CDF, 2 = no quantiser; BOUNDED: the quantiser's rounding form, chosen by the
// host as site_eval_kernel chooses it (make_levels(k, |r| <= 8).yn != 0)
template <int TN, int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(256, 2) void dense_layer_eval_kernel(const DL p) {
  constexpr int BN = 16 * TN;
  constexpr int XPL = HP * LDX;                       // halfwords per pixel-side term plane
  constexpr int WPL = BN * LDX;                       // halfwords per filter tap
  constexpr int NAP = HP * (BK / 4);                  // float4 of the halo tile
  constexpr int NA = (NAP + 255) / 256;
  constexpr int NBP = 9 * BN * (BK / 4);              // 8-byte pieces (4 bins) of the nine filter taps
  constexpr int NB = (NBP + 255) / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + 9 * WPL];
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float ab_s[2 * kMaxC];        // [2][K]
  u16* const Xs = lds;
  u16* const Ws = lds + 3 * XPL;

  if (FORMULA != 2) nerf_tab_load(tab_lds);
  ab_table<256>(ab_s, p.K, p.s);            // (the first barrier of the chunk loop stands in front of the first read)
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev_q = make_levels(p.s.k, fabsf(p.r) <= 8.0f);

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
        ra[i] = *reinterpret_cast<const f32x4*>(p.x + (ok ? (img + (int64_t)h * p.W + w) * p.ldx + k : 0));
        if (!ok) ra[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        live |= (ok ? 1u : 0u) << i;
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        const int k = k0 + 4 * (idx & 7), n = n0 + (idx >> 3) % BN, t = (idx >> 3) / BN;
        const bool ok = idx < NBP && n < p.N && k < p.K;
        rw[i] = *reinterpret_cast<const s16x4*>(p.w + (ok ? ((int64_t)n * 9 + t) * p.K + k : 0));
        if (!ok) rw[i] = (s16x4){0, 0, 0, 0};
      }
    };
    auto park = [&](int kt) {
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int idx = tid + 256 * i;
        if (idx >= NAP) continue;
        const int o = (idx >> 3) * LDX + 4 * (idx & 7);
        const bool ok = (live >> i) & 1u;
        const int cq = ok ? kt * (BK / 4) + (idx & 7) : 0;          // (a quad that was not loaded reads row 0 and is discarded)
        const float4 q = clamp4(site_q<FORMULA, BOUNDED>(make_float4(ra[i][0], ra[i][1], ra[i][2], ra[i][3]), ab_s, p.K, cq, p.s.k,
                                                         nlev_q, p.r, tab), p.s.clamp);
        const f32x4 v = ok ? (f32x4){q.x, q.y, q.z, q.w} : (f32x4){0.f, 0.f, 0.f, 0.f};
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
        *reinterpret_cast<s16x4*>(Ws + ((idx >> 3) / BN) * WPL + ((idx >> 3) % BN) * LDX + 4 * (idx & 7)) = rw[i];
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
      if (h < p.H && w < p.W && n < p.N) st_out(p.y + (img + (int64_t)h * p.W + w) * p.ldy + n, v, p.wt);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// item i = (b, ho, wo, cq): y[(b, ho, wo)][4 cq ..] = (((x00 + x01) + x10) + x11) * 0.25 of the window at (2 ho, 2 wo)
__global__ __launch_bounds__(kPoolThreads) void avgpool2_kernel(const float* __restrict__ x, float* __restrict__ y, int ldy, int H,
                                                                int W, int Ho, int Wo, int CQ, int64_t n_items) {
  const int C = 4 * CQ;
  const int64_t step = (int64_t)gridDim.x * kPoolThreads;
  for (int64_t i = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x; i < n_items; i += step) {
    const int cq = (int)(i % CQ);
    int64_t q = i / CQ;
    const int wo = (int)(q % Wo);
    q /= Wo;
    const int ho = (int)(q % Ho);
    const int64_t b = q / Ho;
    const float* s = x + ((b * H + 2 * ho) * W + 2 * wo) * C + 4 * cq;
    const float4 x00 = *reinterpret_cast<const float4*>(s), x01 = *reinterpret_cast<const float4*>(s + C);
    const float4 x10 = *reinterpret_cast<const float4*>(s + (int64_t)W * C), x11 = *reinterpret_cast<const float4*>(s + (int64_t)W * C + C);
    float4 o;
    o.x = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(x00.x, x01.x), x10.x), x11.x), 0.25f);
    o.y = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(x00.y, x01.y), x10.y), x11.y), 0.25f);
    o.z = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(x00.z, x01.z), x10.z), x11.z), 0.25f);
    o.w = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(x00.w, x01.w), x10.w), x11.w), 0.25f);
    *reinterpret_cast<float4*>(y + ((b * Ho + ho) * Wo + wo) * ldy + 4 * cq) = o;
  }
}

// ------------------------------------------------------------------ host ----------------------
inline bool bad_k(int k) { return !((k >= 1 && k <= 16) || k == 32); }
inline bool bad_formula(int f) { return f != ALIGNQ_FORMULA_ADMM && f != ALIGNQ_FORMULA_CDF; }
inline bool bad_clamp(int c) { return c != ALIGNQ_CLAMP_NONE && c != ALIGNQ_CLAMP_RELU && c != ALIGNQ_CLAMP_RELU6; }
inline bool bad_pitch(int ld, int width) { return (ld & 3) != 0 || ld < width; }

inline bool layer_shape_ok(int B, int H, int W, int CIN, int COUT, int ldx, int ldy) {
  if (CIN < kMinC || CIN > kMaxC || (CIN & 3) || COUT < kMinC || COUT > kMaxC || (COUT & 3) || B < 1 || H < 1 || W < 1) return false;
  return fits31(B, H, W, ldx > ldy ? ldx : ldy);
}

template <int TN>
void launch_layer(const DL& p, int variant, dim3 grid, hipStream_t st) {
  const dim3 blk(256);
  switch (variant) {
    case 0: hipLaunchKernelGGL((dense_layer_eval_kernel<TN, 0, false>), grid, blk, 0, st, p); break;
    case 1: hipLaunchKernelGGL((dense_layer_eval_kernel<TN, 0, true>), grid, blk, 0, st, p); break;
    case 2: hipLaunchKernelGGL((dense_layer_eval_kernel<TN, 1, false>), grid, blk, 0, st, p); break;
    case 3: hipLaunchKernelGGL((dense_layer_eval_kernel<TN, 1, true>), grid, blk, 0, st, p); break;
    default: hipLaunchKernelGGL((dense_layer_eval_kernel<TN, 2, false>), grid, blk, 0, st, p); break;
  }
}

}  // namespace

extern "C" {

int alignq_dense_layer_eval_fwd(const float* x, int ldx, float* y, int ldy, const alignq_dense_site* site, const void* w_bins, int B,
                                int H, int W, int CIN, int COUT, int w_bit, float act_range, int formula, void* stream) {
  if (!x || !y || !w_bins || !site || !site->running_mean || !site->running_var || !aligned16(x) || !aligned16(y) || !aligned16(w_bins))
    return ALIGNQ_EINVAL;
  if (w_bit < 1 || w_bit > 8 || bad_k(site->k) || bad_formula(formula) || bad_clamp(site->clamp)) return ALIGNQ_EINVAL;
  if (bad_pitch(ldx, CIN) || bad_pitch(ldy, COUT)) return ALIGNQ_EINVAL;
  if (!layer_shape_ok(B, H, W, CIN, COUT, ldx, ldy)) return ALIGNQ_EUNSUPPORTED;
  DL p{};
  p.x = x; p.w = (const u16*)w_bins; p.y = y;
  p.s.z = nullptr; p.s.gamma = site->gamma; p.s.beta = site->beta; p.s.mean = site->running_mean; p.s.var = site->running_var;
  p.s.eps = site->bn_eps; p.s.k = site->k; p.s.clamp = site->clamp;
  p.ldx = ldx; p.ldy = ldy;
  p.H = H; p.W = W; p.K = CIN; p.N = COUT;
  p.th = (H + TS - 1) / TS; p.tw = (W + TS - 1) / TS;
  p.s_tiles = B * p.th * p.tw;                       // <= B * H * W
  p.s_blocks = p.s_tiles < kMaxTileBlocks ? p.s_tiles : kMaxTileBlocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.r = act_range;
  p.wt = write_through((int64_t)B * H * W * COUT * (int64_t)sizeof(float));
  const int bn = n_tile_width(COUT);
  p.n_tiles = (COUT + bn - 1) / bn;
  const bool bounded = make_levels(site->k, fabsf(act_range) <= 8.0f).yn != 0.0f;
  const int variant = site->k == 32 ? 4 : (formula == ALIGNQ_FORMULA_CDF ? 2 : 0) + (bounded ? 1 : 0);
  const dim3 grid(p.s_blocks * p.n_tiles);
  hipStream_t st = (hipStream_t)stream;
  if (bn == 64) launch_layer<4>(p, variant, grid, st);
  else if (bn == 32) launch_layer<2>(p, variant, grid, st);
  else launch_layer<1>(p, variant, grid, st);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int alignq_avgpool2_nhwc_fwd(const float* x, float* y, int ldy, int B, int H, int W, int C, void* stream) {
  if (!x || !y || !aligned16(x) || !aligned16(y) || bad_pitch(ldy, C)) return ALIGNQ_EINVAL;
  if (C < 4 || C > kPoolMaxC || (C & 3) || B < 1 || H < 2 || W < 2) return ALIGNQ_EUNSUPPORTED;
  if (!fits31(B, H, W, C) || !fits31(B, H / 2, W / 2, ldy)) return ALIGNQ_EUNSUPPORTED;
  const int Ho = H / 2, Wo = W / 2, CQ = C / 4;
  const int64_t n_items = (int64_t)B * Ho * Wo * CQ;
  const int64_t blocks = (n_items + kPoolThreads - 1) / kPoolThreads;
  const int grid = (int)(blocks > kPoolMaxGrid ? kPoolMaxGrid : blocks);
  hipLaunchKernelGGL(avgpool2_kernel, dim3(grid), dim3(kPoolThreads), 0, (hipStream_t)stream, x, y, ldy, H, W, Ho, Wo, CQ, n_items);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

// digit_eval_kernels.hip — the digit-domain DANN's evaluation pass (the reference's test(), cdf_alignment/dann_digit/main.py:436-487, on
// model/dann.py:143-155) for gfx950; include/alignq_digit.h states the contract.
//
//   alignq_k5conv_site_pool_eval_fwd : conv 5x5 + bias -> eval-mode batch-norm -> act_q -> ReLU -> MaxPool2d(2) as ONE launch.  The main
//       loop is k5conv_kernels.hip's forward, both forms (k5_fwd_body.h: same tile, same staging, same MFMA order); only what a lane
//       does with its finished accumulator differs.  A lane holds ONE output pixel and 4 consecutive channels of each of the tile's
//       16-channel blocks:
//         1. v = acc / n + bias                                   (the plain forward's division and add)
//         2. v = relu(q(a_c v + b_c))                             (eval_site_body.h: the statement alignq_site_eval_fwd runs; the [2][C]
//                                                                  coefficient table of the TILE's channels is formed once per workgroup)
//         3. m = max(v, v of lane ^ 1); m = max(m, m of lane ^ 8) (DPP quad_perm:[1,0,3,2] and row_ror:8 - registers only, no LDS)
//         4. the lane with (fr & 9) == 0 stores the pooled pixel  (NHWC: one float4; FLAT_CHW: four floats PH * PW apart)
//       The lane map of the tile: fr = lane & 15 of wave wv holds pixel (2 wv + (fr >> 3), fr & 7) of the 8 x 8 tile, so the window of
//       pooled pixel (wv, (fr & 7) >> 1) is lanes fr, fr ^ 1 (the column neighbour), fr ^ 8 (the row below) and fr ^ 9 of ONE 16-lane
//       DPP row:
//             fr:   0 1 | 2 3 | 4 5 | 6 7        row 2 wv
//                   8 9 | a b | c d | e f        row 2 wv + 1
//       Tiles start at multiples of 8, so no window straddles two tiles, and a window with a pixel outside the (H-4) x (W-4) output lies
//       outside the floor-divided pooled extent: it is dropped whole by the store's bounds check.  After the ReLU clamp every value is
//       >= +0 and no NaN (values of pixels beyond the output included: they are finite sums over a zero-filled footprint), so the max
//       has no special cases and gives F.max_pool2d's bits.
//   The un-pooled tensor (32 x 24 x 24 floats per image in the DANN's first layer) is never written.
//
// Every sum and product of the site is an individual fp32 operation (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_digit.h"
#include "../../include/alignq_k5conv.h"
#include "alignq_math.h"
#include "eval_site_body.h"
#include "exact_conv_host.h"
#include "exact_mma.h"
#include "k5_fwd_body.h"

using namespace alignq;
using namespace alignq_evalsite;
using namespace alignq_xmma;
using namespace alignq_k5;

namespace {

// what the epilogue needs beyond the convolution's own arguments
struct PoolArgs {
  SiteDev s;                          // the site over the COUT channels (z unused)
  float r;                            // act_range
  float* y;
  int PH, PW;                         // the pooled extent
  int flat;                           // ALIGNQ_DIGIT_OUT_FLAT_CHW
  int wt;                             // write-through output stores
};

// the value of the lane whose fr differs in bit 0 (the column neighbour) / in bit 3 (the row below or above), inside a 16-lane row
__device__ __forceinline__ float lane_xor1(const float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));          // quad_perm:[1,0,3,2]
}
__device__ __forceinline__ float lane_xor8(const float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));         // row_ror:8
}
__device__ __forceinline__ float pool4(const float v) {
  const float m = fmaxf(v, lane_xor1(v));
  return fmaxf(m, lane_xor8(m));
}

// FORMULA: 0 = ALIGNQ_FORMULA_ADMM, 1 = ALIGNQ_FORMULA_CDF, 2 = no quantiser; BOUNDED: the quantiser's rounding form, chosen by the
// host as site_eval_kernel chooses it (make_levels(k, |r| <= 8).yn != 0)
template <int FORMULA, bool BOUNDED>
struct SitePool {
  const float* bias; float nlev;      // the convolution's epilogue
  const float* ab; int C, n0;         // the [2][C] coefficient table of the tile's channels n0 .. n0 + C (LDS)
  int k; Levels lv; float r; NerfTab tab;
  float* y; int PH, PW, N, flat, wt;

  template <int TN>
  __device__ __forceinline__ void operator()(const int b, const int h, const int w, const int n4, const f32x4 (&acc)[TN]) const {
    // (fr & 9) == 0 is "row and column of the tile both even", and tiles start at multiples of 8
    const int ph = h >> 1, pw = w >> 1;
    const bool owner = !((h | w) & 1) && ph < PH && pw < PW;
    const int64_t pix = ((int64_t)b * PH + ph) * PW + pw, plane = (int64_t)PH * PW;
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      const int n = n4 + tn * 16;
      const bool live = n < N;
      const int nl = live ? n : n0;           // (a block beyond N computes on the tile's first quad and stores nothing)
      f32x4 v = acc[tn];
      v = (f32x4){v[0] / nlev, v[1] / nlev, v[2] / nlev, v[3] / nlev};
      if (bias) v = (f32x4){v[0] + bias[nl], v[1] + bias[nl + 1], v[2] + bias[nl + 2], v[3] + bias[nl + 3]};
      const float4 q = clamp4(site_q<FORMULA, BOUNDED>(make_float4(v[0], v[1], v[2], v[3]), ab, C, (nl - n0) >> 2, k, lv, r, tab),
                              ALIGNQ_CLAMP_RELU);
      const f32x4 m = {pool4(q.x), pool4(q.y), pool4(q.z), pool4(q.w)};          // every lane of the wave takes part
      if (!(owner && live)) continue;
      if (!flat) {
        st_out(y + pix * N + n, m, wt);
      } else {
        float* o = y + ((int64_t)b * N + n) * plane + (int64_t)ph * PW + pw;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (wt) alignq_store::st4<alignq_store::kConvOut, false>(o + e * plane, m[e]);
          else o[e * plane] = m[e];
        }
      }
    }
  }
};

// the tables of one workgroup (every thread calls it; ends with the barrier in front of their first read) and its epilogue
template <int TN, int FORMULA, bool BOUNDED>
__device__ __forceinline__ SitePool<FORMULA, BOUNDED> site_pool_setup(float* tab_lds, float* ab_s, const float* bias, const float nlev,
                                                                      const int N, const int n_tiles, const PoolArgs& e) {
  const int n0 = tile_n0<TN>(n_tiles);
  const int C = N - n0 < 16 * TN ? N - n0 : 16 * TN;
  if (FORMULA != 2) nerf_tab_load(tab_lds);
  SiteDev s = e.s;                            // the tile's channels
  s.gamma = s.gamma ? s.gamma + n0 : nullptr; s.beta = s.beta ? s.beta + n0 : nullptr;
  s.mean += n0; s.var += n0;
  ab_table<256>(ab_s, C, s);
  __syncthreads();
  return SitePool<FORMULA, BOUNDED>{bias, nlev, ab_s, C, n0, e.s.k, make_levels(e.s.k, fabsf(e.r) <= 8.0f), e.r, nerf_tab(tab_lds),
                                    e.y, e.PH, e.PW, N, e.flat, e.wt};
}

template <int TN, int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(256, 2) void k5_site_pool_kernel(const K5 p, const PoolArgs e) {
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float ab_s[2 * 16 * TN];
  k5_gemm_body<TN, false>(p, site_pool_setup<TN, FORMULA, BOUNDED>(tab_lds, ab_s, p.bias, p.nlev, p.N, p.n_tiles, e));
}

template <int TN, bool X1, int FORMULA, bool BOUNDED>
__global__ __launch_bounds__(256, 2) void k5_image_site_pool_kernel(const K5I p, const PoolArgs e) {
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float ab_s[2 * 16 * TN];
  k5_image_fwd_body<TN, X1>(p, site_pool_setup<TN, FORMULA, BOUNDED>(tab_lds, ab_s, p.bias, p.nlev, p.N, p.n_tiles, e));
}

// ------------------------------------------------------------------ host ----------------------
inline bool bad_k(int k) { return !((k >= 1 && k <= 16) || k == 32); }
inline bool bad_formula(int f) { return f != ALIGNQ_FORMULA_ADMM && f != ALIGNQ_FORMULA_CDF; }

inline bool shape_ok(int B, int H, int W, int CIN, int COUT) {
  return H >= KS + 1 && W >= KS + 1 && alignq_k5conv_supported(ALIGNQ_K5_FWD, B, H, W, CIN, COUT) == 1;
}

// form: 0 = body, 1 = image from [B][H][W][3], 2 = image from [B][H][W]
template <int TN, int FORMULA, bool BOUNDED>
void launch_variant(int form, const K5& p, const K5I& q, const PoolArgs& e, dim3 grid, hipStream_t st) {
  const dim3 blk(256);
  if (form == 0) hipLaunchKernelGGL((k5_site_pool_kernel<TN, FORMULA, BOUNDED>), grid, blk, 0, st, p, e);
  else if (form == 1) hipLaunchKernelGGL((k5_image_site_pool_kernel<TN, false, FORMULA, BOUNDED>), grid, blk, 0, st, q, e);
  else hipLaunchKernelGGL((k5_image_site_pool_kernel<TN, true, FORMULA, BOUNDED>), grid, blk, 0, st, q, e);
}

template <int TN>
void launch_tile(int variant, int form, const K5& p, const K5I& q, const PoolArgs& e, dim3 grid, hipStream_t st) {
  switch (variant) {
    case 0: launch_variant<TN, 0, false>(form, p, q, e, grid, st); break;
    case 1: launch_variant<TN, 0, true>(form, p, q, e, grid, st); break;
    case 2: launch_variant<TN, 1, false>(form, p, q, e, grid, st); break;
    case 3: launch_variant<TN, 1, true>(form, p, q, e, grid, st); break;
    default: launch_variant<TN, 2, false>(form, p, q, e, grid, st); break;
  }
}

}  // namespace

extern "C" {

int alignq_k5conv_site_pool_eval_supported(int B, int H, int W, int CIN, int COUT) { return shape_ok(B, H, W, CIN, COUT) ? 1 : 0; }

int alignq_k5conv_site_pool_eval_fwd(const float* x, int x_channels, const void* w_bins, const float* bias, const alignq_dense_site* site,
                                     float* y, int out_layout, int B, int H, int W, int CIN, int COUT, int w_bit, float act_range,
                                     int formula, void* stream) {
  if (!x || !w_bins || !y || !site || !site->running_mean || !site->running_var || !aligned16(x) || !aligned16(w_bins) || !aligned16(y) ||
      ((uintptr_t)bias & 3))
    return ALIGNQ_EINVAL;
  if (w_bit < 1 || w_bit > 8 || bad_k(site->k) || bad_formula(formula) || site->clamp != ALIGNQ_CLAMP_RELU) return ALIGNQ_EINVAL;
  if (out_layout != ALIGNQ_DIGIT_OUT_NHWC && out_layout != ALIGNQ_DIGIT_OUT_FLAT_CHW) return ALIGNQ_EINVAL;
  if (x_channels != CIN && !(CIN == 3 && x_channels == 1)) return ALIGNQ_EINVAL;
  if (!shape_ok(B, H, W, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  const int OH = H - (KS - 1), OW = W - (KS - 1), bn = n_tile_width(COUT);
  const float nlev = (float)((1 << w_bit) - 1);
  PoolArgs e{};
  e.s.z = nullptr; e.s.gamma = site->gamma; e.s.beta = site->beta; e.s.mean = site->running_mean; e.s.var = site->running_var;
  e.s.eps = site->bn_eps; e.s.k = site->k; e.s.clamp = site->clamp;
  e.r = act_range; e.y = y; e.PH = OH / 2; e.PW = OW / 2;
  e.flat = out_layout == ALIGNQ_DIGIT_OUT_FLAT_CHW;
  e.wt = write_through((int64_t)B * e.PH * e.PW * COUT * (int64_t)sizeof(float));
  K5 p{};
  K5I q{};
  if (CIN == 3) {
    q.x = x; q.w = (const u16*)w_bins; q.bias = bias; q.y = nullptr;
    q.H = H; q.W = W; q.OH = OH; q.OW = OW; q.N = COUT; q.nlev = nlev;
    tile_geometry(q, B, OH, OW, bn, COUT);
  } else {
    p.a = x; p.w = (const u16*)w_bins; p.bias = bias; p.out = nullptr;
    p.AH = H; p.AW = W; p.OH = OH; p.OW = OW; p.K = CIN; p.N = COUT; p.off = 0; p.nlev = nlev;
    tile_geometry(p, B, OH, OW, bn, COUT);
  }
  const int form = CIN != 3 ? 0 : (x_channels == 3 ? 1 : 2);
  const dim3 grid(CIN == 3 ? q.s_blocks * q.n_tiles : p.s_blocks * p.n_tiles);
  const bool bounded = make_levels(site->k, fabsf(act_range) <= 8.0f).yn != 0.0f;
  const int variant = site->k == 32 ? 4 : (formula == ALIGNQ_FORMULA_CDF ? 2 : 0) + (bounded ? 1 : 0);
  hipStream_t st = (hipStream_t)stream;
  if (bn == 64) launch_tile<4>(variant, form, p, q, e, grid, st);
  else if (bn == 32) launch_tile<2>(variant, form, p, q, e, grid, st);
  else launch_tile<1>(variant, form, p, q, e, grid, st);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"

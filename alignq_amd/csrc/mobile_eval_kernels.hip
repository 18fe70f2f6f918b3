// mobile_eval_kernels.hip — the folded evaluation sites of MobileNet-V2 (the reference's test(): cdf_alignment/mobilenet-v2-svhn/
// main.py, model/mobilenetV2.py:25-62) for gfx950; include/alignq_mobile.h states the contracts.
//
//   alignq_site_eval_fwd      : y = clamp(q(a_c z + b_c) [+ residual]) - bnq_eval_fwd_kernel's structure (eval_kernels.hip: tiles of
//                               kU x 256 float4, 16-byte non-temporal loads, a [2][C] coefficient table in LDS that every workgroup
//                               forms itself) at any C % 4 == 0, with ReLU6 among the clamps.  The channel quad of vector i is
//                               i mod C/4: one 64-bit modulo per THREAD, then 32-bit increments with a conditional subtraction.
//   alignq_site_eval_twin_fwd : the same kernel template with a second operand and a second table:
//                               y = q_A(a_A z_A + b_A) + clamp_B(q_B(a_B z_B + b_B)), the stride-1 block's tail.
//   alignq_dwconv3x3_site_eval_fwd : dwconv_kernel<S, false> (dwconv_kernels.hip: same item mapping, nine loads issued before the
//                               first add, at most 1024 workgroups with a stride that is a multiple of the quads per pixel) with the
//                               site as the epilogue of the accumulator in registers.
//
// Every sum and product is an individual fp32 operation (-ffp-contract=off), so each kernel gives the bits of the launches it replaces.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_mobile.h"
#include "alignq_math.h"
#include "eval_site_body.h"
#include "store_forms.h"

using namespace alignq;
using namespace alignq_evalsite;      // SiteDev, ab_table, site_q, clamp4: eval_site_body.h (shared with dense_eval_kernels.hip)

namespace {

constexpr int kThreads = 256;
constexpr int kU = 4;                      // float4 per thread and tile (eval_kernels.hip)
constexpr int kTile = kThreads * kU;       // float4 per workgroup and pass
constexpr int kSiteBlocks = 2048;          // grid cap of the site kernels: the 8192 waves 256 CUs hold at 8 per SIMD; the rest by grid stride
constexpr int kDwMaxGrid = 1024;           // the depthwise launch: dwconv_kernels.hip's kMaxGrid
constexpr int kMaxC = 2048;
// Outputs of kWtMinBytes .. kWtMaxBytes are stored write-through (store_forms.h); smaller and larger ones plainly.  Measured against the
// plain build (NOTES.md "MobileNet-V2 evaluation"): -23 % at 26 MB, -5 % at 52 MB, +5 % at 105 MB, +12 % at 210 MB per launch.
constexpr int64_t kWtMinBytes = (int64_t)1 << 20, kWtMaxBytes = (int64_t)64 << 20;

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 ld4_stream(const float4* p) {
  const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ void st4_out(float* p, const float4 v, const int wt) {
  if (wt) alignq_store::st16<alignq_store::kConvOut>(p, v);
  else *reinterpret_cast<float4*>(p) = v;
}

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}

// FA / FB: the formulas of site A and of site B (FB == -1: no second site; `res` may then be added).  Vector i holds elements
// 4i .. 4i+3 = channels 4 (i mod CQ) .. + 3 of one pixel.  d_pass = (gridDim.x * kTile) mod CQ, from the host.
template <int FA, int FB>
__global__ __launch_bounds__(kThreads) void site_eval_kernel(const SiteDev A, const SiteDev B, const float* __restrict__ res,
                                                             float* __restrict__ y, int64_t nvec, int C, float r, int d_pass, int wt) {
  constexpr bool kTwin = FB >= 0;
  constexpr bool kQuant = FA != 2 || (kTwin && FB != 2);
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  extern __shared__ __attribute__((aligned(16))) float ab_s[];      // [2][C] of A, then [2][C] of B: sized by the launch
  if (kQuant) nerf_tab_load(tab_lds);
  ab_table<kThreads>(ab_s, C, A);
  if (kTwin) ab_table<kThreads>(ab_s + 2 * C, C, B);
  __syncthreads();
  const NerfTab tab = nerf_tab(tab_lds);
  const bool bounded_r = fabsf(r) <= 8.0f;
  const Levels nlevA = make_levels(A.k, bounded_r), nlevB = make_levels(kTwin ? B.k : A.k, bounded_r);
  // the bounded form only where every quantiser of the launch is bounded; the general form tests yn per site and rounds the same
  Levels sw;
  sw.n = 0.0f;
  sw.yn = ((FA == 2 || nlevA.yn != 0.0f) && (!kTwin || FB == 2 || nlevB.yn != 0.0f) && kQuant) ? 1.0f : 0.0f;
  const int CQ = C >> 2;
  const int d_u = kThreads % CQ;
  const int64_t stride = (int64_t)gridDim.x * kTile;
  const float4* zA = reinterpret_cast<const float4*>(A.z);
  const float4* zB = reinterpret_cast<const float4*>(kTwin ? B.z : res);
  int64_t i0 = (int64_t)blockIdx.x * kTile + threadIdx.x;
  int cq = (int)(i0 % CQ);                                 // the one 64-bit modulo of the thread
  ALIGNQ_BOUNDED_SWITCH(sw,
  for (; i0 < nvec; i0 += stride) {
    float4 v[kU], w[kU];
_Pragma("unroll")
    for (int u = 0; u < kU; u++) {
      const int64_t i = i0 + u * kThreads;
      v[u] = ld4_stream(zA + (i < nvec ? i : i0));
      if (zB) w[u] = ld4_stream(zB + (i < nvec ? i : i0));
    }
    int c = cq;
_Pragma("unroll")
    for (int u = 0; u < kU; u++) {
      float4 o = site_q<FA, kBounded>(v[u], ab_s, C, c, A.k, nlevA, r, tab);   // (beyond nvec: still a valid table row; nothing is stored)
      if constexpr (kTwin) {
        constexpr int FB2 = FB < 0 ? 2 : FB;
        o = add4(o, clamp4(site_q<FB2, kBounded>(w[u], ab_s + 2 * C, C, c, B.k, nlevB, r, tab), B.clamp));
      } else {
        if (zB) o = add4(o, w[u]);
        o = clamp4(o, A.clamp);
      }
      v[u] = o;
      c += d_u;
      c = c >= CQ ? c - CQ : c;
    }
    // ONE branch on the store form per tile, behind the arithmetic: a branch per float4 would cut the four elements' instruction
    // streams apart (measured: +10 % per launch at 105 MB)
    if (wt) {
_Pragma("unroll")
      for (int u = 0; u < kU; u++) {
        const int64_t i = i0 + u * kThreads;
        if (i < nvec) st4_out(y + 4 * i, v[u], 1);
      }
    } else {
_Pragma("unroll")
      for (int u = 0; u < kU; u++) {
        const int64_t i = i0 + u * kThreads;
        if (i < nvec) st4_out(y + 4 * i, v[u], 0);
      }
    }
    cq += d_pass;
    cq = cq >= CQ ? cq - CQ : cq;
  })
}

// Source coordinate of tap k (0..2) along one axis of the forward convolution, and whether the tap exists (dwconv_kernels.hip)
template <int S>
__device__ __forceinline__ bool tap_coord(int d, int k, int n_src, int& s) {
  s = d * S + k - 1;
  return (unsigned)s < (unsigned)n_src;
}

// y [B][Hd][Wd][C] = clamp(q(a_c * dw(x [B][Hs][Ws][C], wq) + b_c)).  n_items = B * Hd * Wd * CQ; dwconv_kernel<S, false>'s body, then
// the site on the accumulator.
template <int S, int FORMULA>
__global__ __launch_bounds__(kThreads) void dwconv_site_eval_kernel(const float* __restrict__ src, const float* __restrict__ wq,
                                                                    const SiteDev A, float* __restrict__ dst, int n_items, int CQ,
                                                                    int Hd, int Wd, int Hs, int Ws, float r, int wt) {
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  extern __shared__ __attribute__((aligned(16))) float ab_s[];      // [2][C]
  const int C = CQ * 4;
  if (FORMULA != 2) nerf_tab_load(tab_lds);
  ab_table<kThreads>(ab_s, C, A);
  __syncthreads();
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev = make_levels(A.k, fabsf(r) <= 8.0f);
  const int step = gridDim.x * kThreads;
  float f[36];                                     // the quad's filters: f[j * 9 + tap] = wq[(4 * cq + j) * 9 + tap]
  int cq_held = -1;
  ALIGNQ_BOUNDED_SWITCH(nlev,
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n_items; i += step) {
    const int cq = i % CQ;
    int p = i / CQ;
    const int wd = p % Wd;
    p /= Wd;
    const int hd = p % Hd, b = p / Hd;
    if (cq != cq_held) {                           // once per thread where step % CQ == 0 (the host picks such a grid: C <= 2048)
_Pragma("unroll")
      for (int q = 0; q < 9; q++) {
        const float4 t = ld4(wq + cq * 36 + q * 4);
        f[q * 4 + 0] = t.x; f[q * 4 + 1] = t.y; f[q * 4 + 2] = t.z; f[q * 4 + 3] = t.w;
      }
      cq_held = cq;
    }
    float4 v[9];
    bool ok[9];
_Pragma("unroll")
    for (int ky = 0; ky < 3; ky++) {
      int hs;
      const bool okh = tap_coord<S>(hd, ky, Hs, hs);
_Pragma("unroll")
      for (int kx = 0; kx < 3; kx++) {
        int ws;
        const bool o = tap_coord<S>(wd, kx, Ws, ws) && okh;
        ok[ky * 3 + kx] = o;
        v[ky * 3 + kx] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o) v[ky * 3 + kx] = ld4(src + ((b * Hs + hs) * Ws + ws) * C + cq * 4);
      }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
_Pragma("unroll")
    for (int t = 0; t < 9; t++) {                  // a tap in the padding is skipped, not added as 0 * w (w may be inf / NaN)
      const float px = v[t].x * f[t], py = v[t].y * f[9 + t], pz = v[t].z * f[18 + t], pw = v[t].w * f[27 + t];
      acc.x = ok[t] ? acc.x + px : acc.x;
      acc.y = ok[t] ? acc.y + py : acc.y;
      acc.z = ok[t] ? acc.z + pz : acc.z;
      acc.w = ok[t] ? acc.w + pw : acc.w;
    }
    const float4 o = clamp4(site_q<FORMULA, kBounded>(acc, ab_s, C, cq, A.k, nlev, r, tab), A.clamp);
    st4_out(dst + i * 4, o, wt);
  })
}

// ------------------------------------------------------------------ host ----------------------
bool bad_k(int k) { return !((k >= 1 && k <= 16) || k == 32); }
bool bad_formula(int f) { return f != ALIGNQ_FORMULA_ADMM && f != ALIGNQ_FORMULA_CDF; }
bool bad_clamp(int c) { return c != ALIGNQ_CLAMP_NONE && c != ALIGNQ_CLAMP_RELU && c != ALIGNQ_CLAMP_RELU6; }
bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
bool bad_c(int C) { return C < 4 || C > kMaxC || (C & 3); }

// ALIGNQ_EINVAL for what the header lists about one site (z_needed: the elementwise forms read s->z)
bool bad_site(const alignq_eval_site* s, bool z_needed) {
  if (!s || !s->running_mean || !s->running_var || (z_needed && !s->z)) return true;
  if (bad_k(s->k) || bad_clamp(s->clamp)) return true;
  return z_needed && mis16(s->z);
}

SiteDev site_dev(const alignq_eval_site* s) {
  SiteDev d;
  d.z = s->z; d.gamma = s->gamma; d.beta = s->beta; d.mean = s->running_mean; d.var = s->running_var;
  d.eps = s->bn_eps; d.k = s->k; d.clamp = s->clamp;
  return d;
}

int site_grid(int64_t nvec) {
  const int64_t b = (nvec + kTile - 1) / kTile;
  return (int)(b > kSiteBlocks ? kSiteBlocks : b);
}

int gcd(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// dwconv_kernels.hip: elementwise_grid.  m = CQ / gcd(CQ, 256) <= 512 here, so a grid whose stride is a multiple of CQ always exists.
int dw_grid(int n_items, int CQ) {
  const int blocks = (n_items + kThreads - 1) / kThreads;
  if (blocks <= kDwMaxGrid) return blocks;
  const int m = CQ / gcd(CQ, kThreads);
  return kDwMaxGrid / m * m;
}

int write_through(int64_t out_bytes) { return out_bytes >= kWtMinBytes && out_bytes <= kWtMaxBytes ? 1 : 0; }

int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int alignq_site_eval_fwd(const alignq_eval_site* site, int64_t P, int C, float act_range, int formula, const float* residual,
                         float* y, void* stream) {
  if (bad_site(site, true) || !y || P < 1 || bad_formula(formula) || mis16(y) || mis16(residual)) return ALIGNQ_EINVAL;
  if (bad_c(C)) return ALIGNQ_EUNSUPPORTED;
  const int64_t nvec = P * (C >> 2);
  const int grid = site_grid(nvec), CQ = C >> 2;
  const int d_pass = (int)(((int64_t)grid * kTile) % CQ);
  const int wt = write_through(nvec * 16);
  const SiteDev A = site_dev(site);
  const size_t lds = (size_t)2 * C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define SITE_LAUNCH(F) \
  hipLaunchKernelGGL((site_eval_kernel<F, -1>), grid, kThreads, lds, st, A, A, residual, y, nvec, C, act_range, d_pass, wt)
  if (site->k == 32) SITE_LAUNCH(2);
  else if (formula == ALIGNQ_FORMULA_CDF) SITE_LAUNCH(1);
  else SITE_LAUNCH(0);
#undef SITE_LAUNCH
  return last_error();
}

int alignq_site_eval_twin_fwd(const alignq_eval_site* a, const alignq_eval_site* b, int64_t P, int C, float act_range, int formula,
                              float* y, void* stream) {
  if (bad_site(a, true) || bad_site(b, true) || !y || P < 1 || bad_formula(formula) || mis16(y)) return ALIGNQ_EINVAL;
  if (a->clamp != ALIGNQ_CLAMP_NONE) return ALIGNQ_EINVAL;
  if (bad_c(C)) return ALIGNQ_EUNSUPPORTED;
  const int64_t nvec = P * (C >> 2);
  const int grid = site_grid(nvec), CQ = C >> 2;
  const int d_pass = (int)(((int64_t)grid * kTile) % CQ);
  const int wt = write_through(nvec * 16);
  const SiteDev A = site_dev(a), B = site_dev(b);
  const size_t lds = (size_t)4 * C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define TWIN_LAUNCH(FA, FB) \
  hipLaunchKernelGGL((site_eval_kernel<FA, FB>), grid, kThreads, lds, st, A, B, (const float*)nullptr, y, nvec, C, act_range, d_pass, wt)
#define TWIN_BY_B(FA, F)           \
  if (b->k == 32) TWIN_LAUNCH(FA, 2); \
  else TWIN_LAUNCH(FA, F)
  if (a->k == 32) {
    if (formula == ALIGNQ_FORMULA_CDF) { TWIN_BY_B(2, 1); } else { TWIN_BY_B(2, 0); }
  } else if (formula == ALIGNQ_FORMULA_CDF) {
    TWIN_BY_B(1, 1);
  } else {
    TWIN_BY_B(0, 0);
  }
#undef TWIN_BY_B
#undef TWIN_LAUNCH
  return last_error();
}

int alignq_dwconv3x3_site_eval_fwd(const float* x, const float* wq, const alignq_eval_site* site, int B, int H_in, int W_in, int C,
                                   int stride, float act_range, int formula, float* y, void* stream) {
  if (!x || !wq || !y || bad_site(site, false) || bad_formula(formula) || B < 1 || H_in < 1 || W_in < 1) return ALIGNQ_EINVAL;
  if (mis16(x) || mis16(wq) || mis16(y)) return ALIGNQ_EINVAL;
  if (bad_c(C) || !alignq_dwconv3x3_supported(B, H_in, W_in, C, stride)) return ALIGNQ_EUNSUPPORTED;
  const int Ho = (H_in - 1) / stride + 1, Wo = (W_in - 1) / stride + 1, CQ = C / 4;
  const int n_items = B * Ho * Wo * CQ;
  const int grid = dw_grid(n_items, CQ);
  const int wt = write_through((int64_t)n_items * 16);
  const SiteDev A = site_dev(site);
  const size_t lds = (size_t)2 * C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define DW_LAUNCH(S, F) \
  hipLaunchKernelGGL((dwconv_site_eval_kernel<S, F>), grid, kThreads, lds, st, x, wq, A, y, n_items, CQ, Ho, Wo, H_in, W_in, act_range, wt)
#define DW_BY_F(S)                                      \
  if (site->k == 32) DW_LAUNCH(S, 2);                   \
  else if (formula == ALIGNQ_FORMULA_CDF) DW_LAUNCH(S, 1); \
  else DW_LAUNCH(S, 0)
  if (stride == 1) { DW_BY_F(1); } else { DW_BY_F(2); }
#undef DW_BY_F
#undef DW_LAUNCH
  return last_error();
}

}  // extern "C"

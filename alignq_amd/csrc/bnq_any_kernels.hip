// bnq_any_kernels.hip - training-mode batch-norm folded into the PLAIN quantiser and a clamp (none / ReLU / ReLU6) at ANY channel
// count C % 4 == 0 in [4, 2048] (include/alignq_bnq_any.h): the sites of MobileNet-V2 (C = 16 ... 1280) and DenseNet-40 (C = 24, 36,
// ..., 456), which bnq_kernels.hip refuses because its thread mapping needs C = 4 * 2^j.  The arithmetic is bnq_kernels.hip's,
// operation for operation (tests/bnq_oracle.py restates it for both families; built with -ffp-contract=off):
//   forward : any_sums<0> (per-channel sum z, sum z^2 in double) -> any_finalize_fwd (mean, invstd, a = gamma * invstd,
//             b = beta - f32(mean) * a, running statistics) -> any_apply_fwd: y = clamp(quantise(fma(a, z, b))) + one mask bit per element;
//   backward: any_sums<1> (dx = gm * act_jac(fma(a, z, b)), gm = g where the mask bit is set; sum dx, sum dx * zhat) ->
//             any_finalize_bwd (k0, k1, dgamma, dbeta) -> any_apply_bwd: dz = a * ((dx - k0) - zhat * k1).
// Three launches each way, no atomics: every sum has a fixed order, so two launches give the same bits.
// The reductions, the finalisations and their geometry live in bnq_any_body.h, which bnq_pool_kernels.hip includes too.
//
// The mapping, which is what differs from bnq_kernels.hip:
//   * reductions: a workgroup owns a contiguous pixel range; its threads are slots x L, L = the lanes one pixel takes: C / 4 channel
//     quads, or half of them (rounded up) above 256 quads, where a thread owns TWO quads (l and l + L).  L does not divide a block in
//     general, so the block size is chosen per launch among seven whole-wave sizes (geo_for) to fill it best and the surplus lanes
//     idle: 448 threads = 3 slots x 144 quads at C = 576, 320 threads = 1 slot x 320 lanes x 2 quads at C = 1280.  A thread keeps its quads'
//     a, b, mean, invstd in registers for the whole launch, has U float4 per array in flight before the first use, accumulates in
//     double; the slots are added through LDS in slot order;
//   * elementwise passes: the flat float4 index, consecutive lanes on consecutive 16 bytes whatever C is; the per-channel constants
//     are staged once per workgroup in LDS and indexed by i mod C/4, advanced by launch-constant steps (one 64-bit modulo per thread).
#include <hip/hip_runtime.h>

#include "../../include/alignq.h"
#include "../../include/alignq_bnq_any.h"
#include "../../include/alignq_mobile.h"
#include "alignq_math.h"
#include "store_forms.h"
#include "bnq_any_body.h"              // the reductions and finalisations (shared with bnq_pool_kernels.hip), geo_for, parts_for

using namespace alignq;

namespace {

constexpr int kMaxC = 2048;
constexpr int kTA = 256;               // threads of the elementwise kernels
constexpr int kUF = 4, kUB = 2;        // float4 per thread and tile: forward / backward apply
constexpr int kApplyBlocks = 2048;     // grid cap of the elementwise kernels; the rest by grid stride

inline int64_t mask_words(int64_t nvec) { return ((nvec + 63) >> 6) * 4; }

// ---- launch geometry (host; Geo, geo_for and parts_for: bnq_any_body.h) -------------------------------------------------------------
inline bool bad_c(int C) { return C < 4 || C > kMaxC || (C & 3) != 0; }
inline bool bad_p(int64_t P) { return P < 2 || P > ((int64_t)1 << 40); }
inline float* ktot_of(void* ws, int64_t P, int C) {
  return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + (size_t)parts_for(P, C, nullptr) * C * 2 * sizeof(double));
}
inline int apply_grid(int64_t nvec, int u) {
  const int64_t b = (nvec + (int64_t)kTA * u - 1) / ((int64_t)kTA * u);
  return (int)(b > kApplyBlocks ? kApplyBlocks : b);
}

// ---- elementwise passes over the flat float4 index --------------------------------------------------------------------------------
// Vector i holds channels 4 (i mod CQ) .. + 3 of one pixel.  d_pass = (gridDim.x * tile) mod CQ, from the host.
__device__ __forceinline__ float clamp1(float v, int clamp) {
  if (clamp == ALIGNQ_CLAMP_NONE) return v;
  const float hi = (clamp == ALIGNQ_CLAMP_RELU6 && !(v < 6.0f)) ? 6.0f : v;
  return v > 0.0f ? hi : 0.0f;
}
__device__ __forceinline__ bool passes1(float v, int clamp) {        // "the gradient passes": 0 < y (ReLU), 0 < y < 6 (ReLU6)
  return v > 0.0f && (clamp != ALIGNQ_CLAMP_RELU6 || v < 6.0f);
}

template <int FORMULA>
__global__ __launch_bounds__(kTA) void any_apply_fwd_kernel(const float* __restrict__ z, const float* __restrict__ ab, int64_t nvec,
                                                            int C, int k, float r, int clamp, int d_pass, int wt,
                                                            float* __restrict__ y, unsigned long long* __restrict__ mask) {
  __shared__ __attribute__((aligned(16))) float nerf_lds[ALIGNQ_NERF_LDS_FLOATS];
  extern __shared__ __attribute__((aligned(16))) float ab_s[];       // [2][C]: a, b
  nerf_tab_load(nerf_lds);
  for (int i = threadIdx.x; i < 2 * C; i += kTA) ab_s[i] = ab[i];
  __syncthreads();
  const NerfTab tab = nerf_tab(nerf_lds);
  const Levels nlev = make_levels(k, fabsf(r) <= 8.0f);
  const int CQ = C >> 2, d_u = kTA % CQ;
  const int64_t stride = (int64_t)gridDim.x * (kTA * kUF);
  int64_t i0 = (int64_t)blockIdx.x * (kTA * kUF) + threadIdx.x;
  int cq = (int)(i0 % CQ);                                           // the one 64-bit modulo of the thread
  ALIGNQ_BOUNDED_SWITCH(nlev,
  for (; i0 < nvec; i0 += stride) {
    float4 v[kUF];
_Pragma("unroll")
    for (int u = 0; u < kUF; u++) {
      const int64_t i = i0 + u * kTA;
      v[u] = ld4_stream(z + 4 * (i < nvec ? i : i0));                // z was read by the statistics pass; this is its last forward use
    }
    int c = cq;
_Pragma("unroll")
    for (int u = 0; u < kUF; u++) {
      const int64_t i = i0 + u * kTA;
      const float4 a4 = ld4(ab_s + 4 * c), b4 = ld4(ab_s + C + 4 * c);
      float t, bin;
      float4 o;
      o.x = act_quant1<FORMULA, kBounded>(__fmaf_rn(a4.x, v[u].x, b4.x), k, nlev, r, &t, &bin, tab);
      o.y = act_quant1<FORMULA, kBounded>(__fmaf_rn(a4.y, v[u].y, b4.y), k, nlev, r, &t, &bin, tab);
      o.z = act_quant1<FORMULA, kBounded>(__fmaf_rn(a4.z, v[u].z, b4.z), k, nlev, r, &t, &bin, tab);
      o.w = act_quant1<FORMULA, kBounded>(__fmaf_rn(a4.w, v[u].w, b4.w), k, nlev, r, &t, &bin, tab);
      if (mask) {
        // the wave's 64 float4 are the consecutive vec indices of ONE chunk (tile bases and kTA are multiples of 64): four wave-wide
        // compares = the chunk's four words, stored by lane 0 (a chunk is written whole or - beyond nvec - not at all)
        const bool in = i < nvec;
        const unsigned long long mx = __ballot(in && passes1(o.x, clamp)), my = __ballot(in && passes1(o.y, clamp));
        const unsigned long long mz = __ballot(in && passes1(o.z, clamp)), mw = __ballot(in && passes1(o.w, clamp));
        const int lane = threadIdx.x & 63;
        const int64_t i_w = i - lane;                                // the wave's first vec index
        if (lane == 0 && i_w < nvec) {                               // (lane 0 is in the loop whenever any lane of its wave is)
          ulonglong2* w2 = reinterpret_cast<ulonglong2*>(mask + (i_w >> 6) * 4);
          w2[0] = make_ulonglong2(mx, my);
          w2[1] = make_ulonglong2(mz, mw);
        }
      }
      v[u] = make_float4(clamp1(o.x, clamp), clamp1(o.y, clamp), clamp1(o.z, clamp), clamp1(o.w, clamp));
      c += d_u;
      c = c >= CQ ? c - CQ : c;
    }
    // one branch on the store form per tile, behind the arithmetic (mobile_eval_kernels.hip)
    if (wt) {
_Pragma("unroll")
      for (int u = 0; u < kUF; u++) {
        const int64_t i = i0 + u * kTA;
        if (i < nvec) alignq_store::st16<alignq_store::kConvOut>(y + 4 * i, v[u]);
      }
    } else {
_Pragma("unroll")
      for (int u = 0; u < kUF; u++) {
        const int64_t i = i0 + u * kTA;
        if (i < nvec) *reinterpret_cast<float4*>(y + 4 * i) = v[u];
      }
    }
    cq += d_pass;
    cq = cq >= CQ ? cq - CQ : cq;
  })
}

// reads g, z and the mask, never y.  tab_s: [6][C] = a, b, mean, invstd, k0, k1 (48 KB at C = 2048)
__global__ __launch_bounds__(kTA) void any_apply_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                            const unsigned long long* __restrict__ mask,
                                                            const float* __restrict__ ab, const float* __restrict__ save,
                                                            const float* __restrict__ ktot, int64_t nvec, int C, float r, int d_pass,
                                                            int wt, float* __restrict__ dz) {
  extern __shared__ __attribute__((aligned(16))) float tab_s[];
  for (int i = threadIdx.x; i < 2 * C; i += kTA) {
    tab_s[i] = ab[i];
    tab_s[2 * C + i] = save[i];
    tab_s[4 * C + i] = ktot[i];
  }
  __syncthreads();
  const int CQ = C >> 2, d_u = kTA % CQ;
  const int64_t stride = (int64_t)gridDim.x * (kTA * kUB);
  int64_t i0 = (int64_t)blockIdx.x * (kTA * kUB) + threadIdx.x;
  int cq = (int)(i0 % CQ);
  for (; i0 < nvec; i0 += stride) {
    float4 gv[kUB], zv[kUB];
    bool mk[kUB][4];
#pragma unroll
    for (int u = 0; u < kUB; u++) {
      const int64_t i = i0 + u * kTA, ic = i < nvec ? i : i0;
      gv[u] = ld4_stream(g + 4 * ic);                                // both are read here for the last time
      zv[u] = ld4_stream(z + 4 * ic);
      if (mask) mask_bits4(mask, ic, mk[u]);
    }
    int c = cq;
#pragma unroll
    for (int u = 0; u < kUB; u++) {
      const int64_t i = i0 + u * kTA;
      const float4 a4 = ld4(tab_s + 4 * c), b4 = ld4(tab_s + C + 4 * c), m4 = ld4(tab_s + 2 * C + 4 * c);
      const float4 i4 = ld4(tab_s + 3 * C + 4 * c), k0 = ld4(tab_s + 4 * C + 4 * c), k1 = ld4(tab_s + 5 * C + 4 * c);
      const float ge[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w}, ze[4] = {zv[u].x, zv[u].y, zv[u].z, zv[u].w};
      const float ae[4] = {a4.x, a4.y, a4.z, a4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
      const float me[4] = {m4.x, m4.y, m4.z, m4.w}, ie[4] = {i4.x, i4.y, i4.z, i4.w};
      const float k0e[4] = {k0.x, k0.y, k0.z, k0.w}, k1e[4] = {k1.x, k1.y, k1.z, k1.w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float x = __fmaf_rn(ae[e], ze[e], be[e]);
        const float gm = (mask && !mk[u][e]) ? 0.f : ge[e];
        const float dx = gm * act_jac(x, r);
        const float zh = (ze[e] - me[e]) * ie[e];
        o[e] = ae[e] * ((dx - k0e[e]) - zh * k1e[e]);
      }
      if (i < nvec) {
        const float4 ov = make_float4(o[0], o[1], o[2], o[3]);
        if (wt) alignq_store::st16<alignq_store::kConvOut>(dz + 4 * i, ov);
        else *reinterpret_cast<float4*>(dz + 4 * i) = ov;
      }
      c += d_u;
      c = c >= CQ ? c - CQ : c;
    }
    cq += d_pass;
    cq = cq >= CQ ? cq - CQ : cq;
  }
}

inline bool bad_clamp(int clamp) { return clamp != ALIGNQ_CLAMP_NONE && clamp != ALIGNQ_CLAMP_RELU && clamp != ALIGNQ_CLAMP_RELU6; }

template <int MODE>
inline void launch_sums(const Geo& ge, int np, hipStream_t st, const float* z, const float* g, const unsigned long long* mask,
                        const float* ab, const float* save, int64_t P, int C, int64_t per, float r, double* part) {
  if (ge.Q == 2)
    hipLaunchKernelGGL((any_sums_kernel<MODE, 2>), dim3(np), dim3(ge.NT), 0, st, z, g, mask, ab, save, P, C, (int64_t)(C >> 2), ge.L, ge.slots, per, r, part);
  else
    hipLaunchKernelGGL((any_sums_kernel<MODE, 1>), dim3(np), dim3(ge.NT), 0, st, z, g, mask, ab, save, P, C, (int64_t)(C >> 2), ge.L, ge.slots, per, r, part);
}

}  // namespace

extern "C" {

int alignq_bnq_any_supported(int64_t P, int C) { return (bad_c(C) || bad_p(P)) ? 0 : 1; }

size_t alignq_bnq_any_ws_bytes(int64_t P, int C) {
  if (bad_c(C) || bad_p(P)) return 0;
  return (size_t)parts_for(P, C, nullptr) * C * 2 * sizeof(double) + (size_t)2 * C * sizeof(float);
}

size_t alignq_bnq_any_mask_bytes(int64_t P, int C) {
  if (bad_c(C) || bad_p(P)) return 0;
  return (size_t)mask_words(P * (C >> 2)) * sizeof(unsigned long long);
}

int alignq_bnq_any_fwd(const float* z, int64_t P, int C, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, float momentum, float bn_eps, int k, float act_range,
                       int formula, int clamp, float* ab, float* save, float* y, void* mask, void* ws, void* stream) {
  if (!z || !ab || !save || !y || !ws || P < 2 || bad_clamp(clamp)) return ALIGNQ_EINVAL;
  if ((clamp != ALIGNQ_CLAMP_NONE) != (mask != nullptr)) return ALIGNQ_EINVAL;      // a mask exactly where there is a clamp
  if (!((k >= 1 && k <= 16) || k == 32)) return ALIGNQ_EINVAL;
  if (formula != ALIGNQ_FORMULA_ADMM && formula != ALIGNQ_FORMULA_CDF) return ALIGNQ_EINVAL;
  if (misaligned(z) || misaligned(y) || misaligned(mask) || misaligned(ws)) return ALIGNQ_EINVAL;
  if (bad_c(C) || bad_p(P)) return ALIGNQ_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const Geo ge = geo_for(C);
  int64_t per;
  const int np = parts_for(P, C, &per);
  launch_sums<0>(ge, np, st, z, nullptr, nullptr, nullptr, nullptr, P, C, per, act_range, part);
  hipLaunchKernelGGL(any_finalize_fwd_kernel, dim3((C + kFinT - 1) / kFinT), dim3(kFinT), 0, st, (const double*)part, np, P, C, gamma,
                     beta, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, bn_eps, ab, save);
  const int64_t nvec = P * (C >> 2);
  const int grid = apply_grid(nvec, kUF), CQ = C >> 2;
  const int d_pass = (int)(((int64_t)grid * kTA * kUF) % CQ);
  const size_t lds = (size_t)2 * C * sizeof(float);
  unsigned long long* mk = reinterpret_cast<unsigned long long*>(mask);
  if (formula == ALIGNQ_FORMULA_ADMM)
    hipLaunchKernelGGL((any_apply_fwd_kernel<0>), dim3(grid), dim3(kTA), lds, st, z, (const float*)ab, nvec, C, k, act_range, clamp,
                       d_pass, wt_for(nvec), y, mk);
  else
    hipLaunchKernelGGL((any_apply_fwd_kernel<1>), dim3(grid), dim3(kTA), lds, st, z, (const float*)ab, nvec, C, k, act_range, clamp,
                       d_pass, wt_for(nvec), y, mk);
  return hipGetLastError() == hipSuccess ? 0 : ALIGNQ_EINVAL;
}

int alignq_bnq_any_bwd(const float* g, const float* z, const void* mask, const float* ab, const float* save, int64_t P, int C,
                       float act_range, int clamp, float* dz, float* dgamma, float* dbeta, void* ws, void* stream) {
  if (!g || !z || !ab || !save || !dz || !ws || P < 2 || bad_clamp(clamp)) return ALIGNQ_EINVAL;
  if ((clamp != ALIGNQ_CLAMP_NONE) != (mask != nullptr)) return ALIGNQ_EINVAL;
  if (misaligned(g) || misaligned(z) || misaligned(dz) || misaligned(mask) || misaligned(ws)) return ALIGNQ_EINVAL;
  if (bad_c(C) || bad_p(P)) return ALIGNQ_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  float* ktot = ktot_of(ws, P, C);
  const unsigned long long* mk = reinterpret_cast<const unsigned long long*>(mask);
  const Geo ge = geo_for(C);
  int64_t per;
  const int np = parts_for(P, C, &per);
  launch_sums<1>(ge, np, st, z, g, mk, ab, save, P, C, per, act_range, part);
  hipLaunchKernelGGL(any_finalize_bwd_kernel, dim3((C + kFinT - 1) / kFinT), dim3(kFinT), 0, st, (const double*)part, np, P, C, ktot,
                     dgamma, dbeta);
  const int64_t nvec = P * (C >> 2);
  const int grid = apply_grid(nvec, kUB), CQ = C >> 2;
  const int d_pass = (int)(((int64_t)grid * kTA * kUB) % CQ);
  hipLaunchKernelGGL(any_apply_bwd_kernel, dim3(grid), dim3(kTA), (size_t)6 * C * sizeof(float), st, g, z, mk, ab, save,
                     (const float*)ktot, nvec, C, act_range, d_pass, wt_for(nvec), dz);
  return hipGetLastError() == hipSuccess ? 0 : ALIGNQ_EINVAL;
}

}  // extern "C"

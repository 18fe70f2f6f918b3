// bnq_pool_kernels.hip - training-mode batch-norm folded into the PLAIN quantiser, a ReLU and a 2 x 2 max-pool
// (include/alignq_bnq_pool.h): the digit DANN's two training sites, z[B][H][W][C] -> y[B][H/2][W/2][C].  The arithmetic per position is
// bnq_any_kernels.hip's with ALIGNQ_CLAMP_RELU, operation for operation (built with -ffp-contract=off):
//   forward : any_sums<0> and any_finalize_fwd of bnq_any_body.h over the P = B * H * W un-pooled pixels (the same code: the same
//             bits) -> pool_apply_fwd: a thread owns one channel quad of one POOLED pixel, loads its window's four float4 of z,
//             quantises the sixteen values, keeps the first maximum per channel and writes one float4 of y and four code bytes;
//   backward: pool_sums_bwd (sum dx, sum dx * zhat over the pooled elements: g, the code and ONE z per element) ->
//             any_finalize_bwd with the full P -> pool_apply_bwd: a thread owns one channel quad of one window and writes its four
//             float4 of dz = a * ((dx - k0) - zhat * k1), dx != 0 only at the selected position.
// Three launches each way, no atomics: every sum has a fixed order, so two launches give the same bits.
//
// What is this file's own:
//   * behind the pool one of four positions carries a gradient, so the backward statistics read a quarter of the elements: g and
//     the code as whole float4 / words per lane, then the selected z of each of the lane's four channels as a scalar load whose
//     address the code byte gives (the four channels of a quad select independently).  Un-pooled y and un-pooled gradient never exist;
//   * the window kernels take no LDS for the per-channel constants and no grid-stride bookkeeping: the flat index i of a (pooled
//     pixel, quad) pair gives quad i mod C/4 and, from the pooled pixel pp = i div C/4 = (b * H/2 + ho) * W/2 + wo, the window's first
//     pixel 4 * (pp div W/2) * W/2 + 2 * wo (b * H + 2 ho = 2 (b * H/2 + ho): no division by H).  Consecutive lanes take consecutive
//     16 bytes of y, g and dz rows and consecutive 4 bytes of the code;
//   * sized for the two real shapes, 36 864 x 32 and 4 096 x 48 elements at batch 64, which are latency-bound: one-wave workgroups
//     (1152 and 192 of them: at most one wave per SIMD, all in flight at once), every load of a thread issued before the first use,
//     4 pooled pixels per slot in the reduction.
#include <hip/hip_runtime.h>

#include "../../include/alignq.h"
#include "../../include/alignq_bnq_pool.h"
#include "alignq_math.h"
#include "store_forms.h"
#include "bnq_any_body.h"              // any_sums_kernel, the finalisations, geo_for, parts_for, slot_reduce

using namespace alignq;

namespace {

constexpr int kPoolMaxC = 1024;        // one channel quad per thread in the reductions (bnq_any_body.h: Q == 1)
constexpr int kTW = 64;                // threads of the two window kernels: one wave
constexpr int kWinBlocks = 1 << 16;    // their grid cap; the rest by grid stride
constexpr int kPoolSlotPixels = 4;     // pooled pixels per slot a reduction workgroup should at least own: one round of loads
constexpr int kUS = 4;                 // pooled pixels per thread in flight in pool_sums_bwd

// i -> (pp, quad) and pp -> the window's first pixel; 32-bit divisions wherever the numbers allow (always, at the sizes of a network)
__device__ __forceinline__ void split(int64_t v, int d, int64_t& quot, int& rem) {
  if (v < ((int64_t)1 << 32)) {
    const unsigned q = (unsigned)v / (unsigned)d;
    quot = q;
    rem = (int)((unsigned)v - q * (unsigned)d);
  } else {
    quot = v / d;
    rem = (int)(v - quot * d);
  }
}
// pooled pixel pp = (b * Ho + ho) * Wo + wo -> un-pooled pixel (b * H + 2 ho) * W + 2 wo, with H = 2 Ho, W = 2 Wo
__device__ __forceinline__ int64_t window_pixel(int64_t pp, int Wo) {
  int64_t row;
  int wo;
  split(pp, Wo, row, wo);
  return 4 * row * Wo + 2 * wo;
}

// ---- forward: site and pool, one channel quad of one pooled pixel per thread ---------------------------------------------------
template <int FORMULA>
__global__ __launch_bounds__(kTW) void pool_apply_fwd_kernel(const float* __restrict__ z, const float* __restrict__ ab, int64_t nvec,
                                                             int C, int Wo, int k, float r, int wt, float* __restrict__ y,
                                                             uint32_t* __restrict__ code) {
  __shared__ __attribute__((aligned(16))) float nerf_lds[ALIGNQ_NERF_LDS_FLOATS];
  nerf_tab_load(nerf_lds);
  __syncthreads();
  const NerfTab tab = nerf_tab(nerf_lds);
  const Levels nlev = make_levels(k, fabsf(r) <= 8.0f);
  const int CQ = C >> 2;
  const int64_t rowf = (int64_t)2 * Wo * C;                          // floats per row of z
  ALIGNQ_BOUNDED_SWITCH(nlev,
  for (int64_t i = (int64_t)blockIdx.x * kTW + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * kTW) {
    int64_t pp;
    int cq;
    split(i, CQ, pp, cq);
    const float* zp = z + window_pixel(pp, Wo) * C + 4 * cq;
    // the statistics pass read z; this is its last forward use
    const float4 v[4] = {ld4_stream(zp), ld4_stream(zp + C), ld4_stream(zp + rowf), ld4_stream(zp + rowf + C)};
    const float4 a4 = ld4(ab + 4 * cq), b4 = ld4(ab + C + 4 * cq);
    const float ae[4] = {a4.x, a4.y, a4.z, a4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
    float best[4];
    uint32_t word = 0;
_Pragma("unroll")
    for (int e = 0; e < 4; e++) {
      uint32_t sel = 0;
_Pragma("unroll")
      for (int p = 0; p < 4; p++) {
        const float ze = e == 0 ? v[p].x : e == 1 ? v[p].y : e == 2 ? v[p].z : v[p].w;
        float t, bin;
        const float q = act_quant1<FORMULA, kBounded>(__fmaf_rn(ae[e], ze, be[e]), k, nlev, r, &t, &bin, tab);
        const float u = q > 0.0f ? q : 0.0f;                           // ALIGNQ_CLAMP_RELU
        if (p == 0) {
          best[e] = u;
        } else if (u > best[e]) {                                      // strictly greater: the FIRST maximum stays
          best[e] = u;
          sel = p;
        }
      }
      word |= (sel | (best[e] > 0.0f ? 4u : 0u)) << (8 * e);
    }
    const float4 o = make_float4(best[0], best[1], best[2], best[3]);
    if (wt) alignq_store::st16<alignq_store::kConvOut>(y + 4 * i, o);
    else *reinterpret_cast<float4*>(y + 4 * i) = o;
    code[i] = word;
  })
}

// ---- backward statistics over the pooled elements ------------------------------------------------------------------------------
// part: [gridDim.x][C][2] doubles {sum dx, sum dx * zhat}.  blockDim.x = the Geo's NT; a thread is (slot, quad l) as in any_sums_kernel.
__global__ __launch_bounds__(kMaxNT) void pool_sums_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                               const uint32_t* __restrict__ code, const float* __restrict__ ab,
                                                               const float* __restrict__ save, int64_t PP, int C, int Wo, int L,
                                                               int slots, int64_t per, float r, double* __restrict__ part) {
  __shared__ double sm[kMaxNT * 4];
  const int tid = threadIdx.x;
  const int slot = tid / L, l = tid - slot * L;
  const bool active = slot < slots;                                  // the surplus lanes of the block idle
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < PP ? p0 + per : PP;
  const int64_t rowf = (int64_t)2 * Wo * C;
  double s0[1][4], s1[1][4];
#pragma unroll
  for (int e = 0; e < 4; e++) { s0[0][e] = 0; s1[0][e] = 0; }
  if (active) {
    const float4 a4 = ld4(ab + 4 * l), b4 = ld4(ab + C + 4 * l), m4 = ld4(save + 4 * l), i4 = ld4(save + C + 4 * l);
    const float ae[4] = {a4.x, a4.y, a4.z, a4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
    const float me[4] = {m4.x, m4.y, m4.z, m4.w}, ie[4] = {i4.x, i4.y, i4.z, i4.w};
    for (int64_t base = p0 + slot; base < p1; base += (int64_t)slots * kUS) {
      float4 gv[kUS];
      uint32_t cd[kUS];
      const float* zp[kUS];
#pragma unroll
      for (int u = 0; u < kUS; u++) {                                // clamped address, masked below
        const int64_t px = base + (int64_t)u * slots, pc = px < p1 ? px : p1 - 1;
        const int64_t i = pc * (C >> 2) + l;
        gv[u] = ld4(g + 4 * i);
        cd[u] = code[i];
        zp[u] = z + window_pixel(pc, Wo) * C + 4 * l;
      }
      float zs[kUS][4];
#pragma unroll
      for (int u = 0; u < kUS; u++)
#pragma unroll
        for (int e = 0; e < 4; e++) {                                // the ONE selected z of each of the four channels' windows
          const uint32_t b = cd[u] >> (8 * e);
          zs[u][e] = zp[u][((b & 1) ? C : 0) + ((b & 2) ? rowf : 0) + e];
        }
#pragma unroll
      for (int u = 0; u < kUS; u++) {
        if (base + (int64_t)u * slots < p1) {
          const float ge[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float x = __fmaf_rn(ae[e], zs[u][e], be[e]);
            const float gm = ((cd[u] >> (8 * e)) & 4) ? ge[e] : 0.f;
            const float dx = gm * act_jac(x, r);
            const float zh = (zs[u][e] - me[e]) * ie[e];
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

// ---- backward apply: the four dz of a window from z, g and the code ------------------------------------------------------------
__global__ __launch_bounds__(kTW) void pool_apply_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                             const uint32_t* __restrict__ code, const float* __restrict__ ab,
                                                             const float* __restrict__ save, const float* __restrict__ ktot,
                                                             int64_t nvec, int C, int Wo, float r, int wt, float* __restrict__ dz) {
  const int CQ = C >> 2;
  const int64_t rowf = (int64_t)2 * Wo * C;
  for (int64_t i = (int64_t)blockIdx.x * kTW + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * kTW) {
    int64_t pp;
    int cq;
    split(i, CQ, pp, cq);
    const int64_t off = window_pixel(pp, Wo) * C + 4 * cq;
    const int64_t po[4] = {off, off + C, off + rowf, off + rowf + C};
    // g, z and the code are read here for the last time
    const float4 gv = ld4_stream(g + 4 * i);
    const uint32_t cd = __builtin_nontemporal_load(code + i);
    const float4 v[4] = {ld4_stream(z + po[0]), ld4_stream(z + po[1]), ld4_stream(z + po[2]), ld4_stream(z + po[3])};
    const float4 a4 = ld4(ab + 4 * cq), b4 = ld4(ab + C + 4 * cq), m4 = ld4(save + 4 * cq), i4 = ld4(save + C + 4 * cq);
    const float4 k04 = ld4(ktot + 4 * cq), k14 = ld4(ktot + C + 4 * cq);
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
    const float ae[4] = {a4.x, a4.y, a4.z, a4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
    const float me[4] = {m4.x, m4.y, m4.z, m4.w}, ie[4] = {i4.x, i4.y, i4.z, i4.w};
    const float k0e[4] = {k04.x, k04.y, k04.z, k04.w}, k1e[4] = {k14.x, k14.y, k14.z, k14.w};
    float o[4][4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const uint32_t b = cd >> (8 * e);
      const int sel = (int)(b & 3);
      float ze[4];
#pragma unroll
      for (int p = 0; p < 4; p++) ze[p] = e == 0 ? v[p].x : e == 1 ? v[p].y : e == 2 ? v[p].z : v[p].w;
      const float zsel = sel == 0 ? ze[0] : sel == 1 ? ze[1] : sel == 2 ? ze[2] : ze[3];
      const float gm = (b & 4) ? ge[e] : 0.f;
      const float dxs = gm * act_jac(__fmaf_rn(ae[e], zsel, be[e]), r);      // one exponential per window and channel
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const float dx = p == sel ? dxs : 0.f;
        const float zh = (ze[p] - me[e]) * ie[e];
        o[p][e] = ae[e] * ((dx - k0e[e]) - zh * k1e[e]);
      }
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const float4 ov = make_float4(o[p][0], o[p][1], o[p][2], o[p][3]);
      if (wt) alignq_store::st16<alignq_store::kConvOut>(dz + po[p], ov);
      else *reinterpret_cast<float4*>(dz + po[p]) = ov;
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct Shape {
  int64_t P, PP;             // un-pooled and pooled pixels
  int rc;                    // 0, ALIGNQ_EINVAL or ALIGNQ_EUNSUPPORTED
};
inline Shape shape_of(int64_t B, int H, int W, int C) {
  Shape s = {0, 0, 0};
  const int64_t lim = (int64_t)1 << 40;
  if (B < 1 || H < 1 || W < 1 || (B == 1 && H == 1 && W == 1)) { s.rc = ALIGNQ_EINVAL; return s; }          // P < 2
  const int64_t hw = (int64_t)H * W;
  if (C < 4 || C > kPoolMaxC || (C & 3) != 0 || (H & 1) || (W & 1) || B > lim / hw) { s.rc = ALIGNQ_EUNSUPPORTED; return s; }
  s.P = B * hw;
  s.PP = s.P >> 2;
  return s;
}
inline int win_grid(int64_t nvec) {
  const int64_t b = (nvec + kTW - 1) / kTW;
  return (int)(b > kWinBlocks ? kWinBlocks : b);
}
inline size_t part_bytes(const Shape& s, int C) {
  const int nf = parts_for(s.P, C, nullptr), nb = parts_for(s.PP, C, nullptr, kPoolSlotPixels);
  return (size_t)(nf > nb ? nf : nb) * C * 2 * sizeof(double);
}

}  // namespace

extern "C" {

int alignq_bnq_pool_supported(int64_t B, int H, int W, int C) { return shape_of(B, H, W, C).rc == 0 ? 1 : 0; }

size_t alignq_bnq_pool_ws_bytes(int64_t B, int H, int W, int C) {
  const Shape s = shape_of(B, H, W, C);
  return s.rc ? 0 : part_bytes(s, C) + (size_t)2 * C * sizeof(float);
}

size_t alignq_bnq_pool_code_bytes(int64_t B, int H, int W, int C) {
  const Shape s = shape_of(B, H, W, C);
  return s.rc ? 0 : (size_t)s.PP * C;
}

int alignq_bnq_pool_fwd(const float* z, int64_t B, int H, int W, int C, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, float momentum, float bn_eps, int k, float act_range,
                        int formula, float* ab, float* save, float* y, void* code, void* ws, void* stream) {
  const Shape s = shape_of(B, H, W, C);
  if (!z || !ab || !save || !y || !code || !ws || s.rc == ALIGNQ_EINVAL) return ALIGNQ_EINVAL;
  if (!((k >= 1 && k <= 16) || k == 32)) return ALIGNQ_EINVAL;
  if (formula != ALIGNQ_FORMULA_ADMM && formula != ALIGNQ_FORMULA_CDF) return ALIGNQ_EINVAL;
  if (misaligned(z) || misaligned(y) || misaligned(code) || misaligned(ws)) return ALIGNQ_EINVAL;
  if (s.rc) return s.rc;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const Geo ge = geo_for(C);                                           // C <= 1024: one quad per thread
  int64_t per;
  const int np = parts_for(s.P, C, &per);
  hipLaunchKernelGGL((any_sums_kernel<0, 1>), dim3(np), dim3(ge.NT), 0, st, z, (const float*)nullptr,
                     (const unsigned long long*)nullptr, (const float*)nullptr, (const float*)nullptr, s.P, C, (int64_t)(C >> 2), ge.L,
                     ge.slots, per, act_range, part);
  hipLaunchKernelGGL(any_finalize_fwd_kernel, dim3((C + kFinT - 1) / kFinT), dim3(kFinT), 0, st, (const double*)part, np, s.P, C, gamma,
                     beta, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, bn_eps, ab, save);
  const int64_t nvec = s.PP * (C >> 2);
  const int Wo = W >> 1;
  uint32_t* cd = reinterpret_cast<uint32_t*>(code);
  if (formula == ALIGNQ_FORMULA_ADMM)
    hipLaunchKernelGGL((pool_apply_fwd_kernel<0>), dim3(win_grid(nvec)), dim3(kTW), 0, st, z, (const float*)ab, nvec, C, Wo, k,
                       act_range, wt_for(nvec), y, cd);
  else
    hipLaunchKernelGGL((pool_apply_fwd_kernel<1>), dim3(win_grid(nvec)), dim3(kTW), 0, st, z, (const float*)ab, nvec, C, Wo, k,
                       act_range, wt_for(nvec), y, cd);
  return hipGetLastError() == hipSuccess ? 0 : ALIGNQ_EINVAL;
}

int alignq_bnq_pool_bwd(const float* g, const float* z, const void* code, const float* ab, const float* save, int64_t B, int H, int W,
                        int C, float act_range, float* dz, float* dgamma, float* dbeta, void* ws, void* stream) {
  const Shape s = shape_of(B, H, W, C);
  if (!g || !z || !code || !ab || !save || !dz || !ws || s.rc == ALIGNQ_EINVAL) return ALIGNQ_EINVAL;
  if (misaligned(g) || misaligned(z) || misaligned(dz) || misaligned(code) || misaligned(ws)) return ALIGNQ_EINVAL;
  if (s.rc) return s.rc;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  float* ktot = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + part_bytes(s, C));
  const uint32_t* cd = reinterpret_cast<const uint32_t*>(code);
  const Geo ge = geo_for(C);
  const int Wo = W >> 1;
  int64_t per;
  const int np = parts_for(s.PP, C, &per, kPoolSlotPixels);
  hipLaunchKernelGGL(pool_sums_bwd_kernel, dim3(np), dim3(ge.NT), 0, st, g, z, cd, ab, save, s.PP, C, Wo, ge.L, ge.slots, per, act_range,
                     part);
  hipLaunchKernelGGL(any_finalize_bwd_kernel, dim3((C + kFinT - 1) / kFinT), dim3(kFinT), 0, st, (const double*)part, np, s.P, C, ktot,
                     dgamma, dbeta);
  const int64_t nvec = s.PP * (C >> 2);
  hipLaunchKernelGGL(pool_apply_bwd_kernel, dim3(win_grid(nvec)), dim3(kTW), 0, st, g, z, cd, ab, save, (const float*)ktot, nvec, C, Wo,
                     act_range, wt_for(s.P * (C >> 2)), dz);
  return hipGetLastError() == hipSuccess ? 0 : ALIGNQ_EINVAL;
}

}  // extern "C"

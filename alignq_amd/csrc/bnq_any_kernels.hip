// bnq_any_kernels.hip - training-mode batch-norm folded into the PLAIN quantiser and a clamp (none / ReLU / ReLU6) at ANY channel
// count C % 4 == 0 in [4, 2048] (include/alignq_bnq_any.h): the sites of MobileNet-V2 (C = 16 ... 1280) and DenseNet-40 (C = 24, 36,
// ..., 456), which bnq_kernels.hip refuses because its thread mapping needs C = 4 * 2^j.  The arithmetic is bnq_kernels.hip's,
// operation for operation (tests/bnq_oracle.py restates it for both families; built with -ffp-contract=off):
//   forward : any_sums<0> (per-channel sum z, sum z^2 in double) -> any_finalize_fwd (mean, invstd, a = gamma * invstd,
//             b = beta - f32(mean) * a, running statistics) -> any_apply_fwd: y = clamp(quantise(fma(a, z, b))) + one mask bit per element;
//   backward: any_sums<1> (dx = gm * act_jac(fma(a, z, b)), gm = g where the mask bit is set; sum dx, sum dx * zhat) ->
//             any_finalize_bwd (k0, k1, dgamma, dbeta) -> any_apply_bwd: dz = a * ((dx - k0) - zhat * k1).
// Three launches each way, no atomics: every sum has a fixed order, so two launches give the same bits.
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

using namespace alignq;

namespace {

constexpr int kMaxC = 2048;
constexpr int kMaxNT = 512;            // largest reduction block
constexpr int kMaxParts = 256;         // partials per channel: one workgroup per CU
constexpr int kSlotPixels = 8;         // pixels per slot a workgroup should at least own (one round of loads in the forward)
constexpr int kTA = 256;               // threads of the elementwise kernels
constexpr int kUF = 4, kUB = 2;        // float4 per thread and tile: forward / backward apply
constexpr int kApplyBlocks = 2048;     // grid cap of the elementwise kernels; the rest by grid stride
constexpr int kFinT = 64, kFinU = 16;  // finalisation: threads per block, partials in flight per thread
// outputs of 1 MiB .. 64 MiB are stored write-through (store_forms.h), as the other elementwise kernels' are
constexpr int64_t kWtMinBytes = (int64_t)1 << 20, kWtMaxBytes = (int64_t)64 << 20;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4_stream(const float* p) {
  const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// The mask: per chunk of 64 consecutive float4 (vec index i, chunk i >> 6) four 64-bit words, one per float4 component,
// bit (i & 63) = "the gradient passes" - bnq_kernels.hip's layout, the forward's wave-wide compare results stored as they come.
__device__ __forceinline__ void mask_bits4(const unsigned long long* __restrict__ mask, int64_t i, bool (&m)[4]) {
  const ulonglong2* p2 = reinterpret_cast<const ulonglong2*>(mask + (i >> 6) * 4);
  const ulonglong2 a = p2[0], b = p2[1];
  const int sh = (int)(i & 63);
  m[0] = (a.x >> sh) & 1ull; m[1] = (a.y >> sh) & 1ull; m[2] = (b.x >> sh) & 1ull; m[3] = (b.y >> sh) & 1ull;
}
inline int64_t mask_words(int64_t nvec) { return ((nvec + 63) >> 6) * 4; }

// ---- launch geometry (host) -------------------------------------------------------------------------------------------------------
struct Geo {
  int Q, L, NT, slots;       // quads per thread, lanes per pixel, block size, pixels in flight per round and workgroup
};
inline Geo geo_for(int C) {
  const int C4 = C >> 2;
  Geo g;
  g.Q = C4 > 256 ? 2 : 1;
  g.L = g.Q == 1 ? C4 : (C4 + 1) / 2;
  // the first of these sizes with the largest filled share slots * L / NT (256 first: the size the other kernels run at)
  const int cand[7] = {256, 192, 128, 320, 384, 448, 512};
  g.NT = 0;
  g.slots = 0;
  for (int i = 0; i < 7; i++) {
    const int s = cand[i] / g.L;
    if (s >= 1 && (g.NT == 0 || (int64_t)s * g.NT > (int64_t)g.slots * cand[i])) { g.NT = cand[i]; g.slots = s; }
  }
  return g;
}
inline bool bad_c(int C) { return C < 4 || C > kMaxC || (C & 3) != 0; }
inline bool bad_p(int64_t P) { return P < 2 || P > ((int64_t)1 << 40); }
// the partial count: every workgroup owns at least kSlotPixels pixels per slot, at most kMaxParts workgroups, at most 4 MiB of
// partials; then the pixels are dealt out evenly so that no workgroup is empty.  per: pixels per workgroup.
inline int parts_for(int64_t P, int C, int64_t* per_out) {
  const Geo g = geo_for(C);
  int64_t n = P / ((int64_t)g.slots * kSlotPixels);
  const int64_t cap = ((int64_t)4 << 20) / ((int64_t)C * 16);
  if (n > cap) n = cap;
  if (n > kMaxParts) n = kMaxParts;
  if (n < 1) n = 1;
  const int64_t per = (P + n - 1) / n;
  if (per_out) *per_out = per;
  return (int)((P + per - 1) / per);
}
inline float* ktot_of(void* ws, int64_t P, int C) {
  return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + (size_t)parts_for(P, C, nullptr) * C * 2 * sizeof(double));
}
inline int apply_grid(int64_t nvec, int u) {
  const int64_t b = (nvec + (int64_t)kTA * u - 1) / ((int64_t)kTA * u);
  return (int)(b > kApplyBlocks ? kApplyBlocks : b);
}

// ---- per-channel sums over a workgroup's pixels -----------------------------------------------------------------------------------
// MODE 0: {sum z, sum z^2};  MODE 1: {sum dx, sum dx * zhat}.  part: [gridDim.x][C][2] doubles.  blockDim.x = the Geo's NT.
template <int Q>
__device__ __forceinline__ void slot_reduce(double* __restrict__ sm, const double (&s)[Q][4], int C, int L, int slots, int which,
                                            double* __restrict__ part) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Q; q++)
#pragma unroll
    for (int e = 0; e < 4; e++) sm[(tid * Q + q) * 4 + e] = s[q][e];
  __syncthreads();
  for (int c = tid; c < C; c += blockDim.x) {
    const int qd = c >> 2, e = c & 3;
    const int q = qd >= L ? 1 : 0, l = qd - q * L;           // the lane of a slot that owns the quad, and which of its quads
    double t = 0;
    for (int sl = 0; sl < slots; sl++) t += sm[((sl * L + l) * Q + q) * 4 + e];      // slot order
    part[((int64_t)blockIdx.x * C + c) * 2 + which] = t;
  }
  __syncthreads();
}

template <int MODE, int Q>
__global__ __launch_bounds__(kMaxNT) void any_sums_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                          const unsigned long long* __restrict__ mask, const float* __restrict__ ab,
                                                          const float* __restrict__ save, int64_t P, int C, int L, int slots,
                                                          int64_t per, float r, double* __restrict__ part) {
  constexpr int U = (MODE == 0 ? 8 : 4) / Q;                 // float4 per thread, array and quad in flight
  __shared__ double sm[kMaxNT * Q * 4];
  const int tid = threadIdx.x, C4 = C >> 2;
  const int slot = tid / L, l = tid - slot * L;
  const bool active = slot < slots;                          // the surplus lanes of the block idle
  // the thread's quads: l and, with Q == 2, l + L (an odd C / 4 leaves the last lane without a second quad: it reads its first
  // one again and nobody collects that sum)
  int qd[Q];
  qd[0] = l;
  if (Q == 2) qd[Q - 1] = l + L < C4 ? l + L : l;
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < P ? p0 + per : P;
  float4 a4[Q], b4[Q], m4[Q], i4[Q];
  if (MODE == 1 && active) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      a4[q] = ld4(ab + 4 * qd[q]); b4[q] = ld4(ab + C + 4 * qd[q]);
      m4[q] = ld4(save + 4 * qd[q]); i4[q] = ld4(save + C + 4 * qd[q]);
    }
  }
  double s0[Q][4], s1[Q][4];
#pragma unroll
  for (int q = 0; q < Q; q++)
#pragma unroll
    for (int e = 0; e < 4; e++) { s0[q][e] = 0; s1[q][e] = 0; }
  if (active) {
    for (int64_t base = p0 + slot; base < p1; base += (int64_t)slots * U) {
      float4 zv[U][Q], gv[U][Q];
      bool mk[U][Q][4];
#pragma unroll
      for (int u = 0; u < U; u++) {                          // clamped address, masked below
        const int64_t px = base + (int64_t)u * slots;
        const int64_t row = (px < p1 ? px : p1 - 1) * C4;
#pragma unroll
        for (int q = 0; q < Q; q++) {
          const int64_t i = row + qd[q];
          zv[u][q] = ld4(z + 4 * i);
          if (MODE == 1) {
            gv[u][q] = ld4(g + 4 * i);
            if (mask) mask_bits4(mask, i, mk[u][q]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (base + (int64_t)u * slots < p1) {
#pragma unroll
          for (int q = 0; q < Q; q++) {
            const float ze[4] = {zv[u][q].x, zv[u][q].y, zv[u][q].z, zv[u][q].w};
            if (MODE == 0) {
#pragma unroll
              for (int e = 0; e < 4; e++) { s0[q][e] += (double)ze[e]; s1[q][e] += (double)ze[e] * (double)ze[e]; }
            } else {
              const float ge[4] = {gv[u][q].x, gv[u][q].y, gv[u][q].z, gv[u][q].w};
              const float ae[4] = {a4[q].x, a4[q].y, a4[q].z, a4[q].w}, be[4] = {b4[q].x, b4[q].y, b4[q].z, b4[q].w};
              const float me[4] = {m4[q].x, m4[q].y, m4[q].z, m4[q].w}, ie[4] = {i4[q].x, i4[q].y, i4[q].z, i4[q].w};
#pragma unroll
              for (int e = 0; e < 4; e++) {
                const float x = __fmaf_rn(ae[e], ze[e], be[e]);
                const float gm = (mask && !mk[u][q][e]) ? 0.f : ge[e];
                const float dx = gm * act_jac(x, r);
                const float zh = (ze[e] - me[e]) * ie[e];
                s0[q][e] += (double)dx;
                s1[q][e] += (double)dx * (double)zh;
              }
            }
          }
        }
      }
    }
  }
  slot_reduce<Q>(sm, s0, C, L, slots, 0, part);
  slot_reduce<Q>(sm, s1, C, L, slots, 1, part);
}

// ---- finalisation: one thread per channel adds the partials in index order, kFinU loads in flight ---------------------------------
__device__ __forceinline__ void channel_totals(const double* __restrict__ part, int nparts, int C, int c, double& a, double& q) {
  a = 0; q = 0;
  for (int base = 0; base < nparts; base += kFinU) {
    double2 v[kFinU];
#pragma unroll
    for (int u = 0; u < kFinU; u++) {
      const int s = base + u < nparts ? base + u : nparts - 1;
      v[u] = *reinterpret_cast<const double2*>(part + ((int64_t)s * C + c) * 2);
    }
#pragma unroll
    for (int u = 0; u < kFinU; u++)
      if (base + u < nparts) { a += v[u].x; q += v[u].y; }
  }
}

__global__ __launch_bounds__(kFinT) void any_finalize_fwd_kernel(const double* __restrict__ part, int nparts, int64_t P, int C,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                 long long* __restrict__ nbt, float momentum, float eps,
                                                                 float* __restrict__ ab, float* __restrict__ save) {
  const int c = blockIdx.x * kFinT + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  double a, q;
  channel_totals(part, nparts, C, c, a, q);
  const double n = (double)P;
  const double mean = a / n;
  double var = q / n - mean * mean;
  if (var < 0) var = 0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float av = (gamma ? gamma[c] : 1.0f) * invstd;
  ab[c] = av;
  ab[C + c] = (beta ? beta[c] : 0.0f) - (float)mean * av;
  save[c] = (float)mean;
  save[C + c] = invstd;
  if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
  if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(var * n / (n - 1.0));
}

__global__ __launch_bounds__(kFinT) void any_finalize_bwd_kernel(const double* __restrict__ part, int nparts, int64_t P, int C,
                                                                 float* __restrict__ ktot, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
  const int c = blockIdx.x * kFinT + threadIdx.x;
  if (c >= C) return;
  double a, q;
  channel_totals(part, nparts, C, c, a, q);
  ktot[c] = (float)(a / (double)P);
  ktot[C + c] = (float)(q / (double)P);
  if (dbeta) dbeta[c] = (float)a;
  if (dgamma) dgamma[c] = (float)q;
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

inline int wt_for(int64_t nvec) {
  const int64_t bytes = nvec * 16;
  return bytes >= kWtMinBytes && bytes <= kWtMaxBytes;
}
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool bad_clamp(int clamp) { return clamp != ALIGNQ_CLAMP_NONE && clamp != ALIGNQ_CLAMP_RELU && clamp != ALIGNQ_CLAMP_RELU6; }

template <int MODE>
inline void launch_sums(const Geo& ge, int np, hipStream_t st, const float* z, const float* g, const unsigned long long* mask,
                        const float* ab, const float* save, int64_t P, int C, int64_t per, float r, double* part) {
  if (ge.Q == 2)
    hipLaunchKernelGGL((any_sums_kernel<MODE, 2>), dim3(np), dim3(ge.NT), 0, st, z, g, mask, ab, save, P, C, ge.L, ge.slots, per, r, part);
  else
    hipLaunchKernelGGL((any_sums_kernel<MODE, 1>), dim3(np), dim3(ge.NT), 0, st, z, g, mask, ab, save, P, C, ge.L, ge.slots, per, r, part);
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

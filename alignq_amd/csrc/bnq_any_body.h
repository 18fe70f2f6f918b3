// bnq_any_body.h - what the any-width batch-norm folds share: the reduction geometry, the per-channel sums over a workgroup's pixels
// and the two finalisations of bnq_any_kernels.hip (include/alignq_bnq_any.h, "Arithmetic" and "Order"), split out so that
// bnq_pool_kernels.hip (include/alignq_bnq_pool.h) runs the SAME statistics code on its un-pooled z: same kernels, same order, same
// bits.  Everything is in an unnamed namespace: each of the two files gets its own copy of the kernels it instantiates.
#pragma once
#include <hip/hip_runtime.h>

#include "alignq_math.h"

namespace {

using namespace alignq;

constexpr int kMaxNT = 512;            // largest reduction block
constexpr int kMaxParts = 256;         // partials per channel: one workgroup per CU
constexpr int kSlotPixels = 8;         // pixels per slot a workgroup should at least own (one round of loads in the forward)
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
// the partial count: every workgroup owns at least slot_pixels pixels per slot, at most kMaxParts workgroups, at most 4 MiB of
// partials; then the pixels are dealt out evenly so that no workgroup is empty.  per: pixels per workgroup.
inline int parts_for(int64_t P, int C, int64_t* per_out, int slot_pixels = kSlotPixels) {
  const Geo g = geo_for(C);
  int64_t n = P / ((int64_t)g.slots * slot_pixels);
  const int64_t cap = ((int64_t)4 << 20) / ((int64_t)C * 16);
  if (n > cap) n = cap;
  if (n > kMaxParts) n = kMaxParts;
  if (n < 1) n = 1;
  const int64_t per = (P + n - 1) / n;
  if (per_out) *per_out = per;
  return (int)((P + per - 1) / per);
}

// ---- per-channel sums over a workgroup's pixels -----------------------------------------------------------------------------------
// MODE 0: {sum z, sum z^2};  MODE 1: {sum dx, sum dx * zhat}.  part: [gridDim.x][C][2] doubles.  blockDim.x = the Geo's NT.
// ldq: float4 between two pixels of z (C / 4 for a dense tensor; dense_train_kernels.hip reads the first C channels of a wider
// buffer: same partition, same order, same bits).  g and the mask are dense.
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
                                                          const float* __restrict__ save, int64_t P, int C, int64_t ldq, int L,
                                                          int slots, int64_t per, float r, double* __restrict__ part) {
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
        const int64_t pc = px < p1 ? px : p1 - 1;
#pragma unroll
        for (int q = 0; q < Q; q++) {
          const int64_t i = pc * C4 + qd[q];
          zv[u][q] = ld4(z + 4 * (pc * ldq + qd[q]));
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

inline int wt_for(int64_t nvec) {
  const int64_t bytes = nvec * 16;
  return bytes >= kWtMinBytes && bytes <= kWtMaxBytes;
}
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

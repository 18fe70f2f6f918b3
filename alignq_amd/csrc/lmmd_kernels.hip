// lmmd_kernels.hip — DSAN's local MMD loss (cdf_alignment_admm/dsan_office/utils/mmd.py:9-41 with the class weights of
// utils/Weight.py:10-54) on the device, forward and backward, with no host round trip:
//   X = [source; target] (n = 2B rows of width D), L2_ij = sum_d (X_jd - X_id)^2 (fp32, from differences),
//   bw = fix_sigma or sum(L2) / (n^2 - n), divided by kernel_mul^(kernel_num // 2); bw_k = bw kernel_mul^k (detached),
//   K = sum_k exp(-L2 / bw_k), loss = sum(W_ss o K_SS + W_tt o K_TT - 2 W_st o K_ST); 0 (and no gradient) if K holds a NaN.
// Launches: lmmd_l2_kernel (16 x 16 row pairs x one slice of D per workgroup, partial sums per slice), lmmd_fwd_finish_kernel
// (one workgroup: slice sums in slice order, bandwidth, class weights in fp64 as NumPy forms them, loss, and the pair
// coefficients C_ij = -W~_ij sum_k exp(-L2_ij / bw_k) / bw_k for the backward), lmmd_bwd_kernel (one workgroup per row:
// dX_i = 2 g sum_j (C_ij + C_ji)(X_i - X_j)).  Every reduction has a fixed order and there are no atomics: bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/alignq.h"

namespace {

constexpr int kMaxB = 64;          // rows per domain
constexpr int kMaxN = 2 * kMaxB;   // rows of X
constexpr int kMaxC = 64;          // classes
constexpr int kMaxKernels = 8;     // kernel_num
constexpr int kTile = 16;          // row pairs per L2 workgroup: kTile x kTile
constexpr int kChunk = 256;        // features staged in LDS per round
constexpr int kMaxSplit = 16;      // slices of D (partial L2 matrices in the workspace)
constexpr int kFinThreads = 1024;
constexpr int kPerThread = kMaxN * kMaxN / kFinThreads;   // 16 matrix entries per finishing thread
constexpr int kBwdThreads = 256;

struct Geometry {
  int n, splits;
  int64_t per;   // features per slice (a multiple of kChunk)
};

Geometry geometry(int B, int64_t D) {
  Geometry g;
  g.n = 2 * B;
  int64_t chunks = (D + kChunk - 1) / kChunk;
  int64_t cps = (chunks + kMaxSplit - 1) / kMaxSplit;
  g.splits = (int)((chunks + cps - 1) / cps);
  g.per = cps * kChunk;
  return g;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: [splits][n][n] partial L2 | [n][n] C | int32 {live, m}
size_t off_c(const Geometry& g) { return align256((size_t)g.splits * g.n * g.n * sizeof(float)); }
size_t off_flags(const Geometry& g) { return off_c(g) + align256((size_t)g.n * g.n * sizeof(float)); }
size_t ws_bytes(const Geometry& g) { return off_flags(g) + 256; }

__device__ inline const float* row_ptr(const float* xs, const float* xt, int B, int64_t D, int r) {
  return r < B ? xs + (int64_t)r * D : xt + (int64_t)(r - B) * D;
}

// grid (tiles, tiles, splits), 256 threads: thread (ty, tx) owns the pair (i0 + ty, j0 + tx) and sums its slice of D
__global__ __launch_bounds__(256) void lmmd_l2_kernel(const float* __restrict__ xs, const float* __restrict__ xt, int B,
                                                      int64_t D, int64_t per, float* __restrict__ part) {
  __shared__ float xi[kTile][kChunk + 1];
  __shared__ float xj[kTile][kChunk + 1];
  const int n = 2 * B;
  const int t = threadIdx.x, tx = t & (kTile - 1), ty = t >> 4;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int64_t d_begin = (int64_t)blockIdx.z * per;
  const int64_t d_end = d_begin + per < D ? d_begin + per : D;
  float acc = 0.f;
  for (int64_t d0 = d_begin; d0 < d_end; d0 += kChunk) {
    const int len = d_end - d0 < kChunk ? (int)(d_end - d0) : kChunk;
    for (int e = t; e < kTile * kChunk; e += 256) {
      const int r = e / kChunk, c = e % kChunk;
      float a = 0.f, b = 0.f;
      if (c < len) {
        if (i0 + r < n) a = row_ptr(xs, xt, B, D, i0 + r)[d0 + c];
        if (j0 + r < n) b = row_ptr(xs, xt, B, D, j0 + r)[d0 + c];
      }
      xi[r][c] = a;
      xj[r][c] = b;
    }
    __syncthreads();
    for (int c = 0; c < len; ++c) {
      const float diff = xj[tx][c] - xi[ty][c];
      acc = fmaf(diff, diff, acc);
    }
    __syncthreads();
  }
  const int i = i0 + ty, j = j0 + tx;
  if (i < n && j < n) part[((size_t)blockIdx.z * n + i) * n + j] = acc;
}

__device__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = kFinThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// one workgroup: everything after the pairwise distances
__global__ __launch_bounds__(kFinThreads) void lmmd_fwd_finish_kernel(const float* __restrict__ part, int splits,
                                                                       const int64_t* __restrict__ s_label,
                                                                       const float* __restrict__ p, int B, int C,
                                                                       double kernel_mul, int kernel_num, double fix_sigma,
                                                                       float* __restrict__ loss, float* __restrict__ coef,
                                                                       int* __restrict__ flags) {
  __shared__ double red[kFinThreads];
  __shared__ float tnl[kMaxB][kMaxC];     // target columns p / column sum, for the common classes in ascending order
  __shared__ double sinv[kMaxC];          // 1 / (source count of the class)
  __shared__ int cnt[kMaxC], t_hit[kMaxC], qidx[kMaxC], cls[kMaxC];
  __shared__ float tsum[kMaxC];
  __shared__ int lab[kMaxB], targ[kMaxB];
  __shared__ int m_sh;
  __shared__ float bws[kMaxKernels];
  const int t = threadIdx.x, n = 2 * B, nn = n * n;

  // pairwise distances: the slices' partial sums in slice order; their total (fp64) for the bandwidth
  float l2[kPerThread];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int e = t + k * kFinThreads;
    float v = 0.f;
    if (e < nn) {
      for (int sp = 0; sp < splits; ++sp) v += part[(size_t)sp * nn + e];
      s += (double)v;
    }
    l2[k] = v;
  }
  const double l2_total = block_sum(s, red);

  // Weight.cal_weight: source one-hot / count, target probabilities / column sum, classes present on both sides
  if (t < B) {
    const int64_t l = s_label[t];
    lab[t] = (l >= 0 && l < C) ? (int)l : -1;      // a label outside [0, C) belongs to no class
    int best = 0;
    float bv = p[(int64_t)t * C];
    for (int c = 1; c < C; ++c) {
      const float v = p[(int64_t)t * C + c];
      if (v > bv) { bv = v; best = c; }            // first maximum (torch.max's index on ties)
    }
    targ[t] = best;
  }
  __syncthreads();
  if (t < C) {
    int k = 0, h = 0;
    float ts = 0.f;
    for (int i = 0; i < B; ++i) {
      k += lab[i] == t;
      h |= targ[i] == t;
      ts += p[(int64_t)i * C + t];
    }
    cnt[t] = k;
    t_hit[t] = h;
    tsum[t] = ts == 0.f ? 100.f : ts;
    sinv[t] = 1.0 / (double)(k == 0 ? 100 : k);
  }
  __syncthreads();
  if (t == 0) {
    int m = 0;
    for (int c = 0; c < C; ++c) {
      qidx[c] = -1;
      if (cnt[c] > 0 && t_hit[c]) { qidx[c] = m; cls[m++] = c; }
    }
    m_sh = m;
  }
  __syncthreads();
  const int m = m_sh;
  for (int e = t; e < B * m; e += kFinThreads) {
    const int i = e / m, q = e % m, c = cls[q];
    tnl[i][q] = p[(int64_t)i * C + c] / tsum[c];
  }
  if (t == 0) {
    // mmd.py:15-19.  Data bandwidth: an fp32 tensor divided by Python floats; fix_sigma: Python float arithmetic throughout
    const double div = pow(kernel_mul, (double)(kernel_num / 2));
    const float bwd = (float)l2_total / (float)((double)n * n - n) / (float)div;
    for (int k = 0; k < kernel_num; ++k)
      bws[k] = fix_sigma > 0.0 ? (float)(fix_sigma / div * pow(kernel_mul, (double)k)) : bwd * (float)pow(kernel_mul, (double)k);
  }
  __syncthreads();

  double lsum = 0.0;
  int nan = 0;
  const double md = (double)m;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int e = t + k * kFinThreads;
    if (e >= nn) continue;
    const int i = e / n, j = e % n;
    float K = 0.f, E = 0.f;
    for (int q = 0; q < kernel_num; ++q) {
      const float ex = expf(-l2[k] / bws[q]);
      K += ex;
      E += ex / bws[q];
    }
    nan |= isnan(K) ? 1 : 0;
    float w = 0.f;      // W~_ij
    if (m > 0) {
      if (i < B && j < B) {
        const int li = lab[i];
        if (li >= 0 && li == lab[j] && qidx[li] >= 0) w = (float)(sinv[li] * sinv[li] / md);
      } else if (i >= B && j >= B) {
        double acc = 0.0;
        for (int q = 0; q < m; ++q) acc += (double)(tnl[i - B][q] * tnl[j - B][q]);
        w = (float)(acc / md);
      } else if (i < B) {
        const int li = lab[i];
        if (li >= 0 && qidx[li] >= 0) w = -2.f * (float)(sinv[li] * (double)tnl[j - B][qidx[li]] / md);
      }
    }
    lsum += (double)w * (double)K;
    coef[e] = -(w * E);
  }
  const double total = block_sum(lsum, red);
  const double any_nan = block_sum((double)nan, red);
  if (t == 0) {
    const int live = any_nan == 0.0 && m > 0;
    loss[0] = live ? (float)total : 0.f;
    flags[0] = live;
    flags[1] = m;
  }
}

// one workgroup per row i of X: dX_i = 2 g sum_j (C_ij + C_ji)(X_i - X_j); exact zeros when the loss is not live
__global__ __launch_bounds__(kBwdThreads) void lmmd_bwd_kernel(const float* __restrict__ g, const float* __restrict__ xs,
                                                                const float* __restrict__ xt, const float* __restrict__ coef,
                                                                const int* __restrict__ flags, int B, int64_t D,
                                                                float* __restrict__ dxs, float* __restrict__ dxt) {
  __shared__ float S[kMaxN];
  const int n = 2 * B, i = blockIdx.x, t = threadIdx.x;
  float* out = i < B ? dxs + (int64_t)i * D : dxt + (int64_t)(i - B) * D;
  if (!flags[0]) {
    for (int64_t d = t; d < D; d += kBwdThreads) out[d] = 0.f;
    return;
  }
  for (int j = t; j < n; j += kBwdThreads) S[j] = coef[(size_t)i * n + j] + coef[(size_t)j * n + i];
  __syncthreads();
  const float scale = 2.f * g[0];
  const float* xi = row_ptr(xs, xt, B, D, i);
  for (int64_t d = t; d < D; d += kBwdThreads) {
    const float v = xi[d];
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc = fmaf(S[j], v - row_ptr(xs, xt, B, D, j)[d], acc);
    out[d] = scale * acc;
  }
}

int check_shape(int B, int64_t D, int C, int kernel_num) {
  if (B < 1 || D < 1 || C < 1 || kernel_num < 1) return ALIGNQ_EINVAL;
  if (B < 2 || B > kMaxB || C > kMaxC || kernel_num > kMaxKernels) return ALIGNQ_EUNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

size_t alignq_lmmd_ws_bytes(int B, int64_t D) {
  if (check_shape(B, D, 1, 1) != 0) return 0;
  return ws_bytes(geometry(B, D));
}

int alignq_lmmd_fwd(const float* x_src, const float* x_tgt, const int64_t* s_label, const float* p_tgt, int B, int64_t D,
                    int C, double kernel_mul, int kernel_num, double fix_sigma, float* loss, void* ws, void* stream) {
  if (!x_src || !x_tgt || !s_label || !p_tgt || !loss || !ws) return ALIGNQ_EINVAL;
  if (!(kernel_mul > 0.0) || isinf(kernel_mul) || isnan(fix_sigma) || isinf(fix_sigma)) return ALIGNQ_EINVAL;
  int rc = check_shape(B, D, C, kernel_num);
  if (rc) return rc;
  const Geometry g = geometry(B, D);
  char* w = (char*)ws;
  float* part = (float*)w;
  float* coef = (float*)(w + off_c(g));
  int* flags = (int*)(w + off_flags(g));
  const int tiles = (g.n + kTile - 1) / kTile;
  hipLaunchKernelGGL(lmmd_l2_kernel, dim3(tiles, tiles, g.splits), 256, 0, (hipStream_t)stream, x_src, x_tgt, B, D, g.per,
                     part);
  hipLaunchKernelGGL(lmmd_fwd_finish_kernel, 1, kFinThreads, 0, (hipStream_t)stream, part, g.splits, s_label, p_tgt, B, C,
                     kernel_mul, kernel_num, fix_sigma, loss, coef, flags);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int alignq_lmmd_bwd(const float* g, const float* x_src, const float* x_tgt, const void* ws, int B, int64_t D, float* dx_src,
                    float* dx_tgt, void* stream) {
  if (!g || !x_src || !x_tgt || !ws || !dx_src || !dx_tgt) return ALIGNQ_EINVAL;
  int rc = check_shape(B, D, 1, 1);
  if (rc) return rc;
  const Geometry geo = geometry(B, D);
  const char* w = (const char*)ws;
  hipLaunchKernelGGL(lmmd_bwd_kernel, geo.n, kBwdThreads, 0, (hipStream_t)stream, g, x_src, x_tgt,
                     (const float*)(w + off_c(geo)), (const int*)(w + off_flags(geo)), B, D, dx_src, dx_tgt);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

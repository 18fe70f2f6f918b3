// eval_kernels.hip — the evaluation pass (the reference's test(): cdf_alignment_admm/resnet-20-cifar-10/main.py:405-441,
// dann_office/main.py:502-545, utils/common.py:78-92) for gfx950.
//
//   alignq_bnq_eval_fwd : y = [relu]([act_q](a_c z + b_c) [+ residual]) with the batch-norm's RUNNING statistics; one elementwise
//                         pass, the structure of act_quant_fwd_kernel (quant_kernels.hip: tiles of kU x 256 float4, 16-byte
//                         non-temporal loads, non-temporal stores from 2^25 elements) plus a [2][C] coefficient table in LDS that
//                         every workgroup forms itself from the four [C] vectors - no statistics pass, no finalisation launch, no
//                         mask, nothing saved, nothing written but y / the level indices.
//   alignq_eval_metrics : cross-entropy sum, top-1 / top-5 counts and the row count of one batch added into a 32-byte accumulator
//                         by ONE workgroup in row order (no atomics: two runs give the same bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "alignq_math.h"

using namespace alignq;

namespace {

constexpr int kThreads = 256;
constexpr int kU = 4;                      // float4 per thread and tile (quant_kernels.hip)
constexpr int kTileBlocks = 256 * 64;      // grid cap: 64 blocks per CU, the rest by grid stride
constexpr int kMaxC = 2048;

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 ld4_stream(const float4* p) {
  const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4_out(float4* p, const float4 v, const int nts) {
  if (nts) {
    f32x4_t t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t*>(p));
  } else {
    *p = v;
  }
}

template <typename T> struct Vec4;
template <> struct Vec4<int8_t> { typedef char4 type; };
template <> struct Vec4<int16_t> { typedef short4 type; };

// the oracle's `v > 0 ? v : 0` (oq_bn_site_fwd): -0.0 and NaN both store +0.0
__device__ __forceinline__ float relu1(float v) { return v > 0.0f ? v : 0.0f; }

// FORMULA: 0 = ALIGNQ_FORMULA_ADMM, 1 = ALIGNQ_FORMULA_CDF, 2 = no quantiser (k == 32: the batch-norm alone).
// T: the packed index type (void: none).  Vec index i holds elements 4i .. 4i+3 = channels 4 (i mod C/4) .. + 3 of one pixel.
template <int FORMULA, typename T>
__global__ __launch_bounds__(kThreads) void bnq_eval_fwd_kernel(const float* __restrict__ z, int64_t nvec, int C,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ var,
                                                                float bn_eps, int k, float r, int relu,
                                                                const float* __restrict__ res, float* __restrict__ y,
                                                                T* __restrict__ bins, int nts) {
  constexpr bool kPack = !__is_same(T, void);
  __shared__ __attribute__((aligned(16))) float tab_lds[ALIGNQ_NERF_LDS_FLOATS];
  extern __shared__ __attribute__((aligned(16))) float ab_s[];      // [2][C], sized by the launch: 128 B at C = 16, 16 KB at C = 2048
  if (FORMULA != 2) nerf_tab_load(tab_lds);
  // a = gamma / sqrt(var + eps), b = beta - a * mean: individually rounded fp32 operations (include/alignq.h)
  for (int c = threadIdx.x; c < C; c += kThreads) {
    // correctly rounded fp32 sqrt and quotient, formed in double and rounded once more: with 53 >= 2 * 24 + 2 significand bits the
    // second rounding cannot change the result (the fp32 sqrt intrinsic maps to the approximate hardware instruction)
    const float s = (float)sqrt((double)__fadd_rn(var[c], bn_eps));
    const float a = (float)((double)(gamma ? gamma[c] : 1.0f) / (double)s);
    ab_s[c] = a;
    ab_s[C + c] = __fsub_rn(beta ? beta[c] : 0.0f, __fmul_rn(a, mean[c]));
  }
  __syncthreads();
  const NerfTab tab = nerf_tab(tab_lds);
  const Levels nlev = make_levels(k, fabsf(r) <= 8.0f);
  const int qmask = (C >> 2) - 1;                    // C is a power of two
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const float4* z4 = reinterpret_cast<const float4*>(z);
  const float4* r4 = reinterpret_cast<const float4*>(res);
  float4* y4 = reinterpret_cast<float4*>(y);
  ALIGNQ_BOUNDED_SWITCH(nlev,
  for (int64_t i0 = (int64_t)blockIdx.x * (kThreads * kU) + threadIdx.x; i0 < nvec; i0 += kU * stride) {
    float4 v[kU], rv[kU];
_Pragma("unroll")
    for (int u = 0; u < kU; u++) {
      const int64_t i = i0 + u * kThreads;
      v[u] = ld4_stream(z4 + (i < nvec ? i : i0));
      if (res) rv[u] = ld4_stream(r4 + (i < nvec ? i : i0));
    }
_Pragma("unroll")
    for (int u = 0; u < kU; u++) {
      const int64_t i = i0 + u * kThreads;
      const int cq = (int)(i & qmask);               // (beyond nvec: still a valid table row; nothing is stored)
      const float4 a4 = *reinterpret_cast<const float4*>(ab_s + 4 * cq);
      const float4 b4 = *reinterpret_cast<const float4*>(ab_s + C + 4 * cq);
      float4 o;
      o.x = __fadd_rn(__fmul_rn(a4.x, v[u].x), b4.x);
      o.y = __fadd_rn(__fmul_rn(a4.y, v[u].y), b4.y);
      o.z = __fadd_rn(__fmul_rn(a4.z, v[u].z), b4.z);
      o.w = __fadd_rn(__fmul_rn(a4.w, v[u].w), b4.w);
      if (FORMULA != 2) {
        constexpr int FQ = FORMULA == 2 ? 0 : FORMULA;
        float t, bx, by, bz, bw;
        o.x = act_quant1<FQ, kBounded>(o.x, k, nlev, r, &t, &bx, tab);
        o.y = act_quant1<FQ, kBounded>(o.y, k, nlev, r, &t, &by, tab);
        o.z = act_quant1<FQ, kBounded>(o.z, k, nlev, r, &t, &bz, tab);
        o.w = act_quant1<FQ, kBounded>(o.w, k, nlev, r, &t, &bw, tab);
        if constexpr (kPack) {           // (host: ADMM formula, no residual, index range within T)
          if (i < nvec) {
            typedef typename Vec4<T>::type V4;
            if (relu) { bx = relu1(bx); by = relu1(by); bz = relu1(bz); bw = relu1(bw); }
            V4 bi;
            bi.x = (T)(int)bx; bi.y = (T)(int)by; bi.z = (T)(int)bz; bi.w = (T)(int)bw;
            reinterpret_cast<V4*>(bins)[i] = bi;
          }
        }
      }
      if (res) {
        o.x = __fadd_rn(o.x, rv[u].x); o.y = __fadd_rn(o.y, rv[u].y);
        o.z = __fadd_rn(o.z, rv[u].z); o.w = __fadd_rn(o.w, rv[u].w);
      }
      if (relu) { o.x = relu1(o.x); o.y = relu1(o.y); o.z = relu1(o.z); o.w = relu1(o.w); }
      if (y && i < nvec) st4_out(y4 + i, o, nts);
    }
  })
}

// ------------------------------------------------------------------ metrics -------------------
// One workgroup of four waves; wave w takes rows r0 + w of each group of four rows, its lanes stride over the K classes.  The
// rows' results meet in LDS and thread 0 adds them in ROW order into its running totals: a fixed order, no atomics.
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum_dd(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void eval_metrics_kernel(const float* __restrict__ logits,
                                                                const int64_t* __restrict__ target, int B, int K,
                                                                void* __restrict__ acc) {
  __shared__ double ce_s[4];
  __shared__ int ok1_s[4], ok5_s[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double ce_tot = 0.0;
  long long n1 = 0, n5 = 0;
  for (int r0 = 0; r0 < B; r0 += 4) {
    const int row = r0 + w;
    if (row < B) {
      const float* l = logits + (int64_t)row * K;
      const int64_t t = target[row];
      const bool valid = t >= 0 && t < (int64_t)K;
      const float tl = valid ? l[t] : 0.0f;
      float m = -INFINITY;
      int gt = 0, nan = 0;
      for (int j = lane; j < K; j += 64) {
        const float v = l[j];
        m = fmaxf(m, v);                 // (ignores NaN; the row is marked instead)
        nan |= (v != v);
        gt += (v > tl);
      }
      m = wave_max(m);
      gt = wave_sum_i(gt);
      nan = wave_sum_i(nan);
      double s = 0.0;
      for (int j = lane; j < K; j += 64) s += (double)expf(l[j] - m);
      s = wave_sum_dd(s);
      if (lane == 0) {
        const bool good = valid && nan == 0;
        ce_s[w] = valid ? ((double)m + log(s)) - (double)tl : 0.0;
        ok1_s[w] = good && gt < 1;
        ok5_s[w] = good && gt < 5;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int nr = B - r0 < 4 ? B - r0 : 4;
      for (int q = 0; q < nr; q++) { ce_tot += ce_s[q]; n1 += ok1_s[q]; n5 += ok5_s[q]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* a_ce = reinterpret_cast<double*>(acc);
    long long* a_n = reinterpret_cast<long long*>(acc);
    a_ce[0] += ce_tot;
    a_n[1] += n1;
    a_n[2] += n5;
    a_n[3] += (long long)B;
  }
}

inline int grid_tiles(int64_t n_vec) {
  int64_t b = (n_vec + (int64_t)kThreads * kU - 1) / ((int64_t)kThreads * kU);
  if (b < 1) b = 1;
  return (int)(b > kTileBlocks ? kTileBlocks : b);
}

}  // namespace

extern "C" {

int alignq_bnq_eval_fwd(const float* z, int64_t P, int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float bn_eps, int k, float act_range, int formula, int relu,
                        const float* residual, float* y, void* bins_out, int pack, void* stream) {
  if (!z || !running_mean || !running_var || P < 1 || (!y && !bins_out)) return ALIGNQ_EINVAL;
  if (!((k >= 1 && k <= 16) || k == 32)) return ALIGNQ_EINVAL;
  if (formula != ALIGNQ_FORMULA_ADMM && formula != ALIGNQ_FORMULA_CDF) return ALIGNQ_EINVAL;
  if (!(pack == 0 || pack == 1 || pack == 2) || (pack != 0) != (bins_out != nullptr)) return ALIGNQ_EINVAL;
  if (pack) {      // the conditions of the training kernels' packed form (N2): ADMM / Office formula, no residual, index within the type
    const int bb = alignq_bin_bytes(k, act_range, ALIGNQ_FORMULA_ADMM);
    if (formula != ALIGNQ_FORMULA_ADMM || residual || bb == 0 || bb > pack) return ALIGNQ_EINVAL;
  }
  if ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual) |
       reinterpret_cast<uintptr_t>(bins_out)) & 15)
    return ALIGNQ_EINVAL;
  if (C < 4 || C > kMaxC || (C & (C - 1))) return ALIGNQ_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nvec = P * (C >> 2);
  const int grid = grid_tiles(nvec);
  const int nts = (nvec << 2) >= ((int64_t)1 << 25) ? 1 : 0;
#define EVAL_LAUNCH(F, T)                                                                                                      \
  hipLaunchKernelGGL((bnq_eval_fwd_kernel<F, T>), grid, kThreads, (size_t)2 * C * sizeof(float), st, z, nvec, C, gamma, beta, running_mean, running_var,   \
                     bn_eps, k, act_range, relu, residual, y, (T*)bins_out, nts)
  if (k == 32) EVAL_LAUNCH(2, void);
  else if (formula == ALIGNQ_FORMULA_CDF) EVAL_LAUNCH(1, void);
  else if (pack == 1) EVAL_LAUNCH(0, int8_t);
  else if (pack == 2) EVAL_LAUNCH(0, int16_t);
  else EVAL_LAUNCH(0, void);
#undef EVAL_LAUNCH
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int alignq_eval_metrics(const float* logits, const int64_t* target, int B, int K, void* acc, void* stream) {
  if (!logits || !target || !acc || B < 1 || K < 1) return ALIGNQ_EINVAL;
  if (reinterpret_cast<uintptr_t>(acc) & 7) return ALIGNQ_EINVAL;
  if (K > 1024) return ALIGNQ_EUNSUPPORTED;
  hipLaunchKernelGGL(eval_metrics_kernel, 1, kThreads, 0, (hipStream_t)stream, logits, target, B, K, acc);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

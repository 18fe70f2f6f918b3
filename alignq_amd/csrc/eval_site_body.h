// eval_site_body.h - the device-side statement of one folded evaluation site (include/alignq_mobile.h: eval-mode batch-norm ->
// quantiser -> clamp), shared by mobile_eval_kernels.hip (the elementwise and depthwise forms) and dense_eval_kernels.hip (the site
// applied while a 3x3 convolution stages its input).  One copy, so every form gives the same bits.
// Translation units including this header are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_mobile.h"
#include "alignq_math.h"

namespace alignq_evalsite {

using namespace alignq;

struct SiteDev {                           // alignq_eval_site / alignq_dense_site as the kernels take it (by value)
  const float *z, *gamma, *beta, *mean, *var;
  float eps;
  int k, clamp;
};

// the oracle's `v > 0 ? v : 0` (oq_bn_site_fwd): -0.0 and NaN both store +0.0; relu6 caps it at 6
__device__ __forceinline__ float clamp1(float v, int clamp) {
  if (clamp == ALIGNQ_CLAMP_NONE) return v;
  const float hi = (clamp == ALIGNQ_CLAMP_RELU6 && !(v < 6.0f)) ? 6.0f : v;
  return v > 0.0f ? hi : 0.0f;
}
__device__ __forceinline__ float4 clamp4(float4 v, int clamp) {
  return make_float4(clamp1(v.x, clamp), clamp1(v.y, clamp), clamp1(v.z, clamp), clamp1(v.w, clamp));
}

// a = gamma / sqrt(var + eps), b = beta - a * mean into ab[0..C) and ab[C..2C): alignq_bnq_eval_fwd's statement (correctly rounded
// fp32 sqrt and quotient, formed in double and rounded once more: with 53 >= 2 * 24 + 2 significand bits the second rounding cannot
// change the result).  Every thread of the NT-thread workgroup calls it; the caller places a barrier before the first read.
template <int NT>
__device__ __forceinline__ void ab_table(float* ab, int C, const SiteDev& s) {
  for (int c = threadIdx.x; c < C; c += NT) {
    const float sd = (float)sqrt((double)__fadd_rn(s.var[c], s.eps));
    const float a = (float)((double)(s.gamma ? s.gamma[c] : 1.0f) / (double)sd);
    ab[c] = a;
    ab[C + c] = __fsub_rn(s.beta ? s.beta[c] : 0.0f, __fmul_rn(a, s.mean[c]));
  }
}

// q(a z + b) of one channel quad.  FORMULA: 0 = ALIGNQ_FORMULA_ADMM, 1 = ALIGNQ_FORMULA_CDF, 2 = no quantiser (k == 32).
template <int FORMULA, bool BOUNDED>
__device__ __forceinline__ float4 site_q(const float4 v, const float* ab, int C, int cq, int k, const Levels& nlev, float r,
                                         const NerfTab tab) {
  const float4 a4 = *reinterpret_cast<const float4*>(ab + 4 * cq);
  const float4 b4 = *reinterpret_cast<const float4*>(ab + C + 4 * cq);
  float4 o;
  o.x = __fadd_rn(__fmul_rn(a4.x, v.x), b4.x);
  o.y = __fadd_rn(__fmul_rn(a4.y, v.y), b4.y);
  o.z = __fadd_rn(__fmul_rn(a4.z, v.z), b4.z);
  o.w = __fadd_rn(__fmul_rn(a4.w, v.w), b4.w);
  if constexpr (FORMULA != 2) {
    float t, bin;
    o.x = act_quant1<FORMULA, BOUNDED>(o.x, k, nlev, r, &t, &bin, tab);
    o.y = act_quant1<FORMULA, BOUNDED>(o.y, k, nlev, r, &t, &bin, tab);
    o.z = act_quant1<FORMULA, BOUNDED>(o.z, k, nlev, r, &t, &bin, tab);
    o.w = act_quant1<FORMULA, BOUNDED>(o.w, k, nlev, r, &t, &bin, tab);
  }
  return o;
}

}  // namespace alignq_evalsite

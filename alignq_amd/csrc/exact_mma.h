// exact_mma.h - the device primitives of the exact-product convolution family (qgemm_kernels.hip, pointwise_kernels.hip,
// k3conv_kernels.hip, dense_eval_kernels.hip): the exact bf16 splits of an fp32 operand, the 16x16x32 MFMA, the transposing LDS
// read, the XCD remap of workgroup ids and the output store.  The family's results are pinned to the bit by its exact tests; they
// rest on every member running THIS text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "store_forms.h"

namespace alignq_xmma {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

// 4 rows x 16 columns block at `p` (this lane's row (lane & 15) >> 2, columns 4 * (lane & 3)), transposed by the LDS hardware:
// the lane receives column (lane & 15) of the 4 rows.  EXEC all ones at every call.
__device__ __forceinline__ s16x4 tr_read(const u16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
__device__ __forceinline__ s16x8 join8(s16x4 a, s16x4 b) { return (s16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }

template <bool F16 = false>
__device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// exact three-way split of four floats: v == hi + mid + lo.  Two values per v_cvt_pk_bf16_f32 and per v_pk_add_f32 (round 5: the
// element-wise form compiled to 26 vector instructions per four values, this one to 20 - the same bits; these kernels are
// bound by vector issue, a wave64 instruction holding its SIMD for four cycles)
__device__ __forceinline__ unsigned cvt_bf16x2(f32x2 v) { return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2)); }
__device__ __forceinline__ f32x2 bf16x2_as_f32(unsigned b) {
  return (f32x2){__builtin_bit_cast(float, b << 16), __builtin_bit_cast(float, b & 0xffff0000u)};
}
__device__ __forceinline__ void split3(const f32x4 v, s16x4& h, s16x4& m, s16x4& l) {
  const f32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
  const unsigned ha = cvt_bf16x2(a), hb = cvt_bf16x2(b);
  const f32x2 ra = a - bf16x2_as_f32(ha), rb = b - bf16x2_as_f32(hb);
  const unsigned ma = cvt_bf16x2(ra), mb = cvt_bf16x2(rb);
  const f32x2 sa = ra - bf16x2_as_f32(ma), sb = rb - bf16x2_as_f32(mb);
  h = __builtin_bit_cast(s16x4, (u32x2){ha, hb});
  m = __builtin_bit_cast(s16x4, (u32x2){ma, mb});
  l = __builtin_bit_cast(s16x4, (u32x2){cvt_bf16x2(sa), cvt_bf16x2(sb)});
}
// integer-valued floats |v| < 2^16 in two exact bf16 terms
__device__ __forceinline__ void split2(const f32x4 v, s16x4& h, s16x4& l) {
  const f32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
  const unsigned ha = cvt_bf16x2(a), hb = cvt_bf16x2(b);
  h = __builtin_bit_cast(s16x4, (u32x2){ha, hb});
  l = __builtin_bit_cast(s16x4, (u32x2){cvt_bf16x2(a - bf16x2_as_f32(ha)), cvt_bf16x2(b - bf16x2_as_f32(hb))});
}

// Workgroups that share operand rows on one XCD (blockIdx round-robins over the 8 XCDs, each with its own L2): bijective for any n.
__device__ __forceinline__ int xcd_remap(int id, int n) {
  const int q = n >> 3, r = n & 7, x = id & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
}

// one lane's float4 of the output; wt: written through to memory (store_forms.h), the launcher's choice by the output's size
__device__ __forceinline__ void st_out(float* p, const f32x4 v, const int wt) {
  if (wt) alignq_store::st16<alignq_store::kConvOut>(p, make_float4(v[0], v[1], v[2], v[3]));
  else *reinterpret_cast<f32x4*>(p) = v;
}

}  // namespace alignq_xmma

// store_forms.h - WRITE-THROUGH stores (the sc1 cache bit) for the large outputs a kernel leaves to the NEXT launch.
// A plain store leaves its line dirty in the writing XCD's L2 until the end-of-kernel release writes it back, and the dependent
// launch waits for that; an sc1 store goes through to memory when it is issued and drops the line, so the release finds nothing
// to write back (measured: tools/src/store_probe.hip, NOTES.md "Write-through output stores" - the epilogue stores carry most of
// the gain, the first-phase ones pay on top of them; a non-temporal store behaves like a plain one).  Same values, same addresses:
// only the cache policy differs.  Only for outputs that no workgroup of the SAME launch reads (they are no hand-off: no flag, no
// drain; the kernel boundary publishes them as before).
//
// -DALIGNQ_PLAIN_STORES restores plain stores everywhere (A/B builds: tools/build_variant.sh plain "-DALIGNQ_PLAIN_STORES").
// ALIGNQ_WT_FAMILIES selects the converted families one by one (A/B only; the default is the set that measured, NOTES.md):
//   1  site forward: first-phase x_q / y         2  site forward: the partial-Gram slab (epilogue; 16 B and, packed part, 4 B)
//   4  site backward: first-phase dres           8  site backward: dx copy-out
//  16  convolutions: the float4 output store (forward z, data gradient dx, transitions, stem)
//  32  convolutions: the filter-gradient slabs (4 B per lane, 64-byte runs)
#pragma once
#include <hip/hip_runtime.h>

#ifdef ALIGNQ_PLAIN_STORES
#undef ALIGNQ_WT_FAMILIES
#define ALIGNQ_WT_FAMILIES 0
#endif
#ifndef ALIGNQ_WT_FAMILIES
#define ALIGNQ_WT_FAMILIES 63
#endif

namespace alignq_store {

constexpr int kSiteFwdEarly = 1, kSiteFwdSlab = 2, kSiteBwdDres = 4, kSiteBwdDx = 8, kConvOut = 16, kConvWgradSlab = 32;
constexpr bool on(int family) { return (ALIGNQ_WT_FAMILIES & family) != 0; }

// base (wave-uniform: a kernel argument or a per-workgroup choice among them) + 32-bit BYTE offset, the addressing of the site
// kernels (their launchers guarantee B * F * 4 < 2^32).  buffer_store_dwordx4 ... offen sc1; the compiler counts and schedules it.
template <int FAMILY>
__device__ __forceinline__ void st16(float* base, unsigned byte_off, float4 v) {
  if constexpr (on(FAMILY)) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0xffffffff, 0x00020000);
    const u32x4 d = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(d, rsrc, (int)byte_off, 0, 16);      // aux 16 = sc1
  } else {
    *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + byte_off) = v;
  }
}

// the 4-byte form of the same store (tools/src/store_probe.hip: per byte it costs about what the 16-byte form does when a wave's
// lanes cover whole lines)
template <int FAMILY>
__device__ __forceinline__ void st4(float* base, unsigned byte_off, float v) {
  if constexpr (on(FAMILY)) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0xffffffff, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc, (int)byte_off, 0, 16);
  } else {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off) = v;
  }
}

// any 16-byte aligned address (64-bit per lane), the addressing of the convolution epilogues.  The statement only reads its
// operands: the compiler does not count the store (its waits for loads only get more conservative) and must not reuse the data
// registers before the store has read them (the trailing s_nop 1).
template <int FAMILY>
__device__ __forceinline__ void st16(float* p, float4 v) {
  if constexpr (on(FAMILY)) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    const f32x4v d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(d));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}

// one float at any address; PLAIN_NT: what the plain build stores it with
template <int FAMILY, bool PLAIN_NT>
__device__ __forceinline__ void st4(float* p, float v) {
  if constexpr (on(FAMILY)) {
    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v));
  } else if constexpr (PLAIN_NT) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

}  // namespace alignq_store

// pack_kernels.hip — k-bit weight checkpoints (gfx950): the quantiser's W_q of every filter of a model as bit-packed level codes
// (alignq_weight_pack_multi), and from those codes everything an evaluation reads (alignq_weight_unpack_multi): fp32 W_q, the GEMM
// convolutions' bf16 / f16 bins and the body convolutions' bf16 filter images, one launch per 64 tensors ("Packed weights").
//
// Code of one element (k = w_bit, n = 2^k - 1, b = rintf(W_q * n), the `*bin` of round_bins):
//   ADMM tree (levels -n..n):     code = b + n        in k + 1 bits
//   CDF tree  (W_q = 2 i/n - 1):  code = i = (b+n)/2  in k bits
// Stream: groups of 32 elements in storage order; group g is the 32*bits-bit little-endian integer words[g*bits .. g*bits + bits),
// element e of the group its bits [e*bits, (e+1)*bits); the last group is zero-padded.  No code straddles a group.
// Dequantisation is the quantiser's own last step (div_levels, or the divider where round_bins takes it; then *2 - 1 for the CDF
// tree) on an integer-to-float conversion of the code, which cannot be -0: W_q = -0 of the ADMM tree comes back as +0.
// As in multi_tensor_kernels.hip the per-tensor tables travel by value in the kernel arguments (every launch is graph-capturable).
#include <hip/hip_runtime.h>

#include "../../include/alignq.h"
#include "alignq_math.h"
#include "filter_image.h"

using namespace alignq;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 64;        // tensors per launch: unpack 64 * (5 pointers + size + geometry word) = 3328 B of arguments
constexpr int kMaxBlk = 256;      // workgroups per tensor
constexpr int kMaxBits = 17;      // k = 16 of the ADMM tree
constexpr int kGroupsPerBlk = kThreads / 32;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// W_q of a code: one IEEE fp32 division (code - n) / n, or (code / n) * 2 - 1
template <int FORMULA>
__device__ __forceinline__ float weight_dequant(unsigned code, const Levels& L, int ni) {
  const float b = FORMULA == 0 ? (float)((int)code - ni) : (float)code;
  const float d = L.yn != 0.0f ? div_levels(b, L.n, L.yn) : __fdiv_rn(b, L.n);
  return FORMULA == 0 ? d : __fsub_rn(__fmul_rn(d, 2.0f), 1.0f);
}

// the code of a quantiser output; *ok = false (and code 0) when no code dequantises to q: NaN, infinities, values off the grid
template <int FORMULA>
__device__ __forceinline__ unsigned weight_code(float q, const Levels& L, int ni, bool* ok) {
  const float b = rintf(__fmul_rn(q, L.n));
  *ok = false;
  if (!(__builtin_fabsf(b) <= L.n)) return 0u;
  const int s = (int)b + ni;                                // 0 .. 2n
  const unsigned code = FORMULA == 0 ? (unsigned)s : (unsigned)(s >> 1);
  *ok = weight_dequant<FORMULA>(code, L, ni) == q;
  return *ok ? code : 0u;
}

struct PChunk {
  const float* q[kChunk];
  unsigned* codes[kChunk];
  long n[kChunk];
};

// A workgroup packs 8 groups (256 consecutive elements, one per thread) per pass: every thread ORs its shifted code into the one or
// two LDS words it touches, then the 8 * bits words are stored side by side.
template <int FORMULA>
__global__ __launch_bounds__(kThreads) void weight_pack_kernel(PChunk c, int k, int bits, int32_t* __restrict__ bad) {
  __shared__ unsigned words[kGroupsPerBlk * kMaxBits];
  const int t = blockIdx.y;
  const float* __restrict__ q = c.q[t];
  unsigned* __restrict__ out = c.codes[t];
  const long n = c.n[t], ngroups = (n + 31) >> 5;
  const Levels L = make_levels(k, true);
  const int ni = (1 << k) - 1, nw = kGroupsPerBlk * bits;
  const int gl = threadIdx.x >> 5, bp = (int)(threadIdx.x & 31) * bits;
  for (long g0 = (long)blockIdx.x * kGroupsPerBlk; g0 < ngroups; g0 += (long)gridDim.x * kGroupsPerBlk) {   // (block-uniform trips)
    if ((int)threadIdx.x < nw) words[threadIdx.x] = 0u;
    __syncthreads();
    const long i = g0 * 32 + threadIdx.x;
    if (i < n) {
      bool ok;
      const unsigned code = weight_code<FORMULA>(q[i], L, ni, &ok);
      if (!ok) atomicAdd(bad, 1);
      const unsigned long long v = (unsigned long long)code << (bp & 31);      // code < 2^bits: stays inside the group's words
      atomicOr(&words[gl * bits + (bp >> 5)], (unsigned)v);
      if (v >> 32) atomicOr(&words[gl * bits + (bp >> 5) + 1], (unsigned)(v >> 32));
    }
    __syncthreads();
    if ((int)threadIdx.x < nw && g0 + (int)threadIdx.x / bits < ngroups) out[g0 * bits + threadIdx.x] = words[threadIdx.x];
    __syncthreads();
  }
}

struct UChunk {
  const unsigned* codes[kChunk];
  float* q[kChunk];
  unsigned short* bf[kChunk];
  unsigned short* hf[kChunk];
  unsigned short* img[kChunk];
  long n[kChunk];
  unsigned geo[kChunk];
};

// A thread owns 4 consecutive elements: their 4 * bits <= 68 bits start at a multiple of 4 inside the group, so they lie in at most
// three of its words; one 16-byte store of W_q, one 8-byte store per bin form, the image scatter of filter_image.h.
template <int FORMULA>
__global__ __launch_bounds__(kThreads) void weight_unpack_kernel(UChunk c, int k, int bits) {
  const int t = blockIdx.y;
  const unsigned* __restrict__ codes = c.codes[t];
  float* __restrict__ q = c.q[t];
  unsigned short* __restrict__ bf = c.bf[t];
  unsigned short* __restrict__ hf = c.hf[t];
  unsigned short* __restrict__ img = c.img[t];
  const unsigned geo = c.geo[t];
  const long n = c.n[t], nquads = (n + 3) >> 2;
  const Levels L = make_levels(k, true);
  const int ni = (1 << k) - 1;
  const unsigned mask = (1u << bits) - 1u;
  for (long j = (long)blockIdx.x * kThreads + threadIdx.x; j < nquads; j += (long)gridDim.x * kThreads) {
    const long e0 = j << 2;
    const int p = (int)(e0 & 31) * bits, w0 = p >> 5, s0 = p & 31;
    const unsigned* __restrict__ gw = codes + (e0 >> 5) * bits;
    const int w1 = w0 + 1 < bits ? w0 + 1 : bits - 1, w2 = w0 + 2 < bits ? w0 + 2 : bits - 1;     // (clamped: read, not used)
    const unsigned W0 = gw[w0], W1 = gw[w1], W2 = gw[w2];
    float v[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int off = s0 + u * bits, wi = off >> 5, sh = off & 31;
      const unsigned lo = wi == 0 ? W0 : (wi == 1 ? W1 : W2), hi = wi == 0 ? W1 : W2;
      const unsigned code = (unsigned)((((unsigned long long)hi << 32) | lo) >> sh) & mask;
      v[u] = weight_dequant<FORMULA>(code, L, ni);
      b[u] = rintf(__fmul_rn(v[u], L.n));                 // the bins as alignq_qconv_pack_weights forms them from W_q
    }
    if (e0 + 4 <= n) {
      if (q) *reinterpret_cast<float4*>(q + e0) = make_float4(v[0], v[1], v[2], v[3]);
      if (bf) {
        const bf16x4 h = {(__bf16)b[0], (__bf16)b[1], (__bf16)b[2], (__bf16)b[3]};
        *reinterpret_cast<s16x4*>(bf + e0) = __builtin_bit_cast(s16x4, h);
      }
      if (hf) {
        const f16x4 h = {(_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
        *reinterpret_cast<s16x4*>(hf + e0) = __builtin_bit_cast(s16x4, h);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (e0 + u < n) {
          if (q) q[e0 + u] = v[u];
          if (bf) bf[e0 + u] = __builtin_bit_cast(unsigned short, (__bf16)b[u]);
          if (hf) hf[e0 + u] = __builtin_bit_cast(unsigned short, (_Float16)b[u]);
        }
      }
    }
    if (img) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (e0 + u < n) img_store(img, geo, e0 + u, v[u], L.n);
      }
    }
  }
}

inline int blocks_for(long max_n) {
  long b = (max_n + 2047) / 2048;
  if (b < 1) b = 1;
  return (int)(b > kMaxBlk ? kMaxBlk : b);
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

#define LAUNCH_CHECK()                          \
  do {                                          \
    hipError_t e__ = hipGetLastError();         \
    if (e__ != hipSuccess) return (int)e__;     \
  } while (0)

extern "C" {

size_t alignq_packed_bytes(int64_t n, int bits) {
  if (n < 0 || bits < 1 || bits > kMaxBits) return 0;
  return (size_t)((n + 31) / 32) * (size_t)bits * sizeof(uint32_t);
}

int alignq_weight_code_bits(int k, int formula) {
  if (k < 1 || k > 16) return 0;
  return formula == ALIGNQ_FORMULA_ADMM ? k + 1 : formula == ALIGNQ_FORMULA_CDF ? k : 0;
}

int alignq_weight_pack_multi(int T, const float* const* q, const int64_t* n, int k, int formula, void* const* codes, int32_t* bad,
                             void* stream) {
  if (T <= 0 || !q || !n || !codes || !bad) return ALIGNQ_EINVAL;
  const int bits = alignq_weight_code_bits(k, formula);
  if (!bits) return ALIGNQ_EINVAL;
  for (int i = 0; i < T; i++) {
    if (!q[i] || !codes[i] || n[i] < 1) return ALIGNQ_EINVAL;
    if (misaligned(codes[i], 4) || misaligned(q[i], 4)) return ALIGNQ_EUNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < T; t0 += kChunk) {
    const int cnt = (T - t0 < kChunk) ? T - t0 : kChunk;
    PChunk c;
    long max_n = 0;
    for (int i = 0; i < cnt; i++) {
      c.q[i] = q[t0 + i]; c.codes[i] = (unsigned*)codes[t0 + i]; c.n[i] = (long)n[t0 + i];
      if (c.n[i] > max_n) max_n = c.n[i];
    }
    dim3 grid(blocks_for(max_n), cnt);
    if (formula == ALIGNQ_FORMULA_ADMM)
      hipLaunchKernelGGL((weight_pack_kernel<0>), grid, kThreads, 0, st, c, k, bits, bad);
    else
      hipLaunchKernelGGL((weight_pack_kernel<1>), grid, kThreads, 0, st, c, k, bits, bad);
    LAUNCH_CHECK();
  }
  return 0;
}

int alignq_weight_unpack_multi(int T, const void* const* codes, const int64_t* n, int k, int formula, float* const* q,
                               void* const* bins_bf16, void* const* bins_f16, void* const* img, const int32_t* geom, void* stream) {
  if (T <= 0 || !codes || !n || (!q && !bins_bf16 && !bins_f16 && !img)) return ALIGNQ_EINVAL;
  const int bits = alignq_weight_code_bits(k, formula);
  if (!bits) return ALIGNQ_EINVAL;
  // every tensor of the call is checked before the first launch
  for (int i = 0; i < T; i++) {
    if (!codes[i] || n[i] < 1) return ALIGNQ_EINVAL;
    const bool bins = (bins_bf16 && bins_bf16[i]) || (bins_f16 && bins_f16[i]), im = img && img[i];
    if ((bins || im) && k > 8) return ALIGNQ_EINVAL;          // the bins must be exact in bf16's 8 significant bits
    if (im && (!geom || !img_geo_word(geom + 4 * (size_t)i, (long)n[i]))) return ALIGNQ_EINVAL;
  }
  for (int i = 0; i < T; i++) {
    if (misaligned(codes[i], 4) || (q && q[i] && misaligned(q[i], 16)) || (bins_bf16 && bins_bf16[i] && misaligned(bins_bf16[i], 8)) ||
        (bins_f16 && bins_f16[i] && misaligned(bins_f16[i], 8)) || (img && img[i] && misaligned(img[i], 16)))
      return ALIGNQ_EUNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < T; t0 += kChunk) {
    const int cnt = (T - t0 < kChunk) ? T - t0 : kChunk;
    UChunk c;
    long max_n = 0;
    for (int i = 0; i < cnt; i++) {
      const int t = t0 + i;
      c.codes[i] = (const unsigned*)codes[t];
      c.q[i] = q ? q[t] : nullptr;
      c.bf[i] = bins_bf16 ? (unsigned short*)bins_bf16[t] : nullptr;
      c.hf[i] = bins_f16 ? (unsigned short*)bins_f16[t] : nullptr;
      c.img[i] = img ? (unsigned short*)img[t] : nullptr;
      c.geo[i] = c.img[i] ? img_geo_word(geom + 4 * (size_t)t, (long)n[t]) : 0u;
      c.n[i] = (c.q[i] || c.bf[i] || c.hf[i] || c.img[i]) ? (long)n[t] : 0;      // nothing to write: no work for the grid row
      if (c.n[i] > max_n) max_n = c.n[i];
    }
    if (max_n == 0) continue;
    dim3 grid(blocks_for(max_n), cnt);
    if (formula == ALIGNQ_FORMULA_ADMM)
      hipLaunchKernelGGL((weight_unpack_kernel<0>), grid, kThreads, 0, st, c, k, bits);
    else
      hipLaunchKernelGGL((weight_unpack_kernel<1>), grid, kThreads, 0, st, c, k, bits);
    LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"

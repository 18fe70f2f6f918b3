// dwconv_kernels.hip — the depthwise 3x3 convolution of MobileNet-V2's blocks (groups == C_in == C_out, padding 1, stride 1 or 2;
// cdf_alignment/mobilenet-v2-svhn/model/mobilenetV2.py:40) for gfx950: forward, data gradient and filter gradient on fp32
// channels-last activations and the fp32 quantised filter [C][1][3][3].
//
//   alignq_dwconv3x3_nhwc_fwd / _dgrad : nine multiply-adds per output element, bound by memory.  One thread per channel quad of one
//                         pixel (one 16-byte load per tap, one 16-byte store), lanes along C first so that a wave reads contiguous rows;
//                         at most kMaxGrid workgroups, the rest by a grid stride that is a multiple of the quads per pixel wherever such
//                         a stride exists, so that a thread keeps its 36 filter values in registers.  The two launches are ONE kernel:
//                         they differ only in which source pixel a tap reads.
//   alignq_dwconv3x3_nhwc_wgrad : 36 accumulators per thread (nine taps x a quad).  A workgroup owns kQB channel quads x one slab of
//                         output pixels; its kPG threads of one quad meet in LDS and are added in index order; one partial row
//                         [slab][C][9] per workgroup, then the slab reduction of wgrad_reduce_body.h.  No atomics: the summation order
//                         is a function of the shape alone.
//
// Arithmetic (include/alignq.h states it; tests/dwconv_oracle.py restates it in NumPy): every product and every sum is an individual
// IEEE-754 fp32 operation (-ffp-contract=off), taps in row-major (ky, kx) order, taps in the padding skipped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "wgrad_reduce_body.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 1024;                     // workgroups of the forward / data-gradient launch: what 256 CUs hold at 4 waves / SIMD
constexpr int kQB = 8;                             // filter gradient: channel quads per workgroup (128 contiguous bytes per pixel)
constexpr int kPG = kThreads / kQB;                // ... and threads per quad, each taking every kPG-th pixel of the slab
constexpr int kRowElems = kQB * 4 * 9;             // filter elements of one channel block, in dw's order c * 9 + tap
constexpr int kRowPad = kRowElems + 1;             // LDS row stride (odd: the 36-float stride between quads spreads over the banks)
constexpr int kSlabTarget = 1024;                  // filter gradient: workgroups aimed at
constexpr int kSlabMax = 256;                      // ... slabs at most (one round of the reduction's sixteen loads in flight)
constexpr int kSlabMinPixels = 128;                // ... pixels per slab at least (four per thread)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Source coordinate of tap k (0..2) along one axis, and whether the tap exists.
//   forward:       the input row   d * S + k - 1          (d: output row),          inside [0, n_src)
//   data gradient: the output row (d + 1 - k) / S         (d: input row), if S divides it, inside [0, n_src)
template <int S, bool DGRAD>
__device__ __forceinline__ bool tap_coord(int d, int k, int n_src, int& s) {
  if constexpr (!DGRAD) {
    s = d * S + k - 1;
    return (unsigned)s < (unsigned)n_src;
  } else {
    const int hh = d + 1 - k;
    if constexpr (S == 1) {
      s = hh;
      return (unsigned)s < (unsigned)n_src;
    } else {
      s = hh >> 1;
      return hh >= 0 && !(hh & 1) && s < n_src;
    }
  }
}

// dst [B][Hd][Wd][C] from src [B][Hs][Ws][C]: dst = y, src = x (forward) or dst = dx, src = dy (DGRAD).  n_items = B * Hd * Wd * CQ.
template <int S, bool DGRAD>
__global__ __launch_bounds__(kThreads) void dwconv_kernel(const float* __restrict__ src, const float* __restrict__ wq,
                                                          float* __restrict__ dst, int n_items, int CQ, int Hd, int Wd, int Hs, int Ws) {
  const int C = CQ * 4;
  const int step = gridDim.x * kThreads;
  float f[36];                                     // the quad's filters: f[j * 9 + tap] = wq[(4 * cq + j) * 9 + tap]
  int cq_held = -1;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n_items; i += step) {
    const int cq = i % CQ;
    int p = i / CQ;
    const int wd = p % Wd;
    p /= Wd;
    const int hd = p % Hd, b = p / Hd;
    if (cq != cq_held) {                           // once per thread where step % CQ == 0 (the host picks such a grid where one exists)
#pragma unroll
      for (int q = 0; q < 9; q++) {
        const float4 t = ld4(wq + cq * 36 + q * 4);
        f[q * 4 + 0] = t.x; f[q * 4 + 1] = t.y; f[q * 4 + 2] = t.z; f[q * 4 + 3] = t.w;
      }
      cq_held = cq;
    }
    float4 v[9];
    bool ok[9];
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
      int hs;
      const bool okh = tap_coord<S, DGRAD>(hd, ky, Hs, hs);
#pragma unroll
      for (int kx = 0; kx < 3; kx++) {
        int ws;
        const bool o = tap_coord<S, DGRAD>(wd, kx, Ws, ws) && okh;
        ok[ky * 3 + kx] = o;
        v[ky * 3 + kx] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o) v[ky * 3 + kx] = ld4(src + ((b * Hs + hs) * Ws + ws) * C + cq * 4);
      }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 9; t++) {                  // a tap in the padding is skipped, not added as 0 * w (w may be inf / NaN)
      const float px = v[t].x * f[t], py = v[t].y * f[9 + t], pz = v[t].z * f[18 + t], pw = v[t].w * f[27 + t];
      acc.x = ok[t] ? acc.x + px : acc.x;
      acc.y = ok[t] ? acc.y + py : acc.y;
      acc.z = ok[t] ? acc.z + pz : acc.z;
      acc.w = ok[t] ? acc.w + pw : acc.w;
    }
    *reinterpret_cast<float4*>(dst + i * 4) = acc;
  }
}

// Partial filter gradient of one channel block (blockIdx.x) over one slab of output pixels (blockIdx.y):
//   ws[slab][c * 9 + tap] = sum over the slab's pixels (b, ho, wo) of x[b, ho * S + ky - 1, wo * S + kx - 1, c] * dy[b, ho, wo, c].
// A thread adds its pixels (slab start + pg, + kPG, ...) in ascending order; the kPG threads of a channel are added in pg order.
template <int S>
__global__ __launch_bounds__(kThreads) void dwconv_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                        float* __restrict__ ws, int N, int slab_len, int CQ, int H,
                                                                        int W, int Ho, int Wo) {
  __shared__ float red[kPG][kRowPad];
  const int C = CQ * 4;
  const int ql = threadIdx.x % kQB, pg = threadIdx.x / kQB;
  const int cq = blockIdx.x * kQB + ql;
  const int p0 = blockIdx.y * slab_len;
  const int p1 = p0 + slab_len < N ? p0 + slab_len : N;
  float4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; t++) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cq < CQ) {
    for (int p = p0 + pg; p < p1; p += kPG) {
      const int wo = p % Wo;
      const int r = p / Wo;
      const int ho = r % Ho, b = r / Ho;
      const float4 g = ld4(dy + p * C + cq * 4);
      float4 v[9];
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        int hi;
        const bool okh = tap_coord<S, false>(ho, ky, H, hi);
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          int wi;
          const bool o = tap_coord<S, false>(wo, kx, W, wi) && okh;
          v[ky * 3 + kx] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (o) v[ky * 3 + kx] = ld4(x + ((b * H + hi) * W + wi) * C + cq * 4);
        }
      }
#pragma unroll
      for (int t = 0; t < 9; t++) {
        acc[t].x += v[t].x * g.x; acc[t].y += v[t].y * g.y; acc[t].z += v[t].z * g.z; acc[t].w += v[t].w * g.w;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; t++) {
    float* row = &red[pg][ql * 36 + t];
    row[0] = acc[t].x; row[9] = acc[t].y; row[18] = acc[t].z; row[27] = acc[t].w;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kRowElems; e += kThreads) {
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < kPG; k++) s += red[k][e];
    const int64_t col = (int64_t)blockIdx.x * kRowElems + e;         // = c * 9 + tap
    if (col < (int64_t)C * 9) ws[(int64_t)blockIdx.y * C * 9 + col] = s;
  }
}

__global__ __launch_bounds__(1024) void dwconv_wgrad_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int n_elem,
                                                                   float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float part[4096];
  alignq_wgr::wgrad_reduce_body(slabs, n_slabs, n_elem, dw, blockIdx.x, part);
}

bool shape_ok(int B, int H, int W, int C, int stride) {
  if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (stride != 1 && stride != 2)) return false;
  return (int64_t)B * H * W * C <= (int64_t)INT32_MAX;               // element offsets are int32 (the output is no larger than the input)
}

bool misaligned(const void* a, const void* b, const void* c) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) != 0;
}

int gcd(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// Workgroups of the forward / data-gradient launch over n_items (pixel, quad) pairs.
int elementwise_grid(int n_items, int CQ) {
  const int blocks = (n_items + kThreads - 1) / kThreads;
  if (blocks <= kMaxGrid) return blocks;
  const int m = CQ / gcd(CQ, kThreads);            // gridDim.x * kThreads is a multiple of CQ iff gridDim.x is one of m
  return m <= kMaxGrid ? kMaxGrid / m * m : kMaxGrid;
}

struct WgradPlan { int ncb, slab_len, n_slabs; };

WgradPlan wgrad_plan(int B, int H, int W, int C, int stride) {
  const int N = B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  WgradPlan p;
  p.ncb = (C / 4 + kQB - 1) / kQB;
  int ns = (kSlabTarget + p.ncb - 1) / p.ncb;
  const int cap = (N + kSlabMinPixels - 1) / kSlabMinPixels;
  if (ns > cap) ns = cap;
  if (ns > kSlabMax) ns = kSlabMax;
  if (ns < 1) ns = 1;
  p.slab_len = (N + ns - 1) / ns;
  p.n_slabs = (N + p.slab_len - 1) / p.slab_len;
  return p;
}

template <bool DGRAD>
int launch_elementwise(const float* src, const float* wq, float* dst, int B, int H, int W, int C, int stride, hipStream_t st) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, CQ = C / 4;
  const int Hd = DGRAD ? H : Ho, Wd = DGRAD ? W : Wo, Hs = DGRAD ? Ho : H, Ws = DGRAD ? Wo : W;
  const int n_items = B * Hd * Wd * CQ;
  const int grid = elementwise_grid(n_items, CQ);
  if (stride == 1)
    hipLaunchKernelGGL((dwconv_kernel<1, DGRAD>), grid, kThreads, 0, st, src, wq, dst, n_items, CQ, Hd, Wd, Hs, Ws);
  else
    hipLaunchKernelGGL((dwconv_kernel<2, DGRAD>), grid, kThreads, 0, st, src, wq, dst, n_items, CQ, Hd, Wd, Hs, Ws);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int alignq_dwconv3x3_supported(int B, int H_in, int W_in, int C, int stride) { return shape_ok(B, H_in, W_in, C, stride) ? 1 : 0; }

int alignq_dwconv3x3_nhwc_fwd(const float* x, const float* wq, float* y, int B, int H_in, int W_in, int C, int stride, void* stream) {
  if (!x || !wq || !y) return ALIGNQ_EINVAL;
  if (!shape_ok(B, H_in, W_in, C, stride) || misaligned(x, wq, y)) return ALIGNQ_EUNSUPPORTED;
  return launch_elementwise<false>(x, wq, y, B, H_in, W_in, C, stride, (hipStream_t)stream);
}

int alignq_dwconv3x3_nhwc_dgrad(const float* dy, const float* wq, float* dx, int B, int H_in, int W_in, int C, int stride, void* stream) {
  if (!dy || !wq || !dx) return ALIGNQ_EINVAL;
  if (!shape_ok(B, H_in, W_in, C, stride) || misaligned(dy, wq, dx)) return ALIGNQ_EUNSUPPORTED;
  return launch_elementwise<true>(dy, wq, dx, B, H_in, W_in, C, stride, (hipStream_t)stream);
}

int64_t alignq_dwconv3x3_wgrad_ws_bytes(int B, int H_in, int W_in, int C, int stride) {
  if (!shape_ok(B, H_in, W_in, C, stride)) return 0;
  const WgradPlan p = wgrad_plan(B, H_in, W_in, C, stride);
  const int64_t bytes = (int64_t)p.n_slabs * C * 9 * (int64_t)sizeof(float);
  return (bytes + 255) / 256 * 256;
}

int alignq_dwconv3x3_nhwc_wgrad(const float* x, const float* dy, float* dw, void* ws, int B, int H_in, int W_in, int C, int stride,
                                void* stream) {
  if (!x || !dy || !dw || !ws) return ALIGNQ_EINVAL;
  if (!shape_ok(B, H_in, W_in, C, stride) || misaligned(x, dy, ws)) return ALIGNQ_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int Ho = (H_in - 1) / stride + 1, Wo = (W_in - 1) / stride + 1, CQ = C / 4;
  const WgradPlan p = wgrad_plan(B, H_in, W_in, C, stride);
  const dim3 grid(p.ncb, p.n_slabs);
  float* slabs = static_cast<float*>(ws);
  if (stride == 1)
    hipLaunchKernelGGL(dwconv_wgrad_partial_kernel<1>, grid, kThreads, 0, st, x, dy, slabs, B * Ho * Wo, p.slab_len, CQ, H_in, W_in, Ho, Wo);
  else
    hipLaunchKernelGGL(dwconv_wgrad_partial_kernel<2>, grid, kThreads, 0, st, x, dy, slabs, B * Ho * Wo, p.slab_len, CQ, H_in, W_in, Ho, Wo);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int n_elem = C * 9;
  hipLaunchKernelGGL(dwconv_wgrad_reduce_kernel, alignq_wgr::wgrad_reduce_blocks(p.n_slabs, n_elem), 1024, 0, st, (const float*)slabs,
                     p.n_slabs, n_elem, dw);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

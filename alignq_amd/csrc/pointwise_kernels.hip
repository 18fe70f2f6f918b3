// pointwise_kernels.hip — Conv2d_Q's 1x1 convolutions (reference: cdf_alignment_admm/dann_office/model/quantization.py:164-181,
// F.conv2d(input, weight_q, ...)) at MobileNet-V2's widths: channel counts that are multiples of 8, not of 64 (16 -> 96, 96 -> 24,
// 24 -> 144, 144 -> 32, 576 -> 160 ...).  Forward, data gradient and filter gradient with the arithmetic of qgemm_kernels.hip's
// general-operand form (MODE 0): the filter's integer bins as bf16, the fp32 operand in three exact bf16 terms,
// v_mfma_f32_16x16x32_bf16, fp32 accumulation in an order the shape fixes, one division (the primitives both files run: exact_mma.h;
// the launchers' shared rules: exact_conv_host.h).  include/alignq_pointwise.h states the
// contract.  What differs from qgemm_kernel is the geometry:
//   K edge  the contraction length is a multiple of 8: the tail of the last 64-deep k step is zero-filled in LDS on both operands
//           (a 32-deep half step that holds nothing but zeros is skipped: a choice the shape makes);
//   N edge  the output width is a multiple of 8: tiles of 16, 32 or 64 channels, filter rows beyond N zero-filled and never read,
//           a lane's float4 of four consecutive channels lies wholly inside or wholly outside (N % 8 == 0);
//   M edge  any row count: rows beyond M are staged as zeros and not stored; more row tiles than the grid cap: a grid stride.
// MFMA roles as in qgemm_kernel: A operand = filter side (rows of D = output channels, 4 consecutive per lane -> one float4 store per
// lane), B operand = pixel side (columns of D).  One workgroup = 256 threads = 4 waves = 64 pixels; every wave owns 16 pixels and
// all of the tile's channels, so a short contraction keeps many rows in flight per CU and a narrow N wastes no wide tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"
#include "../../include/alignq_pointwise.h"
#include "exact_conv_host.h"
#include "exact_mma.h"
#include "wgrad_reduce_body.h"

using namespace alignq_xmma;

namespace {

constexpr int BK = 64;                 // k per step (two MFMA k-substeps)
constexpr int BM = 64;                 // pixels per workgroup tile
constexpr int LDX = BK + 16;           // halfwords per LDS row: 160 B rows keep ds_read_b128 conflict-free (qgemm_kernels.hip)
constexpr int kMaxRowBlocks = 2048;    // grid cap over row tiles; the rest by grid stride
constexpr int kMinC = 8, kMaxC = 2048;

// ---------------------------------------------------------------------------------------------------------------------------
// Forward and data gradient:  out[m][n] = (1 / nlev) * sum_k a[m][k] * Wb(n, k)
//   forward (WTR = false): a = x, K = CIN, N = COUT, Wb(n, k) = w[n][k] - rows k-contiguous;
//   data gradient (WTR = true): a = dy, K = COUT, N = CIN, Wb(n, k) = w[k][n]: 16-byte pieces of 8 n are read along the filter's
//   rows and staged transposed, so both forms read the same [n][k] LDS image.
struct PW {
  const float* a; const u16* w; float* out;
  int M, K, N;
  int m_tiles, m_blocks, n_tiles;     // row tiles, row tiles the grid holds (stride of the rest), column tiles
  float nlev;
  int wt;                             // write-through output stores
};

template <int TN, bool WTR>
__global__ __launch_bounds__(256, 3) void pw_gemm_kernel(const PW p) {
  constexpr int BN = 16 * TN;
  constexpr int XPL = BM * LDX;                       // halfwords per pixel-side plane
  constexpr int NA = (BM * (BK / 4)) / 256;           // float4 per thread of the pixel-side tile
  constexpr int NBP = BN * (BK / 8);                  // 16-byte pieces (8 bins) of the filter tile
  constexpr int NB = (NBP + 255) / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + BN * LDX];
  u16* const Xs = lds;
  u16* const Ws = lds + 3 * XPL;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = pid % p.n_tiles, mb = pid / p.n_tiles;
  const int n0 = nt * BN;
  const int fr = lane & 15, fg = lane >> 4;
  const int c4 = tid & 15, rr = tid >> 4;             // pixel-side share: rows rr + 16 i, float4 column c4
  const int nk = (p.K + BK - 1) / BK;

  for (int mt = mb; mt < p.m_tiles; mt += p.m_blocks) {
    const int m0 = mt * BM;
    f32x4 ra[NA];
    s16x8 rw[NB];
    auto fetch = [&](int kt) {
      const int k0 = kt * BK;
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int m = m0 + rr + 16 * i, k = k0 + 4 * c4;
        const bool ok = m < p.M && k < p.K;
        ra[i] = *reinterpret_cast<const f32x4*>(p.a + (ok ? (int64_t)m * p.K + k : 0));
        if (!ok) ra[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        int n, k;
        if (!WTR) { n = n0 + (idx >> 3); k = k0 + 8 * (idx & 7); }
        else { k = k0 + idx / (BN / 8); n = n0 + 8 * (idx % (BN / 8)); }
        const bool ok = idx < NBP && n < p.N && k < p.K;
        const int64_t off = WTR ? (int64_t)k * p.N + n : (int64_t)n * p.K + k;
        rw[i] = *reinterpret_cast<const s16x8*>(p.w + (ok ? off : 0));
        if (!ok) rw[i] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
      }
    };
    auto park = [&]() {
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int o = (rr + 16 * i) * LDX + 4 * c4;
        s16x4 h, m, l;
        split3(ra[i], h, m, l);
        *reinterpret_cast<s16x4*>(Xs + o) = h;
        *reinterpret_cast<s16x4*>(Xs + XPL + o) = m;
        *reinterpret_cast<s16x4*>(Xs + 2 * XPL + o) = l;
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        if (idx >= NBP) continue;
        if (!WTR) {
          *reinterpret_cast<s16x8*>(Ws + (idx >> 3) * LDX + 8 * (idx & 7)) = rw[i];
        } else {
          const int kr = idx / (BN / 8), n8 = idx % (BN / 8);
#pragma unroll
          for (int j = 0; j < 8; j++) Ws[(8 * n8 + j) * LDX + kr] = (u16)rw[i][j];
        }
      }
    };

    f32x4 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int kt = 0; kt < nk; kt++) {
      __syncthreads();                         // the previous step's fragment reads are done
      park();
      __syncthreads();
      if (kt + 1 < nk) fetch(kt + 1);          // in flight under this step's MFMAs
#pragma unroll
      for (int ks = 0; ks < BK / 32; ks++) {
        if (kt * BK + ks * 32 >= p.K) break;   // a half step of zeros only (workgroup-uniform)
        s16x8 wf[TN];
#pragma unroll
        for (int tn = 0; tn < TN; tn++) wf[tn] = *reinterpret_cast<const s16x8*>(Ws + (tn * 16 + fr) * LDX + ks * 32 + 8 * fg);
        const u16* px = Xs + (wv * 16 + fr) * LDX + ks * 32 + 8 * fg;
#pragma unroll
        for (int t = 2; t >= 0; t--) {         // smallest term first
          const s16x8 xf = *reinterpret_cast<const s16x8*>(px + t * XPL);
#pragma unroll
          for (int tn = 0; tn < TN; tn++) acc[tn] = mfma16(wf[tn], xf, acc[tn]);
        }
      }
    }
    // epilogue: lane = pixel (lane & 15) of the wave's 16, 4 consecutive channels 4 * (lane >> 4) + e of every 16-channel block
    const int m = m0 + wv * 16 + fr;
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      const int n = n0 + tn * 16 + 4 * fg;
      f32x4 v = acc[tn];
      v = (f32x4){v[0] / p.nlev, v[1] / p.nlev, v[2] / p.nlev, v[3] / p.nlev};
      if (m < p.M && n < p.N) st_out(p.out + (int64_t)m * p.N + n, v, p.wt);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Filter gradient:  slab[split][co][ci] = sum over the split's pixels m of dy[m][co] * x[m][ci]   (qgemm_wgrad_kernel's 1x1 form)
// Both tiles are staged [k = pixel][channel] (32 pixels per step) and read through ds_read_b64_tr_b16; lane group g takes pixels
// {4g .. 4g+3} and {16 + 4g .. 16 + 4g + 3} of the step on both operands.  Channels beyond CIN / COUT are staged as zeros and
// never read or stored; pixels beyond the split's end are zeros.  D rows = ci (4 consecutive per lane -> float4 store).
constexpr int WK = 32;
struct PWW {
  const float* x; const float* dy; float* slabs;
  int M, per;                      // pixels in all, pixels per split (multiple of WK)
  int CIN, COUT, c_tiles, n_tiles;
};

template <int TC, int TN>
__global__ __launch_bounds__(256, 2) void pw_wgrad_kernel(const PWW a) {
  constexpr int BC = 32 * TC, BNO = 32 * TN;       // tile: BC input channels x BNO output channels; wave = (16 TC) x (16 TN)
  constexpr int LDC = BC + 16, LDO = BNO + 16;
  constexpr int XPL = WK * LDC, DPL = WK * LDO;
  constexpr int NX = (WK * BC / 4) / 256, ND = (WK * BNO / 4) / 256;
  __shared__ __attribute__((aligned(16))) u16 lds[3 * XPL + 3 * DPL];
  u16* const Xs = lds;
  u16* const Ds = lds + 3 * XPL;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wc = wv & 1, wo = wv >> 1;
  const int tiles = a.c_tiles * a.n_tiles;
  const int pid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = pid / tiles, tile = pid % tiles;
  const int ct = tile % a.c_tiles, ot = tile / a.c_tiles;
  const int c0 = ct * BC, o0 = ot * BNO;
  const int m_begin = split * a.per, m_end = (m_begin + a.per < a.M) ? m_begin + a.per : a.M;

  f32x4 rx[NX], rd[ND];
  auto fetch = [&](int m0) {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i, kr = idx / (BC / 4), q4 = idx % (BC / 4);
      const int m = m0 + kr, c = c0 + 4 * q4;
      const bool ok = m < m_end && c < a.CIN;
      rx[i] = *reinterpret_cast<const f32x4*>(a.x + (ok ? (int64_t)m * a.CIN + c : 0));
      if (!ok) rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (BNO / 4), q4 = idx % (BNO / 4);
      const int m = m0 + kr, o = o0 + 4 * q4;
      const bool ok = m < m_end && o < a.COUT;
      rd[i] = *reinterpret_cast<const f32x4*>(a.dy + (ok ? (int64_t)m * a.COUT + o : 0));
      if (!ok) rd[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i, kr = idx / (BC / 4), q4 = idx % (BC / 4);
      const int o = kr * LDC + 4 * q4;
      s16x4 h, m, l;
      split3(rx[i], h, m, l);
      *reinterpret_cast<s16x4*>(Xs + o) = h;
      *reinterpret_cast<s16x4*>(Xs + XPL + o) = m;
      *reinterpret_cast<s16x4*>(Xs + 2 * XPL + o) = l;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i, kr = idx / (BNO / 4), q4 = idx % (BNO / 4);
      const int o = kr * LDO + 4 * q4;
      s16x4 h, m, l;
      split3(rd[i], h, m, l);
      *reinterpret_cast<s16x4*>(Ds + o) = h;
      *reinterpret_cast<s16x4*>(Ds + DPL + o) = m;
      *reinterpret_cast<s16x4*>(Ds + 2 * DPL + o) = l;
    }
  };

  f32x4 acc[TC][TN];
#pragma unroll
  for (int i = 0; i < TC; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fc = 4 * (lane & 3);
  const int krow = 4 * fg + fq;                       // first pixel row of this lane's block (second: + 16)
  if (m_begin < m_end) fetch(m_begin);
  for (int m0 = m_begin; m0 < m_end; m0 += WK) {
    __syncthreads();
    park();
    __syncthreads();
    if (m0 + WK < m_end) fetch(m0 + WK);
    s16x8 xf[TC][3];
#pragma unroll
    for (int tc = 0; tc < TC; tc++)
#pragma unroll
      for (int t = 0; t < 3; t++) {
        const u16* p = Xs + t * XPL + krow * LDC + (wc * TC + tc) * 16 + fc;
        xf[tc][t] = join8(tr_read(p), tr_read(p + 16 * LDC));
      }
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      s16x8 df[3];
#pragma unroll
      for (int t = 0; t < 3; t++) {
        const u16* p = Ds + t * DPL + krow * LDO + (wo * TN + tn) * 16 + fc;
        df[t] = join8(tr_read(p), tr_read(p + 16 * LDO));
      }
#pragma unroll
      for (int tc = 0; tc < TC; tc++) {     // the six leading pairs, smallest first
        f32x4 v = acc[tc][tn];
        v = mfma16(xf[tc][1], df[1], v);
        v = mfma16(xf[tc][0], df[2], v);
        v = mfma16(xf[tc][2], df[0], v);
        v = mfma16(xf[tc][0], df[1], v);
        v = mfma16(xf[tc][1], df[0], v);
        v = mfma16(xf[tc][0], df[0], v);
        acc[tc][tn] = v;
      }
    }
  }
  // D: column = output channel (lane & 15), rows = input channels 4 * (lane >> 4) + e
  float* slab = a.slabs + (int64_t)split * a.COUT * a.CIN;
#pragma unroll
  for (int tn = 0; tn < TN; tn++) {
    const int o = o0 + (wo * TN + tn) * 16 + (lane & 15);
#pragma unroll
    for (int tc = 0; tc < TC; tc++) {
      const int c = c0 + (wc * TC + tc) * 16 + 4 * fg;
      if (o < a.COUT && c < a.CIN) __builtin_nontemporal_store(acc[tc][tn], reinterpret_cast<f32x4*>(slab + (int64_t)o * a.CIN + c));
    }
  }
}

// The slab reduction of wgrad_reduce_body.h at 256 threads (its filler role's width: same groups, same order, same bits as the
// 1024-thread alignq_conv3x3_wgrad_reduce_multi).  These filters are small (256 to 150 k elements): 1024-thread workgroups of up to
// 4096 elements left a 32 x 32 filter's 512 slabs to four workgroups (measured: 12 us of an 18 us filter gradient; 256 threads: 7 us).
constexpr int kRedThreads = 256;
__global__ __launch_bounds__(kRedThreads) void pw_slab_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int n_elem,
                                                                     float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float part[4 * kRedThreads];
  alignq_wgr::wgrad_reduce_body<kRedThreads>(slabs, n_slabs, n_elem, dw, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------------------
inline bool shape_ok(int64_t M, int CIN, int COUT) {
  if (CIN < kMinC || CIN > kMaxC || (CIN & 7) || COUT < kMinC || COUT > kMaxC || (COUT & 7) || M < 1) return false;
  return M * (CIN > COUT ? CIN : COUT) <= (int64_t)INT32_MAX;
}

inline int gemm_form(int N) {
  const int bn = n_tile_width(N);
  return bn == 64 ? ALIGNQ_PW_FORM_N64 : (bn == 32 ? ALIGNQ_PW_FORM_N32 : ALIGNQ_PW_FORM_N16);
}
inline int wgrad_form(int CIN, int COUT) { return (CIN <= 32 ? 0 : 1) + (COUT <= 32 ? 0 : 2); }

template <bool WTR>
int launch_gemm(const float* a, const void* w, float* out, int64_t M, int K, int N, int w_bit, hipStream_t st) {
  PW p{};
  p.a = a; p.w = (const u16*)w; p.out = out;
  p.M = (int)M; p.K = K; p.N = N;
  p.m_tiles = (int)((M + BM - 1) / BM);
  p.m_blocks = p.m_tiles < kMaxRowBlocks ? p.m_tiles : kMaxRowBlocks;
  p.nlev = (float)((1 << w_bit) - 1);
  p.wt = write_through(M * N * (int64_t)sizeof(float));
  const int bn = n_tile_width(N);
  p.n_tiles = (N + bn - 1) / bn;
  const dim3 grid(p.m_blocks * p.n_tiles), blk(256);
  if (bn == 64) hipLaunchKernelGGL((pw_gemm_kernel<4, WTR>), grid, blk, 0, st, p);
  else if (bn == 32) hipLaunchKernelGGL((pw_gemm_kernel<2, WTR>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((pw_gemm_kernel<1, WTR>), grid, blk, 0, st, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// split-K over pixel slabs: enough workgroups for the chip, at least two 32-pixel steps per slab (qgemm_kernels.hip: wgrad_splits)
inline int wgrad_splits(int64_t M, int tiles, int want = 512) {
  int s = (want + tiles - 1) / tiles;
  const int64_t max_s = (M + 2 * WK - 1) / (2 * WK);
  if (s > max_s) s = (int)max_s;
  if (s < 1) s = 1;
  if (s > 1024) s = 1024;
  return s;
}
inline void wgrad_geometry(int64_t M, int CIN, int COUT, int* tc, int* tn, int* tiles, int* splits) {
  const int form = wgrad_form(CIN, COUT);
  *tc = (form & 1) ? 2 : 1;
  *tn = (form & 2) ? 2 : 1;
  *tiles = ((CIN + 32 * *tc - 1) / (32 * *tc)) * ((COUT + 32 * *tn - 1) / (32 * *tn));
  *splits = wgrad_splits(M, *tiles);
}

}  // namespace

extern "C" {

int alignq_pwconv_supported(int64_t M, int CIN, int COUT) { return shape_ok(M, CIN, COUT) ? 1 : 0; }

int alignq_pwconv_form(int op, int64_t M, int CIN, int COUT) {
  if (!shape_ok(M, CIN, COUT)) return -1;
  if (op == ALIGNQ_PW_FWD) return gemm_form(COUT);
  if (op == ALIGNQ_PW_DGRAD) return gemm_form(CIN);
  if (op == ALIGNQ_PW_WGRAD) return wgrad_form(CIN, COUT);
  return -1;
}

int alignq_pwconv_fwd(const float* x, const void* w_bins, float* y, int64_t M, int CIN, int COUT, int w_bit, void* stream) {
  if (!x || !w_bins || !y || !aligned16(x) || !aligned16(w_bins) || !aligned16(y) || w_bit < 1 || w_bit > 8) return ALIGNQ_EINVAL;
  if (!shape_ok(M, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  return launch_gemm<false>(x, w_bins, y, M, CIN, COUT, w_bit, (hipStream_t)stream);
}

int alignq_pwconv_dgrad(const float* dy, const void* w_bins, float* dx, int64_t M, int CIN, int COUT, int w_bit, void* stream) {
  if (!dy || !w_bins || !dx || !aligned16(dy) || !aligned16(w_bins) || !aligned16(dx) || w_bit < 1 || w_bit > 8) return ALIGNQ_EINVAL;
  if (!shape_ok(M, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  return launch_gemm<true>(dy, w_bins, dx, M, COUT, CIN, w_bit, (hipStream_t)stream);
}

size_t alignq_pwconv_wgrad_ws_bytes(int64_t M, int CIN, int COUT) {
  if (!shape_ok(M, CIN, COUT)) return 0;
  int tc, tn, tiles, splits;
  wgrad_geometry(M, CIN, COUT, &tc, &tn, &tiles, &splits);
  return (size_t)splits * (size_t)COUT * CIN * sizeof(float);
}

int alignq_pwconv_wgrad(const float* x, const float* dy, float* dw, void* ws, int64_t M, int CIN, int COUT, int* n_slabs_out,
                        void* stream) {
  if (!x || !dy || !ws || (!dw && !n_slabs_out) || !aligned16(x) || !aligned16(dy) || !aligned16(ws) || !aligned16(dw))
    return ALIGNQ_EINVAL;
  if (!shape_ok(M, CIN, COUT)) return ALIGNQ_EUNSUPPORTED;
  int tc, tn, tiles, splits;
  wgrad_geometry(M, CIN, COUT, &tc, &tn, &tiles, &splits);
  PWW a{};
  a.x = x; a.dy = dy; a.slabs = (float*)ws;
  a.M = (int)M;
  int64_t per = (M + splits - 1) / splits;
  per = (per + WK - 1) / WK * WK;
  a.per = (int)per;
  a.CIN = CIN; a.COUT = COUT; a.c_tiles = (CIN + 32 * tc - 1) / (32 * tc); a.n_tiles = (COUT + 32 * tn - 1) / (32 * tn);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(tiles * splits), blk(256);
  if (tc == 2 && tn == 2) hipLaunchKernelGGL((pw_wgrad_kernel<2, 2>), grid, blk, 0, st, a);
  else if (tc == 2) hipLaunchKernelGGL((pw_wgrad_kernel<2, 1>), grid, blk, 0, st, a);
  else if (tn == 2) hipLaunchKernelGGL((pw_wgrad_kernel<1, 2>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((pw_wgrad_kernel<1, 1>), grid, blk, 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (n_slabs_out) { *n_slabs_out = splits; return 0; }      // deferred: the caller reduces (alignq_conv3x3_wgrad_reduce_multi)
  const int n_elem = COUT * CIN;
  hipLaunchKernelGGL(pw_slab_reduce_kernel, dim3(alignq_wgr::wgrad_reduce_blocks(splits, n_elem, kRedThreads)), dim3(kRedThreads), 0, st,
                     (const float*)ws, splits, n_elem, dw);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

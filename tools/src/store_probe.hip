// What a kernel's stores cost the NEXT launch (developer tool): a captured chain of producer -> trivial dependent consumer in the
// shape of the batch-128 site forward.  The producer is 256 workgroups of 1024 threads (one per CU); each lane stores 16 (8, 4) B per pass
// of the workgroup's 32 KB share of an 8.4 MB "early" output at the start, the workgroup then works for about WORK_US (default 5)
// in LDS and registers, then writes its 33 KB "epilogue" slab from LDS.  Store flavour (none / plain / nt / sc1) is chosen
// separately for the early output and the epilogue, the bytes per lane and store are 16, 8 or 4, and both outputs are also run
// at half and a quarter of their size.  Prints microseconds per producer + consumer pair (the graph holds PAIRS pairs, replayed
// REPLAYS times) and the difference to the store-free producer.
// Build: hipcc -O3 --offload-arch=gfx950 tools/src/store_probe.hip -o tools/bin/store_probe      Run: tools/bin/store_probe [work_us]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int kWgs = 256, kNT = 1024, kPairs = 20, kReplays = 20;        // 400 pairs per figure
constexpr int kEarlyWg = 32768, kEpiWg = 33024;                          // bytes per workgroup at full size (128 x 64 fp32; 8256 floats)
enum { NONE = 0, PLAIN = 1, NT = 2, SC1 = 3 };

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// W bytes at byte offset `off` of `base` (wave-uniform), flavour FL; `n_bytes` bounds the buffer descriptor of the sc1 form
template <int FL, int W>
__device__ __forceinline__ void put(float* base, unsigned n_bytes, unsigned off, f32x4 v) {
  char* p = reinterpret_cast<char*>(base) + off;
  if constexpr (FL == PLAIN) {
    if constexpr (W == 16) *reinterpret_cast<f32x4*>(p) = v;
    else if constexpr (W == 8) *reinterpret_cast<f32x2*>(p) = f32x2{v.x, v.y};
    else *reinterpret_cast<float*>(p) = v.x;
  } else if constexpr (FL == NT) {
    if constexpr (W == 16) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    else if constexpr (W == 8) __builtin_nontemporal_store(f32x2{v.x, v.y}, reinterpret_cast<f32x2*>(p));
    else __builtin_nontemporal_store(v.x, reinterpret_cast<float*>(p));
  } else if constexpr (FL == SC1) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)n_bytes, 0x00020000);
    if constexpr (W == 16) __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, rsrc, (int)off, 0, 16);
    else if constexpr (W == 8) __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(v.x), __float_as_uint(v.y)}, rsrc, (int)off, 0, 16);
    else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.x), rsrc, (int)off, 0, 16);
  }
}

// early_wg / epi_wg: bytes per workgroup (multiples of 16); early_n / epi_n: bytes of the whole buffers
template <int FE, int FP, int W>
__global__ __launch_bounds__(kNT) void producer(float* early, unsigned early_wg, unsigned early_n, float* epi, unsigned epi_wg,
                                                unsigned epi_n, int work_ticks, float seed) {
  __shared__ __attribute__((aligned(16))) float lds[kEpiWg / 4];
  const unsigned tid = threadIdx.x, wg = blockIdx.x;
  f32x4 v = {seed + (float)tid, seed, (float)wg, 1.0f};
  if constexpr (FE != NONE) {
    for (unsigned o = tid * W; o < early_wg; o += kNT * W) put<FE, W>(early, early_n, wg * early_wg + o, v);
  }
  // ~work_ticks of the 100 MHz clock in LDS and registers
  const unsigned long long t0 = wall_clock64();
  for (unsigned e = tid; e < kEpiWg / 4; e += kNT) lds[e] = seed + (float)e;
  __syncthreads();
  float a = v.x;
  do {
#pragma unroll
    for (int i = 0; i < 16; i++) a = __builtin_fmaf(a, 1.0000001f, lds[(tid + 33 * i) & 8191]);
  } while ((long long)(wall_clock64() - t0) < work_ticks);
  lds[tid] += a * 1e-30f;
  __syncthreads();
  if constexpr (FP != NONE) {
    for (unsigned o = tid * W; o < epi_wg; o += kNT * W) {
      f32x4 c;
      if constexpr (W == 16) c = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds) + o);
      else if constexpr (W == 8) { const f32x2 c2 = *reinterpret_cast<const f32x2*>(reinterpret_cast<const char*>(lds) + o); c = f32x4{c2.x, c2.y, 0.f, 0.f}; }
      else c = f32x4{*reinterpret_cast<const float*>(reinterpret_cast<const char*>(lds) + o), 0.f, 0.f, 0.f};
      put<FP, W>(epi, epi_n, wg * epi_wg + o, c);
    }
  }
}

__global__ void consumer(const float* early, const float* epi, float* out) {
  if (threadIdx.x == 0) out[0] = early[0] + epi[0];
}

typedef void (*prod_fn)(float*, unsigned, unsigned, float*, unsigned, unsigned, int, float);
template <int W>
static prod_fn pick(int fe, int fp) {
#define ROW(FE) (fp == 0 ? producer<FE, 0, W> : fp == 1 ? producer<FE, 1, W> : fp == 2 ? producer<FE, 2, W> : producer<FE, 3, W>)
  return fe == 0 ? ROW(0) : fe == 1 ? ROW(1) : fe == 2 ? ROW(2) : ROW(3);
#undef ROW
}

static float *g_early, *g_epi, *g_out;
static hipStream_t g_st;

// microseconds per pair, median of 3 timed blocks of kReplays replays
static double run(prod_fn fn, int div, int work_ticks) {
  const unsigned early_wg = kEarlyWg / div, epi_wg = (kEpiWg / div) & ~15u;
  hipGraph_t g; hipGraphExec_t ge;
  CK(hipStreamBeginCapture(g_st, hipStreamCaptureModeGlobal));
  for (int i = 0; i < kPairs; i++) {
    hipLaunchKernelGGL(fn, kWgs, kNT, 0, g_st, g_early, early_wg, early_wg * kWgs, g_epi, epi_wg, epi_wg * kWgs, work_ticks, (float)i);
    hipLaunchKernelGGL(consumer, 1, 64, 0, g_st, g_early, g_epi, g_out);
  }
  CK(hipStreamEndCapture(g_st, &g));
  CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 3; i++) CK(hipGraphLaunch(ge, g_st));
  CK(hipStreamSynchronize(g_st));
  std::vector<double> us;
  for (int b = 0; b < 3; b++) {
    CK(hipEventRecord(e0, g_st));
    for (int i = 0; i < kReplays; i++) CK(hipGraphLaunch(ge, g_st));
    CK(hipEventRecord(e1, g_st));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    us.push_back(ms * 1e3 / (kReplays * kPairs));
  }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
  std::sort(us.begin(), us.end());
  return us[1];
}

int main(int argc, char** argv) {
  const double work_us = argc > 1 ? atof(argv[1]) : 5.0;
  const int work_ticks = (int)(work_us * 100.0);
  CK(hipStreamCreate(&g_st));
  CK(hipMalloc(&g_early, (size_t)kEarlyWg * kWgs)); CK(hipMalloc(&g_epi, (size_t)kEpiWg * kWgs)); CK(hipMalloc(&g_out, 64));
  CK(hipMemset(g_early, 0, (size_t)kEarlyWg * kWgs)); CK(hipMemset(g_epi, 0, (size_t)kEpiWg * kWgs));
  static const char* nm[4] = {"none", "plain", "nt", "sc1"};
  // every flavour and width writes every byte of both outputs (checked once per kernel at full size, before anything is timed)
  for (int w : {16, 8, 4}) for (int fl = 1; fl < 4; fl++) {
    prod_fn fn = w == 16 ? pick<16>(fl, fl) : (w == 8 ? pick<8>(fl, fl) : pick<4>(fl, fl));
    CK(hipMemset(g_early, 0, (size_t)kEarlyWg * kWgs)); CK(hipMemset(g_epi, 0, (size_t)kEpiWg * kWgs));
    hipLaunchKernelGGL(fn, kWgs, kNT, 0, g_st, g_early, (unsigned)kEarlyWg, (unsigned)kEarlyWg * kWgs, g_epi, (unsigned)kEpiWg, (unsigned)kEpiWg * kWgs, work_ticks, 3.0f);
    CK(hipStreamSynchronize(g_st));
    std::vector<float> he((size_t)kEarlyWg * kWgs / 4), hp((size_t)kEpiWg * kWgs / 4);
    CK(hipMemcpy(he.data(), g_early, he.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hp.data(), g_epi, hp.size() * 4, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < he.size(); i += w / 4) bad += he[i] != 3.0f + (float)((i / (w / 4)) % kNT);
    for (size_t i = 0; i < hp.size(); i++) bad += hp[i] == 0.0f;
    if (bad) { fprintf(stderr, "flavour %s width %d: %zu wrong words\n", nm[fl], w, bad); return 1; }
  }
  printf("# store_probe: %d workgroups x %d threads, work %.1f us, %d pairs x %d replays per figure (median of 3 blocks)\n", kWgs, kNT, work_us, kPairs, kReplays);
  printf("# us per producer+consumer pair; in brackets: minus the store-free producer of the same run\n");
  for (int div : {1, 2, 4}) {
    const double mb_e = kEarlyWg / div * kWgs / 1e6, mb_p = ((kEpiWg / div) & ~15) * kWgs / 1e6;
    for (int w : {16, 8, 4}) {
      auto pk = [&](int fe, int fp) { return w == 16 ? pick<16>(fe, fp) : (w == 8 ? pick<8>(fe, fp) : pick<4>(fe, fp)); };
      const double base = run(pk(0, 0), div, work_ticks);
      printf("\nearly %.2f MB, epilogue %.2f MB, %2d B per lane and store; store-free pair %.2f us\n", mb_e, mb_p, w, base);
      printf("%-12s", "early\\epi");
      for (int fp = 0; fp < 4; fp++) printf(" %16s", nm[fp]);
      printf("\n");
      for (int fe = 0; fe < 4; fe++) {
        printf("%-12s", nm[fe]);
        for (int fp = 0; fp < 4; fp++) {
          const double t = run(pk(fe, fp), div, work_ticks);
          printf("   %6.2f (%+5.2f)", t, t - base);
        }
        printf("\n");
      }
      fflush(stdout);
    }
  }
  return 0;
}

// data_kernels.hip — the CIFAR / SVHN input pipeline on the device (the reference's host pipeline: RandomCrop(32, padding=4),
// RandomHorizontalFlip, ToTensor, Normalize and the DataLoader's batching, cdf_alignment_admm/resnet-20-cifar-10/data/cifar10.py:11-33,
// cdf_alignment/resnet-20-svhn/data/svhn.py:14-34) for gfx950.
//
//   alignq_data_batch   : ONE launch per batch.  The data set lives in device memory as bytes ([N][32][32][3]); the launch gathers the
//                         batch's samples through the epoch's permutation, crops, flips, normalises through a [3][256] table and writes
//                         fp32 NCHW or channels-last straight into the tensors a captured step reads.  {epoch, position} come from
//                         DEVICE memory, so one captured launch serves every batch of every epoch; the workgroup that is last to
//                         have read them moves the position on for the next launch (no second launch in the captured chain).
//   alignq_data_crop_batch : the same for the Office sets: a crop x crop window (random or centred) of [N][side][side][3] bytes, with the
//                         same cursor protocol and the same draws (data_crop_batch_kernel, below the 32 x 32 one).
//
// 393 KB read and 1.5 MB written per batch of 128: bound by launch and latency.  Four workgroups of three waves per image (512 short
// workgroups per batch of 128), the table in LDS (one float4 load per thread), ONE 16-byte store per thread in either layout, four byte
// loads per thread.  No division on the device: the value of a pixel is table[c][byte], bit-equal to ToTensor + Normalize by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alignq.h"

namespace {

constexpr int kSide = 32;                          // image height and width
constexpr int kImgBytes = kSide * kSide * 3;
constexpr int kParts = 4;                          // workgroups per image: 8 rows each
constexpr int kPartRows = kSide / kParts;
constexpr int kThreads = 192;                      // 8 rows x 32 pixels x 3 channels / 4 floats per store; = 768 table floats / 4
static_assert(kPartRows * kSide * 3 == 4 * kThreads && 3 * 256 == 4 * kThreads, "one float4 of the output and of the table per thread");

// The random draws of sample position `pos` in epoch `epoch` (include/alignq.h states the same sequence of integer operations;
// tests/data_oracle.py restates it in NumPy).  All arithmetic modulo 2^64.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {         // the finaliser of splitmix64
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__device__ __forceinline__ uint64_t draw64(uint64_t seed, uint32_t epoch, uint64_t pos) {
  const uint64_t key = mix64(mix64(seed) + (uint64_t)epoch);
  return mix64(key + 0x9E3779B97F4A7C15ull * (pos + 1ull));
}

template <bool NHWC>
__global__ __launch_bounds__(kThreads) void data_batch_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ labels,
                                                              const int64_t* __restrict__ perm, int32_t* cursor,
                                                              int advance, const float* __restrict__ lut, int64_t N, int B, int rank,
                                                              uint64_t seed, int pad, int flip, float* __restrict__ x_out,
                                                              int64_t* __restrict__ y_out) {
  __shared__ __attribute__((aligned(16))) float lut_s[3 * 256];
  __shared__ int32_t cur_s[2];
  const int t = threadIdx.x;
  reinterpret_cast<float4*>(lut_s)[t] = reinterpret_cast<const float4*>(lut)[t];
  const int i = blockIdx.x, part = blockIdx.y;
  // ONE thread of the workgroup reads the cursor and hands it on through LDS: its loads have returned before the ticket below
  if (t == 0) {
    cur_s[0] = __hip_atomic_load(&cursor[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cur_s[1] = __hip_atomic_load(&cursor[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const uint32_t epoch = (uint32_t)cur_s[0];
  const int32_t first = cur_s[1];
  if (advance && t == 0) {
    // cursor[2] counts the workgroups that have read the cursor; the last one moves the position on for the next launch and re-arms
    // the count (the hand-off idiom of head_body.h: an agent-scope ticket, write-through stores).  Nobody reads the cursor after it.
    unsigned* ticket = reinterpret_cast<unsigned*>(cursor + 2);
    const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == gridDim.x * gridDim.y - 1u) {
      __hip_atomic_store(&cursor[1], first + advance, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  const int64_t pos = (int64_t)first + (int64_t)rank * B + i;
  if (pos < 0 || pos >= N) return;                 // a row past the end of the epoch is not written
  const int64_t s = perm ? perm[pos] : pos;
  if (s < 0 || s >= N) return;                     // (a permutation entry outside the set reads nothing)
  const uint64_t r = draw64(seed, epoch, (uint64_t)pos);
  // 9-way draws by multiply-high of 24 bits: floor(9 u / 2^24), u = bits 0..23 (dy) and bits 24..47 (dx); the flip is bit 48
  const int dy = pad ? (int)((((uint32_t)r & 0xFFFFFFu) * 9u) >> 24) : 0;
  const int dx = pad ? (int)((((uint32_t)(r >> 24) & 0xFFFFFFu) * 9u) >> 24) : 0;
  const int f = flip ? (int)((r >> 48) & 1u) : 0;
  const uint8_t* __restrict__ img = images + s * kImgBytes;
  // thread -> its four output elements (column w[e], channel c[e]) of one row h: consecutive threads store consecutive 16 bytes
  int h, w[4], c[4];
  int64_t o4;                                      // the float4 index of the store inside the batch
  if (NHWC) {
    const int g = t / 3, j = t - 3 * g;            // pixel group (4 pixels = 48 B = 3 float4) of this part, float4 j of it
    h = part * kPartRows + (g >> 3);
    const int w0 = (g & 7) * 4;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int q = 4 * j + e, px = q / 3;
      w[e] = w0 + px;
      c[e] = q - 3 * px;
    }
    o4 = (int64_t)i * (kImgBytes / 4) + ((h * kSide + w0) * 3) / 4 + j;
  } else {
    const int cc = t >> 6, q = t & 63;             // plane, (row, group of 4 columns) of this part
    h = part * kPartRows + (q >> 3);
    const int w0 = (q & 7) * 4;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      w[e] = w0 + e;
      c[e] = cc;
    }
    o4 = (int64_t)i * (kImgBytes / 4) + cc * (kSide * kSide / 4) + h * (kSide / 4) + (w0 >> 2);
  }
  const int sh = h + dy - pad;                     // crop first, then flip (torchvision's order)
  const bool row_in = (unsigned)sh < (unsigned)kSide;
  uint32_t b[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int sw = (f ? kSide - 1 - w[e] : w[e]) + dx - pad;
    const bool in = row_in && (unsigned)sw < (unsigned)kSide;
    const uint32_t v = img[in ? (sh * kSide + sw) * 3 + c[e] : 0];
    b[e] = in ? v : 0u;                            // outside the image the BYTE is 0: the value is table[c][0], not 0.0
  }
  float4 v;
  v.x = lut_s[c[0] * 256 + b[0]];
  v.y = lut_s[c[1] * 256 + b[1]];
  v.z = lut_s[c[2] * 256 + b[2]];
  v.w = lut_s[c[3] * 256 + b[3]];
  reinterpret_cast<float4*>(x_out)[o4] = v;
  if (part == 0 && t == 0) y_out[i] = labels[s];
}

// The Office pipeline (Resize((256, 256)) once at load time; RandomCrop(224) or the centre window, RandomHorizontalFlip, ToTensor,
// Normalize: cdf_alignment_admm/dann_office/data/office.py:13-38): a crop x crop window of a side x side byte image.  4.2 MB read and
// 16.9 MB written per batch of 28: bound by bandwidth.  One workgroup per image and block of kCropRows output rows (28 x 28 = 784
// workgroups for 28 images of 224 rows), the table in LDS, per step of a thread four byte loads and ONE 16-byte store; consecutive
// threads store consecutive 16 bytes in either layout.  The window lies inside the image: no padding branch.
constexpr int kCropRows = 8;
constexpr int kCropThreads = 256;

template <bool NHWC>
__global__ __launch_bounds__(kCropThreads) void data_crop_batch_kernel(const uint8_t* __restrict__ images,
                                                                       const int64_t* __restrict__ labels,
                                                                       const int64_t* __restrict__ perm, int32_t* cursor, int advance,
                                                                       const float* __restrict__ lut, int64_t N, int side, int crop,
                                                                       int span, int off0, int B, int rank, uint64_t seed, int flip,
                                                                       float* __restrict__ x_out, int64_t* __restrict__ y_out) {
  __shared__ __attribute__((aligned(16))) float lut_s[3 * 256];
  __shared__ int32_t cur_s[2];
  const int t = threadIdx.x;
  if (t < 3 * 256 / 4) reinterpret_cast<float4*>(lut_s)[t] = reinterpret_cast<const float4*>(lut)[t];
  const int i = blockIdx.x, part = blockIdx.y;
  // the cursor protocol of data_batch_kernel, verbatim
  if (t == 0) {
    cur_s[0] = __hip_atomic_load(&cursor[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cur_s[1] = __hip_atomic_load(&cursor[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const uint32_t epoch = (uint32_t)cur_s[0];
  const int32_t first = cur_s[1];
  if (advance && t == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(cursor + 2);
    const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == gridDim.x * gridDim.y - 1u) {
      __hip_atomic_store(&cursor[1], first + advance, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  const int64_t pos = (int64_t)first + (int64_t)rank * B + i;
  if (pos < 0 || pos >= N) return;                 // a row past the end of the epoch is not written
  const int64_t s = perm ? perm[pos] : pos;
  if (s < 0 || s >= N) return;                     // (a permutation entry outside the set reads nothing)
  const uint64_t r = draw64(seed, epoch, (uint64_t)pos);
  // span-way draws by multiply-high of 24 bits (span <= 255: the product fits 32 bits); the flip is bit 48
  const int oy = off0 + (int)((((uint32_t)r & 0xFFFFFFu) * (uint32_t)span) >> 24);
  const int ox = off0 + (int)((((uint32_t)(r >> 24) & 0xFFFFFFu) * (uint32_t)span) >> 24);
  const int f = flip ? (int)((r >> 48) & 1u) : 0;
  const uint8_t* __restrict__ img = images + s * ((int64_t)side * side * 3);
  const int h0 = part * kCropRows;
  const int rows = min(kCropRows, crop - h0);
  const int quads = crop >> 2;                     // float4 per row of one plane
  const int row4 = 3 * quads;                      // float4 per row of all three channels
  float4* __restrict__ out4 = reinterpret_cast<float4*>(x_out) + (int64_t)i * crop * row4;
  for (int item = t; item < rows * row4; item += kCropThreads) {
    // item -> its four output elements (column w[e], channel c[e]) of one row h
    int h, w[4], c[4];
    int64_t o4;                                    // the float4 index of the store inside the image
    if (NHWC) {
      const int hr = item / row4, j = item - hr * row4;
      h = h0 + hr;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int q = 4 * j + e, px = q / 3;
        w[e] = px;
        c[e] = q - 3 * px;
      }
      o4 = (int64_t)h * row4 + j;
    } else {
      const int per_plane = rows * quads;
      const int cc = item / per_plane, rem = item - cc * per_plane;
      const int hr = rem / quads, g = rem - hr * quads;
      h = h0 + hr;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        w[e] = 4 * g + e;
        c[e] = cc;
      }
      o4 = ((int64_t)cc * crop + h) * quads + g;
    }
    const uint8_t* __restrict__ src = img + (int64_t)(oy + h) * side * 3;      // crop first, then flip (torchvision's order)
    uint32_t b[4];
#pragma unroll
    for (int e = 0; e < 4; e++) b[e] = src[((f ? crop - 1 - w[e] : w[e]) + ox) * 3 + c[e]];
    float4 v;
    v.x = lut_s[c[0] * 256 + b[0]];
    v.y = lut_s[c[1] * 256 + b[1]];
    v.z = lut_s[c[2] * 256 + b[2]];
    v.w = lut_s[c[3] * 256 + b[3]];
    out4[o4] = v;
  }
  if (part == 0 && t == 0) y_out[i] = labels[s];
}

}  // namespace

extern "C" {

int alignq_data_batch(const uint8_t* images, const int64_t* labels, const int64_t* perm, int32_t* cursor, int advance, const float* lut,
                      int64_t N, int B, int rank, int world, uint64_t seed, int pad, int flip, float* x_out, int nhwc, int64_t* y_out,
                      void* stream) {
  if (!images || !labels || !cursor || !lut || !x_out || !y_out) return ALIGNQ_EINVAL;
  if (N < 1 || B < 1 || world < 1 || rank < 0 || rank >= world || advance < 0) return ALIGNQ_EINVAL;
  if ((pad != 0 && pad != 4) || (flip != 0 && flip != 1) || (nhwc != 0 && nhwc != 1)) return ALIGNQ_EINVAL;
  if ((reinterpret_cast<uintptr_t>(lut) | reinterpret_cast<uintptr_t>(x_out)) & 15) return ALIGNQ_EINVAL;
  if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(perm) | reinterpret_cast<uintptr_t>(y_out)) & 7) return ALIGNQ_EINVAL;
  if (reinterpret_cast<uintptr_t>(cursor) & 3) return ALIGNQ_EINVAL;
  if (N > ((int64_t)1 << 30) || B > 65535 || advance > (1 << 30)) return ALIGNQ_EUNSUPPORTED;      // the cursor is int32; one grid row per image
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(B, kParts);
  if (nhwc)
    hipLaunchKernelGGL(data_batch_kernel<true>, grid, kThreads, 0, st, images, labels, perm, cursor, advance, lut, N, B, rank, seed, pad, flip,
                       x_out, y_out);
  else
    hipLaunchKernelGGL(data_batch_kernel<false>, grid, kThreads, 0, st, images, labels, perm, cursor, advance, lut, N, B, rank, seed, pad, flip,
                       x_out, y_out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int alignq_data_crop_batch(const uint8_t* images, const int64_t* labels, const int64_t* perm, int32_t* cursor, int advance,
                           const float* lut, int64_t N, int side, int crop, int span, int off0, int B, int rank, int world,
                           uint64_t seed, int flip, float* x_out, int nhwc, int64_t* y_out, void* stream) {
  if (!images || !labels || !cursor || !lut || !x_out || !y_out) return ALIGNQ_EINVAL;
  if (N < 1 || B < 1 || world < 1 || rank < 0 || rank >= world || advance < 0) return ALIGNQ_EINVAL;
  if (crop < 4 || (crop & 3) || crop > side || side > 1024) return ALIGNQ_EINVAL;
  if (span < 1 || span > 255 || off0 < 0 || off0 > side - crop || off0 + span - 1 > side - crop) return ALIGNQ_EINVAL;      // the window stays inside the image
  if ((flip != 0 && flip != 1) || (nhwc != 0 && nhwc != 1)) return ALIGNQ_EINVAL;
  if ((reinterpret_cast<uintptr_t>(lut) | reinterpret_cast<uintptr_t>(x_out)) & 15) return ALIGNQ_EINVAL;
  if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(perm) | reinterpret_cast<uintptr_t>(y_out)) & 7) return ALIGNQ_EINVAL;
  if (reinterpret_cast<uintptr_t>(cursor) & 3) return ALIGNQ_EINVAL;
  if (N > ((int64_t)1 << 30) || B > 65535 || advance > (1 << 30)) return ALIGNQ_EUNSUPPORTED;      // the cursor is int32; one grid row per image
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(B, (crop + kCropRows - 1) / kCropRows);
  if (nhwc)
    hipLaunchKernelGGL(data_crop_batch_kernel<true>, grid, kCropThreads, 0, st, images, labels, perm, cursor, advance, lut, N, side, crop, span,
                       off0, B, rank, seed, flip, x_out, y_out);
  else
    hipLaunchKernelGGL(data_crop_batch_kernel<false>, grid, kCropThreads, 0, st, images, labels, perm, cursor, advance, lut, N, side, crop, span,
                       off0, B, rank, seed, flip, x_out, y_out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

// Batch rows from the decoded images kept resident in HBM (yogo_amd/image_cache.py, `yogo train --device-image-cache GIB`):
// out[b] = cache[slots[b]] for every batch row b with slots[b] >= 0, either as uint8 or as fp32 x / 255 (normalize_images,
// yogo_dataset.py: `image / 255` on the host).  The fp32 values are bit-identical to torch's CPU `uint8_tensor / 255`: build.sh
// compiles with -fhip-fp32-correctly-rounded-divide-sqrt, so x / 255.f is the correctly rounded quotient (blobgen.hip's compose
// relies on the same).  Rows with slots[b] < 0 (uploaded rows, blob images) are not touched.
//
// One pass, HBM-bound: per row C*H*W bytes are read and C*H*W * (1 or 4) bytes written.  When a row is a whole number of
// 16-byte pieces and both buffers are 16-byte aligned (772 x 1032 = 796,704 bytes = 49,794 pieces), every lane moves UNROLL
// pieces: 16-byte loads, then 16-byte stores (uint8) or four 16-byte stores of fp32 / 255.  Other shapes take a byte-wise kernel.
#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int UNROLL = 4;   // 16-byte pieces per lane: 16 KiB of cache per workgroup

// grid (pieces of a row / (BLOCK * UNROLL), B)
template <bool F32>
__global__ __launch_bounds__(BLOCK) void image_cache_gather_vec_kernel(const uint4* __restrict__ cache, int S, const int* __restrict__ slots,
                                                                       long long n16, void* __restrict__ out) {
  const int b = blockIdx.y;
  const int s = slots[b];
  if (s < 0 || s >= S) return;
  const uint4* src = cache + (size_t)s * n16;
  const long long i0 = (long long)blockIdx.x * (BLOCK * UNROLL) + threadIdx.x;
  uint4 v[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const long long i = i0 + (long long)u * BLOCK;
    if (i < n16) v[u] = src[i];
  }
  if (!F32) {
    uint4* dst = static_cast<uint4*>(out) + (size_t)b * n16;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long i = i0 + (long long)u * BLOCK;
      if (i < n16) dst[i] = v[u];
    }
  } else {
    float4* dst = static_cast<float4*>(out) + (size_t)b * n16 * 4;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long i = i0 + (long long)u * BLOCK;
      if (i < n16) {
        const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          dst[i * 4 + k] = make_float4((float)(w[k] & 0xffu) / 255.f, (float)((w[k] >> 8) & 0xffu) / 255.f,
                                       (float)((w[k] >> 16) & 0xffu) / 255.f, (float)(w[k] >> 24) / 255.f);
      }
    }
  }
}

// any row size / alignment: one byte per lane and step.  grid (bytes of a row / (BLOCK * UNROLL), B)
template <bool F32>
__global__ __launch_bounds__(BLOCK) void image_cache_gather_byte_kernel(const unsigned char* __restrict__ cache, int S,
                                                                        const int* __restrict__ slots, long long n, void* __restrict__ out) {
  const int b = blockIdx.y;
  const int s = slots[b];
  if (s < 0 || s >= S) return;
  const unsigned char* src = cache + (size_t)s * n;
  const long long i0 = (long long)blockIdx.x * (BLOCK * UNROLL) + threadIdx.x;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const long long i = i0 + (long long)u * BLOCK;
    if (i < n) {
      if (F32)
        static_cast<float*>(out)[(size_t)b * n + i] = (float)src[i] / 255.f;
      else
        static_cast<unsigned char*>(out)[(size_t)b * n + i] = src[i];
    }
  }
}

}  // namespace

extern "C" int yogo_image_cache_gather(const unsigned char* cache, int S, const int* slots, int B, int C, int H, int W, void* out,
                                       int out_fp32, hipStream_t stream) {
  YOGO_CHECK_ARG(cache && slots && out && S > 0 && B >= 0, "image_cache_gather: bad arguments");
  YOGO_CHECK_ARG(C >= 1 && H >= 1 && W >= 1, "image_cache_gather: bad image shape %d x %d x %d", C, H, W);
  YOGO_CHECK_ARG(B <= 65535, "image_cache_gather: B = %d rows, at most 65535 per call", B);
  YOGO_CHECK_ARG(out_fp32 == 0 || out_fp32 == 1, "image_cache_gather: out_fp32 must be 0 (uint8) or 1 (float32)");
  if (B == 0) return YOGO_OK;
  const long long n = (long long)C * H * W;
  const bool vec = n % 16 == 0 && (reinterpret_cast<uintptr_t>(cache) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const long long per_block = (long long)BLOCK * UNROLL;
  if (vec) {
    const long long n16 = n / 16;
    const dim3 grid((unsigned)((n16 + per_block - 1) / per_block), B);
    if (out_fp32)
      hipLaunchKernelGGL(image_cache_gather_vec_kernel<true>, grid, dim3(BLOCK), 0, stream, reinterpret_cast<const uint4*>(cache), S, slots,
                         n16, out);
    else
      hipLaunchKernelGGL(image_cache_gather_vec_kernel<false>, grid, dim3(BLOCK), 0, stream, reinterpret_cast<const uint4*>(cache), S,
                         slots, n16, out);
  } else {
    const dim3 grid((unsigned)((n + per_block - 1) / per_block), B);
    if (out_fp32)
      hipLaunchKernelGGL(image_cache_gather_byte_kernel<true>, grid, dim3(BLOCK), 0, stream, cache, S, slots, n, out);
    else
      hipLaunchKernelGGL(image_cache_gather_byte_kernel<false>, grid, dim3(BLOCK), 0, stream, cache, S, slots, n, out);
  }
  YOGO_CHECK_LAUNCH("image_cache_gather");
  if (yogo_launch_log_enabled())
    yogo_launch_log("image_cache_gather_%s_kernel<%s> | B=%d n=%lld", vec ? "vec" : "byte", out_fp32 ? "f32" : "u8", B, n);
  return YOGO_OK;
}

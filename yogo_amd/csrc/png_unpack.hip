// The inflated scanlines of 8-bit greyscale PNG files -> image batches on the device (yogo_amd/png_feed.py, behind inflate.hip):
// the PNG filters reversed, the centre crop and the optional / 255 in one launch.
//   table[b] = { off, raw }   (int64 each)
// off: where image b lies in `scan`; raw == 0: H scanlines of 1 + W bytes, the filter-type byte first; raw != 0: H x W pixels as
// they are (an image the host decoded).  out: [B][1][OH][OW] uint8 or fp32 x / 255 (bit-identical to torch's CPU
// uint8_tensor / 255: build.sh compiles with correctly rounded division), out[b][0][oy][ox] = image_b[top + oy][left + ox].
// status[b] = 0, 1 (a filter-type byte above 4) or 2 (the image does not lie inside scan: nothing of it was read).
//
// The filters are reversed by csrc/png_unfilter.h's loop at one byte per pixel (one wavefront per image, 64 rows at a time; `scan` is
// WRITTEN: the last row of every band of 64 is unfiltered in place); this file says where a pixel goes: crop and put.
#include "png_unfilter.h"

namespace {

using namespace yogo_png;

template <bool FP32>
__device__ __forceinline__ void put(void* out, long long i, unsigned v) {
  if (FP32) static_cast<float*>(out)[i] = (float)v / 255.f;
  else static_cast<unsigned char*>(out)[i] = (unsigned char)v;
}

// a pixel of the image into the crop: out[oy][ox] = image[top + oy][left + ox]
template <bool FP32>
struct CropSink {
  void* out;
  long long obase;
  int top, left, OH, OW, oy;
  bool row_out;
  __device__ __forceinline__ void row(int y, bool active) {
    oy = y - top;
    row_out = active && oy >= 0 && oy < OH;
  }
  __device__ __forceinline__ void pixel(int x, unsigned v) const {
    const int ox = x - left;
    if (row_out && ox >= 0 && ox < OW) put<FP32>(out, obase + (long long)oy * OW + ox, v);
  }
};

template <bool FP32>
__global__ __launch_bounds__(WAVE) void png_unpack_kernel(unsigned char* scan, long long scan_bytes, const long long* __restrict__ table,
                                                          int H, int W, int top, int left, int OH, int OW, void* out,
                                                          int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long off = table[2LL * b], raw = table[2LL * b + 1];
  const long long need = raw ? (long long)H * W : (long long)H * (W + 1);
  if (off < 0 || off > scan_bytes || need > scan_bytes - off) {
    if (lane == 0) status[b] = ST_BAD_IMAGE;
    return;
  }
  const long long obase = (long long)b * OH * OW;
  if (raw) {
    const unsigned char* img = scan + off;
    for (int i = lane; i < OH * OW; i += WAVE) {   // (OH * OW < 2^31: the entry point checks)
      const int oy = i / OW, ox = i - oy * OW;
      put<FP32>(out, obase + i, img[(long long)(top + oy) * W + left + ox]);
    }
    if (lane == 0) status[b] = ST_OK;
    return;
  }
  const int st = unfilter<1>(scan + off, H, W, CropSink<FP32>{out, obase, top, left, OH, OW, 0, false}, lane);
  if (lane == 0) status[b] = st;
}

}  // namespace

extern "C" int yogo_png_unpack(unsigned char* scan, long long scan_bytes, const long long* table, int B, int H, int W, int top, int left,
                               int OH, int OW, void* out, int out_fp32, int* status, hipStream_t stream) {
  YOGO_CHECK_ARG(scan && table && out && status && scan_bytes > 0 && B >= 0, "png_unpack: bad arguments");
  YOGO_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "png_unpack: bad image shape %d x %d (1 .. 65535 each)", H, W);
  YOGO_CHECK_ARG(top >= 0 && left >= 0 && top < H && left < W, "png_unpack: crop origin (%d, %d) outside the %d x %d image", top, left, H, W);
  YOGO_CHECK_ARG(OH >= 1 && OH <= H - top && OW >= 1 && OW <= W - left, "png_unpack: a %d x %d crop at (%d, %d) of a %d x %d image", OH,
                 OW, top, left, H, W);
  YOGO_CHECK_ARG(B <= 65535, "png_unpack: B = %d images, at most 65535 per call", B);
  YOGO_CHECK_ARG(out_fp32 == 0 || out_fp32 == 1, "png_unpack: out_fp32 must be 0 (uint8) or 1 (float32)");
  YOGO_CHECK_ARG((long long)OH * OW < (1LL << 31), "png_unpack: a crop of %d x %d pixels", OH, OW);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                 "png_unpack: the table must be 8-byte, the status and the output 4-byte aligned");
  if (B == 0) return YOGO_OK;
  if (out_fp32)
    hipLaunchKernelGGL(png_unpack_kernel<true>, dim3(B), dim3(WAVE), 0, stream, scan, scan_bytes, table, H, W, top, left, OH, OW, out, status);
  else
    hipLaunchKernelGGL(png_unpack_kernel<false>, dim3(B), dim3(WAVE), 0, stream, scan, scan_bytes, table, H, W, top, left, OH, OW, out, status);
  YOGO_CHECK_LAUNCH("png_unpack");
  if (yogo_launch_log_enabled())
    yogo_launch_log("png_unpack_kernel<%s> | B=%d image=%dx%d crop=%dx%d@(%d,%d)", out_fp32 ? "f32" : "u8", B, H, W, OH, OW, top, left);
  return YOGO_OK;
}

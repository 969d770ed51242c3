// The inflated scanlines of 8-bit greyscale and 8-bit RGB PNG files -> full frames of the device image cache
// (yogo_amd/png_prefill.py, behind inflate.hip): the PNG filters reversed and the file's channels converted to the cache's.
//   table[b] = { off, kind }   (int64 each)
// off: where image b lies in `scan`.  kind 0: H scanlines of 1 + W bytes (8-bit grey), the filter-type byte first; kind 2: H
// scanlines of 1 + 3 W bytes (8-bit RGB, the filters at 3 bytes per pixel); kind 1: C_out x H x W planar pixels as they are (an
// image the host decoded).  out: [B][C_out][H][W] uint8, C_out 1 or 3 -- no crop, no / 255.  The conversions are those of
// yogo_amd.yogo_dataset.read_image(path, rgb): grey -> 1 plane as it is, grey -> 3 planes the plane three times, RGB -> 3 planes
// de-interleaved, RGB -> 1 plane L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (PIL's convert("L")).
// status[b] = 0, 1 (a filter-type byte above 4) or 2 (an unknown kind, or the image does not lie inside scan: nothing of it was
// read), as in png_unpack.hip.
//
// The filters are reversed by csrc/png_unfilter.h's loop at 1 or 3 bytes per pixel, as in png_unpack.hip (one wavefront per image;
// `scan` is WRITTEN: the last row of every band of 64 rows is unfiltered in place); this file says where a pixel goes: emit.
#include "png_unfilter.h"

namespace {

using namespace yogo_png;

enum : long long { KIND_GREY = 0, KIND_PLANAR = 1, KIND_RGB = 2 };

// one unfiltered pixel into its planes: i = y * W + x, plane = H * W
template <int BPP, int COUT>
__device__ __forceinline__ void emit(unsigned char* out, long long plane, long long i, unsigned v) {
  if (BPP == 1) {
#pragma unroll
    for (int c = 0; c < COUT; ++c) out[c * plane + i] = (unsigned char)v;
  } else if (COUT == 3) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane + i] = (unsigned char)(v >> (8 * c));
  } else {
    out[i] = (unsigned char)((19595u * (v & 255u) + 38470u * ((v >> 8) & 255u) + 7471u * (v >> 16) + 0x8000u) >> 16);
  }
}

// a pixel of row y into the COUT planes at out
template <int BPP, int COUT>
struct PlaneSink {
  unsigned char* out;
  long long plane;
  int W;
  long long row0;
  __device__ __forceinline__ void row(int y, bool) { row0 = (long long)y * W; }
  __device__ __forceinline__ void pixel(int x, unsigned v) const { emit<BPP, COUT>(out, plane, row0 + x, v); }
};

template <int COUT>
__global__ __launch_bounds__(WAVE) void png_unpack_planes_kernel(unsigned char* scan, long long scan_bytes, const long long* __restrict__ table,
                                                                 int H, int W, unsigned char* out, int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long off = table[2LL * b], kind = table[2LL * b + 1];
  const long long plane = (long long)H * W;
  const long long need = kind == KIND_GREY ? (long long)H * (W + 1) : kind == KIND_RGB ? (long long)H * (3LL * W + 1) : COUT * plane;
  if (kind < KIND_GREY || kind > KIND_RGB || off < 0 || off > scan_bytes || need > scan_bytes - off) {
    if (lane == 0) status[b] = ST_BAD_IMAGE;
    return;
  }
  unsigned char* img = scan + off;
  unsigned char* o = out + (long long)b * COUT * plane;
  int st = ST_OK;
  if (kind == KIND_PLANAR) {
    if (((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
      const long long n16 = need / 16;
      for (long long i = lane; i < n16; i += WAVE) reinterpret_cast<uint4*>(o)[i] = reinterpret_cast<const uint4*>(img)[i];
      for (long long i = n16 * 16 + lane; i < need; i += WAVE) o[i] = img[i];
    } else {
      for (long long i = lane; i < need; i += WAVE) o[i] = img[i];
    }
  } else if (kind == KIND_GREY) {
    st = unfilter<1>(img, H, W, PlaneSink<1, COUT>{o, plane, W, 0}, lane);
  } else {
    st = unfilter<3>(img, H, W, PlaneSink<3, COUT>{o, plane, W, 0}, lane);
  }
  if (lane == 0) status[b] = st;
}

}  // namespace

extern "C" int yogo_png_unpack_planes(unsigned char* scan, long long scan_bytes, const long long* table, int B, int H, int W, int C_out,
                                      unsigned char* out, int* status, hipStream_t stream) {
  YOGO_CHECK_ARG(scan && table && out && status && scan_bytes > 0 && B >= 0, "png_unpack_planes: bad arguments");
  YOGO_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "png_unpack_planes: bad image shape %d x %d (1 .. 65535 each)", H, W);
  YOGO_CHECK_ARG(C_out == 1 || C_out == 3, "png_unpack_planes: C_out = %d output planes, 1 or 3", C_out);
  YOGO_CHECK_ARG(B <= 65535, "png_unpack_planes: B = %d images, at most 65535 per call", B);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "png_unpack_planes: the table must be 8-byte, the status 4-byte aligned");
  if (B == 0) return YOGO_OK;
  if (C_out == 3)
    hipLaunchKernelGGL(png_unpack_planes_kernel<3>, dim3(B), dim3(WAVE), 0, stream, scan, scan_bytes, table, H, W, out, status);
  else
    hipLaunchKernelGGL(png_unpack_planes_kernel<1>, dim3(B), dim3(WAVE), 0, stream, scan, scan_bytes, table, H, W, out, status);
  YOGO_CHECK_LAUNCH("png_unpack_planes");
  if (yogo_launch_log_enabled()) yogo_launch_log("png_unpack_planes_kernel<%d> | B=%d image=%dx%d", C_out, B, H, W);
  return YOGO_OK;
}

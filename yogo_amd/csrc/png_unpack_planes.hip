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
// The scheme is png_unpack.hip's: one wavefront per image takes 64 consecutive rows at a time, lane r on row r, skewed by one
// PIXEL per row -- at step t lane r makes pixel t - r of its row, the pixel above it is what lane r - 1 made one step earlier (one
// shuffle) and the upper-left one what that shuffle brought the step before.  A pixel of 3 bytes travels as one packed register
// (R in the low byte); the five filters act on each byte of it (the byte `bpp` to the left is the same channel of the pixel to the
// left).  Lane 63 writes its unfiltered row back to `scan` IN PLACE for the next band, which reads it 64 pixels at a time;
// __syncthreads() between two bands orders those stores before the loads.  The filtered bytes of a row are fetched four pixels per
// lane at a time, one fetch ahead of their use.  For kind 0 and C_out = 1 the arithmetic and the stores are png_unpack.hip's.
#include "common.h"

namespace {

constexpr int WAVE = 64;
enum : int { ST_OK = 0, ST_BAD_FILTER = 1, ST_BAD_IMAGE = 2 };
enum : long long { KIND_GREY = 0, KIND_PLANAR = 1, KIND_RGB = 2 };

// pixels x0 .. x0 + 3 of the row at p (W pixels of BPP bytes), one packed pixel per element; zero outside the row
template <int BPP>
__device__ __forceinline__ void fetch4(const unsigned char* p, int x0, int W, bool active, unsigned (&px)[4]) {
  px[0] = px[1] = px[2] = px[3] = 0;
  if (!active || x0 >= W || x0 + 3 < 0) return;
  if (x0 >= 0 && x0 + 4 <= W) {
    unsigned w[BPP];
    __builtin_memcpy(w, p + x0 * BPP, 4 * BPP);
    if constexpr (BPP == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) px[k] = (w[0] >> (8 * k)) & 255u;
    } else {
      px[0] = w[0] & 0xffffffu;
      px[1] = (w[0] >> 24) | ((w[BPP - 2] & 0xffffu) << 8);
      px[2] = (w[BPP - 2] >> 16) | ((w[BPP - 1] & 0xffu) << 16);
      px[3] = w[BPP - 1] >> 8;
    }
  } else {
    for (int k = 0; k < 4; ++k)
      if (x0 + k >= 0 && x0 + k < W)
        for (int j = 0; j < BPP; ++j) px[k] |= (unsigned)p[(x0 + k) * BPP + j] << (8 * j);
  }
}

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

// the scanlines at img (H rows of 1 + BPP * W bytes, all inside scan) -> out (COUT planes of H x W); ST_OK or ST_BAD_FILTER
template <int BPP, int COUT>
__device__ __forceinline__ int unfilter(unsigned char* img, int H, int W, unsigned char* out, int lane) {
  const int stride = BPP * W + 1;
  const long long plane = (long long)H * W;
  for (int band = 0; band < H; band += WAVE) {
    const int y = band + lane;
    const bool active = y < H;
    unsigned char* rowp = img + (long long)(active ? y : 0) * stride + 1;
    const int ft = active ? rowp[-1] : 0;
    if (__ballot(ft > 4)) return ST_BAD_FILTER;
    const unsigned char* abovep = band ? img + (long long)(band - 1) * stride + 1 : nullptr;
    unsigned cur = 0, upleft = 0, abv = 0;   // what this lane made last step; what the shuffle brought last step; lane 0's row above
    unsigned next[4];
    fetch4<BPP>(rowp, -lane, W, active, next);
    for (int t0 = 0; t0 < W + WAVE - 1; t0 += 4) {
      if ((t0 & (WAVE - 1)) == 0) {
        abv = 0;
        if (abovep && t0 + lane < W)
          for (int j = 0; j < BPP; ++j) abv |= (unsigned)abovep[(t0 + lane) * BPP + j] << (8 * j);
      }
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = next[k];
      fetch4<BPP>(rowp, t0 + 4 - lane, W, active, next);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t = t0 + k, x = t - lane;
        unsigned up = (unsigned)__shfl_up((int)cur, 1);
        const unsigned first_up = (unsigned)__builtin_amdgcn_readlane((int)abv, t & (WAVE - 1));
        if (lane == 0) up = first_up;
        const bool valid = active && x >= 0 && x < W;
        unsigned val = 0;
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int a = (int)((cur >> (8 * j)) & 255u), bb = (int)((up >> (8 * j)) & 255u), c = (int)((upleft >> (8 * j)) & 255u);
          int pred = 0;
          if (ft == 1) pred = a;
          else if (ft == 2) pred = bb;
          else if (ft == 3) pred = (a + bb) >> 1;
          else if (ft == 4) {
            const int pa = abs(bb - c), pb = abs(a - c), pc = abs(a + bb - 2 * c);
            pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c);
          }
          val |= ((((w[k] >> (8 * j)) & 255u) + (unsigned)pred) & 255u) << (8 * j);
        }
        upleft = up;
        cur = valid ? val : 0u;
        if (valid) {
          if (lane == WAVE - 1) {
#pragma unroll
            for (int j = 0; j < BPP; ++j) rowp[x * BPP + j] = (unsigned char)(val >> (8 * j));
          }
          emit<BPP, COUT>(out, plane, (long long)y * W + x, val);
        }
      }
    }
    __syncthreads();   // lane 63's row is visible to the loads of the next band
  }
  return ST_OK;
}

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
    st = unfilter<1, COUT>(img, H, W, o, lane);
  } else {
    st = unfilter<3, COUT>(img, H, W, o, lane);
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

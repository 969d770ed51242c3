// The inflated scanlines of 8-bit greyscale PNG files -> image batches on the device (yogo_amd/png_feed.py, behind inflate.hip):
// the PNG filters reversed, the centre crop and the optional / 255 in one launch.
//   table[b] = { off, raw }   (int64 each)
// off: where image b lies in `scan`; raw == 0: H scanlines of 1 + W bytes, the filter-type byte first; raw != 0: H x W pixels as
// they are (an image the host decoded).  out: [B][1][OH][OW] uint8 or fp32 x / 255 (bit-identical to torch's CPU
// uint8_tensor / 255: build.sh compiles with correctly rounded division), out[b][0][oy][ox] = image_b[top + oy][left + ox].
// status[b] = 0, 1 (a filter-type byte above 4) or 2 (the image does not lie inside scan: nothing of it was read).
//
// Filters (bytes per pixel = 1, the row above row 0 is zeros, arithmetic mod 256): 0 None, 1 Sub (+ left), 2 Up (+ above),
// 3 Average (+ floor((left + above) / 2)), 4 Paeth (+ whichever of left, above, upper-left is nearest left + above - upper-left,
// ties in that order).  Sub, Average and Paeth are serial along a row, Up, Average and Paeth need the row above: one wavefront
// per image takes 64 consecutive rows at a time, lane r on row r, skewed by one pixel per row -- at step t lane r makes pixel
// t - r of its row, so that the pixel above it is what lane r - 1 made one step earlier (one DPP-style shuffle) and the
// upper-left one is what that shuffle brought the step before.  Every mix of filter types keeps the 64 lanes busy; a band of 64
// rows costs W + 63 steps.  Lane 0's row above is the last row of the band before: lane 63 writes its unfiltered pixels back to
// `scan` IN PLACE (only that row of each band is written back; `scan` is not left whole), and the wave reads them 64 at a time.
// __syncthreads() between two bands orders those stores before the loads, as in blosc_lz4.hip.  The filtered bytes of a row are
// fetched four pixels per lane at a time, one fetch ahead of their use.
#include "common.h"

namespace {

constexpr int WAVE = 64;
enum : int { ST_OK = 0, ST_BAD_FILTER = 1, ST_BAD_IMAGE = 2 };

template <bool FP32>
__device__ __forceinline__ void put(void* out, long long i, unsigned v) {
  if (FP32) static_cast<float*>(out)[i] = (float)v / 255.f;
  else static_cast<unsigned char*>(out)[i] = (unsigned char)v;
}

// pixels x0 .. x0 + 3 of the row at p (W bytes), one per byte of the result; zero outside the row
__device__ __forceinline__ unsigned fetch4(const unsigned char* p, int x0, int W, bool active) {
  unsigned w = 0;
  if (!active || x0 >= W || x0 + 3 < 0) return 0;
  if (x0 >= 0 && x0 + 4 <= W) {
    __builtin_memcpy(&w, p + x0, 4);
  } else {
    for (int k = 0; k < 4; ++k)
      if (x0 + k >= 0 && x0 + k < W) w |= (unsigned)p[x0 + k] << (8 * k);
  }
  return w;
}

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
  const int stride = W + 1;
  int st = ST_OK;
  for (int band = 0; band < H; band += WAVE) {
    const int y = band + lane;
    const bool active = y < H;
    unsigned char* rowp = scan + off + (long long)(active ? y : 0) * stride + 1;
    const int ft = active ? rowp[-1] : 0;
    if (__ballot(ft > 4)) {
      st = ST_BAD_FILTER;
      break;
    }
    const unsigned char* abovep = band ? scan + off + (long long)(band - 1) * stride + 1 : nullptr;
    const int oy = y - top;
    const bool row_out = active && oy >= 0 && oy < OH;
    unsigned cur = 0, upleft = 0, abv = 0;   // what this lane made last step; what the shuffle brought last step; lane 0's row above
    unsigned next = fetch4(rowp, -lane, W, active);
    for (int t0 = 0; t0 < W + WAVE - 1; t0 += 4) {
      if ((t0 & (WAVE - 1)) == 0) abv = abovep && t0 + lane < W ? abovep[t0 + lane] : 0u;
      const unsigned w = next;
      next = fetch4(rowp, t0 + 4 - lane, W, active);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t = t0 + k, x = t - lane;
        unsigned up = (unsigned)__shfl_up((int)cur, 1);
        const unsigned first_up = (unsigned)__builtin_amdgcn_readlane((int)abv, t & (WAVE - 1));
        if (lane == 0) up = first_up;
        const bool valid = active && x >= 0 && x < W;
        const int a = (int)cur, bb = (int)up, c = (int)upleft;
        int pred = 0;
        if (ft == 1) pred = a;
        else if (ft == 2) pred = bb;
        else if (ft == 3) pred = (a + bb) >> 1;
        else if (ft == 4) {
          const int pa = abs(bb - c), pb = abs(a - c), pc = abs(a + bb - 2 * c);
          pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c);
        }
        const unsigned val = (((w >> (8 * k)) & 255u) + (unsigned)pred) & 255u;
        upleft = up;
        cur = valid ? val : 0u;
        if (valid) {
          if (lane == WAVE - 1) rowp[x] = (unsigned char)val;
          const int ox = x - left;
          if (row_out && ox >= 0 && ox < OW) put<FP32>(out, obase + (long long)oy * OW + ox, val);
        }
      }
    }
    __syncthreads();   // lane 63's row is visible to the loads of the next band
  }
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

// The inflated scanlines of PNG files of EVERY colour type, bit depth and interlace method -> image batches or cache frames on the
// device (yogo_amd/png_feed.py and yogo_amd/png_prefill.py under --device-image-decode-all, behind inflate.hip): the PNG filters
// reversed, Adam7 undone, the file's samples converted to 1 or 3 planes of 8 bits, the centre crop and the optional / 255 in one
// launch; the images of a launch may each be of another format.
//   table[b] = { off, fmt, pal }   (int64 each)
// off: where image b lies in `scan`.  fmt = colour type | bit depth << 8 | interlace << 16 (IHDR's three fields; the pairs the PNG
// specification allows: 0 at 1 2 4 8 16, 2 at 8 16, 3 at 1 2 4 8, 4 and 6 at 8 16; interlace 0 or 1): the scanlines as the file's
// zlib stream inflates to -- rows of one filter-type byte and ceil(w * channels * depth / 8) bytes, for Adam7 the seven reduced
// images one after the other, a pass without pixels without scanlines.  fmt = 1 (no colour type): C_out x H x W planar pixels as
// they are (an image the host decoded), kind 1 of png_unpack_planes.hip.  pal: for colour type 3 where the image's palette lies in
// `scan`, 256 x 3 bytes R G B (the host pads a shorter PLTE with zeros); ignored otherwise.
// The conversions are those of yogo_amd.yogo_dataset.read_image(path, rgb) (PIL), restated in yogo_amd.png.decode_any:
//   grey 1 / 2 / 4: v * 255 / (2^depth - 1);  grey 8: as it is;  grey 16: min(v, 255) (PIL's I;16 -> L clips, it does not shift);
//   grey+alpha, RGB, RGBA at 8 / 16: the high byte of each sample, alpha dropped;  palette: PLTE[index];
//   one plane from colour: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;  three planes from grey: the plane three times.
// tRNS, gAMA, sBIT and a PLTE in a file that is not of colour type 3 change nothing.
// out: [B][C_out][OH][OW] uint8 or fp32 x / 255 (bit-identical to torch's CPU uint8_tensor / 255: build.sh compiles with correctly
// rounded division), out[b][c][oy][ox] = image_b[c][top + oy][left + ox].  status[b] = 0, 1 (a filter-type byte above 4, in any
// pass) or 2 (an unknown fmt, or the image or its palette does not lie inside scan: nothing of it was read).
//
// The filters are reversed by csrc/png_unfilter.h's loop at max(1, channels * depth / 8) = 1, 2, 3, 4, 6 or 8 bytes per pixel (one
// wavefront per image; `scan` is WRITTEN: the last row of every band of 64 is unfiltered in place), once per Adam7 pass over that
// pass's reduced image; this file says where a pixel goes: expand (depths below 8: the loop runs over the row's bytes), scatter
// (x0 + dx x, y0 + dy y), convert, crop and put.
#include "png_unfilter.h"

namespace {

using namespace yogo_png;

constexpr long long FMT_PLANAR = 1;
constexpr int PALETTE_BYTES = 768;
enum : int { M_GREY = 0, M_GREY16 = 1, M_PAL = 2, M_RGB = 3 };

template <bool FP32>
__device__ __forceinline__ void put(void* out, long long i, unsigned v) {
  if (FP32) static_cast<float*>(out)[i] = (float)v / 255.f;
  else static_cast<unsigned char*>(out)[i] = (unsigned char)v;
}

// Adam7 pass p (0 .. 6): first column, first row, column step, row step (a nibble each); the whole image is { 0, 0, 1, 1 }
__device__ __forceinline__ int adam7_x0(int p) { return (0x0102040u >> (4 * p)) & 15; }
__device__ __forceinline__ int adam7_y0(int p) { return (0x1020400u >> (4 * p)) & 15; }
__device__ __forceinline__ int adam7_dx(int p) { return (0x1224488u >> (4 * p)) & 15; }
__device__ __forceinline__ int adam7_dy(int p) { return (0x2244888u >> (4 * p)) & 15; }

__device__ __forceinline__ int channels_of(int ct) { return ct == 2 ? 3 : ct == 4 ? 2 : ct == 6 ? 4 : 1; }

__device__ __forceinline__ bool format_ok(int ct, int depth, long long lace) {
  if (lace != 0 && lace != 1) return false;
  if (ct == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
  if (ct == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
  if (ct == 2 || ct == 4 || ct == 6) return depth == 8 || depth == 16;
  return false;
}

// a unit of the unfilter loop (a pixel of BPP bytes; at depths below 8 a byte of 8 / depth pixels) of the reduced image
// (x0, y0, dx, dy; pw pixels wide) into the crop of the whole one
template <int BPP, int COUT, bool FP32>
struct AnySink {
  void* out;
  long long obase, plane;   // of image b; OH * OW
  int top, left, OH, OW;
  int mode, depth;
  unsigned scale;           // of a grey sample: 255 / (2^depth - 1) below 8 bits, else 1
  const unsigned char* pal;
  int x0, dx, y0, dy, pw;
  long long orow;
  bool row_out;
  __device__ __forceinline__ void row(int y, bool active) {
    const int oy = y0 + dy * y - top;
    row_out = active && oy >= 0 && oy < OH;
    orow = obase + (long long)oy * OW;
  }
  // sample(s) s of pixel px of the reduced row
  __device__ __forceinline__ void put1(int px, pix_t<BPP> s) const {
    const int ox = x0 + dx * px - left;
    if (ox < 0 || ox >= OW) return;
    const long long i = orow + ox;
    constexpr int STEP = BPP >= 6 ? 2 : 1;   // bytes per sample
    unsigned r = 0, g = 0, b = 0;
    bool colour = false;
    if (BPP == 1 && mode == M_PAL) {
      const unsigned char* e = pal + 3 * ((unsigned)s & 255u);
      r = e[0], g = e[1], b = e[2], colour = true;
    } else if (BPP >= 3 && mode == M_RGB) {
      r = (unsigned)s & 255u, g = (unsigned)(s >> (8 * STEP)) & 255u, b = (unsigned)(s >> (16 * STEP)) & 255u, colour = true;
    } else if (BPP == 2 && mode == M_GREY16) {
      g = ((unsigned)s & 255u) ? 255u : ((unsigned)s >> 8) & 255u;   // big-endian: the low byte of s is the sample's high one
    } else {
      g = ((unsigned)s & 255u) * scale;
    }
    if (colour && COUT == 1) {
      put<FP32>(out, i, (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16);
    } else if (colour) {
      put<FP32>(out, i, r);
      put<FP32>(out, i + plane, g);
      put<FP32>(out, i + 2 * plane, b);
    } else {
#pragma unroll
      for (int c = 0; c < COUT; ++c) put<FP32>(out, i + c * plane, g);
    }
  }
  __device__ __forceinline__ void pixel(int x, pix_t<BPP> v) const {
    if (!row_out) return;
    if (BPP == 1 && depth < 8) {
      // most significant bits first; the padding bits of the row's last byte are dropped
      const int n = 8 / depth;
      const unsigned mask = (1u << depth) - 1u;
      for (int k = 0; k < n && x * n + k < pw; ++k) put1(x * n + k, (pix_t<BPP>)(((unsigned)v >> (8 - depth * (k + 1))) & mask));
    } else {
      put1(x, v);
    }
  }
};

// the scanlines at img, H x W pixels of `bits` bits, interlaced or not -> status
template <int BPP, int COUT, bool FP32>
__device__ __forceinline__ int unpack_image(unsigned char* img, int H, int W, int bits, bool lace, AnySink<BPP, COUT, FP32> sink, int lane) {
  int st = ST_OK;
  for (int p = 0; p < (lace ? 7 : 1) && st == ST_OK; ++p) {
    sink.x0 = lace ? adam7_x0(p) : 0, sink.y0 = lace ? adam7_y0(p) : 0, sink.dx = lace ? adam7_dx(p) : 1, sink.dy = lace ? adam7_dy(p) : 1;
    if (W <= sink.x0 || H <= sink.y0) continue;   // a pass without pixels has no scanlines
    const int pw = (W - sink.x0 + sink.dx - 1) / sink.dx, ph = (H - sink.y0 + sink.dy - 1) / sink.dy;
    const int row_bytes = (pw * bits + 7) >> 3;
    sink.pw = pw;
    st = unfilter<BPP>(img, ph, row_bytes / BPP, sink, lane);
    img += (long long)ph * (row_bytes + 1);
  }
  return st;
}

template <int COUT, bool FP32>
__global__ __launch_bounds__(WAVE) void png_unpack_any_kernel(unsigned char* scan, long long scan_bytes, const long long* __restrict__ table,
                                                              int H, int W, int top, int left, int OH, int OW, void* out,
                                                              int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long off = table[3LL * b], fmt = table[3LL * b + 1], pal = table[3LL * b + 2];
  const int ct = (int)(fmt & 255), depth = (int)((fmt >> 8) & 255);
  const long long lace = fmt >> 16;
  const bool planar = fmt == FMT_PLANAR;
  const int bits = channels_of(ct) * depth;
  bool ok = planar || (fmt >= 0 && format_ok(ct, depth, lace));
  long long need = 0;
  if (planar) {
    need = (long long)COUT * H * W;
  } else if (ok) {
    for (int p = 0; p < (lace ? 7 : 1); ++p) {
      const int x0 = lace ? adam7_x0(p) : 0, y0 = lace ? adam7_y0(p) : 0, dx = lace ? adam7_dx(p) : 1, dy = lace ? adam7_dy(p) : 1;
      if (W <= x0 || H <= y0) continue;
      const long long pw = (W - x0 + dx - 1) / dx, ph = (H - y0 + dy - 1) / dy;
      need += ph * (((pw * bits + 7) >> 3) + 1);
    }
  }
  ok = ok && off >= 0 && off <= scan_bytes && need <= scan_bytes - off;
  if (ok && !planar && ct == 3) ok = pal >= 0 && pal <= scan_bytes - PALETTE_BYTES;
  if (!ok) {
    if (lane == 0) status[b] = ST_BAD_IMAGE;
    return;
  }
  const long long plane = (long long)OH * OW, obase = (long long)b * COUT * plane;
  unsigned char* img = scan + off;
  if (planar) {
    for (int c = 0; c < COUT; ++c)
      for (int i = lane; i < OH * OW; i += WAVE) {   // (OH * OW < 2^31: the entry point checks)
        const int oy = i / OW, ox = i - oy * OW;
        put<FP32>(out, obase + c * plane + i, img[((long long)c * H + top + oy) * W + left + ox]);
      }
    if (lane == 0) status[b] = ST_OK;
    return;
  }
  const int mode = ct == 3 ? M_PAL : (ct == 2 || ct == 6) ? M_RGB : (ct == 0 && depth == 16) ? M_GREY16 : M_GREY;
  const unsigned scale = depth < 8 ? 255u / ((1u << depth) - 1u) : 1u;
  const unsigned char* palp = ct == 3 ? scan + pal : scan;
  const bool il = lace != 0;
  int st;
#define YOGO_PNG_ANY(BPP) \
  st = unpack_image<BPP, COUT, FP32>(img, H, W, bits, il, AnySink<BPP, COUT, FP32>{out, obase, plane, top, left, OH, OW, mode, depth, scale, palp, 0, 1, 0, 1, W, 0, false}, lane)
  switch (bits >> 3) {
    case 2: YOGO_PNG_ANY(2); break;
    case 3: YOGO_PNG_ANY(3); break;
    case 4: YOGO_PNG_ANY(4); break;
    case 6: YOGO_PNG_ANY(6); break;
    case 8: YOGO_PNG_ANY(8); break;
    default: YOGO_PNG_ANY(1); break;   // 8 bits or fewer per pixel
  }
#undef YOGO_PNG_ANY
  if (lane == 0) status[b] = st;
}

}  // namespace

extern "C" int yogo_png_unpack_any(unsigned char* scan, long long scan_bytes, const long long* table, int B, int H, int W, int top, int left,
                                   int OH, int OW, int C_out, void* out, int out_fp32, int* status, hipStream_t stream) {
  YOGO_CHECK_ARG(scan && table && out && status && scan_bytes > 0 && B >= 0, "png_unpack_any: bad arguments");
  YOGO_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "png_unpack_any: bad image shape %d x %d (1 .. 65535 each)", H, W);
  YOGO_CHECK_ARG(top >= 0 && left >= 0 && top < H && left < W, "png_unpack_any: crop origin (%d, %d) outside the %d x %d image", top, left, H, W);
  YOGO_CHECK_ARG(OH >= 1 && OH <= H - top && OW >= 1 && OW <= W - left, "png_unpack_any: a %d x %d crop at (%d, %d) of a %d x %d image", OH,
                 OW, top, left, H, W);
  YOGO_CHECK_ARG(C_out == 1 || C_out == 3, "png_unpack_any: C_out = %d output planes, 1 or 3", C_out);
  YOGO_CHECK_ARG(B <= 65535, "png_unpack_any: B = %d images, at most 65535 per call", B);
  YOGO_CHECK_ARG(out_fp32 == 0 || out_fp32 == 1, "png_unpack_any: out_fp32 must be 0 (uint8) or 1 (float32)");
  YOGO_CHECK_ARG((long long)OH * OW < (1LL << 31), "png_unpack_any: a crop of %d x %d pixels", OH, OW);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0 &&
                     (!out_fp32 || (reinterpret_cast<uintptr_t>(out) & 3) == 0),
                 "png_unpack_any: the table must be 8-byte, the status and an fp32 output 4-byte aligned");
  if (B == 0) return YOGO_OK;
#define YOGO_PNG_ANY_LAUNCH(C, F) \
  hipLaunchKernelGGL((png_unpack_any_kernel<C, F>), dim3(B), dim3(WAVE), 0, stream, scan, scan_bytes, table, H, W, top, left, OH, OW, out, status)
  if (C_out == 3 && out_fp32) YOGO_PNG_ANY_LAUNCH(3, true);
  else if (C_out == 3) YOGO_PNG_ANY_LAUNCH(3, false);
  else if (out_fp32) YOGO_PNG_ANY_LAUNCH(1, true);
  else YOGO_PNG_ANY_LAUNCH(1, false);
#undef YOGO_PNG_ANY_LAUNCH
  YOGO_CHECK_LAUNCH("png_unpack_any");
  if (yogo_launch_log_enabled())
    yogo_launch_log("png_unpack_any_kernel<%d,%s> | B=%d image=%dx%d crop=%dx%d@(%d,%d)", C_out, out_fp32 ? "f32" : "u8", B, H, W, OH, OW, top,
                    left);
  return YOGO_OK;
}

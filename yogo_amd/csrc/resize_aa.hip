// Antialiased bilinear (triangle filter) resampling of planar uint8 images, separable: what yogo_amd.yogo_dataset.resize_image
// computes (torch._upsample_bilinear2d_aa, align_corners = False, then round-half-even and a clamp to 0 .. 255) for the images the
// device image cache is filled with when their files have another size than the cache (yogo_amd/png_prefill.py, `yogo train
// --device-image-resize`).  src: [n][C][Hs][Ws] uint8, dst: [N][C][Hd][Wd] uint8; image k goes to dst[dst_index[k]].
//
// The taps come from the host (yogo_amd/resize.py, aa_taps), per axis start[n_out] (int32) and weights[n_out][K] (fp32, zero-padded
// to K), packed into one buffer of which the entry point gets the host copy -- which it checks -- and the device copy:
//   int64 dst_index[n] | int32 start_y[Hd] | int32 start_x[Wd] | float wy[Hd][Ky] | float wx[Wd][Kx]
//
// Arithmetic: the horizontal pass first, into an fp32 intermediate, then the vertical pass, as torch does; every sum starts at 0 and
// runs in ascending tap order with fmaf; rintf (half-even), then the clamp.  A padded tap has weight 0 and reads a clamped index:
// fmaf(0, v, acc) = acc.
//
// A workgroup takes one (image, plane, TH x 64 output tile): it stages the source rows and columns the tile needs in LDS as bytes
// (4 per lane and load when Ws and src are 4-byte aligned, one otherwise), runs the horizontal pass into an fp32 LDS tile [rows][64],
// and the vertical pass out of it with 16-byte LDS reads, 4 output pixels per lane, one 4-byte store each: a 16-lane group stores a
// whole 64-byte row piece.  TH is sized on the host from the tables' own spans so that the workgroup's LDS stays within LDS_BUDGET
// (32 KiB of the CU's 160 KiB: 5 workgroups = 20 of 32 waves per CU): 32 rows for an exact 2 x down-scale (K = 4: 66 x 136 source bytes
// + 66 x 64 floats = 25.5 KiB, 6 workgroups per CU) and for up-scaling (K <= 3), 4 to 8 rows near 8 x (K = 16 or 17).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int TW = 64;                 // output columns per tile: 16 lanes x 4 pixels
constexpr int MAX_TAPS = 18;           // above the K of an 8 x down-scale (2 * 8 + 1)
constexpr int MAX_DOWNSCALE = 8;
constexpr int LDS_BUDGET = 32 * 1024;

struct Tile {
  int TH, SH, SWp;   // output rows per tile; the most source rows a tile needs; the byte pitch of a staged source row (a multiple of 4)
};

__host__ __device__ inline int lds_floats(int Ky, int Kx, const Tile& t) { return t.SH * TW + Kx * TW + Ky * t.TH; }
__host__ __device__ inline int lds_bytes(int Ky, int Kx, const Tile& t) {
  return 4 * (lds_floats(Ky, Kx, t) + TW + t.TH) + t.SH * t.SWp;
}

__device__ __forceinline__ unsigned to_u8(float v) { return (unsigned)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// grid (tiles_x * tiles_y, C, n)
template <bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void resize_aa_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                          const long long* __restrict__ dst_index, const int* __restrict__ start_y,
                                                          const int* __restrict__ start_x, const float* __restrict__ wy,
                                                          const float* __restrict__ wx, int C, int Hs, int Ws, int Hd, int Wd, int Ky,
                                                          int Kx, Tile tile, int tiles_x, int vec_store) {
  extern __shared__ uint4 lds_raw[];
  const int TH = tile.TH, SWp = tile.SWp;
  float* s_int = reinterpret_cast<float*>(lds_raw);   // [SH][TW]
  float* s_wx = s_int + tile.SH * TW;                 // [Kx][TW]
  float* s_wy = s_wx + Kx * TW;                       // [TH][Ky]
  int* s_sx = reinterpret_cast<int*>(s_wy + Ky * TH); // [TW]
  int* s_sy = s_sx + TW;                              // [TH]
  unsigned char* s_src = reinterpret_cast<unsigned char*>(s_sy + TH);   // [SH][SWp]

  const int t = threadIdx.x;
  const int x0 = (int)(blockIdx.x % tiles_x) * TW, y0 = (int)(blockIdx.x / tiles_x) * TH;
  const int nx = min(TW, Wd - x0), ny = min(TH, Hd - y0);
  const int c = blockIdx.y, k = blockIdx.z;
  const int xs0 = start_x[x0], xs1 = min(Ws, start_x[x0 + nx - 1] + Kx);
  const int ys0 = start_y[y0], ys1 = min(Hs, start_y[y0 + ny - 1] + Ky);
  const int SH = ys1 - ys0, SW = xs1 - xs0;

  // the tile's taps; a column or row past the image's edge gets weight 0
  if (t < TW) {
    const bool in = t < nx;
    s_sx[t] = in ? start_x[x0 + t] - xs0 : 0;
    for (int j = 0; j < Kx; ++j) s_wx[j * TW + t] = in ? wx[(long long)(x0 + t) * Kx + j] : 0.f;
  }
  for (int y = t; y < TH; y += BLOCK) {
    const bool in = y < ny;
    s_sy[y] = in ? start_y[y0 + y] - ys0 : 0;
    for (int j = 0; j < Ky; ++j) s_wy[y * Ky + j] = in ? wy[(long long)(y0 + y) * Ky + j] : 0.f;
  }
  // the source rows ys0 .. ys1 - 1, columns xs0 .. xs1 - 1 (ALIGNED: from the 4-byte boundary at or below xs0, whole words: Ws is a
  // multiple of 4, so the last word ends inside the row)
  const unsigned char* plane = src + ((long long)k * C + c) * Hs * (long long)Ws;
  int shift = 0;
  if (ALIGNED) {
    const int xa0 = xs0 & ~3;
    shift = xs0 - xa0;
    const int ndw = (xs1 - xa0 + 3) >> 2;
    for (int i = t; i < SH * ndw; i += BLOCK) {
      const int r = i / ndw, d = i - r * ndw;
      reinterpret_cast<unsigned*>(s_src)[r * (SWp >> 2) + d] =
          *reinterpret_cast<const unsigned*>(plane + (long long)(ys0 + r) * Ws + xa0 + 4 * d);
    }
  } else {
    for (int i = t; i < SH * SW; i += BLOCK) {
      const int r = i / SW, d = i - r * SW;
      s_src[r * SWp + d] = plane[(long long)(ys0 + r) * Ws + xs0 + d];
    }
  }
  __syncthreads();

  // horizontal: s_int[r][x] for every staged row (BLOCK is a multiple of TW: a lane keeps its column)
  {
    const int x = t & (TW - 1);
    const int sx = s_sx[x] + shift, lim = SW - 1 + shift;
    for (int r = t / TW; r < SH; r += BLOCK / TW) {
      const unsigned char* row = s_src + r * SWp;
      float acc = 0.f;
      for (int j = 0; j < Kx; ++j) acc = fmaf(s_wx[j * TW + x], (float)row[min(sx + j, lim)], acc);
      s_int[r * TW + x] = acc;
    }
  }
  __syncthreads();

  // vertical: 4 pixels of one output row per lane
  unsigned char* out = dst + (dst_index[k] * C + c) * Hd * (long long)Wd;
  for (int i = t; i < ny * (TW / 4); i += BLOCK) {
    const int y = i / (TW / 4), q = i % (TW / 4);
    const int gx = x0 + 4 * q;
    if (gx >= Wd) continue;
    const int sy = s_sy[y], lim = SH - 1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < Ky; ++j) {
      const float w = s_wy[y * Ky + j];
      const float4 v = *reinterpret_cast<const float4*>(s_int + min(sy + j, lim) * TW + 4 * q);
      acc.x = fmaf(w, v.x, acc.x);
      acc.y = fmaf(w, v.y, acc.y);
      acc.z = fmaf(w, v.z, acc.z);
      acc.w = fmaf(w, v.w, acc.w);
    }
    const unsigned p[4] = {to_u8(acc.x), to_u8(acc.y), to_u8(acc.z), to_u8(acc.w)};
    unsigned char* o = out + (long long)(y0 + y) * Wd + gx;
    if (vec_store) {   // (Wd a multiple of 4: the four pixels are inside the row)
      *reinterpret_cast<unsigned*>(o) = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
    } else {
      for (int e = 0; e < 4; ++e)
        if (gx + e < Wd) o[e] = (unsigned char)p[e];
    }
  }
}

// one axis' table: every tap with a weight inside [0, n_in), starts ascending, weights in [0, 1] summing to 1
const char* check_axis(const int* start, const float* w, int K, int n_in, int n_out) {
  int prev = 0;
  for (int i = 0; i < n_out; ++i) {
    const int s = start[i];
    if (s < prev || s >= n_in) return "a start index is outside the source or below the one before it";
    prev = s;
    double sum = 0.0;
    for (int j = 0; j < K; ++j) {
      const float v = w[(long long)i * K + j];
      if (!(v >= 0.f && v <= 1.f)) return "a weight is outside [0, 1]";
      if (v != 0.f && s + j >= n_in) return "a tap with a weight lies past the end of the source";
      sum += v;
    }
    if (std::fabs(sum - 1.0) > 1e-4) return "the weights of an output do not sum to 1";
  }
  return nullptr;
}

// the most source indices one tile of T outputs spans
int max_span(const int* start, int K, int n_in, int n_out, int T) {
  int span = 0;
  for (int i0 = 0; i0 < n_out; i0 += T) {
    const int i1 = std::min(n_out, i0 + T) - 1;
    span = std::max(span, std::min(n_in, start[i1] + K) - start[i0]);
  }
  return span;
}

}  // namespace

extern "C" int yogo_resize_aa_u8(const unsigned char* src, int n, int C, int Hs, int Ws, unsigned char* dst, int N, int Hd, int Wd,
                                 const void* tables_host, const void* tables_dev, int Ky, int Kx, hipStream_t stream) {
  YOGO_CHECK_ARG(src && dst && tables_host && tables_dev && n >= 0 && N >= 1, "resize_aa_u8: bad arguments");
  YOGO_CHECK_ARG(C >= 1 && C <= 65535 && n <= 65535, "resize_aa_u8: n = %d images of C = %d planes, 1 .. 65535 each per call", n, C);
  YOGO_CHECK_ARG(Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1 && Hs <= 65535 && Ws <= 65535 && Hd <= 65535 && Wd <= 65535,
                 "resize_aa_u8: bad image shapes %d x %d -> %d x %d (1 .. 65535 each)", Hs, Ws, Hd, Wd);
  YOGO_CHECK_ARG(Hs <= MAX_DOWNSCALE * Hd && Ws <= MAX_DOWNSCALE * Wd,
                 "resize_aa_u8: %d x %d -> %d x %d scales down by more than %d", Hs, Ws, Hd, Wd, MAX_DOWNSCALE);
  YOGO_CHECK_ARG(Ky >= 1 && Kx >= 1 && Ky <= MAX_TAPS && Kx <= MAX_TAPS, "resize_aa_u8: Ky = %d, Kx = %d taps, 1 .. %d each", Ky, Kx, MAX_TAPS);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(tables_host) & 7) == 0 && (reinterpret_cast<uintptr_t>(tables_dev) & 7) == 0,
                 "resize_aa_u8: the tables must be 8-byte aligned");
  if (n == 0) return YOGO_OK;
  // the packed tables, on the host (checked here) and on the device (read by the kernel)
  const long long* index_h = static_cast<const long long*>(tables_host);
  const int* sy_h = reinterpret_cast<const int*>(index_h + n);
  const int* sx_h = sy_h + Hd;
  const float* wy_h = reinterpret_cast<const float*>(sx_h + Wd);
  const float* wx_h = wy_h + (long long)Hd * Ky;
  std::vector<long long> seen(index_h, index_h + n);
  std::sort(seen.begin(), seen.end());
  YOGO_CHECK_ARG(seen.front() >= 0 && seen.back() < N, "resize_aa_u8: dst_index %lld .. %lld outside the %d destination images",
                 seen.front(), seen.back(), N);
  YOGO_CHECK_ARG(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "resize_aa_u8: two images go to the same destination");
  const char* bad = check_axis(sy_h, wy_h, Ky, Hs, Hd);
  YOGO_CHECK_ARG(!bad, "resize_aa_u8: the vertical table: %s", bad);
  bad = check_axis(sx_h, wx_h, Kx, Ws, Wd);
  YOGO_CHECK_ARG(!bad, "resize_aa_u8: the horizontal table: %s", bad);
  // the tallest tile whose LDS fits the budget (ALIGNED staging starts up to 3 bytes early and ends up to 3 late)
  Tile tile{0, 0, round_up(max_span(sx_h, Kx, Ws, Wd, TW) + 6, 4)};
  for (int th = 32; th >= 1; th >>= 1) {
    const Tile cand{th, max_span(sy_h, Ky, Hs, Hd, th), tile.SWp};
    if (lds_bytes(Ky, Kx, cand) <= LDS_BUDGET) {
      tile = cand;
      break;
    }
  }
  YOGO_CHECK_ARG(tile.TH > 0, "resize_aa_u8: the tables span more source than a tile holds (%d bytes per staged row)", tile.SWp);
  const int tiles_x = cdiv(Wd, TW);
  const long long tiles = (long long)tiles_x * cdiv(Hd, tile.TH);
  const bool aligned = Ws % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
  const int vec_store = Wd % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  const long long* index_d = static_cast<const long long*>(tables_dev);
  const int* sy_d = reinterpret_cast<const int*>(index_d + n);
  const int* sx_d = sy_d + Hd;
  const float* wy_d = reinterpret_cast<const float*>(sx_d + Wd);
  const float* wx_d = wy_d + (long long)Hd * Ky;
  const dim3 grid((unsigned)tiles, C, n);
  const int lds = lds_bytes(Ky, Kx, tile);
  if (aligned)
    hipLaunchKernelGGL(resize_aa_kernel<true>, grid, dim3(BLOCK), lds, stream, src, dst, index_d, sy_d, sx_d, wy_d, wx_d, C, Hs, Ws, Hd, Wd,
                       Ky, Kx, tile, tiles_x, vec_store);
  else
    hipLaunchKernelGGL(resize_aa_kernel<false>, grid, dim3(BLOCK), lds, stream, src, dst, index_d, sy_d, sx_d, wy_d, wx_d, C, Hs, Ws, Hd, Wd,
                       Ky, Kx, tile, tiles_x, vec_store);
  YOGO_CHECK_LAUNCH("resize_aa_u8");
  if (yogo_launch_log_enabled())
    yogo_launch_log("resize_aa_kernel<%s> | n=%d C=%d %dx%d->%dx%d K=%dx%d tile=%dx%d rows=%d pitch=%d lds=%d vec=%d", aligned ? "words" : "bytes",
                    n, C, Hs, Ws, Hd, Wd, Ky, Kx, tile.TH, TW, tile.SH, tile.SWp, lds, vec_store);
  return YOGO_OK;
}

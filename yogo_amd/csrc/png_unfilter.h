// The PNG filters reversed by one wavefront per image, defined once: included by png_unpack.hip (8-bit grey -> cropped batches),
// png_unpack_planes.hip (8-bit grey / RGB -> planes of the device image cache) and png_unpack_any.hip (every colour type, bit depth
// and Adam7 -> either).  They differ in where an unfiltered pixel goes, which a Sink says; the loop, the arithmetic and the status
// codes are here.
//
// Filters (BPP bytes per pixel, the row above row 0 is zeros, arithmetic mod 256 on each byte of a pixel; the byte BPP to the left is
// the same channel of the pixel to the left): 0 None, 1 Sub (+ left), 2 Up (+ above), 3 Average (+ floor((left + above) / 2)),
// 4 Paeth (+ whichever of left, above, upper-left is nearest left + above - upper-left, ties in that order).  Sub, Average and Paeth
// are serial along a row, Up, Average and Paeth need the row above: the wavefront takes 64 consecutive rows at a time, lane r on
// row r, skewed by one PIXEL per row -- at step t lane r makes pixel t - r of its row, so that the pixel above it is what lane r - 1
// made one step earlier (one DPP-style shuffle) and the upper-left one is what that shuffle brought the step before.  A pixel of 3
// bytes travels as one packed register (R in the low byte), one of 6 or 8 bytes (16-bit RGB / RGBA) as a packed pair (pix_t).  Depths
// below 8 run at BPP 1 over the row's BYTES: the caller passes the row's byte count as W and its sink expands a byte into pixels.
// Every mix of filter types keeps the 64 lanes busy; a band of 64 rows
// costs W + 63 steps.  Lane 0's row above is the last row of the band before: lane 63 writes its unfiltered pixels back to the
// scanlines IN PLACE (only that row of each band is written back; the buffer is not left whole), and the wave reads them 64 pixels
// at a time.  __syncthreads() between two bands orders those stores before the loads, as in blosc_lz4.hip.  The filtered bytes of a
// row are fetched four pixels per lane at a time, one fetch ahead of their use.
#pragma once
#include <type_traits>

#include "common.h"

namespace yogo_png {

constexpr int WAVE = 64;
// a packed pixel of BPP bytes, byte j at bits 8 j: one register up to 4 bytes, two beyond
template <int BPP>
using pix_t = std::conditional_t<(BPP <= 4), unsigned, unsigned long long>;
// per image: fine, a filter-type byte above 4, the image does not lie inside the scanline buffer (nothing of it was read)
enum : int { ST_OK = 0, ST_BAD_FILTER = 1, ST_BAD_IMAGE = 2 };

// four consecutive pixels of a row.  One byte per pixel: the four in one word, as they lie in memory (four registers there took
// png_unpack_kernel from 36 / 38 to 42 / 43 VGPRs); else one packed pixel per element
template <int BPP>
struct Px4 {
  pix_t<BPP> v[BPP == 1 ? 1 : 4];
  __device__ __forceinline__ pix_t<BPP> at(int k) const {
    if constexpr (BPP == 1) return (v[0] >> (8 * k)) & 255u;
    else return v[k];
  }
};

// byte j of a packed pixel (nothing lies above its last byte)
template <int BPP>
__device__ __forceinline__ unsigned byte_of(pix_t<BPP> v, int j) {
  return j == BPP - 1 ? (unsigned)(v >> (8 * j)) : (unsigned)(v >> (8 * j)) & 255u;
}

// what the lane below holds / what lane l holds, for either width of a packed pixel
template <class T>
__device__ __forceinline__ T from_lane_below(T v) {
  if constexpr (sizeof(T) == 4) {
    return (T)__shfl_up((int)v, 1);
  } else {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, 1), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), 1);
    return (T)lo | ((T)hi << 32);
  }
}
template <class T>
__device__ __forceinline__ T from_lane(T v, int l) {
  if constexpr (sizeof(T) == 4) {
    return (T)__builtin_amdgcn_readlane((int)v, l);
  } else {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return (T)lo | ((T)hi << 32);
  }
}

// pixels x0 .. x0 + 3 of the row at p (W pixels of BPP bytes); zero outside the row
template <int BPP>
__device__ __forceinline__ Px4<BPP> fetch4(const unsigned char* p, int x0, int W, bool active) {
  Px4<BPP> q = {};
  if (!active || x0 >= W || x0 + 3 < 0) return q;
  if (x0 >= 0 && x0 + 4 <= W) {
    unsigned w[BPP];
    __builtin_memcpy(w, p + x0 * BPP, 4 * BPP);
    if constexpr (BPP == 1) {
      q.v[0] = w[0];
    } else if constexpr (BPP == 2) {
      for (int k = 0; k < 4; ++k) q.v[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    } else if constexpr (BPP == 4) {
      for (int k = 0; k < 4; ++k) q.v[k] = w[k];
    } else if constexpr (BPP == 6) {
      q.v[0] = w[0] | ((unsigned long long)(w[1] & 0xffffu) << 32);
      q.v[1] = (w[1] >> 16) | ((unsigned long long)w[2] << 16);
      q.v[2] = w[3] | ((unsigned long long)(w[4] & 0xffffu) << 32);
      q.v[3] = (w[4] >> 16) | ((unsigned long long)w[5] << 16);
    } else if constexpr (BPP == 8) {
      for (int k = 0; k < 4; ++k) q.v[k] = w[2 * k] | ((unsigned long long)w[2 * k + 1] << 32);
    } else {
      static_assert(BPP == 3, "a pixel is 1, 2, 3, 4, 6 or 8 bytes");
      q.v[0] = w[0] & 0xffffffu;
      q.v[1] = (w[0] >> 24) | ((w[BPP - 2] & 0xffffu) << 8);
      q.v[2] = (w[BPP - 2] >> 16) | ((w[BPP - 1] & 0xffu) << 16);
      q.v[3] = w[BPP - 1] >> 8;
    }
  } else {
    for (int k = 0; k < 4; ++k)
      if (x0 + k >= 0 && x0 + k < W)
        for (int j = 0; j < BPP; ++j) q.v[BPP == 1 ? 0 : k] |= (pix_t<BPP>)p[(x0 + k) * BPP + j] << (8 * (BPP == 1 ? k : j));
  }
  return q;
}

// The scanlines at img (H rows of 1 + BPP * W bytes, inside the buffer: the caller has checked; H, W >= 1) unfiltered by the 64 lanes of one
// block -> ST_OK, or ST_BAD_FILTER: the rows of the bands before the bad byte's delivered, nothing after.  Sink: row(y, active) once
// per band and lane (active: row y exists), then pixel(x, v) for every pixel of that row, x ascending, v packed as above.
template <int BPP, class Sink>
__device__ __forceinline__ int unfilter(unsigned char* img, int H, int W, Sink sink, int lane) {
  const int stride = BPP * W + 1;
  int st = ST_OK;
  for (int band = 0; band < H; band += WAVE) {
    const int y = band + lane;
    const bool active = y < H;
    unsigned char* rowp = img + (long long)(active ? y : 0) * stride + 1;
    const int ft = active ? rowp[-1] : 0;
    if (__ballot(ft > 4)) { st = ST_BAD_FILTER; break; }
    const unsigned char* abovep = band ? img + (long long)(band - 1) * stride + 1 : nullptr;
    sink.row(y, active);
    pix_t<BPP> cur = 0, upleft = 0, abv = 0;   // what this lane made last step; what the shuffle brought last step; lane 0's row above
    Px4<BPP> next = fetch4<BPP>(rowp, -lane, W, active);
    for (int t0 = 0; t0 < W + WAVE - 1; t0 += 4) {
      if ((t0 & (WAVE - 1)) == 0) {
        abv = 0;
        if (abovep && t0 + lane < W)
          for (int j = 0; j < BPP; ++j) abv |= (pix_t<BPP>)abovep[(t0 + lane) * BPP + j] << (8 * j);
      }
      const Px4<BPP> w = next;
      next = fetch4<BPP>(rowp, t0 + 4 - lane, W, active);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t = t0 + k, x = t - lane;
        pix_t<BPP> up = from_lane_below(cur);
        const pix_t<BPP> first_up = from_lane(abv, t & (WAVE - 1));
        if (lane == 0) up = first_up;
        const bool valid = active && x >= 0 && x < W;
        const pix_t<BPP> px = w.at(k);
        pix_t<BPP> val = 0;
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int a = (int)byte_of<BPP>(cur, j), bb = (int)byte_of<BPP>(up, j), c = (int)byte_of<BPP>(upleft, j);
          int pred = 0;
          if (ft == 1) pred = a;
          else if (ft == 2) pred = bb;
          else if (ft == 3) pred = (a + bb) >> 1;
          else if (ft == 4) {
            const int pa = abs(bb - c), pb = abs(a - c), pc = abs(a + bb - 2 * c);
            pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c);
          }
          val |= (pix_t<BPP>)((byte_of<BPP>(px, j) + (unsigned)pred) & 255u) << (8 * j);
        }
        upleft = up;
        cur = valid ? val : (pix_t<BPP>)0;
        if (valid) {
          if (lane == WAVE - 1) {
#pragma unroll
            for (int j = 0; j < BPP; ++j) rowp[x * BPP + j] = (unsigned char)(val >> (8 * j));
          }
          sink.pixel(x, val);
        }
      }
    }
    __syncthreads();   // lane 63's row is visible to the loads of the next band
  }
  return st;
}

}  // namespace yogo_png

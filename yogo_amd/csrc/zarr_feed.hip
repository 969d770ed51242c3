// Batch rows from decoded zarr chunks (yogo_amd/zarr_feed.py, `yogo infer --path-to-zarr`): what the reference does per image on
// the host -- `store[:, :, idx][None]`, CenterCrop, `/ 255` (yogo/data/image_path_dataset.py:115-126, yogo/infer.py:221-226) --
// as one launch per batch over the chunks as they came off the disk.
//
// `staged` holds whole decoded chunks of shape (ch, cw, cn) at 16-byte aligned offsets.  tile_off[b][ty][tx] is the offset of
// the chunk with tile (ty, tx) of batch row b's frame (-1, or a chunk that would not lie inside `staged`: the tile reads as
// `fill`), tile_k[b] the frame's position on the chunk's innermost axis.  out[b][0][oy][ox] = frame_b[top + oy][left + ox], as
// uint8 or as fp32 x / 255, bit-identical to torch's CPU `uint8_tensor / 255` (build.sh compiles with
// -fhip-fp32-correctly-rounded-divide-sqrt; image_cache.hip relies on the same).
//
// Three paths, chosen on the host by which stride of the chunk is 1:
//   rows         C order, cn == 1: image rows are contiguous in the chunk.  16-byte loads and stores when one tile spans the
//                width and every source and destination segment is 16-byte aligned: row by row (OW, cw and left multiples of
//                16), or, when the crop keeps whole rows of a single tile, the cropped image as ONE contiguous span (772 x 1032:
//                1032 is no multiple of 16, 772 * 1032 is).  Otherwise byte-wise.
//   deinterleave C order, 1 < cn <= 1024: the cn frames of a chunk alternate byte by byte along x.  A workgroup loads a
//                contiguous slab [x-range][cn] of one chunk row with 16-byte loads into LDS and writes one contiguous row
//                segment per batch row that asks for a frame of this chunk.  Batch rows that share a chunk are consecutive
//                (the feed walks the indices in order): the first of a run serves the whole run from its one read of the
//                slab, the others leave at once.
//   gather       F order, any cn (and C order with cn > 1024): one byte per lane and step through the general index
//                arithmetic.  It has to be correct; it is not tuned (F-order image stacks are not what the scopes write).
#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int UNROLL = 4;
constexpr int SLAB = 4096;        // bytes of a chunk row one deinterleave workgroup stages
constexpr int DEINT_MAX_CN = 1024;
// the slab starts up to 15 bytes before its first pixel (16-byte aligned loads) and ends on a whole piece: <= 257 pieces = 1028
// dwords, plus one pad dword per 32
constexpr int SLAB_DW = 1028 + 1028 / 32 + 4;

struct Geo {
  int gh, gw, ch, cw, cn, fill, top, left, OH, OW;
  long long chunk_bytes, staged_bytes;
};

// offset of the chunk of tile (ty, tx) of batch row b, -1 when the tile reads as fill
__device__ __forceinline__ long long tile_base(const long long* __restrict__ tile_off, const Geo& g, int b, int ty, int tx) {
  const long long off = tile_off[((long long)b * g.gh + ty) * g.gw + tx];
  return (off < 0 || off + g.chunk_bytes > g.staged_bytes) ? -1 : off;
}

template <bool F32>
__device__ __forceinline__ void store_px(void* __restrict__ out, long long i, unsigned v) {
  if (F32)
    static_cast<float*>(out)[i] = (float)v / 255.f;
  else
    static_cast<unsigned char*>(out)[i] = (unsigned char)v;
}

// ---- rows, 16-byte pieces: nseg segments of seg16 pieces per batch row; segment s starts at image row top + s * rows_per_seg.
// grid (seg16 / (BLOCK * UNROLL), nseg, B)
template <bool F32>
__global__ __launch_bounds__(BLOCK) void zarr_unpack_rows_vec_kernel(const unsigned char* __restrict__ staged,
                                                                     const long long* __restrict__ tile_off, const int* __restrict__ tile_k,
                                                                     Geo g, int rows_per_seg, long long seg16, void* __restrict__ out) {
  const int b = blockIdx.z, s = blockIdx.y;
  const int iy = g.top + s * rows_per_seg;
  const int ty = iy / g.ch;
  // a row whose tile_k is no position of the chunk is fill, as on the byte path: one test per workgroup (b is uniform)
  const bool k_ok = (unsigned)tile_k[b] < (unsigned)g.cn;
  const long long off = k_ok ? tile_base(tile_off, g, b, ty, 0) : -1;
  const uint4* src = off < 0 ? nullptr : reinterpret_cast<const uint4*>(staged + off + (long long)(iy - ty * g.ch) * g.cw + g.left);
  const unsigned f4 = 0x01010101u * (unsigned)g.fill;
  const long long i0 = (long long)blockIdx.x * (BLOCK * UNROLL) + threadIdx.x;
  const long long d0 = ((long long)b * gridDim.y + s) * seg16;
  uint4 v[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const long long i = i0 + (long long)u * BLOCK;
    v[u] = make_uint4(f4, f4, f4, f4);
    if (i < seg16 && src) v[u] = src[i];
  }
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const long long i = i0 + (long long)u * BLOCK;
    if (i >= seg16) continue;
    if (!F32) {
      static_cast<uint4*>(out)[d0 + i] = v[u];
    } else {
      float4* dst = static_cast<float4*>(out) + (d0 + i) * 4;
      const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        dst[k] = make_float4((float)(w[k] & 0xffu) / 255.f, (float)((w[k] >> 8) & 0xffu) / 255.f, (float)((w[k] >> 16) & 0xffu) / 255.f,
                             (float)(w[k] >> 24) / 255.f);
    }
  }
}

// ---- byte-wise, any tiling / crop / alignment: one pixel per lane and step.  grid (OH * OW / (BLOCK * UNROLL), B)
template <bool ORDER_F, bool F32>
__device__ __forceinline__ void unpack_bytes(const unsigned char* __restrict__ staged, const long long* __restrict__ tile_off,
                                             const int* __restrict__ tile_k, const Geo& g, void* __restrict__ out) {
  const int b = blockIdx.y;
  const int k = tile_k[b];
  const bool k_ok = (unsigned)k < (unsigned)g.cn;
  const int n = g.OH * g.OW;
  const int i0 = blockIdx.x * (BLOCK * UNROLL) + threadIdx.x;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int i = i0 + u * BLOCK;
    if (i >= n) continue;
    const int oy = i / g.OW, ox = i - oy * g.OW;
    const int iy = g.top + oy, ix = g.left + ox;
    const int ty = iy / g.ch, tx = ix / g.cw;
    const int ly = iy - ty * g.ch, lx = ix - tx * g.cw;
    const long long off = k_ok ? tile_base(tile_off, g, b, ty, tx) : -1;
    unsigned v = (unsigned)g.fill;
    if (off >= 0)
      v = staged[off + (ORDER_F ? ly + (long long)g.ch * (lx + (long long)g.cw * k) : ((long long)ly * g.cw + lx) * g.cn + k)];
    store_px<F32>(out, (long long)b * n + i, v);
  }
}

template <bool F32>
__global__ __launch_bounds__(BLOCK) void zarr_unpack_rows_byte_kernel(const unsigned char* __restrict__ staged,
                                                                      const long long* __restrict__ tile_off, const int* __restrict__ tile_k,
                                                                      Geo g, void* __restrict__ out) {
  unpack_bytes<false, F32>(staged, tile_off, tile_k, g, out);
}

template <bool ORDER_F, bool F32>
__global__ __launch_bounds__(BLOCK) void zarr_unpack_gather_kernel(const unsigned char* __restrict__ staged,
                                                                   const long long* __restrict__ tile_off, const int* __restrict__ tile_k,
                                                                   Geo g, void* __restrict__ out) {
  unpack_bytes<ORDER_F, F32>(staged, tile_off, tile_k, g, out);
}

// ---- deinterleave.  grid (tiles the crop touches along x * slabs_per_tile, OH, B): a workgroup owns XS pixels of one image row
// inside one tile.  The slab's bytes [x][k] are contiguous in the chunk: lane l loads the 16-byte piece l and writes it to LDS as
// four dwords.  LDS layout: dword d of the slab lives at d + d / 32, i.e. every 128-byte row is padded by one dword (Guideline 4).
// The reads that follow are byte reads at lane stride cn (pixel per lane) or 4 * cn (quad per lane): for cn = 2, 4, 8, 16 that is
// a dword stride S of 1/2 .. 16 between lanes, and the 32 lanes of a group hit banks (S * j + (S * j) / 32) % 32 -- all distinct
// for every power of two S <= 32 (the pad moves each wrap of the 32 banks on by one); lanes that share a dword (cn = 2 pixels)
// broadcast.  cn = 3 strides 3 or 12 bytes: consecutive lanes, consecutive or neighbouring dwords.  The piece writes are dword
// writes at lane stride 4 dwords: the same argument with S = 4.
template <bool F32>
__global__ __launch_bounds__(BLOCK) void zarr_unpack_deinterleave_kernel(const unsigned char* __restrict__ staged,
                                                                         const long long* __restrict__ tile_off,
                                                                         const int* __restrict__ tile_k, int B, Geo g, int XS,
                                                                         int slabs_per_tile, int tx0, int out_al16, void* __restrict__ out) {
  __shared__ unsigned lds[SLAB_DW];
  const int b = blockIdx.z, oy = blockIdx.y;
  const int tx = tx0 + blockIdx.x / slabs_per_tile, sl = blockIdx.x % slabs_per_tile;
  const int iy = g.top + oy, ty = iy / g.ch, ly = iy - ty * g.ch;
  // the pixels [xa, xb) of the image row: this tile, inside the crop, slab sl
  const int xa = max(g.left, tx * g.cw) + sl * XS;
  const int xb = min(min(g.left + g.OW, (tx + 1) * g.cw), xa + XS);
  if (xa >= xb) return;
  const int nx = xb - xa;
  const long long tstride = (long long)g.gh * g.gw;
  const long long tidx = ((long long)b * g.gh + ty) * g.gw + tx;
  const long long raw = tile_off[tidx];
  const bool valid = raw >= 0 && raw + g.chunk_bytes <= g.staged_bytes;
  const long long row0 = ((long long)b * g.OH + oy) * g.OW + (xa - g.left);
  if (!valid) {   // an absent chunk: this batch row's segment is fill
    for (int j = threadIdx.x; j < nx; j += BLOCK) store_px<F32>(out, row0 + j, (unsigned)g.fill);
    return;
  }
  if (b > 0 && tile_off[tidx - tstride] == raw) return;   // the first row of the run serves this one
  int nmem = 1;
  while (b + nmem < B && tile_off[tidx + nmem * tstride] == raw) ++nmem;

  const long long start = raw + ((long long)ly * g.cw + (xa - tx * g.cw)) * g.cn;
  const long long a0 = start & ~15LL;
  const int head = (int)(start - a0);
  const int npieces = (head + nx * g.cn + 15) >> 4;   // <= 257: nx * cn <= SLAB
  for (int l = threadIdx.x; l < npieces; l += BLOCK) {
    const long long a = a0 + 16LL * l;
    uint4 v;
    if (a + 16 <= g.staged_bytes) {
      v = *reinterpret_cast<const uint4*>(staged + a);
    } else {   // the last piece of the buffer: only the bytes that exist
      unsigned w[4] = {0u, 0u, 0u, 0u};
      for (int i = 0; i < 16; ++i)
        if (a + i < g.staged_bytes) w[i >> 2] |= (unsigned)staged[a + i] << (8 * (i & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const int d = 4 * l + (l >> 3);   // (4 l .. 4 l + 3 lie in one 32-dword row)
    lds[d] = v.x;
    lds[d + 1] = v.y;
    lds[d + 2] = v.z;
    lds[d + 3] = v.w;
  }
  __syncthreads();
  const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
  const int nq = (nx + 3) >> 2;
  for (int it = threadIdx.x; it < nmem * nq; it += BLOCK) {
    const int m = it / nq, q = it - m * nq;
    const int k = tile_k[b + m];
    const bool k_ok = (unsigned)k < (unsigned)g.cn;
    const long long o = row0 + (long long)m * g.OH * g.OW + 4 * q;
    const int cnt = min(4, nx - 4 * q);
    unsigned px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = head + (4 * q + (i < cnt ? i : 0)) * g.cn + (k_ok ? k : 0);
      px[i] = k_ok ? lb[p + ((p >> 7) << 2)] : (unsigned)g.fill;
    }
    if (cnt == 4 && out_al16 && (o & 3) == 0) {
      if (F32)
        *reinterpret_cast<float4*>(static_cast<float*>(out) + o) =
            make_float4((float)px[0] / 255.f, (float)px[1] / 255.f, (float)px[2] / 255.f, (float)px[3] / 255.f);
      else
        *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(out) + o) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    } else {
      for (int i = 0; i < cnt; ++i) store_px<F32>(out, o + i, px[i]);
    }
  }
}

}  // namespace

extern "C" int yogo_zarr_unpack(const unsigned char* staged, long long staged_bytes, const long long* tile_off, const int* tile_k, int B,
                                int gh, int gw, int ch, int cw, int cn, int order_f, int fill, int H, int W, int top, int left, int OH,
                                int OW, void* out, int out_fp32, hipStream_t stream) {
  YOGO_CHECK_ARG(staged && tile_off && tile_k && out && staged_bytes > 0 && B >= 0, "zarr_unpack: bad arguments");
  YOGO_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "zarr_unpack: bad frame shape %d x %d (1 .. 65535 each)", H, W);
  YOGO_CHECK_ARG(ch >= 1 && cw >= 1 && cn >= 1, "zarr_unpack: bad chunk shape %d x %d x %d", ch, cw, cn);
  YOGO_CHECK_ARG(gh == cdiv(H, ch) && gw == cdiv(W, cw), "zarr_unpack: a %d x %d tile grid for %d x %d frames in %d x %d chunks", gh, gw,
                 H, W, ch, cw);
  YOGO_CHECK_ARG(top >= 0 && left >= 0 && top < H && left < W, "zarr_unpack: crop origin (%d, %d) outside the %d x %d frame", top, left,
                 H, W);
  YOGO_CHECK_ARG(OH >= 1 && OH <= H - top && OW >= 1 && OW <= W - left, "zarr_unpack: a %d x %d crop at (%d, %d) of a %d x %d frame", OH,
                 OW, top, left, H, W);
  YOGO_CHECK_ARG(B <= 65535, "zarr_unpack: B = %d rows, at most 65535 per call", B);
  YOGO_CHECK_ARG(out_fp32 == 0 || out_fp32 == 1, "zarr_unpack: out_fp32 must be 0 (uint8) or 1 (float32)");
  YOGO_CHECK_ARG(order_f == 0 || order_f == 1, "zarr_unpack: order_f must be 0 (C) or 1 (F)");
  YOGO_CHECK_ARG(fill >= 0 && fill <= 255, "zarr_unpack: fill %d is no uint8", fill);
  YOGO_CHECK_ARG((long long)OH * OW < (1LL << 31), "zarr_unpack: a crop of %d x %d pixels", OH, OW);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(staged) & 15) == 0, "zarr_unpack: the staged chunks must be 16-byte aligned");
  if (B == 0) return YOGO_OK;
  Geo g;
  g.gh = gh, g.gw = gw, g.ch = ch, g.cw = cw, g.cn = cn, g.fill = fill, g.top = top, g.left = left, g.OH = OH, g.OW = OW;
  g.chunk_bytes = (long long)ch * cw * cn;
  g.staged_bytes = staged_bytes;
  const bool out_al = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const long long n = (long long)OH * OW;
  const char* path;
  if (!order_f && cn == 1 && gw == 1 && out_al &&
      ((gh == 1 && left == 0 && OW == cw && ((long long)top * cw) % 16 == 0 && n % 16 == 0) ||
       (OW % 16 == 0 && cw % 16 == 0 && left % 16 == 0))) {
    // whole rows of one tile: the cropped image is one span; otherwise one segment per row
    const bool span = gh == 1 && left == 0 && OW == cw && ((long long)top * cw) % 16 == 0 && n % 16 == 0;
    const int nseg = span ? 1 : OH, rows_per_seg = span ? OH : 1;
    const long long seg16 = (span ? n : (long long)OW) / 16, per_block = (long long)BLOCK * UNROLL;
    const dim3 grid((unsigned)((seg16 + per_block - 1) / per_block), nseg, B);
    if (out_fp32)
      hipLaunchKernelGGL(zarr_unpack_rows_vec_kernel<true>, grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, rows_per_seg, seg16,
                         out);
    else
      hipLaunchKernelGGL(zarr_unpack_rows_vec_kernel<false>, grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, rows_per_seg, seg16,
                         out);
    path = "rows_vec";
  } else if (!order_f && cn > 1 && cn <= DEINT_MAX_CN) {
    const int XS = (SLAB / cn) & ~3;   // >= 4 pixels, a whole number of quads
    const int tx0 = left / cw, tx1 = (left + OW - 1) / cw;
    const int slabs_per_tile = cdiv(cw < OW ? cw : OW, XS);
    const dim3 grid((unsigned)((tx1 - tx0 + 1) * slabs_per_tile), OH, B);
    if (out_fp32)
      hipLaunchKernelGGL(zarr_unpack_deinterleave_kernel<true>, grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, B, g, XS,
                         slabs_per_tile, tx0, out_al ? 1 : 0, out);
    else
      hipLaunchKernelGGL(zarr_unpack_deinterleave_kernel<false>, grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, B, g, XS,
                         slabs_per_tile, tx0, out_al ? 1 : 0, out);
    path = "deinterleave";
  } else {
    const long long per_block = (long long)BLOCK * UNROLL;
    const dim3 grid((unsigned)((n + per_block - 1) / per_block), B);
    if (order_f) {
      if (out_fp32)
        hipLaunchKernelGGL((zarr_unpack_gather_kernel<true, true>), grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, out);
      else
        hipLaunchKernelGGL((zarr_unpack_gather_kernel<true, false>), grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, out);
      path = "gather";
    } else if (cn == 1) {
      if (out_fp32)
        hipLaunchKernelGGL(zarr_unpack_rows_byte_kernel<true>, grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, out);
      else
        hipLaunchKernelGGL(zarr_unpack_rows_byte_kernel<false>, grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, out);
      path = "rows_byte";
    } else {   // C order, more frames per chunk than a slab holds pixels for
      if (out_fp32)
        hipLaunchKernelGGL((zarr_unpack_gather_kernel<false, true>), grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, out);
      else
        hipLaunchKernelGGL((zarr_unpack_gather_kernel<false, false>), grid, dim3(BLOCK), 0, stream, staged, tile_off, tile_k, g, out);
      path = "gather";
    }
  }
  YOGO_CHECK_LAUNCH("zarr_unpack");
  if (yogo_launch_log_enabled())
    yogo_launch_log("zarr_unpack_%s_kernel<%s> | B=%d chunk=%dx%dx%d order=%c crop=%dx%d@(%d,%d)", path, out_fp32 ? "f32" : "u8", B, ch, cw,
                    cn, order_f ? 'F' : 'C', OH, OW, top, left);
  return YOGO_OK;
}

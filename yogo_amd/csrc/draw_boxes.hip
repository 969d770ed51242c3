// `yogo infer --draw-boxes --device-draw` (yogo_amd/draw.py): the RGBA frames PIL would draw, rendered for a whole batch in one launch.
// The host route (yogo_amd/utils/utils.py: draw_yogo_prediction) makes, per image, an RGBA copy and per kept row one
// ImageDraw.rectangle and one ImageDraw.text call.  This kernel restates those calls as arithmetic (tests/_draw_ref.py is the same in
// numpy, held to PIL itself):
//   background  uint8 as it is; float32 truncated toward zero, after one fp32 multiply by 255 when normalised (img * 255 then
//               .to(uint8): some grey levels come out one lower than the source pixel; kept); grey three times; alpha 255
//   box         x = fp32(W) * row[0|2], y = fp32(H) * row[1|3] (plain fp32 multiplies: build.sh compiles this file without
//               contraction); class = first maximum of row[5:]; the corners are the coordinates truncated toward zero
//   outline     one pixel wide, clipped: rows y0 and y1 from x0 to x1, columns x0 and x1 from min(y0 + 1, y1) to max(y0 + 1, y1)
//               (so a box with y0 == y1 also covers row y0 + 1 at its two columns, as PIL's does); colour table[class]
//   text        the label's mask at (int(x0) + offset x, int(y0) + offset y), the variant picked by the fractions of x0 and y0 (they
//               carry the coordinate's sign): per axis the number of cuts at or below the fraction.  Every channel blends as
//               t = m * ink + (255 - m) * old + 128, new = ((t >> 8) + t) >> 8 with ink (0, 0, 0, 255): alpha stays 255
//   order       row by row, outline then text: a later outline overwrites earlier text, later text blends over whatever is there
// A workgroup owns a tile of TILE_H x 64 pixels, each lane TILE_H / 4 pixels of one column, kept in registers.  The image's rows
// are taken 256 at a time: every lane turns one row into an operation record, the ones whose outline or text box meets the tile
// are compacted IN ORDER into LDS (ballot + prefix), and every lane then walks the survivors for its pixels.
#include "common.h"

namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int TILE_W = 64;
constexpr int TILE_H = 16;
constexpr int PIX = TILE_H / (THREADS / WAVE);   // pixels per lane
constexpr int COORD_LIMIT = 1 << 24;

struct Op {
  int x0, y0, x1, y1;      // the outline's corners, y0 <= y1
  int tx, ty, tw, th;      // the text mask's box in the image (tw = 0: no text)
  unsigned colour;         // RGBA, R in the low byte
  int glyph;               // where the mask's bytes start
};

// an order-preserving integer image of a float: a < b (both not NaN, -0 below +0) iff key(a) < key(b)
__device__ __forceinline__ int float_key(float f) {
  const int b = __builtin_bit_cast(int, f);
  return b < 0 ? b ^ 0x7fffffff : b;
}

__device__ __forceinline__ int trunc_coord(float v) {
  if (!(v > -(float)COORD_LIMIT)) return -COORD_LIMIT;   // (NaN too)
  if (v > (float)COORD_LIMIT) return COORD_LIMIT;
  return (int)v;
}

__device__ __forceinline__ unsigned blend_black(unsigned px, unsigned m) {
  unsigned out = 0xff000000u;   // m * 255 + (255 - m) * 255 + 128 -> 255
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned old = (px >> (8 * c)) & 255u;
    const unsigned t = (255u - m) * old + 128u;
    out |= ((((t >> 8) + t) >> 8) & 255u) << (8 * c);
  }
  return out;
}

template <bool FP32>
__device__ __forceinline__ unsigned load_level(const void* img, long long i, bool normalised) {
  if (FP32) {
    float v = static_cast<const float*>(img)[i];
    if (normalised) v = __fmul_rn(v, 255.0f);
    return (unsigned)(int)v & 255u;
  }
  return static_cast<const unsigned char*>(img)[i];
}

template <bool FP32>
__global__ __launch_bounds__(THREADS) void draw_boxes_kernel(const void* __restrict__ img, int normalised, int Cimg, int H, int W,
                                                             const float* __restrict__ rows, const int* __restrict__ counts, int cap, int P,
                                                             const unsigned* __restrict__ colours, const int* __restrict__ label_meta,
                                                             const float* __restrict__ cuts, int n_cuts, const int* __restrict__ variants,
                                                             int n_variants, const unsigned char* __restrict__ glyphs, long long glyph_bytes,
                                                             unsigned* __restrict__ out) {
  __shared__ Op ops[THREADS];
  __shared__ int wave_kept[THREADS / WAVE];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int tile_x = blockIdx.x * TILE_W, tile_y = blockIdx.y * TILE_H;
  const int x = tile_x + lane, ybase = tile_y + wave * PIX;
  const long long plane = (long long)H * W;
  const bool in_x = x < W;

  unsigned px[PIX];
#pragma unroll
  for (int k = 0; k < PIX; ++k) {
    px[k] = 0;
    const int y = ybase + k;
    if (in_x && y < H) {
      const long long i = (long long)b * Cimg * plane + (long long)y * W + x;
      const unsigned r = load_level<FP32>(img, i, normalised != 0);
      const unsigned g = Cimg == 3 ? load_level<FP32>(img, i + plane, normalised != 0) : r;
      const unsigned bl = Cimg == 3 ? load_level<FP32>(img, i + 2 * plane, normalised != 0) : r;
      px[k] = r | (g << 8) | (bl << 16) | 0xff000000u;
    }
  }

  int n = counts[b];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const int C = P - 5;
  const float fW = (float)W, fH = (float)H;
  for (int first = 0; first < n; first += THREADS) {
    // one row per lane -> its operation, and whether it meets this tile
    Op op = {};
    bool keep = false;
    const int r = first + tid;
    if (r < n) {
      const float* row = rows + ((long long)b * cap + r) * P;
      const float xf0 = __fmul_rn(fW, row[0]), yf0 = __fmul_rn(fH, row[1]), xf1 = __fmul_rn(fW, row[2]), yf1 = __fmul_rn(fH, row[3]);
      int cls = 0;
      float best = row[5];
      for (int c = 1; c < C; ++c) {
        const float v = row[5 + c];
        if (v > best) best = v, cls = c;
      }
      const int x0 = trunc_coord(xf0), y0 = trunc_coord(yf0), x1 = trunc_coord(xf1), y1 = trunc_coord(yf1);
      op.x0 = x0, op.x1 = x1, op.y0 = y0 < y1 ? y0 : y1, op.y1 = y0 < y1 ? y1 : y0;
      op.colour = colours[cls];
      // the text: the variant by the fractions of the first corner (exact in fp32)
      const int* meta = label_meta + 6 * cls;
      const int fxk = float_key(xf0 - (float)x0), fyk = float_key(yf0 - (float)y0);
      int ix = 0, iy = 0;
      for (int k = 0; k < meta[1]; ++k) {
        const int at = meta[0] + k;
        if (at >= 0 && at < n_cuts && float_key(cuts[at]) <= fxk) ++ix;
      }
      for (int k = 0; k < meta[3]; ++k) {
        const int at = meta[2] + k;
        if (at >= 0 && at < n_cuts && float_key(cuts[at]) <= fyk) ++iy;
      }
      const int v = meta[4] + ix * (meta[3] + 1) + iy;
      op.tw = 0;
      if (v >= 0 && v < n_variants) {
        const int* var = variants + 5 * v;
        const int tw = var[0], th = var[1];
        const long long at = var[4];
        if (tw > 0 && th > 0 && tw < 65536 && th < 65536 && at >= 0 && at + (long long)tw * th <= glyph_bytes) {
          op.tw = tw, op.th = th, op.tx = x0 + var[2], op.ty = y0 + var[3], op.glyph = (int)at;
        }
      }
      const int xa = min(op.x0, op.x1), xb = max(op.x0, op.x1);
      const bool box_hit = xa < tile_x + TILE_W && xb >= tile_x && op.y0 < tile_y + TILE_H && op.y1 + 1 >= tile_y;   // (+1: the y0 == y1 rule)
      const bool text_hit = op.tw > 0 && op.tx < tile_x + TILE_W && op.tx + op.tw > tile_x && op.ty < tile_y + TILE_H && op.ty + op.th > tile_y;
      keep = box_hit || text_hit;
    }
    // compact the survivors in row order
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_kept[wave] = __popcll(mask);
    __syncthreads();   // (also: the previous walk is over before ops is rewritten)
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / WAVE; ++w) {
      if (w < wave) base += wave_kept[w];
      total += wave_kept[w];
    }
    if (keep) ops[base + __popcll(mask & ((1ull << lane) - 1ull))] = op;
    __syncthreads();
    // every lane applies the survivors to its pixels, in order
    for (int k = 0; k < total; ++k) {
      const Op o = ops[k];
      const int xa = min(o.x0, o.x1), xb = max(o.x0, o.x1);
      const int ya = min(o.y0 + 1, o.y1), yb = max(o.y0 + 1, o.y1);
      const bool in_row_span = x >= xa && x <= xb, on_col = x == o.x0 || x == o.x1;
      const int mx = x - o.tx;
      const bool in_text_x = o.tw > 0 && mx >= 0 && mx < o.tw;
#pragma unroll
      for (int q = 0; q < PIX; ++q) {
        const int y = ybase + q;
        if ((in_row_span && (y == o.y0 || y == o.y1)) || (on_col && y >= ya && y <= yb)) px[q] = o.colour;
        const int my = y - o.ty;
        if (in_text_x && my >= 0 && my < o.th) px[q] = blend_black(px[q], glyphs[o.glyph + my * o.tw + mx]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < PIX; ++k) {
    const int y = ybase + k;
    if (in_x && y < H) out[(long long)b * plane + (long long)y * W + x] = px[k];
  }
}

}  // namespace

extern "C" int yogo_draw_boxes(const void* img, int img_fp32, int normalised, int B, int Cimg, int H, int W, const float* rows,
                               const int* counts, int cap, int P, const unsigned char* colours, const int* label_meta, const float* cuts,
                               int n_cuts, const int* variants, int n_variants, const unsigned char* glyphs, long long glyph_bytes,
                               unsigned char* out, hipStream_t stream) {
  YOGO_CHECK_ARG(img && rows && counts && colours && label_meta && cuts && variants && glyphs && out, "draw_boxes: null argument");
  YOGO_CHECK_ARG(B >= 0 && B <= 65535, "draw_boxes: B = %d images, at most 65535 per call", B);
  YOGO_CHECK_ARG(Cimg == 1 || Cimg == 3, "draw_boxes: %d image channels, 1 or 3", Cimg);
  YOGO_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "draw_boxes: bad image shape %d x %d (1 .. 65535 each)", H, W);
  YOGO_CHECK_ARG(cap >= 0 && P >= 6, "draw_boxes: cap = %d rows of %d values (at least one class)", cap, P);
  YOGO_CHECK_ARG(n_cuts >= 0 && n_variants >= 0 && glyph_bytes >= 0 && glyph_bytes < (1LL << 31), "draw_boxes: bad atlas sizes");
  YOGO_CHECK_ARG((img_fp32 == 0 || img_fp32 == 1) && (normalised == 0 || normalised == 1), "draw_boxes: img_fp32 and normalised are 0 or 1");
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(colours) & 3) == 0 &&
                     (!img_fp32 || (reinterpret_cast<uintptr_t>(img) & 3) == 0),
                 "draw_boxes: the output, the colour table and a float32 image must be 4-byte aligned");
  if (B == 0) return YOGO_OK;
  const dim3 grid(cdiv(W, TILE_W), cdiv(H, TILE_H), B);
  YOGO_CHECK_ARG(grid.y <= 65535, "draw_boxes: an image of %d rows", H);
  if (img_fp32)
    hipLaunchKernelGGL((draw_boxes_kernel<true>), grid, dim3(THREADS), 0, stream, img, normalised, Cimg, H, W, rows, counts, cap, P,
                       reinterpret_cast<const unsigned*>(colours), label_meta, cuts, n_cuts, variants, n_variants, glyphs, glyph_bytes,
                       reinterpret_cast<unsigned*>(out));
  else
    hipLaunchKernelGGL((draw_boxes_kernel<false>), grid, dim3(THREADS), 0, stream, img, normalised, Cimg, H, W, rows, counts, cap, P,
                       reinterpret_cast<const unsigned*>(colours), label_meta, cuts, n_cuts, variants, n_variants, glyphs, glyph_bytes,
                       reinterpret_cast<unsigned*>(out));
  YOGO_CHECK_LAUNCH("draw_boxes");
  if (yogo_launch_log_enabled())
    yogo_launch_log("draw_boxes_kernel<%s> | B=%d image=%dx%dx%d cap=%d", img_fp32 ? "f32" : "u8", B, Cimg, H, W, cap);
  return YOGO_OK;
}

// The launch plan of wgrad_bf16_kernel (wgrad_bf16.hip): tiling, column chunks, LDS ring, split-K -- and which loop of the kernel runs.
// Host code without any HIP in it, so that tools/wgrad_plan_sweep.cpp can compile it alone and walk the whole shape space
// (profiles/wgrad_bf16_one_definition.log has its table: which (instantiation, steps per row, ring depth) exist at all).
#pragma once

#define WGB_LDS_MAX (160 * 1024)
#define WGB_GSLOTS 4  // LDS-DMA slots per lane and unit: gradient tile
#define WGB_XSLOTS 6  // ... input tile
constexpr int WGB_BLK4_W = 36;  // BLK4: staged gradient columns of a unit (the input image: two more); the kernel's row pitches are built from it

// What the kernel reads of a plan: WbPlan holds it, WgradBf16Params embeds it, the launcher assigns it once.
struct WbGeom {
  int nchunk_w, base_w, rem_w, wce;   // column chunks per row (balanced), staged chunk width (zero padded; a multiple of 16 but for BLK4's 36)
  int nrowg;                          // row groups per image (R output rows each)
  int xw;                             // staged input columns per unit
  int units, units_per_split;
  int ngs, nxs, bufu;                 // g / x slots in use, 16-byte units per LDS buffer
  int xoff;                           // first unit of the x image inside an LDS buffer (ngs * threads, or the g image rounded up to a whole piece)
  int xcb;                            // channel blocks per pixel of the staged x image: 4, or 2 for 16-channel inputs
  int depth;                          // LDS buffers in the ring (2 or 3): units in flight ahead of the MFMAs = depth - 1
};

// MBW x NBW x KS x (3 kernel rows | 1) wavefronts; each holds MPW co-blocks x one ci-block of 32 channels; R output rows per unit.
// The three decisions the kernel's template arguments, the bias rows and the launch log all read:
//   blk4   the 128 x 64 tiling at stride 1: k-steps of 4 x 4 pixels, chunks of at most 36 columns
//   pack2  16 input channels on the tall tiling: two taps per MFMA
//   lean   KS == 1: every wavefront of the first ci-block workgroup sums the bias and writes its own partial row
struct WbPlan {
  WbGeom g;
  bool blk4, pack2, lean;
  int MBW, NBW, MPW, KS, R, T, S, OH, OW, pad, Mpad, Npad, nsplit, lds_bytes;
  unsigned grid[3];
  int threads() const { return 64 * MBW * NBW * KS * (T == 1 ? 1 : 3); }
  int slabs() const { return nsplit * KS; }
  // rows of the bias partial-sum region behind the slabs (the kernel's `brow`): ONE definition for the workspace query, the launcher's
  // pointer arithmetic and the reduction's row count
  int bias_rows() const { return slabs() * (lean ? NBW * (T == 1 ? 1 : 3) : 1); }
  unsigned long long slab_floats() const { return (unsigned long long)slabs() * T * Mpad * Npad; }
};

namespace wbp {
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_to(int a, int b) { return ceil_div(a, b) * b; }
inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
}  // namespace wbp

// false: no plan fits the slots and the LDS (the caller reports "no LDS plan"; nothing is launched)
inline bool wb_plan(int B, int N, int M, int IH, int IW, int ks, int stride, WbPlan* pl) {
  using namespace wbp;
  WbGeom& g = pl->g;
  const int pad = ks == 3 ? 1 : 0;
  const int OH = (IH + 2 * pad - ks) / stride + 1, OW = (IW + 2 * pad - ks) / stride + 1;
  pl->OH = OH; pl->OW = OW; pl->pad = pad; pl->T = ks * ks; pl->S = stride;
  const int mblocks = ceil_div(M, 32), nblocks = ceil_div(N, 32);
  int MBW = imin(4, mblocks);
  if (MBW == 3) MBW = 2;
  int NBW = imin(4 / MBW, nblocks);
  if (NBW == 3) NBW = 2;
  // 128 output channels x >= 64 input channels: a 128 x 64 workgroup tile as 2 x 2 wavefronts of two co-blocks x one ci-block each, so
  // the gradient tile is staged once per 64 (not 32) input channels and an MFMA costs a third less LDS read traffic
  int MPW = 1;
  if (MBW == 4 && NBW == 1 && nblocks >= 2 && ks == 3) { MBW = 2; NBW = 2; MPW = 2; }
  const int KS = 4 / (MBW * NBW);
  // rows per unit: few channels -> little MFMA work per row, so take more rows per barrier
  const bool tall = MBW == 1 && NBW == 1 && ks == 3 && stride == 1 && OH >= 64;
  const int R = stride == 2 ? 2 : (tall ? 8 : 4);
  pl->blk4 = MPW == 2 && stride == 1;   // 4 x 4-pixel k-steps (wgrad_bf16_kernel, BLK4)
  pl->MBW = MBW; pl->NBW = NBW; pl->MPW = MPW; pl->KS = KS; pl->R = R;
  pl->lean = KS == 1;
  pl->Mpad = round_to(M, 32 * MBW * MPW);
  pl->Npad = round_to(N, 32 * NBW);
  const int TG = ks == 3 ? 3 : 1;
  const int NT = 64 * MBW * NBW * KS * TG;
  const int XR = ks == 3 ? (R - 1) * stride + 3 : R;
  g.xcb = (NBW == 1 && N <= 16 && KS != 1) ? 2 : 4;  // 16-channel inputs: 32-byte pixels in the staged image (not on the lean KS = 1 path)
  pl->pack2 = R == 8 && g.xcb == 2;
  bool found = false;
  if (pl->blk4) {
    // chunks of at most 36 columns = 8 four-column steps + a ninth for a wide chunk (33 - 36 columns); the two images are packed
    // piece-tight (the kernel does not issue a piece that lies wholly behind its image): 3 + 3 slots, two buffers of 65 KB.  Among the
    // chunk counts the one with the fewest steps per row: 129 columns = 33 + 3 x 32 (33 steps), 258 = 2 x 33 + 6 x 32 (66).
    const int w = WGB_BLK4_W, xw = w + 2, nsb = 8;
    const int gtot = MBW * MPW * 4 * R * w, xtot = NBW * g.xcb * XR * xw;
    g.ngs = ceil_div(gtot, NT); g.nxs = ceil_div(xtot, NT);
    g.xoff = round_to(gtot, 64); g.bufu = g.xoff + round_to(xtot, 64);
    g.depth = 2;
    if (g.ngs > WGB_GSLOTS || g.nxs > WGB_XSLOTS || g.depth * g.bufu * 16 > WGB_LDS_MAX) return false;
    int best_steps = 1 << 30;
    for (int nc = ceil_div(OW, w); nc <= ceil_div(OW, w) + 3 && nc <= OW; ++nc) {   // (the first count always fits: a balanced chunking of <= 36 columns)
      const int base = OW / nc, rem = OW - base * nc;
      if (base + (rem ? 1 : 0) > w) continue;
      const int steps = rem * (base + 1 > 4 * nsb ? nsb + 1 : nsb) + (nc - rem) * (base > 4 * nsb ? nsb + 1 : nsb);
      if (steps < best_steps) { best_steps = steps; g.nchunk_w = nc; }
    }
    g.wce = w; g.xw = xw;
    found = true;
  }
  // column chunks: staged width a multiple of 16, at most 64; the widest that fits the slots and two LDS buffers, then the count with
  // the least zero padding
  int best_waste = 1 << 30;
  for (int wmax = 64; wmax >= 16 && !found; wmax -= 16) {
    for (int nc = ceil_div(OW, wmax); nc <= ceil_div(OW, wmax) + 4 && nc <= OW; ++nc) {
      const int w = round_to(ceil_div(OW, nc), 16);
      if (w > wmax) continue;
      const int xw = (w - 1) * stride + (ks == 3 ? 3 : 1);
      const int ngs = ceil_div(MBW * MPW * 4 * R * w, NT), nxs = ceil_div(NBW * g.xcb * XR * xw, NT);
      const int bufu = (ngs + nxs) * NT;
      if (ngs > WGB_GSLOTS || nxs > WGB_XSLOTS || 2 * bufu * 16 > WGB_LDS_MAX) continue;
      const int waste = nc * w - OW;
      if (waste < best_waste) {
        best_waste = waste;
        g.nchunk_w = nc; g.wce = w; g.xw = xw; g.ngs = ngs; g.nxs = nxs; g.bufu = bufu; g.xoff = ngs * NT;
        g.depth = 3 * bufu * 16 <= WGB_LDS_MAX ? 3 : 2;
        found = true;
      }
    }
  }
  if (!found) return false;
  g.base_w = OW / g.nchunk_w;
  g.rem_w = OW - g.base_w * g.nchunk_w;
  pl->lds_bytes = g.depth * g.bufu * 16;
  g.nrowg = ceil_div(OH, R);
  g.units = B * g.nrowg * g.nchunk_w;
  const int gy = pl->Npad / (32 * NBW), gz = pl->Mpad / (32 * MBW * MPW);
  const int nsplit = imax(1, imin(g.units, 256 / imax(1, gy * gz)));
  g.units_per_split = ceil_div(g.units, nsplit);
  pl->nsplit = ceil_div(g.units, g.units_per_split);
  pl->grid[0] = (unsigned)pl->nsplit; pl->grid[1] = (unsigned)gy; pl->grid[2] = (unsigned)gz;
  return true;
}

// Weight (+bias) gradient on the bf16 matrix cores: v_mfma_f32_32x32x16_bf16 with the contraction over OUTPUT PIXELS.
// bf16 training counterpart of wgrad_f32.hip (cuDNN backward-filter behind loss.backward(), yogo/train.py:322, under --half).
//
//   dW[t][co][ci] = sum_{b, pixel} g[b][co][pixel] * x[b][ci][pixel*stride + tap t]
//
// Both operands arrive in NCHW8c (channel-fastest 16-byte units) but the MFMA wants, per lane, 8 consecutive PIXELS of one
// channel.  The transpose is done by the LDS hardware: tiles are staged as [pixel][32 channels] bf16 (64 B per pixel, plain
// 16-byte copies of the global units) and read with ds_read_b64_tr_b16, which hands each lane 4 pixels of "its" channel per
// instruction; tap shifts move the address by whole 64-byte pixels, so every read stays aligned.
//
// Work decomposition: a "unit" is R output rows x one column chunk of one image.  A workgroup owns MBW * MPW co-blocks x
// NBW ci-blocks of 32 channels and walks its share of the units (split-K over pixels); its wavefronts are
// MBW x NBW x KS pixel-splits x 3 kernel rows, each holding MPW x 3 accumulator tiles.  Units stream through a ring of LDS buffers
// by LDS-DMA (buffer_load ... lds): every lane owns a fixed set of 16-byte elements of the tile image, their source offsets
// are decoded once, per unit only the unit's origin is added and the image / chunk borders are turned into out-of-range
// offsets (which the buffer unit writes as zeros).  One barrier per unit, up to two units in flight ahead of the MFMAs.  Split-K
// slabs + the fixed-order reduction of wgrad_reduce.hip (clamp, OIHW, bias) finish the gradient.
//
// The plan (tiling, chunks, ring, which loop) is wgrad_bf16_plan.h's; the kernel has ONE step skeleton (run_steps below) that the
// three unrolled loops -- BLK4, LEAN, LEAN2 -- fill with their operand addresses, their step count and their DMA slot schedule,
// and a run-time loop (generic) for the tilings whose steps have no affine addresses, built from the same pieces.
#include "bf16_dev.h"
#include "wgrad_bf16_plan.h"
#include "wgrad_reduce.h"

struct WgradBf16Params {
  const u32x4* x;   // [B][Nb][IH][IW] units
  const u32x4* g;   // [B][Mbk][OH][OW] units
  float* slab;      // [nsplit*KS][T][Mpad][Npad]
  float* bias_part; // optional [nsplit*KS][Mpad]
  int Nb, Mbk, Npad, Mpad, IH, IW, OH, OW, pad;
  WbGeom geo;       // the plan's part (wgrad_bf16_plan.h)
};
// compile-time ablations of the product build (build.sh variant TAG wgrad_bf16 -DWGB_ABL=bits + tools/ab_variants.py; timings only, the
// results are wrong): 1 = no MFMAs, 2 = no operand reads, 4 = no LDS-DMA, 8 = every DMA piece out of range (zero fill, no memory traffic)
#ifndef WGB_ABL
#define WGB_ABL 0
#endif
constexpr bool wb_abl(int bit) { return (WGB_ABL & bit) != 0; }

// counted wait for this wavefront's LDS-DMA (dma16 of bf16_dev.h: the loads are invisible to hipcc): at most n of its newest loads
// may still be in flight
__device__ __forceinline__ void wait_dma(int n) {
  switch (n) {
#define WD_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    WD_CASE(1) WD_CASE(2) WD_CASE(3) WD_CASE(4) WD_CASE(5) WD_CASE(6) WD_CASE(7) WD_CASE(8) WD_CASE(9) WD_CASE(10) WD_CASE(11) WD_CASE(12) WD_CASE(13) WD_CASE(14) WD_CASE(15) WD_CASE(16)
#undef WD_CASE
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// f(integral_constant<int, k>) for the run-time k in 1 .. MAXK (the planner gives no other): one copy of a loop per number of steps in a
// staged row, so that the steps of a unit unroll completely
template <int MAXK, class F>
__device__ __forceinline__ void with_steps_per_row(int k, F&& f) {
  static_assert(MAXK == 3 || MAXK == 4, "steps per row: wce / 16 <= 4");
  switch (k) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: if constexpr (MAXK == 4) f(std::integral_constant<int, 4>{}); break;
  }
}

// Which of the next unit's WGB_GSLOTS + WGB_XSLOTS DMA slots (gradient slots first) ride behind the MFMAs of step e: [lo(e), hi(e)).
// Issued in one block behind the barrier, the DMA of 12 wavefronts (address checks + 96 kilobyte-pieces through the CU's one address
// unit) kept the matrix pipe idle for a quarter of every unit (stamps: 1.5 k of 9 k ticks, plus the skew it leaves between the
// wavefronts at the next barrier) -- so every unrolled loop spreads the slots over its steps:
//   SlotsPerStep  BLK4: one slot behind each of the NS ordinary steps, the rest behind the last of them (none behind a wide chunk's extra step)
//   SlotsPerRow   LEAN / LEAN2: KSL slots behind the first step of each of the ROWS rows a wavefront walks (KR steps per row)
constexpr int WGB_SLOTS = WGB_GSLOTS + WGB_XSLOTS;
template <int NS>
struct SlotsPerStep {
  static constexpr int lo(int e) { return e < NS ? e : WGB_SLOTS; }
  static constexpr int hi(int e) { return e < NS - 1 ? e + 1 : WGB_SLOTS; }
};
template <int ROWS, int KR>
struct SlotsPerRow {
  static constexpr int KSL = (WGB_SLOTS + ROWS - 1) / ROWS;
  static constexpr int lo(int e) { return e % KR == 0 && e / KR * KSL < WGB_SLOTS ? e / KR * KSL : WGB_SLOTS; }
  static constexpr int hi(int e) { return e % KR == 0 && (e / KR + 1) * KSL < WGB_SLOTS ? (e / KR + 1) * KSL : WGB_SLOTS; }
};

// MPW: co-blocks per wavefront (the wavefront grid is MBW x NBW x KS x kernel rows; a workgroup covers MBW * MPW co-blocks and
// NBW ci-blocks).  MPW = 2 reads 4 + 6 transposed operand halves per 6 MFMAs where two ci-blocks per wavefront would read 2 + 12.
// PACK2 (16 input channels): the 32 output columns of an MFMA hold TWO taps -- lanes of columns 16-31 read the input one pixel
// further instead of re-reading channels that do not exist -- so a kernel row costs 2 MFMAs and 4 B reads instead of 3 and 6.
// BLK4 (the 128 x 64 tiling, stride 1): a k-step is a BLOCK of 4 rows x 4 columns of the unit (R = 4 rows, staged width 36 = 9 steps) instead of
// 16 consecutive pixels of a row.  A row of 129 (= 8 x 16 + 1) or 258 output columns cannot be cut into 16-column steps without 10 - 12 %
// zero padding whatever the chunking; cut into 4-column blocks the chunks are 32 or 33 columns wide (8 steps, a ninth for the wide ones) and
// the padding is 2.3 % in the columns + 1.6 - 3 % in the rows: 7.4 - 7.9 % fewer MFMAs on layers 3 / 5 / 6.
template <int MBW, int NBW, int KS, int T, int S, int R, int MPW = 1, bool PACK2 = false, bool BLK4 = false>
__global__ __launch_bounds__(64 * MBW * NBW * KS * (T == 1 ? 1 : 3)) void wgrad_bf16_kernel(const WgradBf16Params p) {
  static_assert(!BLK4 || (KS == 1 && !PACK2 && S == 1 && T == 9 && R == 4), "BLK4: the lean 3x3 stride-1 loop only");
  static_assert(MPW == 1 || KS == 1, "two co-blocks per wavefront: the lean loops only");
  // LEAN: the instruction-lean step loop below (one pixel split per wavefront grid, 64-byte pixels in the staged x image; the
  // planner only gives KS = 1 tilings xcb = 4)
  constexpr bool LEAN = KS == 1 && !PACK2;
  const WbGeom& q = p.geo;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  constexpr int TG = (T == 1) ? 1 : 3;
  constexpr int TT = T / TG;
  constexpr int TM = PACK2 ? (TT + 1) / 2 : TT;  // MFMAs (B operands, accumulator tiles) per k-step and (co, ci) block pair
  constexpr int NT = 64 * MBW * NBW * KS * TG;
  constexpr int XR = (T == 1) ? R : (R - 1) * S + 3;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tg = wave % TG;
  const int ks = (wave / TG) % KS;
  const int nb = (wave / (TG * KS)) % NBW;
  const int mb = wave / (TG * KS * NBW);
  const int split = blockIdx.x;
  const int n0b = blockIdx.y * (NBW * 4);  // first channel BLOCK (of 8) of this workgroup's ci range
  const int m0b = blockIdx.z * (MBW * MPW * 4);

  f32x16 acc[MPW][TM];
#pragma unroll
  for (int m = 0; m < MPW; ++m)
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.f;
  float bsum[MPW];
#pragma unroll
  for (int m = 0; m < MPW; ++m) bsum[m] = 0.f;
  // bias gradient = row sums of the gradient operand.  LEAN: every wavefront of the first ci-block workgroup takes part (the
  // NBW * TG wavefronts that hold the same operand sum alternate steps, each writes its own partial row); otherwise one does.
  const bool do_bias = p.bias_part != nullptr && blockIdx.y == 0 && (LEAN || (tg == 0 && nb == 0));
  [[maybe_unused]] int bias_turn = nb * TG + tg;   // LEAN: steps until this wavefront's next turn

  const int u_begin = split * q.units_per_split;
  const int u_end = min(q.units, u_begin + q.units_per_split);
  const int gplane = p.OH * p.OW, xplane = p.IH * p.IW;

  // ---- this lane's elements of the tile image: slot i covers LDS unit i*NT + tid -------------------------------------------
  // g image [MBW * MPW][R][wce][4 channel blocks], x image [NBW][XR][xw][4 channel blocks]; element -> (cb, r, c).
  // lc = byte offset inside the image for unit origin (0, 0), rc = r << 16 | c (all ones: never valid)
  int glc[WGB_GSLOTS], xlc[WGB_XSLOTS];
  unsigned grc[WGB_GSLOTS], xrc[WGB_XSLOTS];
  const int gtot = MBW * MPW * 4 * R * q.wce, xtot = NBW * q.xcb * XR * q.xw;
  // a piece (this wavefront's 64 units of a slot) that lies wholly behind the image is not issued: the images can then be packed
  // piece-tight (xoff), and the counted waits below go by what THIS wavefront issues per unit
  int my_pieces = 0;
#pragma unroll
  for (int i = 0; i < WGB_GSLOTS; ++i) my_pieces += (i < q.ngs && i * NT + wave * 64 < gtot) ? 1 : 0;
#pragma unroll
  for (int i = 0; i < WGB_XSLOTS; ++i) my_pieces += (i < q.nxs && i * NT + wave * 64 < xtot) ? 1 : 0;
  {
#pragma unroll
    for (int i = 0; i < WGB_GSLOTS; ++i) {
      const int e = tid + i * NT;
      const int cb3 = e & 3, pix = e >> 2;
      const int rr = pix / q.wce, c = pix - rr * q.wce;
      const int cbg = rr / R, r = rr - cbg * R;
      const int cb = m0b + cbg * 4 + cb3;
      const bool ok = e < gtot && cb < p.Mbk;
      glc[i] = (cb * gplane + r * p.OW + c) * 16;
      grc[i] = ok ? (unsigned)(r << 16 | c) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int i = 0; i < WGB_XSLOTS; ++i) {
      const int e = tid + i * NT;
      const int pix = q.xcb == 4 ? e >> 2 : e >> 1, cb3 = e - pix * q.xcb;
      const int rr = pix / q.xw, c = pix - rr * q.xw;
      const int cbg = rr / XR, r = rr - cbg * XR;
      const int cb = n0b + cbg * 4 + cb3;
      const bool ok = e < xtot && cb < p.Nb;
      xlc[i] = (cb * xplane + r * p.IW + c) * 16;
      xrc[i] = ok ? (unsigned)(r << 16 | c) : 0xFFFFFFFFu;
    }
  }

  // ---- LDS-DMA of the next unit ------------------------------------------------------------------------------------------
  // the unit whose DMA is issued next: (image, row group, column chunk), stepped without divisions
  int iu_cw = u_begin % q.nchunk_w, iu_rg = (u_begin / q.nchunk_w) % q.nrowg, iu_b = u_begin / (q.nchunk_w * q.nrowg);
  // geometry of that unit (scalars) for LDS buffer `buf`; advances the iterators
  struct NextUnit {
    i32x4 rs_g, rs_x;
    unsigned lb;
    int gorg, rmax, iy0, ix0, xorg, wc, xneed;
  };
  auto next_unit = [&](int buf) __attribute__((always_inline)) {
    const int b_ = iu_b, oy0_ = iu_rg * R, ox0_ = iu_cw * q.base_w + min(iu_cw, q.rem_w);
    const int wc_ = q.base_w + (iu_cw < q.rem_w ? 1 : 0);
    if (++iu_cw == q.nchunk_w) {
      iu_cw = 0;
      if (++iu_rg == q.nrowg) { iu_rg = 0; ++iu_b; }
    }
    NextUnit n;
    n.rs_g = rsrc(p.g + (size_t)b_ * p.Mbk * gplane, p.Mbk * gplane * 16);
    n.rs_x = rsrc(p.x + (size_t)b_ * p.Nb * xplane, p.Nb * xplane * 16);
    n.lb = (unsigned)((buf * q.bufu + wave * 64) * 16);  // the dynamic LDS block starts at LDS address 0
    n.gorg = (oy0_ * p.OW + ox0_) * 16; n.rmax = p.OH - oy0_;
    n.iy0 = oy0_ * S - p.pad; n.ix0 = ox0_ * S - p.pad;
    n.xorg = (n.iy0 * p.IW + n.ix0) * 16;
    n.wc = wc_;
    // input columns this chunk's VALID gradient columns touch: the rest of the staged width is zero-filled, not fetched
    n.xneed = (wc_ - 1) * S + (T == 1 ? 1 : 3);
    return n;
  };
  // slots [LO, HI) of it, one piece each (gradient slots first)
  auto issue_slots = [&](const NextUnit& n, auto lo_tag, auto hi_tag) __attribute__((always_inline)) {
    constexpr int LO = decltype(lo_tag)::value, HI = decltype(hi_tag)::value;
#pragma unroll
    for (int sl = LO; sl < HI; ++sl) {
      if (sl < WGB_GSLOTS) {
        const int i = sl;
        if (i < q.ngs && i * NT + wave * 64 < gtot && !wb_abl(4)) {
          const int c_ = (int)(grc[i] & 0xFFFFu), r_ = (int)(grc[i] >> 16);
          const bool ok_ = (c_ < n.wc) && (r_ < n.rmax) && !wb_abl(8);
          dma16(n.rs_g, n.lb + i * NT * 16, ok_ ? glc[i] + n.gorg : (int)OOB);
        }
      } else {
        const int i = sl - WGB_GSLOTS;
        if (i < q.nxs && i * NT + wave * 64 < xtot && !wb_abl(4)) {
          const int c_ = (int)(xrc[i] & 0xFFFFu), r_ = (int)(xrc[i] >> 16);
          const bool ok_ = ((unsigned)(n.iy0 + r_) < (unsigned)p.IH) && ((unsigned)(n.ix0 + c_) < (unsigned)p.IW) && (c_ < n.xneed) && !wb_abl(8);
          dma16(n.rs_x, n.lb + (q.xoff + i * NT) * 16, ok_ ? xlc[i] + n.xorg : (int)OOB);
        }
      }
    }
  };
  constexpr std::integral_constant<int, 0> SLOT0{};
  constexpr std::integral_constant<int, WGB_SLOTS> SLOTS_END{};

  // ---- per-lane operand addressing for the transposed reads ----------------------------------------------------------
  // 16-lane group gi: channel half (gi & 1) of the 32-channel block, pixel half (gi >> 1) of the 16-pixel k-step;
  // inside the group lane 4q + pc supplies the address of pixel row q, channels 4pc .. 4pc+3.
  const int gi = lane >> 4, q4 = (lane & 15) >> 2, pc = lane & 3;
  const int lane_ch_off = ((gi & 1) * 16 + pc * 4) * 2;   // bytes inside the 64-byte pixel
  const int lane_px = (gi >> 1) * 8 + q4;                 // pixel inside the k-step (second read: +4)
  const int ksteps_row = q.wce >> 4;
  const int nsteps = R * ksteps_row;
  const int cnt = (nsteps - ks + KS - 1) / KS;
  const int xpb = q.xcb * 16;                             // bytes per pixel of the x image (64, or 32 for 16-channel inputs)
  const int xblk = XR * q.xw * xpb;                       // bytes of one channel-block group of the x image
  const int gbase = mb * MPW * (R * q.wce * 64) + lane_ch_off;
  // 16-channel image: the lanes of channels 16-31 re-read channels 0-15 (those output columns lie beyond N and are dropped)
  const int xbase = q.xoff * 16 + nb * xblk + (lane_ch_off & (xpb - 1)) + (PACK2 ? (gi & 1) * xpb : 0);
  // (BLK4: k = 8 (gi >> 1) + 4 j + q -> block row 2 (gi >> 1) + j (j = the first / second transposed read), block column q)
  [[maybe_unused]] const int lean_a0 = BLK4 ? gbase + ((gi >> 1) * 2 * q.wce + q4) * 64 : gbase + lane_px * 64;                                     // (xpb = 64 on this path)
  [[maybe_unused]] const int lean_b0 = BLK4 ? xbase + (((gi >> 1) * 2 + tg) * q.xw + q4) * 64 : xbase + ((T == 1 ? 0 : tg) * q.xw + lane_px * S) * 64;

  // ---- the pieces of a step: MFMAs of one operand set, bias sum of its A operand --------------------------------------
  auto mfma = [&](const bf16x8 (&av)[MPW], const bf16x8 (&bv)[TM]) __attribute__((always_inline)) {
    if (wb_abl(1)) return;
#pragma unroll
    for (int m = 0; m < MPW; ++m)
#pragma unroll
      for (int t = 0; t < TM; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[m], bv[t], acc[m][t], 0, 0, 0);
  };
  // bias gradient: the A operand already holds 8 pixels of "this lane's" output channel (padding pixels are zeros).  TURNS: the
  // NBW * TG wavefronts that hold the same gradient operand take turns summing it
  auto bias = [&](const bf16x8 (&av)[MPW], auto turns_tag) __attribute__((always_inline)) {
    if (do_bias) {
      if constexpr (decltype(turns_tag)::value) {
        if (--bias_turn >= 0) return;
        bias_turn = NBW * TG - 1;
      }
#pragma unroll
      for (int m = 0; m < MPW; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[m] += (float)av[m][j];
    }
  };

  // ---- the step skeleton of the unrolled loops --------------------------------------------------------------------------
  // fetch(0); per step e: fetch(e + 1) into the other register set, the MFMAs of set e, the slots of the next unit that Slots puts
  // behind step e, the bias sum, sched_barrier.  A wavefront beside two MFMA-busy partners issues an instruction only every 5-10
  // cycles, so a step is kept to the ds_reads and the MFMAs themselves -- the NS steps of a unit are unrolled, every step-dependent
  // part of an operand address (step * 1 KB, tap * 64 B, second pixel half + 256 B) is an immediate of the ds_read, and the operands
  // of step e + 1 are requested before the MFMAs of step e (two register sets): with one set the 10 transposed reads of a step and
  // its 6 MFMAs alternated, and the three wavefronts of a SIMD did not cover each other (stamps: reads alone 4.5 k, MFMAs alone
  // 4.4 k, together 8.2 k ticks per unit).  `extra` (BLK4's wide chunk, uniform): one more step behind the NS unrolled ones.
  auto run_steps = [&](auto ns_tag, auto slots, auto turns_tag, bool extra, const NextUnit& nu, bool issue_, auto&& fetch) __attribute__((always_inline)) {
    constexpr int NS = decltype(ns_tag)::value;
    using Slots = decltype(slots);
    if (wb_abl(2)) {   // (ablation: no operand reads -- the DMA still goes out)
      if (issue_) issue_slots(nu, SLOT0, SLOTS_END);
      return;
    }
    bf16x8 av[2][MPW], bvv[2][TM];
    fetch(std::integral_constant<int, 0>{}, av[0], bvv[0]);
    auto step = [&](auto e_tag) __attribute__((always_inline)) {
      constexpr int e = decltype(e_tag)::value, set = e & 1;
      if constexpr (e + 1 < NS) fetch(std::integral_constant<int, e + 1>{}, av[set ^ 1], bvv[set ^ 1]);
      else if constexpr (BLK4 && e + 1 == NS) { if (extra) fetch(std::integral_constant<int, NS>{}, av[set ^ 1], bvv[set ^ 1]); }
      mfma(av[set], bvv[set]);
      if (issue_) issue_slots(nu, std::integral_constant<int, Slots::lo(e)>{}, std::integral_constant<int, Slots::hi(e)>{});
      bias(av[set], turns_tag);
      __builtin_amdgcn_sched_barrier(0);
    };
    static_for(step, std::make_integer_sequence<int, NS>{});
    if constexpr (BLK4) { if (extra) step(std::integral_constant<int, NS>{}); }
  };

  // ring of q.depth LDS buffers: unit u + depth - 1 streams in while unit u is multiplied.  Ordering (LDS-DMA is invisible to
  // the barrier): every wave waits for ITS loads of unit u with a counted vmcnt, then the barrier makes all of them visible and
  // proves that nobody still reads the buffer the next issue overwrites.
  for (int d = 0; d + 1 < q.depth; ++d)
    if (u_begin + d < u_end) issue_slots(next_unit(d), SLOT0, SLOTS_END);
  int ib = 0;
  // LEAN2: the pixel-split tilings (KS > 1: the 16/32/64-channel layers) with whole ROWS dealt to the splits (row r belongs to
  // split r mod KS) instead of single steps: a wavefront's steps then have affine addresses -- a per-wavefront base plus
  // immediates -- and unroll like the lean loop; the generic loop divides and multiplies its way to every operand address
  // (and, with the DMA switched off entirely, still takes 0.65 of the layer-1 kernel's 0.76 ms: it is bound by instruction
  // issue, not by memory).  Needs R % KS == 0 and the pixel size of the staged input image known at compile time.
  constexpr bool LEAN2_OK = KS > 1 && (R % KS == 0) && MPW == 1;
  // mode 1: BLK4 / LEAN, 2: LEAN2, 0: generic; KR: 16-pixel steps per staged row (BLK4: unused)
  auto unit_loop = [&](auto kr_tag, auto mode_tag) {
    [[maybe_unused]] constexpr int KR = decltype(kr_tag)::value;
    constexpr int MODE = decltype(mode_tag)::value;
    for (int u = u_begin; u < u_end; ++u) {
      wait_dma(max(0, min(q.depth - 2, u_end - 1 - u)) * my_pieces);   // (the units behind u that are already in flight)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const int ahead = q.depth - 1;
      const bool issue_ = u + ahead < u_end;
      int nb_ = ib + ahead;
      nb_ = nb_ >= q.depth ? nb_ - q.depth : nb_;
      if constexpr (MODE == 0) {
        if (issue_) issue_slots(next_unit(nb_), SLOT0, SLOTS_END);
      }
      const unsigned char* buf = smem_b + ib * q.bufu * 16;
      ib = ib + 1 == q.depth ? 0 : ib + 1;
      if constexpr (BLK4) {
        const NextUnit nu = next_unit(nb_);
        // this unit's chunk: 33 - 36 columns take a ninth step
        constexpr int NSB = 8;
        const int cwi_ = u % q.nchunk_w;
        const bool wide = q.base_w + (cwi_ < q.rem_w ? 1 : 0) > 4 * NSB;   // uniform
        // (one staged width, WGB_BLK4_W: the row pitches of both images are immediates of the ds_reads, two base registers in all)
        constexpr int ROWA = WGB_BLK4_W * 64, ROWX = (WGB_BLK4_W + 2) * 64;
        const unsigned char* pa0 = buf + lean_a0;
        const unsigned char* pb0 = buf + lean_b0;
        run_steps(std::integral_constant<int, NSB>{}, SlotsPerStep<NSB>{}, std::true_type{}, wide, nu, issue_,
                  [&](auto e_tag, bf16x8 (&av)[MPW], bf16x8 (&bv)[TM]) __attribute__((always_inline)) {
                    constexpr int e = decltype(e_tag)::value;
                    av[0] = lds_tr8(pa0 + e * 256, pa0 + (ROWA + e * 256));
#pragma unroll
                    for (int t = 0; t < TM; ++t) bv[t] = lds_tr8(pb0 + (e * 256 + t * 64), pb0 + (ROWX + e * 256 + t * 64));
                    if constexpr (MPW == 2) av[1] = lds_tr8(pa0 + (R * ROWA + e * 256), pa0 + (R * ROWA + ROWA + e * 256));
                  });
      } else if constexpr (LEAN) {
        const NextUnit nu = next_unit(nb_);
        const unsigned char* pa0 = buf + lean_a0;
        const unsigned char* pa1 = buf + lean_a0 + R * q.wce * 64;
        const unsigned char* pb0 = buf + lean_b0;
        const int rowb = S * q.xw * 64;
        run_steps(std::integral_constant<int, R * KR>{}, SlotsPerRow<R, KR>{}, std::true_type{}, false, nu, issue_,
                  [&](auto e_tag, bf16x8 (&av)[MPW], bf16x8 (&bv)[TM]) __attribute__((always_inline)) {
                    constexpr int e = decltype(e_tag)::value, r = e / KR, kx = e % KR;
                    av[0] = lds_tr8(pa0 + e * 1024, pa0 + (e * 1024 + 256));
                    const unsigned char* pb = pb0 + r * rowb;
#pragma unroll
                    for (int t = 0; t < TM; ++t) bv[t] = lds_tr8(pb + (kx * 1024 * S + t * 64), pb + (kx * 1024 * S + t * 64 + 256 * S));
                    if constexpr (MPW == 2) av[1] = lds_tr8(pa1 + e * 1024, pa1 + (e * 1024 + 256));
                  });
      } else if constexpr (MODE == 2) {
        constexpr int RJ = (R / KS) > 0 ? R / KS : 1, XPB = PACK2 ? 32 : 64;  // (RJ >= 1 wherever LEAN2_OK holds)
        const NextUnit nu = next_unit(nb_);
        const int rowb = S * q.xw * XPB;
        const unsigned char* pa = buf + gbase + lane_px * 64 + ks * (KR * 1024);
        const unsigned char* pb0 = buf + xbase + ((T == 1 ? 0 : tg) * q.xw + lane_px * S) * XPB + ks * rowb;
        run_steps(std::integral_constant<int, RJ * KR>{}, SlotsPerRow<RJ, KR>{}, std::false_type{}, false, nu, issue_,
                  [&](auto e_tag, bf16x8 (&av)[MPW], bf16x8 (&bv)[TM]) __attribute__((always_inline)) {
                    constexpr int e = decltype(e_tag)::value, j = e / KR, kx = e % KR;
                    av[0] = lds_tr8(pa + (j * KS * KR + kx) * 1024, pa + ((j * KS * KR + kx) * 1024 + 256));
                    const unsigned char* pb = pb0 + (j * KS) * rowb;
#pragma unroll
                    for (int t = 0; t < TM; ++t)
                      bv[t] = lds_tr8(pb + (kx * 16 * S + (PACK2 ? 2 * t : t)) * XPB, pb + ((kx * 16 * S + (PACK2 ? 2 * t : t)) * XPB + 4 * S * XPB));
                  });
      } else if (cnt > 0) {
        // generic: step i of this wavefront is step ks + i * KS of the unit; operands of step i + 1 are fetched before the MFMAs of step i
        auto load = [&](bf16x8 (&av)[MPW], bf16x8 (&bv)[TM], int i) __attribute__((always_inline)) {
          const int st_ = ks + min(i, cnt - 1) * KS;
          const int r_ = st_ / ksteps_row;
          const int px_ = (st_ - r_ * ksteps_row) * 16 + lane_px;
          const unsigned char* pa = buf + (gbase + (r_ * q.wce + px_) * 64);
          av[0] = lds_tr8(pa, pa + 4 * 64);
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            const unsigned char* pb = buf + (xbase + (((r_ * S + (T == 1 ? 0 : tg)) * q.xw) + px_ * S + (PACK2 ? 2 * t : t)) * xpb);
            bv[t] = lds_tr8(pb, pb + 4 * S * xpb);
          }
        };
        bf16x8 a0[MPW], a1[MPW], b0[TM], b1[TM];
        load(a0, b0, 0);
        int i = 0;
        for (; i + 1 < cnt; i += 2) {
          load(a1, b1, i + 1);
          __builtin_amdgcn_sched_barrier(0);
          mfma(a0, b0);
          bias(a0, std::false_type{});
          __builtin_amdgcn_sched_barrier(0);
          load(a0, b0, i + 2);
          __builtin_amdgcn_sched_barrier(0);
          mfma(a1, b1);
          bias(a1, std::false_type{});
          __builtin_amdgcn_sched_barrier(0);
        }
        if (i < cnt) {
          mfma(a0, b0);
          bias(a0, std::false_type{});
        }
      }
    }
  };
  if constexpr (BLK4) {
    unit_loop(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
  } else if constexpr (LEAN) {
    // (no KS = 1 plan stages 64 columns -- the planner sweep of profiles/wgrad_bf16_one_definition.log; the launcher refuses one)
    with_steps_per_row<3>(ksteps_row, [&](auto kr_tag) { unit_loop(kr_tag, std::integral_constant<int, 1>{}); });
  } else if constexpr (LEAN2_OK) {
    if (q.xcb == (PACK2 ? 2 : 4)) with_steps_per_row<4>(ksteps_row, [&](auto kr_tag) { unit_loop(kr_tag, std::integral_constant<int, 2>{}); });
    else unit_loop(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
  } else {
    unit_loop(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
  }

  // ---- write the slab: [split*KS + ks][t][m][n] ----------------------------------------------------------------------
  float* sl = p.slab + (size_t)(split * KS + ks) * T * p.Mpad * p.Npad;
  const int m0 = m0b * 8, n0 = n0b * 8;
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      // PACK2: column l31 of tile t = input channel l31 & 15 of tap 2t + (l31 >> 4)
      const int tap = PACK2 ? 2 * t + (l31 >> 4) : t;
      const int n = n0 + nb * 32 + (PACK2 ? (l31 & 15) : l31);
      if (tap < TT) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + (mb * MPW + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          sl[((size_t)(tg * TT + tap) * p.Mpad + m) * p.Npad + n] = acc[mi][t][r];
        }
      }
    }
  if (do_bias) {  // lane l31 and lane l31 + 32 hold the two pixel halves of channel (mb*MPW + mi)*32 + l31
    const int brow = LEAN ? (split * KS + ks) * (NBW * TG) + nb * TG + tg : split * KS + ks;   // (host: WbPlan::bias_rows)
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const float tot = bsum[mi] + __shfl_xor(bsum[mi], 32, 64);
      if (half == 0) p.bias_part[(size_t)brow * p.Mpad + m0 + (mb * MPW + mi) * 32 + l31] = tot;
    }
  }
}

namespace {

thread_local char g_wb_plan_txt[320] = "";  // planner parameters of the launch in flight (launch log)

// One instantiation: the plan it serves and its launch.
template <int MBW, int NBW, int KS, int T, int S, int R, int MPW = 1, bool PACK2 = false, bool BLK4 = false>
struct WbInst {
  static bool serves(const WbPlan& pl) {
    return pl.MBW == MBW && pl.NBW == NBW && pl.KS == KS && pl.T == T && pl.S == S && pl.R == R && pl.MPW == MPW && pl.pack2 == PACK2 && pl.blk4 == BLK4;
  }
  static int launch(const WgradBf16Params& p, const WbPlan& pl, hipStream_t stream) {
    const auto kernel = &wgrad_bf16_kernel<MBW, NBW, KS, T, S, R, MPW, PACK2, BLK4>;
    if (int e = yogo_func_dynamic_lds(reinterpret_cast<const void*>(kernel), WGB_LDS_MAX, "wgrad_bf16")) return e;
    hipLaunchKernelGGL(kernel, dim3(pl.grid[0], pl.grid[1], pl.grid[2]), dim3(pl.threads()), pl.lds_bytes, stream, p);
    yogo_launch_log("wgrad_bf16_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s> | %s", MBW, NBW, KS, T, S, R, MPW, PACK2 ? "true" : "false", BLK4 ? "true" : "false",
                    g_wb_plan_txt);
    return YOGO_OK;
  }
};
// a wavefront grid at 1x1, at 3x3 stride 1 and at 3x3 stride 2
template <int MBW, int NBW, int KS>
using WbGrid = std::tuple<WbInst<MBW, NBW, KS, 1, 1, 4>, WbInst<MBW, NBW, KS, 9, 1, 4>, WbInst<MBW, NBW, KS, 9, 2, 2>>;
// THE table: every instantiation a plan of wb_plan can ask for (22; tests/test_gpu_conv_bf16_exact.py: WGRAD_EXPECTED launches each)
using WbTable = decltype(std::tuple_cat(WbGrid<4, 1, 1>{}, WbGrid<2, 2, 1>{}, WbGrid<2, 1, 2>{}, WbGrid<1, 4, 1>{}, WbGrid<1, 2, 2>{}, WbGrid<1, 1, 4>{},
                                        std::tuple<WbInst<2, 2, 1, 9, 1, 4, 2, false, true>,    // 128 x 64 workgroup tile, stride 1: BLK4
                                                   WbInst<2, 2, 1, 9, 2, 2, 2>,                 // ... stride 2
                                                   WbInst<1, 1, 4, 9, 1, 8, 1, true>,           // tall units, 16 input channels: PACK2
                                                   WbInst<1, 1, 4, 9, 1, 8>>{}));               // tall units
template <class... I>
int wb_launch(std::tuple<I...>, const WgradBf16Params& p, const WbPlan& pl, hipStream_t stream) {
  int rc = YOGO_ERR_ARG;
  const bool hit = ((I::serves(pl) && ((rc = I::launch(p, pl, stream)), true)) || ...);
  if (!hit) yogo_set_error("wgrad_bf16: no kernel for the plan <%d, %d, %d, %d, %d, %d, %d, %d, %d>", pl.MBW, pl.NBW, pl.KS, pl.T, pl.S, pl.R, pl.MPW, (int)pl.pack2, (int)pl.blk4);
  return rc;
}

}  // namespace

extern "C" int yogo_conv2d_wgrad_bf16_workspace_bytes(int B, int Cin, int Cout, int IH, int IW, int ks, int stride, size_t* bytes) {
  YOGO_CHECK_ARG(bytes && B > 0 && Cin > 0 && Cout > 0 && IH > 0 && IW > 0 && (ks == 1 || ks == 3) && (stride == 1 || stride == 2),
                 "wgrad_bf16_workspace_bytes: bad arguments");
  WbPlan pl;
  YOGO_CHECK_ARG(wb_plan(B, Cin, Cout, IH, IW, ks, stride, &pl), "wgrad_bf16: no LDS plan");
  // slabs + bias partial rows
  *bytes = ((size_t)pl.slab_floats() + (size_t)pl.bias_rows() * pl.Mpad) * sizeof(float);
  return YOGO_OK;
}

// fp32 dw (OIHW) / db from bf16 NCHW8c x and g on the bf16 matrix cores (fp32 accumulation); clamped to +-clip when clip > 0
static int conv2d_wgrad_bf16_impl(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout, int IH, int IW,
                                 int ks, int stride, float clip, void* queue, hipStream_t stream);
extern "C" int yogo_conv2d_wgrad_bf16(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout,
                                      int IH, int IW, int ks, int stride, float clip, hipStream_t stream) {
  return conv2d_wgrad_bf16_impl(x, g, dw, db, workspace, B, Cin, Cout, IH, IW, ks, stride, clip, nullptr, stream);
}
// the same with the split-K reduction DEFERRED: it is recorded in `queue` (yogo_wgrad_reduce_queue_create) and runs, together with
// every other recorded one, when yogo_wgrad_reduce_flush(queue, stream) is called -- one launch for the weight gradients of a
// whole backward pass instead of one per layer.  dw / db / workspace must stay valid until then; same bits as the immediate form.
extern "C" int yogo_conv2d_wgrad_bf16_deferred(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout,
                                               int IH, int IW, int ks, int stride, float clip, void* queue, hipStream_t stream) {
  YOGO_CHECK_ARG(queue != nullptr, "conv2d_wgrad_bf16_deferred: null queue");
  return conv2d_wgrad_bf16_impl(x, g, dw, db, workspace, B, Cin, Cout, IH, IW, ks, stride, clip, queue, stream);
}
static int conv2d_wgrad_bf16_impl(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout, int IH, int IW,
                                 int ks, int stride, float clip, void* queue, hipStream_t stream) {
  YOGO_CHECK_ARG(x && g && dw && workspace, "conv2d_wgrad_bf16: null pointer");
  YOGO_CHECK_ARG(B > 0 && Cin > 0 && Cout > 0 && IH > 0 && IW > 0 && (ks == 1 || ks == 3) && (stride == 1 || stride == 2) &&
                     !(ks == 1 && stride != 1), "conv2d_wgrad_bf16: bad shape");
  WbPlan pl;
  YOGO_CHECK_ARG(wb_plan(B, Cin, Cout, IH, IW, ks, stride, &pl), "wgrad_bf16: no LDS plan");
  // (the LEAN loop has copies for 1, 2 and 3 steps per row: the planner sweep finds no KS = 1 row-step plan that stages 64 columns)
  YOGO_CHECK_ARG(!(pl.lean && !pl.blk4 && pl.g.wce > 48), "wgrad_bf16: a KS = 1 plan with more than 3 steps per row");
  WgradBf16Params p{};
  p.x = reinterpret_cast<const u32x4*>(x); p.g = reinterpret_cast<const u32x4*>(g);
  p.slab = reinterpret_cast<float*>(workspace);
  p.bias_part = db ? p.slab + pl.slab_floats() : nullptr;
  p.Nb = ((Cin + 15) / 16) * 2; p.Mbk = ((Cout + 15) / 16) * 2; p.Npad = pl.Npad; p.Mpad = pl.Mpad;
  p.IH = IH; p.IW = IW; p.OH = pl.OH; p.OW = pl.OW; p.pad = pl.pad;
  p.geo = pl.g;
  if (yogo_launch_log_enabled())
    snprintf(g_wb_plan_txt, sizeof(g_wb_plan_txt), "N=%d M=%d in=%dx%d s=%d T=%d B=%d R=%d wce=%d nchunk_w=%d base_w=%d rem_w=%d xw=%d xcb=%d slots=%d+%d depth=%d lds=%d units=%d units_per_split=%d grid=%ux%ux%u",
             Cin, Cout, IH, IW, stride, pl.T, B, pl.R, pl.g.wce, pl.g.nchunk_w, pl.g.base_w, pl.g.rem_w, pl.g.xw, pl.g.xcb, pl.g.ngs, pl.g.nxs, pl.g.depth, pl.lds_bytes,
             pl.g.units, pl.g.units_per_split, pl.grid[0], pl.grid[1], pl.grid[2]);
  if (int lrc = wb_launch(WbTable{}, p, pl, stream)) return lrc;
  YOGO_CHECK_LAUNCH("conv2d_wgrad_bf16");
  return yogo_internal_wgrad_reduce_q(queue, p.slab, pl.slabs(), pl.T, Cout, Cin, pl.Mpad, pl.Npad, clip, dw, p.bias_part, pl.bias_rows(), db, stream);
}

// Layers 1 and 2 of base_model forward (yogo/model_defns.py:39-46: 3x3 stride 1 out of 16 into <= 32 channels, then 3x3 stride 2 out of those
// into <= 64, both LeakyReLU blocks without BatchNorm) in ONE launch: layer 2 takes y1 from LDS, not from memory.  conv_bf16_staged.hip's
// scheme -- both layers' packed weights resident in LDS (9 + 36 KB, staged once per workgroup), INDEPENDENT wavefronts, every wavefront stages
// ITS y0 rows into ITS OWN piece of LDS by LDS-DMA and waits for them with its own vmcnt, no barrier after the weight staging -- and layer 1's
// epilogue writes the y1 tile image, in the layout the stride-2 staged kernel reads, INTO THAT SAME PIECE (below).
//
// y1 and its sign map are STILL WRITTEN (layer 2's weight and data gradients read them): what goes is layer 2's read of y1, 1.8 of the pair's
// 5.35 GB.  Every stored tensor is bit-identical to the two conv_bf16_staged_kernel launches: the same products in the same order per
// accumulator (layer 1: taps 0..8 of its one 16-channel chunk; layer 2: chunk-major, tap-minor), the same lean epilogue statement by statement,
// and layer 2 multiplies the very bf16 units layer 1 stores.
//
// Tile: R2 rows x 31 columns of y2.  Its y1 need is rows 2 oy0 - 1 .. 2 oy0 + 2 R2 - 1 and columns 62 j - 1 .. 62 j + 61: 2 R2 + 1 rows of two
// 32-pixel MFMA blocks (64 columns, the last one spare), of which the tile OWNS -- stores to memory -- rows 2 oy0 .. and columns 62 j .. 62 j + 61;
// row / column -1 of the image belong to the neighbour tile, which stores them.  Computed per tile that is (2 R2 + 1) x 64 pixels of layer 1 for
// 2 R2 x 62 owned, 1.55 x the unfused MFMA count at R2 = 1; the first row is the previous tile's last, and a wavefront that walks DOWN a column
// strip keeps it in registers (below): 1.07 x with runs of 13 tiles (the launch log carries the factor).  y1 positions outside y1's plane
// (row / column -1, row / column OH1 / OW1 where the dimension is odd, the spare column) enter the image as ZEROS -- layer 2's padding -- never
// as layer 1 evaluated on padded y0.
//
// What the forms on the way measured (profiles/pair_fwd_ab.log; the two launches: 1.03 - 1.08 ms by box) and what stayed of each:
//   - LDS decides the occupancy, and one wavefront per SIMD is too few whatever it overlaps (a separate y1 image, 24 KB per wavefront, four per
//     CU: 1.44 ms; the same with a second image and a tile-ahead DMA: 1.36).  So the y1 image costs NO LDS of its own.  It lives in the y0
//     image: layer 1 goes through the tile's y1 rows in order, row r reads y0 image rows r .. r + 2, and once row r's MFMAs are done y0 image
//     row r is dead -- y1 row r of channel block kb lands in the slot of y0 row r of channel block kb (both 66 units).  The y0 image has two
//     channel blocks, y1 has four; layer 2 is chunk-major, its first 16-channel chunk needs y1 blocks 0 / 1 only, so blocks 2 / 3 wait in
//     registers (one 16-byte unit per lane, row and 32-pixel block) and go into the same slots between the two chunks.  11 KB per wavefront at
//     R2 = 1: eight per CU beside the 46 KB of weights, as the stride-2 staged kernel runs.
//   - DMA issue -> vmcnt(0) -> compute -> stores, as the staged kernels run, made every tile wait for the previous tile's stores to be
//     acknowledged (1.11 ms).  Vector-memory operations retire in order (conv_bf16_ws.hip waits the same way), so the next tile's DMA is
//     issued as soon as the image is dead -- behind layer 2's MFMAs -- and IN FRONT of every store of this tile: y1's units wait in registers
//     for that.  "All but the youngest NSTORE", a tile's store count, every one issued unconditionally, is then exactly "the image has
//     landed" (1.09 -> 1.02 ms together with the next item).  The channel scales ride along as LDS-DMA pieces: a vector load into registers
//     would make hipcc wait for everything at its use.
//   - the row carried in registers needs a wavefront to walk down a strip, and the wavefronts of a workgroup to stay side by side: on
//     strips far apart their 1-KB stores lose the neighbours that complete a DRAM page (1.22 ms).
//
// A tile's life: wait for its image -> layer 1 row by row (first row: the carry; MFMAs, epilogue, ds_write of blocks 0 / 1) -> layer 2 chunk 0
// -> ds_write of blocks 2 / 3 -> layer 2 chunk 1 -> DMA issue of the next tile -> y1's stores -> layer 2's epilogue and stores.
#include "bf16_dev.h"
#include "conv_bf16_plan.h"

struct ConvPairParams {
  const u32x4* in;                 // y0: bf16 NCHW8c [B][2][IH][IW] units
  const u32x4* wp1;                // layer 1's packed weights (mode 0): [9][2][32] units
  const float* bias1;              // [M1] or null
  u32x4* out1;                     // y1: [B][4][IH][IW] units
  unsigned char* signs1;           // [B][2][IH][IW][2] bytes
  const float* scale1;             // optional [B][M1]
  const u32x4* wp2;                // layer 2's packed weights (mode 0): [9][4][64] units
  const float* bias2;
  u32x4* out2;                     // y2: [B][Mb2][OH2][OW2] units
  unsigned char* signs2;           // [B][2][OH2][OW2][4] bytes
  const float* scale2;             // optional [B][M2]
  int B, M1, M2, Mb2, IH, IW, OH2, OW2, act;
  int tiles_per_col, tiles_per_row, nstrip, nq, nunit, ntiles;   // nstrip = B x tiles_per_row column strips, nq runs per strip, nunit workgroup units
  unsigned m_tpr, m_nq;            // ceil(2^32 / d) magic numbers
};

#define CP_TW 31   // y2 columns of a tile
#define CP_RUN 13  // tiles of a run: a wavefront walks this many tiles down a column strip (the first one computes one y1 row more)
// (a few taps at a time between scheduling barriers, as conv_bf16_staged.hip; a variant build without them lets hipcc schedule a whole tile)
#ifdef BF_PAIR_NO_SB
#define CP_SCHED_BARRIER()
#else
#define CP_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#endif

namespace {
// (conv_bf16_staged.hip's cs_dma16 / cs_wait_dma: one LDS-DMA piece from inline asm, and the one place the kernel waits for them)
__device__ __forceinline__ void cp_dma16(i32x4 rs, unsigned lds_addr, int voff) { dma16_uniform(uniform4(rs), lds_addr, voff); }
__device__ __forceinline__ void cp_wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// ... but for the N youngest vector-memory operations (N < 64: the counter has six bits)
template <int N>
__device__ __forceinline__ void cp_wait_dma_but() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// the y0 image's LDS reads have all returned (their MFMAs are behind us): its pieces may be overwritten
__device__ __forceinline__ void cp_reads_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// the lean epilogue of one group of eight accumulator registers, conv_bf16_staged_kernel's statement by statement: fma(acc, scale, bias * scale),
// LeakyReLU as max(v, 0.01 v), the sign byte, bf16, half-wave exchange -> lanes 0-31 hold the 16-byte unit of channel block cb, lanes 32-63 of cb + 1
__device__ __forceinline__ u32x4 cp_epi_group(const f32x16& acc, int gp, const float* lds_b, const float* my_scale, int cl, bool leaky, unsigned* sign) {
  const float4 bA = *reinterpret_cast<const float4*>(lds_b + cl), bB = *reinterpret_cast<const float4*>(lds_b + cl + 8);
  const float4 sA = *reinterpret_cast<const float4*>(my_scale + cl), sB = *reinterpret_cast<const float4*>(my_scale + cl + 8);
  const float ba[8] = {bA.x, bA.y, bA.z, bA.w, bB.x, bB.y, bB.z, bB.w};
  const float sa[8] = {sA.x, sA.y, sA.z, sA.w, sB.x, sB.y, sB.z, sB.w};
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = fmaf(acc[8 * gp + i], sa[i], ba[i] * sa[i]);
  if (leaky) {
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      const f32x2 sv = (f32x2){v[i], v[i + 1]} * (f32x2){LEAKY_SLOPE, LEAKY_SLOPE};
      asm("v_max_f32 %0, %1, %2" : "=v"(v[i]) : "v"(v[i]), "v"(sv.x));
      asm("v_max_f32 %0, %1, %2" : "=v"(v[i + 1]) : "v"(v[i + 1]), "v"(sv.y));
    }
  }
  unsigned m = 0;
#pragma unroll
  for (int i = 7; i >= 0; --i) asm("v_cmp_lt_f32_e32 vcc, 0, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(m) : "v"(v[i]) : "vcc");
  *sign = m;
  bf16x8 ob;
#pragma unroll
  for (int i = 0; i < 8; ++i) ob[i] = (__bf16)v[i];
  const u32x4 w = __builtin_bit_cast(u32x4, ob);
  const auto r0 = __builtin_amdgcn_permlane32_swap(w.x, w.z, false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(w.y, w.w, false, false);
  return u32x4{r0[0], r1[0], r0[1], r1[1]};
}
}  // namespace

// R2: y2 rows of a tile; NWV: wavefronts per workgroup
template <int R2, int NWV>
struct PairGeom {
  static constexpr int PW = 33, ROWU = 66;           // units of a staged row: y0 columns 62 j - 2 .. 62 j + 63; y1 [33 even | 33 odd]
  static constexpr int NR1 = 2 * R2 + 1;             // y1 rows of a tile
  static constexpr int NR0 = NR1 + 2;                // y0 rows of a tile
  static constexpr int TU0 = 2 * NR0 * ROWU;         // units of the y0 image
  static constexpr int NDMA = (TU0 + 63) / 64;
  static constexpr int IMGU = NDMA * 64;             // units of an image: the y0 image, then the y1 image in its rows 0 .. NR1 - 1
  static constexpr int WVU = IMGU;                   // units of a wavefront's private piece
  static constexpr int NSTORE = 2 * R2 * 2 * 3 + R2 * 5;   // vector-memory stores of a tile: per owned y1 row and 32-pixel block two units + sign bytes; per y2 row four units + sign bytes
  static constexpr int W1U = 9 * 2 * 32, W2U = 9 * 4 * 64;
  // LDS: weights 1 | weights 2 | bias 1 [32] | bias 2 [64] fp32 | channel scales [NWV][2 images][64 + 64] fp32 | tile images [NWV][WVU]
  static constexpr int OFF_W2 = W1U, OFF_B1 = OFF_W2 + W2U, OFF_B2 = OFF_B1 + 8, OFF_S = OFF_B2 + 16, OFF_T = OFF_S + NWV * 64;
  static constexpr int LDS_BYTES = (OFF_T + NWV * WVU) * 16;
  static_assert(NDMA <= 16, "y0 image too large");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

template <int R2, int NWV>
__global__ __launch_bounds__(64 * NWV) void conv_bf16_staged_pair_kernel(const ConvPairParams p) {
  extern __shared__ __attribute__((aligned(16))) u32x4 lds_u[];   // (the dynamic block starts at LDS address 0: LDS-DMA takes addresses, not pointers)
  using G = PairGeom<R2, NWV>;
  constexpr int PW = G::PW, ROWU = G::ROWU, NR1 = G::NR1, NR0 = G::NR0, TU0 = G::TU0, NDMA = G::NDMA, NT = 64 * NWV;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* lds_b1 = reinterpret_cast<float*>(lds_u + G::OFF_B1);
  float* lds_b2 = reinterpret_cast<float*>(lds_u + G::OFF_B2);
  // a tile's channel scales ride along with its image, as LDS-DMA pieces of their own (a vector load into registers would make hipcc wait
  // for EVERY vector-memory operation where its result is used): per image 64 floats for either layer, the scale of channel `lane`, zeros
  // for the padding channels (out of the descriptor's range); without a scale tensor the slots hold 1 / 0 from here on
  float* const scale0 = reinterpret_cast<float*>(lds_u + G::OFF_S) + wave * 256;
  const unsigned scale0_addr = (unsigned)(G::OFF_S * 16 + wave * 1024);
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    scale0[w * 128 + lane] = lane < p.M1 ? 1.f : 0.f;
    scale0[w * 128 + 64 + lane] = lane < p.M2 ? 1.f : 0.f;
  }
  for (int i = tid; i < G::W1U; i += NT) lds_u[i] = p.wp1[i];
  for (int i = tid; i < G::W2U; i += NT) lds_u[G::OFF_W2 + i] = p.wp2[i];
  for (int i = tid; i < 96; i += NT) {
    if (i < 32) lds_b1[i] = (p.bias1 != nullptr && i < p.M1) ? p.bias1[i] : 0.f;
    else lds_b2[i - 32] = (p.bias2 != nullptr && i - 32 < p.M2) ? p.bias2[i - 32] : 0.f;
  }
  __syncthreads();
  const int IH = p.IH, IW = p.IW, OH2 = p.OH2, OW2 = p.OW2;
  const int kcb = IH * IW * 16, plane1 = IH * IW, plane1_16 = plane1 * 16, plane2 = OH2 * OW2, plane2_16 = plane2 * 16;
  const bool leaky = p.act == ACT_LEAKY;   // uniform
  u32x4* const img0 = lds_u + G::OFF_T + wave * G::WVU;   // image `cur` of this wavefront: img0 + cur * IMGU
  const unsigned img0_addr = (unsigned)((G::OFF_T + wave * G::WVU) * 16);
  // this lane's elements of the y0 image: piece i covers units 64 i + lane -> (channel block, row, column) -> byte offset relative to the
  // tile's first y0 pixel (iy0, ix0), and (row << 16 | column) for the border tests; all ones = beyond the image of the tile
  int rel[NDMA];
  unsigned rc[NDMA];
#pragma unroll
  for (int i = 0; i < NDMA; ++i) {
    const int u = i * 64 + lane;
    const int kb = u / (NR0 * ROWU), rem = u - kb * (NR0 * ROWU);
    const int r = rem / ROWU, col = rem - r * ROWU;
    rel[i] = kb * kcb + (r * IW + col) * 16;
    rc[i] = u < TU0 ? (unsigned)(r << 16 | col) : 0xFFFFFFFFu;
  }
  // stage a tile's y0 image (zeros where layer 1's padding or the image border is: out-of-range offsets)
  // (need0: y0 image row 0 feeds y1 row 0 of the tile only -- not fetched where that row comes out of the carry registers)
  auto stage = [&](int b, int j, int oy0, int which, bool need0) {
    const unsigned y0_addr = img0_addr;   // (`which`: the scale slots, below)
    const int iy0 = 2 * oy0 - 2, ix0 = 2 * CP_TW * j - 2;
    const i32x4 rs_in = rsrc(p.in + (size_t)b * 2 * IH * IW, (unsigned)(2 * kcb));
    const int base = (iy0 * IW + ix0) * 16;
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int r = (int)(rc[i] >> 16), c = (int)(rc[i] & 0xFFFFu);
      const bool ok = ((unsigned)(iy0 + r) < (unsigned)IH) && ((unsigned)(ix0 + c) < (unsigned)IW) && (r > 0 || need0);   // (all ones: r = 65535 fails the row test)
      cp_dma16(rs_in, y0_addr + (unsigned)i * 1024u, ok ? rel[i] + base : (int)OOB);
    }
    if (p.scale1 != nullptr) dma_dword_uniform(rsrc(p.scale1 + (size_t)b * p.M1, (unsigned)(p.M1 * 4)), scale0_addr + (unsigned)(which * 512), lane * 4, 0u);
    if (p.scale2 != nullptr) dma_dword_uniform(rsrc(p.scale2 + (size_t)b * p.M2, (unsigned)(p.M2 * 4)), scale0_addr + (unsigned)(which * 512 + 256), lane * 4, 0u);
  };
  // The walk.  A column strip (image b, tile column j) is cut into RUNS of CP_RUN tiles; a workgroup UNIT is one run of NWV adjacent strips, one
  // strip per wavefront, so that the wavefronts of a workgroup go down the plane side by side and store adjacent 1-KB row segments at about
  // the same time (a wavefront walking a strip of its own far from the others' measured 1.22 ms against 1.09: profiles/pair_fwd_ab.log).
  // Workgroup -> XCD -> a contiguous eighth of the units (conv_bf16_staged.hip); consecutive units are the runs of one strip group, top to bottom.
  // Within a run the last y1 row of a tile is the first of the next (row 2 oy0 + 2 R2 - 1): its eight units per lane stay in registers
  // (`carry`), so layer 1 computes it once.  A run's first tile computes it afresh, but at the top of a strip it is row -1 of the plane: zeros.
  struct Pos { int unit, b, j, ty, ty_end; };
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
  const int u8 = (p.nunit + 7) >> 3, u_end = min(p.nunit, (xcd + 1) * u8);
  // the first unit from `unit` on (stepping by the workgroups of the XCD) in which this wavefront has a strip; false: none
  auto open_unit = [&](int unit, Pos* q) {
    for (; unit < u_end; unit += nslot) {
      const int sg = udivm1(unit, p.nq, p.m_nq), run = unit - sg * p.nq;
      const int strip = sg * NWV + wave;
      if (strip >= p.nstrip) continue;
      q->unit = unit;
      q->b = udivm1(strip, p.tiles_per_row, p.m_tpr);
      q->j = strip - q->b * p.tiles_per_row;
      q->ty = run * CP_RUN;
      q->ty_end = min(p.tiles_per_col, q->ty + CP_RUN);
      return true;
    }
    return false;
  };
  int cur = 0;   // (uniform)
  u32x4 carry[2][2] = {};   // [32-pixel block][channel group]: this lane's units of the previous tile's last y1 row
  cp_reads_done();   // (the scale slots are written: a tile's DMA may overwrite them)
  Pos at;
  bool have = open_unit(xcd * u8 + slot, &at), first = true, started = false;
  if (have) stage(at.b, at.j, at.ty * R2, 0, at.ty != 0);
  for (; have; cur ^= 1) {
    const int b = at.b, j = at.j, oy0 = at.ty * R2;
    // the tile after this one: the next of the run, or the first of this wavefront's next unit
    Pos nx = at;
    bool have_n = true, first_n = false;
    if (at.ty + 1 < at.ty_end) nx.ty = at.ty + 1;
    else { have_n = open_unit(at.unit + nslot, &nx); first_n = true; }
    const u32x4* y0img = img0;
    u32x4* y1img = img0;   // [2 channel blocks at the y0 image's pitch NR0 * ROWU][NR1 rows][33 even | 33 odd]
    const float* my_scale1 = scale0 + cur * 128;
    const float* my_scale2 = my_scale1 + 64;
    // this tile's image: issued before ALL of the previous tile's NSTORE stores (the first tile: before nothing) -- y1's units wait in
    // registers until the next tile's DMA is out, so that no tile ever waits for a store to be acknowledged
    if (!started) cp_wait_dma();
    else cp_wait_dma_but<G::NSTORE>();
    started = true;
    const bool top = oy0 == 0, fresh = first && !top;   // (uniform)
    // ---- layer 1, one y1 row of the tile at a time: two 32-pixel blocks, taps 0 .. 8 of the one 16-channel chunk
    u32x4 hold[NR1][2];   // y1 channel blocks 2 / 3 of the tile (this lane: block 2 + half, its pixel of either 32-pixel block) until layer 2's second chunk
    u32x4 st0[NR1][2];    // ... and blocks 0 / 1 of the owned rows, with the sign bytes, until the stores (issued behind the next tile's DMA)
    unsigned sg1[NR1][2];
    int hold_iu[2];
#pragma unroll
    for (int bk = 0; bk < 2; ++bk) hold_iu[bk] = half * NR0 * ROWU + ((32 * bk + l31) & 1) * PW + ((32 * bk + l31) >> 1);
    {
      const u32x4* bt = y0img + half * NR0 * ROWU + l31;   // this lane's pixel of y0 image row 0, channel block `half`, tap (0, 0)
      const u32x4* wk = lds_u + half * 32 + l31;           // weight unit [tap][half][l31]
#pragma unroll
      for (int r = 0; r < NR1; ++r) {
        if (r == 0 && !fresh) {   // the row the previous tile of the column computed last, or the padding above the plane
#pragma unroll
          for (int bk = 0; bk < 2; ++bk) {
            y1img[hold_iu[bk]] = top ? u32x4{0u, 0u, 0u, 0u} : carry[bk][0];
            hold[0][bk] = top ? u32x4{0u, 0u, 0u, 0u} : carry[bk][1];
          }
          continue;
        }
        f32x16 acc[2];
#pragma unroll
        for (int bk = 0; bk < 2; ++bk)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[bk][q] = 0.f;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
          const int ky = tp / 3, kx = tp % 3;
          if (tp % 3 == 0) CP_SCHED_BARRIER();
          const bf16x8 av = __builtin_bit_cast(bf16x8, wk[tp * 2 * 32]);
#pragma unroll
          for (int bk = 0; bk < 2; ++bk) {
            const bf16x8 bv = __builtin_bit_cast(bf16x8, bt[(r + ky) * ROWU + 32 * bk + kx]);
            acc[bk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[bk], 0, 0, 0);
          }
        }
        CP_SCHED_BARRIER();
        const int yy = 2 * oy0 - 1 + r;
#pragma unroll
        for (int bk = 0; bk < 2; ++bk) {
          const int c = 32 * bk + l31, xx = 2 * CP_TW * j - 1 + c;
          const bool inside = (unsigned)yy < (unsigned)IH && (unsigned)xx < (unsigned)IW;
          const int iu = hold_iu[bk] + r * ROWU;   // (blocks 0 / 1 now, 2 / 3 later: slot `half`)
          unsigned sg = 0;
#pragma unroll
          for (int gp = 0; gp < 2; ++gp) {
            unsigned m;
            const u32x4 st = cp_epi_group(acc[bk], gp, lds_b1, my_scale1, 16 * gp + 4 * half, leaky, &m);
            sg |= m << (8 * gp);
            const u32x4 unit = inside ? st : u32x4{0u, 0u, 0u, 0u};   // (what is stored is inside the plane: stored unit = image unit)
            if (gp == 0) { y1img[iu] = unit; st0[r][bk] = unit; }   // (y0 image row r is dead: row r's MFMAs are behind the epilogue that made `st`)
            else hold[r][bk] = unit;
            if (r == NR1 - 1) carry[bk][gp] = unit;
          }
          sg1[r][bk] = sg;
        }
      }
    }
    // ---- layer 2 out of the y1 image: chunk-major, tap-minor; the second chunk's channel blocks take the place of the first's
    f32x16 acc[R2][2];
#pragma unroll
    for (int rr = 0; rr < R2; ++rr)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[rr][mb][q] = 0.f;
    {
      const u32x4* bt = y1img + half * NR0 * ROWU + l31;
      const u32x4* wk = lds_u + G::OFF_W2 + half * 64 + l31;   // weight unit [tap][2 kc + half][32 mb + l31]
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        if (kc == 1) {
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int r = 0; r < NR1; ++r)
#pragma unroll
            for (int bk = 0; bk < 2; ++bk) y1img[hold_iu[bk] + r * ROWU] = hold[r][bk];
        }
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
          const int ky = tp / 3, kx = tp % 3;
          const int boff = ky * ROWU + (kx & 1) * PW + (kx >> 1);
          if (tp % (R2 * 2 >= 4 ? 1 : 3) == 0) CP_SCHED_BARRIER();
          bf16x8 av[2];
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) av[mb] = __builtin_bit_cast(bf16x8, wk[(tp * 4 + 2 * kc) * 64 + 32 * mb]);
#pragma unroll
          for (int rr = 0; rr < R2; ++rr) {
            const bf16x8 bv = __builtin_bit_cast(bf16x8, bt[boff + rr * 2 * ROWU]);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) acc[rr][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[mb], bv, acc[rr][mb], 0, 0, 0);
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- the image is dead: the next tile's DMA is issued in front of layer 2's epilogue and stores, and runs under them
    if (have_n) {
      cp_reads_done();
      stage(nx.b, nx.j, nx.ty * R2, cur ^ 1, first_n && nx.ty != 0);
    }
    // ---- y1 and its sign map: the pixels this tile owns (row / column 0 of the image are the neighbour tile's, column 63 is spare) and that lie in the plane
    {
      const auto rs_o = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out1 + (size_t)b * 4 * plane1), (short)0, 4 * plane1_16, RSRC_WORD3);
      const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)(p.signs1 + (size_t)b * plane1 * 4), (short)0, plane1 * 4, RSRC_WORD3);
#pragma unroll
      for (int r = 1; r < NR1; ++r)
#pragma unroll
        for (int bk = 0; bk < 2; ++bk) {
          const int c = 32 * bk + l31, yy = 2 * oy0 - 1 + r, xx = 2 * CP_TW * j - 1 + c;
          const bool own = (unsigned)yy < (unsigned)IH && (unsigned)xx < (unsigned)IW && c >= 1 && c <= 2 * CP_TW;
          const int o = yy * IW + xx;
          __builtin_amdgcn_raw_buffer_store_b128(st0[r][bk], rs_o, own ? o * 16 + half * plane1_16 : (int)OOB, 0, 2);
          __builtin_amdgcn_raw_buffer_store_b128(hold[r][bk], rs_o, own ? o * 16 + (2 + half) * plane1_16 : (int)OOB, 0, 2);
          __builtin_amdgcn_raw_buffer_store_b16((unsigned short)sg1[r][bk], rs_s, own ? (half * plane1 + o) * 2 : (int)OOB, 0, 0);
        }
    }
    // ---- layer 2's epilogue
    const auto rs_o = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out2 + (size_t)b * p.Mb2 * plane2), (short)0, p.Mb2 * plane2_16, RSRC_WORD3);
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)(p.signs2 + (size_t)b * plane2 * 8), (short)0, plane2 * 8, RSRC_WORD3);
    const int ox0 = CP_TW * j;
#pragma unroll
    for (int rr = 0; rr < R2; ++rr) {
      const bool ov = l31 < CP_TW && ox0 + l31 < OW2 && oy0 + rr < OH2;
      const int o = (oy0 + rr) * OW2 + ox0 + l31;
      unsigned sg = 0;   // this lane's sign bytes: byte j = channel group 2 mb + gp
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          unsigned m;
          const u32x4 st = cp_epi_group(acc[rr][mb], gp, lds_b2, my_scale2, 32 * mb + 16 * gp + 4 * half, leaky, &m);
          sg |= m << (8 * (2 * mb + gp));
          const int cb = 4 * mb + 2 * gp + half;
          __builtin_amdgcn_raw_buffer_store_b128(st, rs_o, (ov && cb < p.Mb2) ? o * 16 + cb * plane2_16 : (int)OOB, 0, 0);
        }
      __builtin_amdgcn_raw_buffer_store_b32(sg, rs_s, ov ? (half * plane2 + o) * 4 : (int)OOB, 0, 0);
    }
    at = nx; have = have_n; first = first_n;
  }
}

static int cp_rows() {   // y2 rows of a tile: 1 (eight wavefronts per CU) unless a variant build says 2 (six)
#ifdef BF_PAIR_R2
  return BF_PAIR_R2;
#else
  return 1;
#endif
}

bool conv_bf16_staged_pair_eligible(int C0, int C1, int C2, int IH, int IW, int B) {
  // the packed layouts the kernel indexes ([9][2][32] and [9][4][64]), and C1 = 32 exactly: with fewer channels the second of the two launches
  // is not conv_bf16_staged_kernel (it takes 16 or 32 input channels) but the tiled kernel, which may step a 32-channel chunk tap-major -- another
  // order of the same sums, one bf16 step apart on a few values; the pair promises the two launches' bytes, so it leaves those to them
  if (C0 != 16 || C1 != 32 || C2 <= 32 || C2 > 64) return false;
  if (IH < 1 || IW < 1 || B <= 0 || IH >= 32000 || IW >= 32768) return false;
  const long long OH2 = (IH - 1) / 2 + 1, OW2 = (IW - 1) / 2 + 1;
  const long long Mb2 = ((C2 + 15) / 16) * 2;
  // every per-image byte extent a lane's 32-bit offset addresses: y0 (2 blocks), y1 (4 blocks), y2
  if (4ll * IH * IW * 16 >= (1ll << 31) || Mb2 * OH2 * OW2 * 16 >= (1ll << 31)) return false;
  const long long tpr = (OW2 + CP_TW - 1) / CP_TW, nstrip = (long long)B * tpr;
  const int R2 = cp_rows();
  const long long tpc = (OH2 + R2 - 1) / R2, nq = (tpc + CP_RUN - 1) / CP_RUN;
  const long long nunit = ((nstrip + 5) / 6 + 1) * nq;   // (at most: strip groups of six to eight wavefronts)
  if (nstrip + 8 >= (1ll << 31) || nunit >= (1ll << 31)) return false;
  // the kernel's divisions by multiplication: unit -> strip group (by runs per strip), strip -> image (by tiles per row)
  if (!magic_div_exact(nunit, (int)nq) || !magic_div_exact(nstrip + 8, (int)tpr)) return false;
  return true;
}

namespace {
template <int R2, int NWV>
int cp_launch(ConvPairParams p, int n_cu, hipStream_t stream) {
  using G = PairGeom<R2, NWV>;
  p.tiles_per_col = cdiv(p.OH2, R2);
  p.tiles_per_row = cdiv(p.OW2, CP_TW);
  p.nstrip = p.B * p.tiles_per_row;
  p.nq = cdiv(p.tiles_per_col, CP_RUN);
  p.nunit = cdiv(p.nstrip, NWV) * p.nq;
  p.ntiles = p.nstrip * p.tiles_per_col;
  p.m_tpr = magic_u32(p.tiles_per_row); p.m_nq = magic_u32(p.nq);
  constexpr int lds = G::LDS_BYTES;
  const int per_cu = max(1, min(16 / NWV, (160 * 1024) / lds));   // workgroups a CU holds
  const int grid = 8 * max(1, min(cdiv(p.nunit, 8), per_cu * n_cu / 8));
  const void* kernel = reinterpret_cast<const void*>(&conv_bf16_staged_pair_kernel<R2, NWV>);
  if (int e = yogo_func_dynamic_lds(kernel, lds, "conv_bf16_staged_pair")) return e;
  hipLaunchKernelGGL((conv_bf16_staged_pair_kernel<R2, NWV>), dim3(grid), dim3(64 * NWV), lds, stream, p);
  if (yogo_launch_log_enabled())
    yogo_launch_log("conv_bf16_staged_pair_kernel<%d, %d> | C1=%d C2=%d in=%dx%d out=%dx%d tiles=%d grid=%d lds=%d act=%d bias=%d,%d scale=%d,%d units=%d l1_mfma_factor=%.2f",
                    R2, NWV, p.M1, p.M2, p.IH, p.IW, p.OH2, p.OW2, p.ntiles, grid, lds, p.act, p.bias1 != nullptr, p.bias2 != nullptr,
                    p.scale1 != nullptr, p.scale2 != nullptr, p.nunit, (double)((2 * R2 * min(CP_RUN, p.tiles_per_col) + 1) * 64) / (2 * R2 * min(CP_RUN, p.tiles_per_col) * 2 * CP_TW));
  return YOGO_OK;
}
}  // namespace

int launch_conv_bf16_staged_pair(const void* in, const void* packed1, const float* bias1, void* out1, void* signs1, const float* scale1, const void* packed2,
                                 const float* bias2, void* out2, void* signs2, const float* scale2, int B, int C1, int C2, int IH, int IW, int act,
                                 hipStream_t stream) {
  int n_cu;
  if (int e = yogo_device_cus("conv_bf16_staged_pair", &n_cu)) return e;
  ConvPairParams p{};
  p.in = reinterpret_cast<const u32x4*>(in);
  p.wp1 = reinterpret_cast<const u32x4*>(packed1); p.bias1 = bias1; p.out1 = reinterpret_cast<u32x4*>(out1);
  p.signs1 = reinterpret_cast<unsigned char*>(signs1); p.scale1 = scale1;
  p.wp2 = reinterpret_cast<const u32x4*>(packed2); p.bias2 = bias2; p.out2 = reinterpret_cast<u32x4*>(out2);
  p.signs2 = reinterpret_cast<unsigned char*>(signs2); p.scale2 = scale2;
  p.B = B; p.M1 = C1; p.M2 = C2; p.Mb2 = ((C2 + 15) / 16) * 2; p.IH = IH; p.IW = IW; p.OH2 = (IH - 1) / 2 + 1; p.OW2 = (IW - 1) / 2 + 1; p.act = act;
  if (B <= 0) return YOGO_OK;
  int rc;
  if (cp_rows() == 2) rc = cp_launch<2, 6>(p, n_cu, stream);
  else rc = cp_launch<1, 8>(p, n_cu, stream);
  if (rc != YOGO_OK) return rc;
  YOGO_CHECK_LAUNCH("conv_bf16_staged_pair");
  return YOGO_OK;
}

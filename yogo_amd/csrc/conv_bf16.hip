// The host side of the bf16 convolution engine: one request per launch, the planner of the tiled kernel, the dispatcher that hands a
// request to the kernel that takes it, and the C entry points.  No kernel lives here (conv_bf16_plan.h says which file holds which);
// every plan switch is an accessor of plan_switches.h.
#include "conv_bf16_plan.h"
#include "conv_bf16_ws.h"
#include "conv_bf16_ws16.h"
#include "conv_bf16_ws3.h"
#include "plan_switches.h"

#ifdef YOGO_DIAG
// diagnostic build only: ablation bits, synchronous staging, and a caller-owned stamp buffer ([workgroups][4] u64)
static int g_diag_dbg = 0, g_diag_nodma = 0;
static unsigned long long* g_diag_stamps = nullptr;
static size_t g_diag_stamps_bytes = 0;
// stamps: [workgroups][16] u64 (see ConvBf16Params::stamps)
extern "C" int yogo_diag_conv_bf16(int dbg_bits, int no_dma, void* stamps, size_t stamps_bytes) {
  g_diag_dbg = dbg_bits; g_diag_nodma = no_dma;
  g_diag_stamps = reinterpret_cast<unsigned long long*>(stamps); g_diag_stamps_bytes = stamps_bytes;
  return YOGO_OK;
}
// the ablation bits and the (cleared) stamp buffer of a persistent kernel's launch: Q = ConvWsParams / ConvWs3Params
template <typename Q>
void bf_diag_persistent(Q* q, hipStream_t stream) {
  q->dbg = g_diag_dbg;
  q->stamps = (g_diag_stamps != nullptr && g_diag_stamps_bytes >= 512 * 128) ? g_diag_stamps : nullptr;
  if (q->stamps) (void)hipMemsetAsync(g_diag_stamps, 0, 512 * 128, stream);
}
#else
template <typename Q>
void bf_diag_persistent(Q*, hipStream_t) {}
#endif

namespace {

// (OH, OW): the grid the workgroups tile (output pixels; quads for the stride-2 data gradient), T: weight slices staged at
// most, PF: DMA slots of the kernel variant.  LDS image of a chunk: input tile from unit 0, weight slices from ldsw_off.
bool bf_plan(int OH, int OW, int a, int T, int span, int Kb, int MW, int NW, int NWV, int PF, int budget, BfTiling* out,
             bool force_single = false, int force_ckb = 0, int force_nbuf = 0, int force_ni = 0) {
  const int BM = 32 * MW, PT = 32 * NWV * NW, NT = 64 * NWV;
  BfTiling best{};
  long long best_score = -1;
  for (int ncb = 1; ncb <= 24 && ncb <= OW; ++ncb) {
    const int TW = cdiv(OW, ncb);
    const int bw_min = OW - (cdiv(OW, TW) - 1) * TW;
    if (cdiv(OW, TW) != ncb || bw_min <= 0) continue;
    const int LW = (TW - 1) * a + span;
    const int nrow_lat = min(OH, 1 + cdiv(PT - 1, bw_min));
    const int rows_max = (nrow_lat - 1) * a + span;
    const int chs = rows_max * LW;
    for (int CKb : {8, 4, 2}) {
      if (Kb % CKb || (force_ckb && CKb != force_ckb)) continue;
      const int ni_need = cdiv(CKb * chs, NT), nw = cdiv(T * CKb * BM, NT);
      if (force_ni && ni_need > force_ni) continue;
      const int ni = force_ni ? force_ni : ni_need;  // (a fixed slot layout: unused slots carry out-of-range offsets)
      const int ldsw_off = ni * NT;  // slot-aligned, so a DMA slot is all input or all weights
      const int bufu = (ni + nw) * NT;
      const int nbuf = force_nbuf ? force_nbuf : ((Kb / CKb <= 2 || force_single) ? 1 : 2);  // short contractions: one buffer (more workgroups per CU)
      const int dma = (ni + nw <= PF && nbuf * bufu * 16 <= budget) ? (nbuf == 1 ? 2 : 1) : 0;
      if (force_nbuf && !dma) continue;
      const int dummy = ldsw_off + T * CKb * BM;
      const int bytes = dma ? nbuf * bufu * 16 : (dummy + 1) * 16;
      if (bytes > budget) continue;
      // pipelined chunks first, then deep chunks, then the least staged input over the whole image (halo overhead)
      const long long staged = (long long)ncb * cdiv(OH * TW, PT) * rows_max * LW;  // units per channel block and image
      const long long score = (dma ? 1 : 0) * 100000000000000LL + (long long)CKb * 100000000000LL - staged * 100 - ncb;
      if (best_score < 0 || score > best_score) {
        best_score = score;
        best = BfTiling{ncb, TW, cdiv(OH * TW, PT), CKb, rows_max, LW, ldsw_off, dummy, bytes, dma, ni, ni + nw, bufu};
      }
    }
  }
  if (best_score < 0) return false;
  *out = best;
  return true;
}

// Row-staged tiling of the single-buffer 4-wavefront kernels (ConvBf16Params::rowdma): rows at a pitch of 64 or 128 units, so
// the band may be as wide as the pitch allows at no extra LDS -- fewer bands, less halo, fewer pieces.  16-channel chunks only.
bool bf_plan_rows(int OH, int OW, int a, int T, int span, int Kb, int MW, int NW, int NWV, int budget, BfTiling* out, int* lwp_out) {
  const int BM = 32 * MW, PT = 32 * NWV * NW, CKb = 2;
  if (Kb % CKb || Kb / CKb > 2 || T * CKb * BM / 64 > 8 * NWV) return false;
  long long best_score = -1;
  BfTiling best{};
  int best_lwp = 0;
  for (int ncb = 1; ncb <= 24 && ncb <= OW; ++ncb) {
    const int TW = cdiv(OW, ncb);
    const int bw_min = OW - (cdiv(OW, TW) - 1) * TW;
    if (cdiv(OW, TW) != ncb || bw_min <= 0) continue;
    const int LW = (TW - 1) * a + span;
    const int lwp = LW <= 64 ? 64 : ((LW <= 128 && a == 1) ? 128 : 0);   // (stride 2: one piece per row, or the piece count doubles)
    if (!lwp) continue;
    const int nrow_lat = min(OH, 1 + cdiv(PT - 1, bw_min));
    const int rows_max = (nrow_lat - 1) * a + span;
    const int units_in = CKb * rows_max * lwp, wunits = T * CKb * BM;
    const int bytes = (units_in + wunits) * 16;
    if (bytes > budget) continue;
    const long long staged = (long long)ncb * cdiv(OH * TW, PT) * rows_max * lwp;  // staged units per channel block and image
    if (best_score < 0 || staged < best_score) {
      best_score = staged;
      best = BfTiling{ncb, TW, cdiv(OH * TW, PT), CKb, rows_max, LW, units_in, units_in + wunits, bytes, 2, 0, 0, units_in + wunits};
      best_lwp = lwp;
    }
  }
  if (best_score < 0) return false;
  *out = best;
  *lwp_out = best_lwp;
  return true;
}

enum BfDirection { BF_FORWARD, BF_DGRAD };

// the request of the forward pass (direction BF_FORWARD) or the data gradient (BF_DGRAD) of a Cin -> Cout convolution on IH x IW inputs
int bf_request(int B, int Cin, int Cout, int IH, int IW, int ks, int stride, BfDirection dir, ConvBf16Request* r) {
  YOGO_CHECK_ARG((ks == 3 || ks == 1) && (stride == 1 || stride == 2) && !(ks == 1 && stride != 1) && B >= 0 && Cin > 0 &&
                     Cout > 0 && IH > 0 && IW > 0, "conv_bf16: unsupported shape");
  const int pad = ks == 3 ? 1 : 0;
  const int OHf = (IH + 2 * pad - ks) / stride + 1, OWf = (IW + 2 * pad - ks) / stride + 1;
  *r = ConvBf16Request{};
  r->B = B; r->ks = ks; r->act = ACT_NONE;
#ifdef YOGO_DIAG
  r->dbg = g_diag_dbg; r->stamps = g_diag_stamps; r->stamps_bytes = g_diag_stamps_bytes;
#endif
  if (dir == BF_FORWARD) {
    r->K = Cin; r->M = Cout; r->IH = IH; r->IW = IW; r->OH = OHf; r->OW = OWf; r->a = stride; r->s2d = 0;
  } else {
    r->K = Cout; r->M = Cin; r->IH = OHf; r->IW = OWf; r->OH = IH; r->OW = IW; r->a = 1; r->s2d = (stride == 2 && ks == 3) ? 1 : 0;
  }
  return YOGO_OK;
}

int bf_plan_tiled(const ConvBf16Request& r, BfTiledPlan* pl) {
  const int K = r.K, M = r.M, OH = r.OH, OW = r.OW, ks = r.ks, a = r.a, s2d = r.s2d, T = ks * ks;
  const int MW = bf_pick_mw(M);
  const bool small_n = s2d || a == 2;  // two accumulator sets / four-fold input tile: half the pixel groups per wavefront
  // 64 GEMM rows at stride 1 with a long contraction: 8 wavefronts x 4 pixel groups (64 rows x 1024 px), the same staged
  // bytes per MFMA as the 128-row tile; everything else with <= 64 rows stays on 4-wavefront workgroups
  const bool wide64 = MW == 2 && !small_n && K >= 64 && OH * OW >= 4096;
  const int NW = MW == 1 ? (small_n ? 2 : 4) : (small_n ? 1 : (wide64 ? 4 : 2));
  const int NWV = (MW == 4 || wide64) ? 8 : 4;  // 128-channel tiles: 8 wavefronts share the staged weight slice
  const int PF = NWV == 8 ? 10 : 16;  // = 160 KB / 128 KB of LDS for the two buffers at most
  const int Kb = bf_kb_of(K), Mpad = bf_mpad_of(M);
  // the grid the workgroups tile: output pixels, or 2x2 output quads of one row parity
  const int OHt = s2d ? (OH + 1) / 2 : OH, OWt = s2d ? (OW + 1) / 2 : OW;
  BfTiling tl;
  // 4-wavefront workgroups: as many per CU as a pipelined tiling allows (4, 3, 2)
  bool planned = false;
  if (NWV == 4) {
    const int ladder[3] = {40 * 1024, 53 * 1024, BF_LDS_BUDGET};
    for (int i = 0; i < 3 && !planned; ++i)
      planned = bf_plan(OHt, OWt, s2d ? 1 : a, s2d ? 6 : T, s2d ? 2 : ks, Kb, MW, NW, NWV, PF, ladder[i], &tl) && tl.dma;
  }
  // stride-2 data gradient of the 128-channel tile: 16-channel chunks in a ring of four buffers with the fixed 2 + 3 slot layout
  bool ring = false;
  if (s2d && MW == 4 && Kb >= 8 && plan_tiled_ring()) {
    ring = bf_plan(OHt, OWt, 1, 6, 2, Kb, MW, NW, NWV, 5, BF_LDS_MAX, &tl, false, 2, 4, 2);
    planned = ring;
  }
  if (!planned) planned = bf_plan(OHt, OWt, s2d ? 1 : a, s2d ? 6 : T, s2d ? 2 : ks, Kb, MW, NW, NWV, PF, BF_LDS_MAX, &tl);
  if (!planned) {
    yogo_set_error("conv_bf16: no LDS tiling fits (K=%d M=%d OW=%d a=%d)", K, M, OW, a);
    return YOGO_ERR_ARG;
  }
  // the lean single-buffer 4-wavefront tiles (3x3, 16-channel chunks): stage the input row by row when that keeps the
  // workgroups-per-CU level of the slot plan
  const bool lean4 = !s2d && NWV == 4 && T == 9 && tl.CKb == 2 && tl.dma == 2 && r.out_f32 == nullptr && plan_tiled_lean4();
  int rowdma = 0, lwp = 0;
  // (measured: -2.5 ... -5 % on the 16 <-> 32 channel layer in both directions; the stride-2 forward -2 ... -3.5 % with ONE piece
  //  per row -- bands of at most 31 output columns -- and +1 % with 87-unit rows in two pieces, so its pitch stays 64)
  if (lean4 && plan_tiled_rowdma()) {
    const int ladder[3] = {40 * 1024, 53 * 1024, BF_LDS_BUDGET};
    int level = 0;
    while (level < 2 && tl.lds_bytes > ladder[level]) ++level;
    BfTiling tr;
    if (tl.lds_bytes <= ladder[level] && bf_plan_rows(OHt, OWt, a, T, ks, Kb, MW, NW, NWV, ladder[level], &tr, &lwp)) {
      tl = tr;
      rowdma = 1;
    }
  }
  pl->MW = MW; pl->NW = NW; pl->NWV = NWV; pl->PF = PF; pl->wide64 = wide64;
  pl->tl = tl; pl->ring = ring; pl->rowdma = rowdma; pl->lwp = lwp;
  // (the row-staged tiling keeps CKb = 2 and dma = 2, so `lean4` holds for the tiling the launch uses too)
  pl->lean4 = lean4 ? 1 : 0;
  pl->grid = dim3(tl.ncb * tl.tiles_per_band, (Mpad / (32 * MW)) * (s2d ? 2 : 1), r.B);
  pl->rows = r.B * (int)pl->grid.x;
  pl->mpad = Mpad;
  pl->dma = tl.dma;
#ifdef YOGO_DIAG
  if (g_diag_nodma && (tl.lds_dummy + 1) * 16 <= BF_LDS_MAX) pl->dma = 0;  // synchronous staging through registers
#endif
  pl->ni_slots = tl.ni_slots; pl->n_slots = tl.n_slots; pl->ldsw_off = tl.ldsw_off; pl->bufu = tl.bufu; pl->bufs = tl.dma == 1 ? tl.bufu : 0;
  pl->lds_bytes = max(pl->dma ? tl.lds_bytes : (tl.lds_dummy + 1) * 16, (2 + 2 * NWV) * 32 * MW * 4);
  // ping-pong main loop: 3x3 taps, 16-channel chunks (one step per tap) through the double-buffered LDS-DMA pipeline, with its
  // fixed slot layout: 5 slots for the input tile, 5 for the weight slices, two buffers of 10 slots = all of the LDS
  pl->use_pp = NWV == 8 && !s2d && T == 9 && pl->dma == 1 && tl.CKb == 2 && tl.ni_slots <= 5 && tl.n_slots - tl.ni_slots <= 5 && plan_tiled_pp();
  if (pl->use_pp) {
    pl->ni_slots = 5; pl->n_slots = 10; pl->ldsw_off = 5 * 64 * NWV; pl->bufu = 10 * 64 * NWV; pl->bufs = pl->bufu;
    pl->lds_bytes = 2 * pl->bufu * 16;
  }
  return YOGO_OK;
}

// One launcher for forward and data-gradient: the specialised kernels take the requests their gates accept, in this order; everything
// else runs on the tiled kernel with the plan of bf_plan_tiled.
int launch_conv_bf16(const ConvBf16Request& r, hipStream_t stream) {
  const int B = r.B, K = r.K, M = r.M, IH = r.IH, IW = r.IW, OH = r.OH, OW = r.OW, ks = r.ks, a = r.a, s2d = r.s2d, act = r.act;
  // what every specialised kernel leaves to the tiled one: a second (pre-activation) output, a reference tensor, BatchNorm statistics
  const bool plain = r.out_pre == nullptr && r.act_ref == nullptr && r.stats_part == nullptr;
  // the LEAN EPILOGUE: plain, one bf16 output, no sign map to read, identity or LeakyReLU, a sign map written only beside LeakyReLU
  const bool lean = plain && r.out_f32 == nullptr && !r.signs_read && (act == ACT_NONE || act == ACT_LEAKY) && !(r.signs != nullptr && act != ACT_LEAKY);
  // stride-1 3x3 convolutions with 128 output channels and the lean epilogue: the persistent wavefront-specialised kernel
  if (plan_ws() && lean && !s2d && a == 1 && ks == 3 && conv_bf16_ws_eligible(K, M, IH, IW, B)) {
    ConvWsParams q{};
    q.in = r.in; q.wp = r.packed; q.bias = r.bias; q.out = r.out; q.signs = reinterpret_cast<unsigned char*>(r.signs); q.chan_scale = r.chan_scale;
    q.B = B; q.Kb = bf_kb_of(K); q.IH = IH; q.IW = IW; q.act = act;
    bf_diag_persistent(&q, stream);
    if (conv_bf16_ws_plan(&q)) {
      // the plain epilogue without a bias (the data gradients of the 128 -> 128 layers): the 16x16x32 member of the family.  With a bias
      // (layer 5's forward) it measured +7 % inside the training step (profiles/r06_kernel_stats.txt history) and stays
      // on conv_bf16_ws_kernel<0>
      if ((plan_ws16_mode() == 2 || (plan_ws16_mode() == 1 && r.bias == nullptr)) && act == ACT_NONE && r.signs == nullptr && r.chan_scale == nullptr &&
          conv_bf16_ws16_eligible(K, M, IH, IW, B))
        return launch_conv_bf16_ws16(q, stream);
      return launch_conv_bf16_ws(q, stream);
    }
  }
  // stride-2 3x3 forward with 128 output channels and the lean epilogue: its persistent wavefront-specialised member (conv_bf16_ws3.hip)
  if (plan_ws() && lean && !s2d && a == 2 && ks == 3 && conv_bf16_ws3_eligible(K, M, IH, IW, B)) {
    ConvWs3Params q{};
    q.in = r.in; q.wp = r.packed; q.bias = r.bias; q.out = r.out; q.signs = reinterpret_cast<unsigned char*>(r.signs); q.chan_scale = r.chan_scale;
    q.B = B; q.Kb = bf_kb_of(K); q.IH = IH; q.IW = IW; q.OH = OH; q.OW = OW; q.act = act;
    bf_diag_persistent(&q, stream);
    if (conv_bf16_ws3_plan(&q)) return launch_conv_bf16_ws3(q, stream);
  }
  // the 1x1 head's forward with the weights in registers.  NOT the lean epilogue: the output is fp32 (and there is no bf16 one), bias only --
  // no activation, no sign map in either role, no channel scale
  if (plan_head() && plain && ks == 1 && a == 1 && !s2d && act == ACT_NONE && r.out_f32 != nullptr && r.out == nullptr && r.signs == nullptr &&
      r.chan_scale == nullptr && conv_bf16_head_fwd_eligible(K, M, OH * OW, B))
    return launch_conv_bf16_head_fwd(r.in, r.packed, r.bias, r.out_f32, B, K, M, OH * OW, stream);
  // 3x3 convolutions out of 16 / 32 channels into <= 64 with the lean epilogue: independent wavefronts, weights resident, private LDS staging
  if (plan_staged() && lean && !s2d && ks == 3 && conv_bf16_staged_eligible(K, M, a, IH, IW, OH, OW, B))
    return launch_conv_bf16_staged(r.in, r.packed, r.bias, r.out, r.signs, r.chan_scale, B, K, M, IH, IW, OH, OW, a, act, stream);
  // stride-2 3x3 data gradient into <= 32 or 65 - 128 channels (scale / LeakyReLU-sign-map epilogue): weights resident in LDS, operands straight
  // from memory.  NOT the lean epilogue either: no bias and no activation of its own, and the sign map is one it READS (a LeakyReLU reference's),
  // never one it writes
  if (plan_direct() && plain && s2d && ks == 3 && r.out_f32 == nullptr && r.bias == nullptr && act == ACT_NONE &&
      (r.signs_read ? (r.signs != nullptr && r.ref_act == ACT_LEAKY) : r.signs == nullptr) && conv_bf16_s2d_direct_eligible(K, M, OH, OW, B))
    return launch_conv_bf16_s2d_direct(r.in, r.packed, r.out, r.signs_read ? r.signs : nullptr, r.chan_scale, B, K, M, IH, IW, OH, OW, stream);
  BfTiledPlan pl;
  if (int e = bf_plan_tiled(r, &pl)) return e;
  return launch_conv_bf16_tiled(r, pl, stream);
}

}  // namespace

// rows / row stride of the BatchNorm partial-sum buffer a forward launch fills when stats_part != NULL: those of the tiled plan (a
// launch with statistics always runs on the tiled kernel).  No device is needed.
extern "C" int yogo_conv2d_fwd_bf16_stats_shape(int B, int Cin, int Cout, int IH, int IW, int ks, int stride, int* rows, int* mpad) {
  ConvBf16Request r;
  if (int e = bf_request(B, Cin, Cout, IH, IW, ks, stride, BF_FORWARD, &r)) return e;
  BfTiledPlan pl;
  if (int e = bf_plan_tiled(r, &pl)) return e;
  if (rows) *rows = pl.rows;
  if (mpad) *mpad = pl.mpad;
  return YOGO_OK;
}

// in: bf16 NCHW8c [B][kb(Cin)][IH][IW][8]; out: bf16 NCHW8c [B][kb(Cout)][OH][OW][8], or fp32 NCHW when out_f32 != NULL.
// y = chan_scale * act(conv(x, packed) + bias); stats_part (optional) receives (sum, sumsq) of conv + bias per channel.
extern "C" int yogo_conv2d_fwd_bf16(const void* in, const void* packed, const float* bias, void* out, float* out_f32,
                                    const float* chan_scale, float* stats_part, int B, int Cin, int Cout, int IH, int IW,
                                    int ks, int stride, int act, hipStream_t stream) {
  YOGO_CHECK_ARG(in && packed && (out || out_f32), "conv2d_fwd_bf16: null pointer");
  ConvBf16Request r;
  if (int e = bf_request(B, Cin, Cout, IH, IW, ks, stride, BF_FORWARD, &r)) return e;
  r.in = in; r.packed = packed; r.bias = bias; r.out = out; r.out_f32 = out_f32; r.chan_scale = chan_scale; r.stats_part = stats_part; r.act = act;
  return launch_conv_bf16(r, stream);
}

// the same with a second bf16 output `out_pre` = conv + bias before the activation (what the backward pass of a SiLU block
// without BatchNorm needs: silu'(z) is a function of the pre-activation); bf16 NCHW8c outputs only
extern "C" int yogo_conv2d_fwd_bf16_pre(const void* in, const void* packed, const float* bias, void* out, void* out_pre,
                                        const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ks, int stride,
                                        int act, hipStream_t stream) {
  YOGO_CHECK_ARG(in && packed && out && out_pre, "conv2d_fwd_bf16_pre: null pointer");
  ConvBf16Request r;
  if (int e = bf_request(B, Cin, Cout, IH, IW, ks, stride, BF_FORWARD, &r)) return e;
  r.in = in; r.packed = packed; r.bias = bias; r.out = out; r.out_pre = out_pre; r.chan_scale = chan_scale; r.act = act;
  return launch_conv_bf16(r, stream);
}

// bytes of the LeakyReLU sign map of a bf16 NCHW8c tensor with C channels: [B][2][H][W][Cpad/16] bytes, Cpad = C rounded up
// to the channel tile (32 / 64 / 128 for C <= 32 / <= 64 / more); byte (h, pixel, q), bit i + 4e = (channel 4h + i of channel
// block 2q + e > 0) -- the lane order of the conv epilogue, so a lane's signs of one pixel are one contiguous store
extern "C" int yogo_bf16_signs_bytes(int B, int C, int H, int W, size_t* bytes) {
  YOGO_CHECK_ARG(bytes && B >= 0 && C > 0 && H > 0 && W > 0, "bf16_signs_bytes: bad arguments");
  *bytes = (size_t)B * H * W * (bf_mpad_of(C) / 8);
  return YOGO_OK;
}

// yogo_conv2d_fwd_bf16 (bf16 output) that also writes the sign map of its output: what the data gradient of the NEXT layer
// needs of a LeakyReLU block without BatchNorm (yogo_conv2d_dgrad_bf16_signs), at 1/16 of the bytes of the output itself
extern "C" int yogo_conv2d_fwd_bf16_signs(const void* in, const void* packed, const float* bias, void* out, void* signs,
                                          const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ks, int stride,
                                          int act, hipStream_t stream) {
  YOGO_CHECK_ARG(in && packed && out && signs, "conv2d_fwd_bf16_signs: null pointer");
  ConvBf16Request r;
  if (int e = bf_request(B, Cin, Cout, IH, IW, ks, stride, BF_FORWARD, &r)) return e;
  r.in = in; r.packed = packed; r.bias = bias; r.out = out; r.signs = signs; r.chan_scale = chan_scale; r.act = act;
  return launch_conv_bf16(r, stream);
}

// A stride-1 3x3 C0 -> C1 block and the stride-2 3x3 C1 -> C2 block behind it (both with bias / activation / channel scale and a sign map,
// yogo/model_defns.py:39-46) in one call: bit-identical to yogo_conv2d_fwd_bf16_signs twice.  Shapes conv_bf16_staged_pair_kernel takes run
// in ONE launch in which layer 2 reads y1 from LDS; every other shape, and every shape with the plan switch off, runs the two launches.
extern "C" int yogo_conv2d_fwd_bf16_signs_pair_eligible(int B, int C0, int C1, int C2, int IH, int IW) {
  return conv_bf16_staged_pair_eligible(C0, C1, C2, IH, IW, B) ? 1 : 0;
}
extern "C" int yogo_conv2d_fwd_bf16_signs_pair(const void* in, const void* packed1, const float* bias1, void* out1, void* signs1, const float* scale1,
                                               const void* packed2, const float* bias2, void* out2, void* signs2, const float* scale2, int B, int C0,
                                               int C1, int C2, int IH, int IW, int act, hipStream_t stream) {
  YOGO_CHECK_ARG(in && packed1 && out1 && signs1 && packed2 && out2 && signs2, "conv2d_fwd_bf16_signs_pair: null pointer");
  YOGO_CHECK_ARG(B >= 0 && C0 > 0 && C1 > 0 && C2 > 0 && IH > 0 && IW > 0, "conv2d_fwd_bf16_signs_pair: unsupported shape");
  if (plan_staged_pair() && act == ACT_LEAKY && conv_bf16_staged_pair_eligible(C0, C1, C2, IH, IW, B))
    return launch_conv_bf16_staged_pair(in, packed1, bias1, out1, signs1, scale1, packed2, bias2, out2, signs2, scale2, B, C1, C2, IH, IW, act, stream);
  if (int e = yogo_conv2d_fwd_bf16_signs(in, packed1, bias1, out1, signs1, scale1, B, C0, C1, IH, IW, 3, 1, act, stream)) return e;
  return yogo_conv2d_fwd_bf16_signs(out1, packed2, bias2, out2, signs2, scale2, B, C1, C2, IH, IW, 3, 2, act, stream);
}

// yogo_conv2d_dgrad_bf16 with act = LeakyReLU and the sign map of the reference in place of the reference:
// dx = conv_transpose(dy) * (sign bit ? 1 : 0.01) * chan_scale
extern "C" int yogo_conv2d_dgrad_bf16_signs(const void* dy, const void* packed_dgrad, void* dx, const void* signs,
                                            const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ks, int stride,
                                            hipStream_t stream) {
  YOGO_CHECK_ARG(dy && packed_dgrad && dx && signs, "conv2d_dgrad_bf16_signs: null pointer");
  ConvBf16Request r;
  if (int e = bf_request(B, Cin, Cout, IH, IW, ks, stride, BF_DGRAD, &r)) return e;
  r.in = dy; r.packed = packed_dgrad; r.out = dx; r.ref_act = ACT_LEAKY; r.signs = const_cast<void*>(signs); r.signs_read = true; r.chan_scale = chan_scale;
  return launch_conv_bf16(r, stream);
}

// dx = conv_transpose(dy) * act'(act_ref) * chan_scale, all bf16 NCHW8c; (IH, IW) = the forward conv's INPUT dims.
// Stride 1: weights packed with mode 1.  Stride 2 (3x3): weights packed with mode 2; the gradient is computed per output
// parity class from the un-upsampled dy tile (9 tap-GEMMs per 2x2 output quad).
extern "C" int yogo_conv2d_dgrad_bf16(const void* dy, const void* packed_dgrad, void* dx, const void* act_ref, int ref_act,
                                      const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ks, int stride,
                                      hipStream_t stream) {
  YOGO_CHECK_ARG(dy && packed_dgrad && dx, "conv2d_dgrad_bf16: null pointer");
  ConvBf16Request r;
  if (int e = bf_request(B, Cin, Cout, IH, IW, ks, stride, BF_DGRAD, &r)) return e;
  r.in = dy; r.packed = packed_dgrad; r.out = dx; r.act_ref = act_ref; r.ref_act = ref_act; r.chan_scale = chan_scale;
  return launch_conv_bf16(r, stream);
}

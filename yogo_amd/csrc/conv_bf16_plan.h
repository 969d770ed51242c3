// What the files of the bf16 convolution engine share (host side): the request one launch is described by, the plan of the tiled
// kernel, the padding arithmetic of the packed weights, and the launchers the dispatcher (conv_bf16.hip: launch_conv_bf16) chooses among.
//   conv_bf16.hip        request, planner (bf_plan, bf_plan_rows, bf_plan_tiled), dispatcher, the C entry points -- no kernel
//   conv_bf16_tiled.hip  conv_bf16_kernel, its instantiation table and launch_conv_bf16_tiled
//   conv_bf16_pack.hip   the weight-packing kernels and their entry points
//   conv_bf16_{ws,ws3,ws16}.hip (own headers), conv_bf16_{direct,staged,staged_pair,head}.hip (declared below): the specialised kernels
#pragma once
#include "common.h"

#define BF_LDS_BUDGET (80 * 1024)      // two 4-wavefront workgroups per CU
#define BF_LDS_MAX (160 * 1024)        // one workgroup per CU (all of the LDS)

// packed weights are [T][Kb][Mpad] units: Kb channel blocks of the contraction (padded to 16 channels = 2 blocks), Mpad GEMM rows
// (padded to the channel tile, 32 * mw).  One definition for the planner, the packing entry points and the packing kernels.
__host__ __device__ inline int bf_pick_mw(int M) { return M <= 32 ? 1 : (M <= 64 ? 2 : 4); }
__host__ __device__ inline int bf_kb_of(int K) { return (K + 15) / 16 * 2; }
__host__ __device__ inline int bf_mpad_of(int M) { const int t = 32 * bf_pick_mw(M); return (M + t - 1) / t * t; }

// One bf16 convolution launch as the GEMM sees it: (K, M) the contraction / output channel counts, (IH, IW) the physical input dims,
// (OH, OW) the output dims, `a` the input step per output pixel; s2d = 1: parity-decomposed data gradient of a stride-2 3x3
// convolution (input = dy, output = dx, weights packed with mode 2).  The pointers a launch does not use stay null.
struct ConvBf16Request {
  const void* in;
  const void* packed;
  const float* bias;
  void* out;              // bf16 NCHW8c ...
  float* out_f32;         // ... or fp32 NCHW
  void* out_pre;          // second bf16 output: conv + bias before the activation
  const void* act_ref;    // data gradient: the activation's reference tensor (REF = 1) ...
  int ref_act;
  void* signs;            // ... or its sign map (signs_read; REF = 2); forward: the sign map to write (REF = 3)
  bool signs_read;
  const float* chan_scale;
  float* stats_part;
  int B, K, M, IH, IW, OH, OW, ks, a, s2d, act;
#ifdef YOGO_DIAG
  // diagnostic build only (yogo_diag_conv_bf16): what launch_conv_bf16 hands to the tiled kernel's ConvBf16Params::dbg / stamps
  int dbg;
  unsigned long long* stamps;
  size_t stamps_bytes;
#endif
};

struct BfTiling {
  int ncb, TW, tiles_per_band, CKb, rows_max, LW, ldsw_off, lds_dummy, lds_bytes, dma, ni_slots, n_slots, bufu;
};

// The plan of the tiled conv_bf16_kernel for a request: the tile (MW x NW x NWV, PF DMA slots), the LDS tiling, the loop variant
// (ring / row-staged lean loop / ping-pong) and the grid.  Host arithmetic only: the shape query runs it without a device.
struct BfTiledPlan {
  int MW, NW, NWV, PF;
  bool wide64;
  BfTiling tl;          // as planned; the log prints its slots
  bool ring;
  int lean4, rowdma, lwp;
  int dma;              // tl.dma (the diagnostic build: 0 = synchronous staging through registers)
  bool use_pp;
  int ni_slots, n_slots, ldsw_off, bufu, bufs, lds_bytes;   // the launch's slot layout: tl's, or the ping-pong loop's fixed one
  dim3 grid;
  int rows, mpad;       // of the BatchNorm partial-sum buffer a forward launch with stats_part fills
};

// conv_bf16_tiled.hip: fills conv_bf16_kernel's parameters from the request and its finished plan (bf_plan_tiled) and launches
int launch_conv_bf16_tiled(const ConvBf16Request& r, const BfTiledPlan& pl, hipStream_t stream);
// conv_bf16_direct.hip
bool conv_bf16_s2d_direct_eligible(int K, int M, int OH, int OW, int B);
int launch_conv_bf16_s2d_direct(const void* in, const void* packed, void* out, const void* signs, const float* chan_scale, int B, int K, int M, int IH, int IW,
                                int OH, int OW, hipStream_t stream);
// conv_bf16_staged.hip
bool conv_bf16_staged_eligible(int K, int M, int stride, int IH, int IW, int OH, int OW, int B);
int launch_conv_bf16_staged(const void* in, const void* packed, const float* bias, void* out, void* signs, const float* chan_scale, int B, int K, int M, int IH,
                            int IW, int OH, int OW, int stride, int act, hipStream_t stream);
// conv_bf16_staged_pair.hip: a stride-1 16 -> C1 layer and the stride-2 C1 -> C2 layer behind it in one launch (y1 through LDS)
bool conv_bf16_staged_pair_eligible(int C0, int C1, int C2, int IH, int IW, int B);
int launch_conv_bf16_staged_pair(const void* in, const void* packed1, const float* bias1, void* out1, void* signs1, const float* scale1, const void* packed2,
                                 const float* bias2, void* out2, void* signs2, const float* scale2, int B, int C1, int C2, int IH, int IW, int act,
                                 hipStream_t stream);
// conv_bf16_head.hip
bool conv_bf16_head_fwd_eligible(int K, int M, int plane, int B);
int launch_conv_bf16_head_fwd(const void* in, const void* packed, const float* bias, float* out_f32, int B, int K, int M, int plane, hipStream_t stream);

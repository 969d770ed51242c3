// Box decode (yogo/model.py:277-313) and the grid-cell loss (yogo/yogo_loss.py:38-129), forward + backward.
// SURVEY.md K10, K13-K15.  Both are one pass over [B, 5+C, Sy, Sx] cells: HBM-bound, one lane per cell, channel
// planes read/written coalesced along Sx.  The loss kernel replaces ~30 ATen launches, two boolean-mask gathers
// (each a host sync) and three .item() syncs by one launch: per-cell CIoU / label-smoothed CE / weighted MSE,
// analytic gradients, wavefront-shuffle + LDS block reduction, fixed-order fp64 final sum (deterministic).
//
// The per-cell arithmetic is head_math.h's (one definition, shared with nms.hip and conv_bf16_head.hip); the kernels here load a cell's
// operands, call it and store.  This TU is compiled with -ffp-contract=off, as that header requires.
#include "head_math.h"

#define MAX_CLASSES 64

// ---- decode forward ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_fwd_kernel(const float* __restrict__ raw, float* __restrict__ out,
                                                         const float* __restrict__ cxs, const float* __restrict__ cys,
                                                         float inv_sx, float inv_sy, float anchor_w, float anchor_h,
                                                         float wmul, float hmul, int P, int cells, int inference) {
  const int b = blockIdx.y;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const float* r = raw + (size_t)b * P * cells + cell;
  float* o = out + (size_t)b * P * cells + cell;
  const float t0 = r[0], t1 = r[(size_t)cells], t2 = r[(size_t)2 * cells], t3 = r[(size_t)3 * cells], t4 = r[(size_t)4 * cells];
  o[0] = hm_centre(inv_sx, t0, cxs[cell]);
  o[(size_t)cells] = hm_centre(inv_sy, t1, cys[cell]);
  o[(size_t)2 * cells] = hm_size(anchor_w, t2, wmul);
  o[(size_t)3 * cells] = hm_size(anchor_h, t3, hmul);
  o[(size_t)4 * cells] = hm_sigmoid(t4);
  const int C = P - 5;
  if (inference) {
    float mx, sum;
    hm_softmax_terms(r, cells, P, mx, sum);
    for (int c = 0; c < C; ++c) o[(size_t)(5 + c) * cells] = hm_softmax(r[(size_t)(5 + c) * cells], mx, sum);
  } else {
    for (int c = 0; c < C; ++c) o[(size_t)(5 + c) * cells] = r[(size_t)(5 + c) * cells];
  }
}

// ---- decode backward: graw = gout * d(out)/d(raw) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ out,
                                                         const float* __restrict__ gout, float* __restrict__ graw,
                                                         float inv_sx, float inv_sy, int P, int cells, int inference) {
  const int b = blockIdx.y;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const size_t base = (size_t)b * P * cells + cell;
  const float* r = raw + base;
  const float* o = out + base;
  const float* g = gout + base;
  float* d = graw + base;
  const float s0 = hm_sigmoid(r[0]), s1 = hm_sigmoid(r[(size_t)cells]), s4 = o[(size_t)4 * cells];
  d[0] = hm_centre_bwd(g[0], inv_sx, s0);
  d[(size_t)cells] = hm_centre_bwd(g[(size_t)cells], inv_sy, s1);
  d[(size_t)2 * cells] = hm_size_bwd(g[(size_t)2 * cells], r[(size_t)2 * cells], o[(size_t)2 * cells]);
  d[(size_t)3 * cells] = hm_size_bwd(g[(size_t)3 * cells], r[(size_t)3 * cells], o[(size_t)3 * cells]);
  d[(size_t)4 * cells] = hm_obj_bwd(g[(size_t)4 * cells], s4);
  const int C = P - 5;
  if (inference) {
    const float dot = hm_softmax_bwd_dot(g, o, cells, P);
    for (int c = 0; c < C; ++c) d[(size_t)(5 + c) * cells] = hm_softmax_bwd(g[(size_t)(5 + c) * cells], o[(size_t)(5 + c) * cells], dot);
  } else {
    for (int c = 0; c < C; ++c) d[(size_t)(5 + c) * cells] = g[(size_t)(5 + c) * cells];
  }
}

// the same with the gradient written as bf16 NCHW8c [B][kb(P)][cells][8] (padding channels zero): what the bf16 backward pass of
// the head convolution reads -- saves the fp32 tensor and the conversion pass
__global__ __launch_bounds__(256) void decode_bwd_bf16_kernel(const float* __restrict__ raw, const float* __restrict__ out,
                                                              const float* __restrict__ gout, hm_u32x4* __restrict__ g8, float inv_sx,
                                                              float inv_sy, int P, int Pb, int cells, int inference) {
  const int b = blockIdx.y;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const size_t base = (size_t)b * P * cells + cell;
  const float* r = raw + base;
  const float* o = out + base;
  const float* g = gout + base;
  const float dot = inference ? hm_softmax_bwd_dot(g, o, cells, P) : 0.f;
  const float s0 = hm_sigmoid(r[0]), s1 = hm_sigmoid(r[(size_t)cells]), s4 = o[(size_t)4 * cells];
  hm_store_bf16_8c(g8, b, cell, cells, P, Pb, [&](int ch) {
    const float gv = g[(size_t)ch * cells];
    if (ch == 0) return hm_centre_bwd(gv, inv_sx, s0);
    if (ch == 1) return hm_centre_bwd(gv, inv_sy, s1);
    if (ch == 2 || ch == 3) return hm_size_bwd(gv, r[(size_t)ch * cells], o[(size_t)ch * cells]);
    if (ch == 4) return hm_obj_bwd(gv, s4);
    return inference ? hm_softmax_bwd(gv, o[(size_t)ch * cells], dot) : gv;
  });
}

// ---- loss forward + backward -------------------------------------------------------------------------------------
struct LossWeights {
  float no_obj_weight, iou_weight, classify_weight, label_smoothing, inv_batch;
};
static LossWeights loss_weights(float no_obj_weight, float iou_weight, float classify_weight, float label_smoothing, int B) {
  return {no_obj_weight, iou_weight, classify_weight, label_smoothing, 1.0f / (float)B};
}

struct LossParams {
  const float* pred;   // [B][P][cells] decoded boxes + objectness, raw class logits
  const float* label;  // [B][6][cells] mask, x1, y1, x2, y2, class
  float* grad;         // [B][P][cells]  d(total loss)/d(pred)
  float* part;         // [B*gridDim.x][3] per-workgroup partial sums (iou, obj, cls) -- unweighted by 1/B
  int B, P, cells;
  LossWeights w;
};

__global__ __launch_bounds__(256) void yogo_loss_kernel(const LossParams p) {
  const int b = blockIdx.y;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const int cells = p.cells;
  const int C = p.P - 5;
  float l_iou = 0.f, l_obj = 0.f, l_cls = 0.f;
  if (cell < cells) {
    const float* pr = p.pred + (size_t)b * p.P * cells + cell;
    const float* lb = p.label + (size_t)b * 6 * cells + cell;
    float* gr = p.grad + (size_t)b * p.P * cells + cell;
    const float m = lb[0];
    l_obj = hm_obj_term(pr[(size_t)4 * cells], m, p.w.no_obj_weight, p.w.inv_batch, gr[(size_t)4 * cells]);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    if (m != 0.f)
      l_iou = hm_ciou_cell(pr[0], pr[(size_t)cells], pr[(size_t)2 * cells], pr[(size_t)3 * cells], lb, cells,
                           p.w.iou_weight * p.w.inv_batch, g0, g1, g2, g3);
    gr[0] = g0;
    gr[(size_t)cells] = g1;
    gr[(size_t)2 * cells] = g2;
    gr[(size_t)3 * cells] = g3;
    if (m != 0.f) {
      HmCeTerms ce;
      l_cls = hm_ce_cell(pr, cells, lb[(size_t)5 * cells], p.P, m, p.w.label_smoothing, p.w.classify_weight, p.w.inv_batch, ce);
      for (int c = 0; c < C; ++c) gr[(size_t)(5 + c) * cells] = hm_ce_grad(pr[(size_t)(5 + c) * cells], c, C, p.w.label_smoothing, ce);
    } else {
      for (int c = 0; c < C; ++c) gr[(size_t)(5 + c) * cells] = 0.f;
    }
  }
  hm_block_sum3(l_iou, l_obj, l_cls, p.part, b);
}

// ---- training step, fused: decode + loss forward/backward + decode backward in ONE pass over the cells ------------------
// (SURVEY.md K10 + K13-K15 for the trainer: yogo/model.py:277-313 -> yogo/yogo_loss.py:38-129 -> autograd of both.)  The three
// kernels above move 780 MB per 128-image step (decoded prediction and its gradient written and read back as fp32 tensors); a
// cell's decode, loss and both backward steps only need its own P raw values and 6 label values: 166 MB.  The same head_math.h
// calls as the three kernels, with the decoded box and its gradient in registers; training mode only (class logits pass through
// the decode).
struct FusedParams {
  const float* raw;    // [B][P][cells] head output
  const float* label;  // [B][6][cells]
  const float *cxs, *cys;
  hm_u32x4* g8;        // d total / d raw as bf16 NCHW8c [B][Pb][cells][8]
  float* part;         // as LossParams::part
  int B, P, Pb, cells;
  float inv_sx, inv_sy, anchor_w, anchor_h, wmul, hmul;
  LossWeights w;
};

__global__ __launch_bounds__(256) void decode_loss_bwd_bf16_kernel(const FusedParams p) {
  const int b = blockIdx.y;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const int cells = p.cells;
  const int C = p.P - 5;
  float l_iou = 0.f, l_obj = 0.f, l_cls = 0.f;
  if (cell < cells) {
    const float* r = p.raw + (size_t)b * p.P * cells + cell;
    const float* lb = p.label + (size_t)b * 6 * cells + cell;
    // decode
    const float t0 = r[0], t1 = r[(size_t)cells], t2 = r[(size_t)2 * cells], t3 = r[(size_t)3 * cells], t4 = r[(size_t)4 * cells];
    const float s0 = hm_sigmoid(t0), s1 = hm_sigmoid(t1);
    const float pcx = hm_centre(p.inv_sx, t0, p.cxs[cell]);
    const float pcy = hm_centre(p.inv_sy, t1, p.cys[cell]);
    const float pw = hm_size(p.anchor_w, t2, p.wmul);
    const float ph = hm_size(p.anchor_h, t3, p.hmul);
    const float po = hm_sigmoid(t4);
    // loss + gradient w.r.t. the decoded prediction
    const float m = lb[0];
    float gobj, g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    l_obj = hm_obj_term(po, m, p.w.no_obj_weight, p.w.inv_batch, gobj);
    HmCeTerms ce{};
    if (m != 0.f) {
      l_iou = hm_ciou_cell(pcx, pcy, pw, ph, lb, cells, p.w.iou_weight * p.w.inv_batch, g0, g1, g2, g3);
      l_cls = hm_ce_cell(r, cells, lb[(size_t)5 * cells], p.P, m, p.w.label_smoothing, p.w.classify_weight, p.w.inv_batch, ce);
    }
    // decode backward (training mode), written as bf16 NCHW8c units
    hm_store_bf16_8c(p.g8, b, cell, cells, p.P, p.Pb, [&](int ch) {
      if (ch == 0) return hm_centre_bwd(g0, p.inv_sx, s0);
      if (ch == 1) return hm_centre_bwd(g1, p.inv_sy, s1);
      if (ch == 2) return hm_size_bwd(g2, t2, pw);
      if (ch == 3) return hm_size_bwd(g3, t3, ph);
      if (ch == 4) return hm_obj_bwd(gobj, po);
      return m != 0.f ? hm_ce_grad(r[(size_t)ch * cells], ch - 5, C, p.w.label_smoothing, ce) : 0.f;
    });
  }
  hm_block_sum3(l_iou, l_obj, l_cls, p.part, b);
}

// out[0] = total, out[1] = iou_loss, out[2] = objectness_loss, out[3] = classification_loss
__global__ __launch_bounds__(256) void yogo_loss_finalize_kernel(const float* __restrict__ part, int rows, float iou_weight,
                                                                 float classify_weight, float inv_batch,
                                                                 float* __restrict__ out) {
  __shared__ double sh[3][4];
  double s[3] = {0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < rows; r += 256)
    for (int k = 0; k < 3; ++k) s[k] += (double)part[(size_t)r * 3 + k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < 3; ++k) {
    s[k] = wave_sum_d(s[k]);
    if (lane == 0) sh[k][wave] = s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float iou = (float)(iou_weight * (sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]) * inv_batch);
    const float obj = (float)((sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]) * inv_batch);
    const float cls = (float)(classify_weight * (sh[2][0] + sh[2][1] + sh[2][2] + sh[2][3]) * inv_batch);
    out[0] = obj + iou + cls;
    out[1] = iou;
    out[2] = obj;
    out[3] = cls;
  }
}

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" int yogo_decode_fwd(const float* raw, float* out, const float* cxs, const float* cys, int B, int P, int Sy,
                               int Sx, float anchor_w, float anchor_h, float width_multiplier, float height_multiplier,
                               int inference, hipStream_t stream) {
  YOGO_CHECK_ARG(raw && out && cxs && cys, "decode_fwd: null pointer");
  YOGO_CHECK_ARG(B >= 0 && P > 5 && P - 5 <= MAX_CLASSES && Sy > 0 && Sx > 0 && B <= 65535, "decode_fwd: bad shape");
  if (B == 0) return YOGO_OK;
  const int cells = Sy * Sx;
  yogo_launch_log("decode_fwd_kernel | B=%d cells=%d P=%d inference=%d", B, cells, P, inference);
  hipLaunchKernelGGL(decode_fwd_kernel, dim3(cdiv(cells, 256), B), dim3(256), 0, stream, raw, out, cxs, cys,
                     (float)(1.0 / Sx), (float)(1.0 / Sy), anchor_w, anchor_h, width_multiplier, height_multiplier, P, cells,
                     inference);
  YOGO_CHECK_LAUNCH("decode_fwd");
  return YOGO_OK;
}

extern "C" int yogo_decode_bwd(const float* raw, const float* out, const float* gout, float* graw, int B, int P, int Sy,
                               int Sx, int inference, hipStream_t stream) {
  YOGO_CHECK_ARG(raw && out && gout && graw, "decode_bwd: null pointer");
  YOGO_CHECK_ARG(B >= 0 && P > 5 && Sy > 0 && Sx > 0 && B <= 65535, "decode_bwd: bad shape");
  if (B == 0) return YOGO_OK;
  const int cells = Sy * Sx;
  hipLaunchKernelGGL(decode_bwd_kernel, dim3(cdiv(cells, 256), B), dim3(256), 0, stream, raw, out, gout, graw,
                     (float)(1.0 / Sx), (float)(1.0 / Sy), P, cells, inference);
  YOGO_CHECK_LAUNCH("decode_bwd");
  return YOGO_OK;
}

// graw8c: bf16 NCHW8c [B][2 * ceil(P / 16)][Sy][Sx][8]
extern "C" int yogo_decode_bwd_bf16(const float* raw, const float* out, const float* gout, void* graw8c, int B, int P, int Sy, int Sx,
                                    int inference, hipStream_t stream) {
  YOGO_CHECK_ARG(raw && out && gout && graw8c, "decode_bwd_bf16: null pointer");
  YOGO_CHECK_ARG(B >= 0 && P > 5 && Sy > 0 && Sx > 0 && B <= 65535, "decode_bwd_bf16: bad shape");
  if (B == 0) return YOGO_OK;
  const int cells = Sy * Sx;
  hipLaunchKernelGGL(decode_bwd_bf16_kernel, dim3(cdiv(cells, 256), B), dim3(256), 0, stream, raw, out, gout,
                     reinterpret_cast<hm_u32x4*>(graw8c), (float)(1.0 / Sx), (float)(1.0 / Sy), P, ((P + 15) / 16) * 2, cells, inference);
  YOGO_CHECK_LAUNCH("decode_bwd_bf16");
  return YOGO_OK;
}

extern "C" int yogo_loss_workspace_bytes(int B, int Sy, int Sx, size_t* bytes) {
  YOGO_CHECK_ARG(bytes && B > 0 && Sy > 0 && Sx > 0, "loss_workspace_bytes: bad arguments");
  *bytes = (size_t)B * cdiv(Sy * Sx, 256) * 3 * sizeof(float);
  return YOGO_OK;
}

// loss_out: 4 device floats (total, iou, objectness, classification); grad: d total / d pred, same shape as pred
extern "C" int yogo_loss_fwd_bwd(const float* pred, const float* label, float* grad, float* loss_out, void* workspace,
                                 int B, int P, int Sy, int Sx, float no_obj_weight, float iou_weight, float classify_weight,
                                 float label_smoothing, hipStream_t stream) {
  YOGO_CHECK_ARG(pred && label && grad && loss_out && workspace, "loss_fwd_bwd: null pointer");
  YOGO_CHECK_ARG(B > 0 && B <= 65535 && P > 5 && P - 5 <= MAX_CLASSES && Sy > 0 && Sx > 0, "loss_fwd_bwd: bad shape");
  LossParams p{};
  p.pred = pred; p.label = label; p.grad = grad; p.part = reinterpret_cast<float*>(workspace);
  p.B = B; p.P = P; p.cells = Sy * Sx;
  p.w = loss_weights(no_obj_weight, iou_weight, classify_weight, label_smoothing, B);
  const int nb = cdiv(p.cells, 256);
  hipLaunchKernelGGL(yogo_loss_kernel, dim3(nb, B), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(yogo_loss_finalize_kernel, dim3(1), dim3(256), 0, stream, p.part, B * nb, iou_weight, classify_weight,
                     p.w.inv_batch, loss_out);
  YOGO_CHECK_LAUNCH("loss_fwd_bwd");
  return YOGO_OK;
}

// the trainer's fused form of yogo_decode_fwd + yogo_loss_fwd_bwd + yogo_decode_bwd_bf16 (training mode: class logits pass through
// the decode).  graw8c: bf16 NCHW8c [B][2 * ceil(P / 16)][Sy][Sx][8]; loss_out / workspace as yogo_loss_fwd_bwd.
extern "C" int yogo_decode_loss_bwd_bf16(const float* raw, const float* label, const float* cxs, const float* cys, void* graw8c, float* loss_out,
                                         void* workspace, int B, int P, int Sy, int Sx, float anchor_w, float anchor_h, float width_multiplier,
                                         float height_multiplier, float no_obj_weight, float iou_weight, float classify_weight,
                                         float label_smoothing, hipStream_t stream) {
  YOGO_CHECK_ARG(raw && label && cxs && cys && graw8c && loss_out && workspace, "decode_loss_bwd_bf16: null pointer");
  YOGO_CHECK_ARG(B > 0 && B <= 65535 && P > 5 && P - 5 <= MAX_CLASSES && Sy > 0 && Sx > 0, "decode_loss_bwd_bf16: bad shape");
  FusedParams p{};
  p.raw = raw; p.label = label; p.cxs = cxs; p.cys = cys; p.g8 = reinterpret_cast<hm_u32x4*>(graw8c); p.part = reinterpret_cast<float*>(workspace);
  p.B = B; p.P = P; p.Pb = ((P + 15) / 16) * 2; p.cells = Sy * Sx;
  p.inv_sx = (float)(1.0 / Sx); p.inv_sy = (float)(1.0 / Sy); p.anchor_w = anchor_w; p.anchor_h = anchor_h; p.wmul = width_multiplier; p.hmul = height_multiplier;
  p.w = loss_weights(no_obj_weight, iou_weight, classify_weight, label_smoothing, B);
  const int nb = cdiv(p.cells, 256);
  hipLaunchKernelGGL(decode_loss_bwd_bf16_kernel, dim3(nb, B), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(yogo_loss_finalize_kernel, dim3(1), dim3(256), 0, stream, p.part, B * nb, iou_weight, classify_weight, p.w.inv_batch, loss_out);
  YOGO_CHECK_LAUNCH("decode_loss_bwd_bf16");
  return YOGO_OK;
}

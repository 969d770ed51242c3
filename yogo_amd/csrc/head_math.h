// The head's per-cell arithmetic, defined once: the box decode (yogo/model.py:277-313), its backward, and the grid-cell loss with its
// analytic gradient (yogo/yogo_loss.py:38-129).  Included by decode_loss.hip, nms.hip and conv_bf16_head.hip.
//
// Contract:
//   * every includer is compiled with -ffp-contract=off (build.sh, the product and the `variant` build alike), so "mul then add" stays two
//     roundings as on the CPU;
//   * the bits these functions produce are what the tests, the fixtures and the recorded runs hold: a kernel that needs one of these values
//     calls the function, it does not restate it;
//   * the operation order here is the order of yogo/model.py:277-313 and yogo/yogo_loss.py:38-129 -- regrouping an expression is a change
//     of results, not of style.
// A cell's P channels are addressed as col[ch * stride]: col points at the cell's channel 0, class c of the P - 5 is channel 5 + c.
#pragma once
#include "common.h"

typedef __bf16 hm_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int hm_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float hm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- decode forward ---------------------------------------------------------------------------------------------
// box centre from the raw value t, the cell's grid offset c and inv_s = 1 / grid size
__device__ __forceinline__ float hm_centre(float inv_s, float t, float c) { return inv_s * hm_sigmoid(t) + c; }
__device__ __forceinline__ float hm_size(float anchor, float t, float mul) { return anchor * expf(fminf(t, 80.f)) * mul; }
// softmax normalisation of a cell's class logits: the largest, then the sum in channel order
__device__ __forceinline__ void hm_softmax_terms(const float* col, size_t stride, int P, float& mx, float& sum) {
  const int C = P - 5;
  mx = -INFINITY;
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, col[(size_t)(5 + c) * stride]);
  sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(col[(size_t)(5 + c) * stride] - mx);
}
__device__ __forceinline__ float hm_softmax(float x, float mx, float sum) { return expf(x - mx) / sum; }

// ---- decode backward: g = d loss / d (decoded value) -> d loss / d (raw value) ---------------------------------------
__device__ __forceinline__ float hm_centre_bwd(float g, float inv_s, float s) { return g * (inv_s * (s * (1.f - s))); }   // s = sigmoid(t)
__device__ __forceinline__ float hm_size_bwd(float g, float t, float o) { return t <= 80.f ? g * o : 0.f; }               // o = the decoded size
__device__ __forceinline__ float hm_obj_bwd(float g, float s4) { return g * (s4 * (1.f - s4)); }                          // s4 = the decoded objectness
// softmax backward: dot over the cell's classes of gradient x output, then one element
__device__ __forceinline__ float hm_softmax_bwd_dot(const float* g, const float* o, size_t stride, int P) {
  const int C = P - 5;
  float dot = 0.f;
  for (int c = 0; c < C; ++c) dot += g[(size_t)(5 + c) * stride] * o[(size_t)(5 + c) * stride];
  return dot;
}
__device__ __forceinline__ float hm_softmax_bwd(float g, float o, float dot) { return o * (g - dot); }

// One cell's P channel values v(ch) as bf16 NCHW8c [B][Pb][cells][8]: 8 channels to one 16-byte store, padding channels zero.
template <class F>
__device__ __forceinline__ void hm_store_bf16_8c(hm_u32x4* g8, int b, int cell, int cells, int P, int Pb, F v) {
  for (int kb = 0; kb < Pb; ++kb) {
    hm_bf16x8 u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = kb * 8 + j;
      u[j] = (__bf16)(ch < P ? v(ch) : 0.f);
    }
    g8[((size_t)b * Pb + kb) * cells + cell] = __builtin_bit_cast(hm_u32x4, u);
  }
}

// ---- loss -------------------------------------------------------------------------------------------------------
// objectness: (pred4 - mask)^2 * (mask*(1-w) + w); g = d total / d pred4
__device__ __forceinline__ float hm_obj_term(float po, float m, float no_obj_weight, float inv_batch, float& g) {
  const float wgt = m * (1.f - no_obj_weight) + no_obj_weight;
  const float df = po - m;
  g = 2.f * df * wgt * inv_batch;
  return df * df * wgt;
}

// d max(a,b)/da as torch's `maximum` backward: 1 if a > b, 0.5 on ties, 0 otherwise (min likewise)
__device__ __forceinline__ float dmax_a(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float dmin_a(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

// CIoU of a labelled cell on clamp(xyxy(pred), 0, 1) vs the label's xyxy (lb[1..4 * stride]); returns the value, g0..g3 = its gradient
// w.r.t. (cx, cy, w, h) times sc = iou_weight * inv_batch.  A box without width or height has value and gradient zero.
__device__ __forceinline__ float hm_ciou_cell(float cx, float cy, float w, float h, const float* lb, size_t stride, float sc, float& g0,
                                              float& g1, float& g2, float& g3) {
  g0 = g1 = g2 = g3 = 0.f;
  const float x1 = cx - 0.5f * w, y1 = cy - 0.5f * h, x2 = cx + 0.5f * w, y2 = cy + 0.5f * h;
  if (!(x1 != x2 && y1 != y2)) return 0.f;
  const float X1 = fminf(fmaxf(x1, 0.f), 1.f), Y1 = fminf(fmaxf(y1, 0.f), 1.f);
  const float X2 = fminf(fmaxf(x2, 0.f), 1.f), Y2 = fminf(fmaxf(y2, 0.f), 1.f);
  const float c1 = (x1 >= 0.f && x1 <= 1.f) ? 1.f : 0.f, c2 = (y1 >= 0.f && y1 <= 1.f) ? 1.f : 0.f;
  const float c3 = (x2 >= 0.f && x2 <= 1.f) ? 1.f : 0.f, c4 = (y2 >= 0.f && y2 <= 1.f) ? 1.f : 0.f;
  const float x1g = lb[stride], y1g = lb[2 * stride], x2g = lb[3 * stride], y2g = lb[4 * stride];
  const float eps = 1e-7f;
  const float xk1 = fmaxf(X1, x1g), yk1 = fmaxf(Y1, y1g), xk2 = fminf(X2, x2g), yk2 = fminf(Y2, y2g);
  const bool has = (yk2 > yk1) && (xk2 > xk1);
  const float iw = xk2 - xk1, ih = yk2 - yk1;
  const float I = has ? iw * ih : 0.f;
  const float wp = X2 - X1, hp = Y2 - Y1, wg = x2g - x1g, hg = y2g - y1g;
  const float U = wp * hp + wg * hg - I;
  const float Ue = U + eps;
  const float iou = I / Ue;
  const float xc1 = fminf(X1, x1g), yc1 = fminf(Y1, y1g), xc2 = fmaxf(X2, x2g), yc2 = fmaxf(Y2, y2g);
  const float ex = xc2 - xc1, ey = yc2 - yc1;
  const float D = ex * ex + ey * ey + eps;
  const float dxc = (X2 + X1) / 2.f - (x1g + x2g) / 2.f, dyc = (Y2 + Y1) / 2.f - (y1g + y2g) / 2.f;
  const float dist = dxc * dxc + dyc * dyc;
  const float kv = 4.f / (3.14159265358979323846f * 3.14159265358979323846f);
  const float th = atanf(wg / hg) - atanf(wp / hp);
  const float v = kv * th * th;
  const float alpha = v / (1.f - iou + v + eps);
  // ---- gradient w.r.t. (X1, Y1, X2, Y2) ------------------------------------------------------------------------
  float dI1 = 0.f, dI2 = 0.f, dI3 = 0.f, dI4 = 0.f;
  if (has) {
    dI1 = -ih * dmax_a(X1, x1g);
    dI2 = -iw * dmax_a(Y1, y1g);
    dI3 = ih * dmin_a(X2, x2g);
    dI4 = iw * dmin_a(Y2, y2g);
  }
  const float dU1 = -hp - dI1, dU2 = -wp - dI2, dU3 = hp - dI3, dU4 = wp - dI4;
  const float iU2 = 1.f / (Ue * Ue);
  const float di1 = (dI1 * Ue - I * dU1) * iU2, di2 = (dI2 * Ue - I * dU2) * iU2;
  const float di3 = (dI3 * Ue - I * dU3) * iU2, di4 = (dI4 * Ue - I * dU4) * iU2;
  const float dD1 = -2.f * ex * dmin_a(X1, x1g), dD2 = -2.f * ey * dmin_a(Y1, y1g);
  const float dD3 = 2.f * ex * dmax_a(X2, x2g), dD4 = 2.f * ey * dmax_a(Y2, y2g);
  const float iD2 = 1.f / (D * D);
  const float dr1 = (dxc * D - dist * dD1) * iD2, dr2 = (dyc * D - dist * dD2) * iD2;
  const float dr3 = (dxc * D - dist * dD3) * iD2, dr4 = (dyc * D - dist * dD4) * iD2;
  const float den = hp * hp + wp * wp;
  const float dv_dw = -2.f * kv * th * hp / den, dv_dh = 2.f * kv * th * wp / den;
  const float gX1 = -di1 + dr1 - alpha * dv_dw, gY1 = -di2 + dr2 - alpha * dv_dh;
  const float gX2 = -di3 + dr3 + alpha * dv_dw, gY2 = -di4 + dr4 + alpha * dv_dh;
  g0 = (gX1 * c1 + gX2 * c3) * sc;
  g1 = (gY1 * c2 + gY2 * c4) * sc;
  g2 = 0.5f * (gX2 * c3 - gX1 * c1) * sc;
  g3 = 0.5f * (gY2 * c4 - gY1 * c2) * sc;
  return 1.f - iou + dist / D + alpha * v;
}

// log-softmax of one logit x, from the cell's largest logit mx and lsum = log(sum exp(x - mx)).  While |mx| <= LSE_FOLD_MAX the two
// constants are folded, x - (mx + lsum): mx + lsum < 32 there (lsum <= log 64), so folding rounds by at most 2^-20, 8 float32 spacings
// of the softmax, and these are the bits that every recorded run and fixture of ordinary logits holds.  Beyond, the folded sum would
// round at the size of the largest logit (5e-4 at 1e4), so the shift goes first, (x - mx) - lsum, as in torch's log_softmax.
#define LSE_FOLD_MAX 16.f
__device__ __forceinline__ float log_softmax_(float x, float mx, float lsum) {
  return fabsf(mx) <= LSE_FOLD_MAX ? x - (mx + lsum) : (x - mx) - lsum;
}

// what a labelled cell's per-class gradient needs of its cross entropy
struct HmCeTerms {
  float mx, lsum;   // largest logit, log(sum exp(x - mx))
  float scl;        // mask value * classify_weight * inv_batch
  int tgt;          // the label's class
};
// label-smoothed cross entropy of a labelled cell, weighted by the mask VALUE m (yogo_loss.py:107-114); cls = the label's class channel
__device__ __forceinline__ float hm_ce_cell(const float* col, size_t stride, float cls, int P, float m, float ls, float classify_weight,
                                            float inv_batch, HmCeTerms& t) {
  const int C = P - 5;
  t.tgt = (int)cls;
  float sum;
  hm_softmax_terms(col, stride, P, t.mx, sum);
  t.lsum = logf(sum);
  float nll_t = 0.f, nll_sum = 0.f;
  for (int c = 0; c < C; ++c) {
    const float lp = log_softmax_(col[(size_t)(5 + c) * stride], t.mx, t.lsum);
    nll_sum -= lp;
    if (c == t.tgt) nll_t = -lp;
  }
  t.scl = m * classify_weight * inv_batch;
  return m * ((1.f - ls) * nll_t + (ls / (float)C) * nll_sum);
}
// d total / d (logit x of class c) of that cell
__device__ __forceinline__ float hm_ce_grad(float x, int c, int C, float ls, const HmCeTerms& t) {
  const float sm = expf(log_softmax_(x, t.mx, t.lsum));
  return t.scl * (sm - (c == t.tgt ? (1.f - ls) : 0.f) - ls / (float)C);
}

// The three per-cell loss terms summed over a 256-lane workgroup (wavefront DPP sums, then LDS in fixed order) into
// part[(b * gridDim.x + blockIdx.x) * 3 + k], k = iou, obj, cls.  Every lane of the workgroup calls it.
__device__ __forceinline__ void hm_block_sum3(float l_iou, float l_obj, float l_cls, float* part, int b) {
  __shared__ float sh[3][4];
  l_iou = wave_sum(l_iou);
  l_obj = wave_sum(l_obj);
  l_cls = wave_sum(l_cls);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][wave] = l_iou;
    sh[1][wave] = l_obj;
    sh[2][wave] = l_cls;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    part[((size_t)b * gridDim.x + blockIdx.x) * 3 + k] = sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
  }
}

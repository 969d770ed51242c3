// BatchNorm2d (training + eval) around the conv kernels, and the small deterministic reductions the backward
// pass needs.  Replaces ATen batch_norm / batch_norm_backward behind nn.BatchNorm2d(…) in the reference
// (yogo/model_defns.py:35,55,60).
//
// Training statistics: the conv epilogues write per-workgroup partial (sum, sumsq) rows; bn_finalize adds them
// in fp64 in a fixed order (deterministic), producing mean / invstd and the momentum-0.1 running-stat update
// (biased variance to normalise, unbiased into running_var -- torch semantics).
// All element-wise kernels here are HBM-bound: one read + one write per element, float4 where the plane allows.
#include "bf16_dev.h"

// ---- what the kernels of this file share, each defined once ------------------------------------------------------
// the elements i < n of a plane that this thread takes: the plane's gridDim.x workgroups stride over it together.  (A macro: as a function
// taking the body as a lambda the backward kernels contract their products differently -- other bits.)
#define PLANE_WALK(i, n) for (int i = blockIdx.x * 256 + threadIdx.x; i < (n); i += gridDim.x * 256)

// per-channel parameters of N channels.  bn_chan_load fills them for channels c0 .. c0 + N - 1: scalars (N = 1, the fp32 kernels) or a
// 16-byte unit (8); a channel beyond C - 1 (a padding lane of a unit) takes channel C - 1's: what it computes is never stored.  The head
// pair fills a lane's half unit (N = 4) in its own loop (see there).
// stat_is_var != 0: `invstd_or_var` holds a variance (eval mode: running_var) and invstd is computed here.
template <int N>
struct BnChan {
  float mu[N], is[N], ga[N], be[N], sc[N];   // mean, invstd, gamma, beta, invstd * gamma
};
template <int N>
__device__ __forceinline__ void bn_chan_load(BnChan<N>& q, int c0, int C, const float* mean, const float* invstd_or_var, int stat_is_var,
                                             float eps, const float* gamma, const float* beta) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int c = min(c0 + j, C - 1);
    const float is = stat_is_var ? 1.0f / sqrtf(invstd_or_var[c] + eps) : invstd_or_var[c];
    q.mu[j] = mean[c];
    q.is[j] = is;
    q.ga[j] = gamma[c];
    q.be[j] = beta[c];
    q.sc[j] = is * gamma[c];
  }
}
// a mean term of dz, sum_g / n or sum_gx / n of channel c: with batch statistics; nothing with frozen ones
__device__ __forceinline__ float bn_mean_term(const float* sum, int c, float inv_count, int training) {
  return training ? sum[c] * inv_count : 0.f;
}

// One element of the backward pass.  g is the gradient w.r.t. the block output; when act != none the activation derivative is applied
// here, from the recomputed pre-activation xhat*gamma + beta (so no pre-activation tensor has to be saved, LeakyReLU and SiLU alike).
struct BnGrad {
  float xh, ge;   // xhat, g' = g * act'(xhat*gamma + beta)
};
template <int N>
__device__ __forceinline__ BnGrad bn_grad(const BnChan<N>& q, int j, float z, float g, int act) {
  const float xh = (z - q.mu[j]) * q.is[j];
  return {xh, g * act_bwd_factor(fmaf(xh, q.ga[j], q.be[j]), act)};
}
// the apply sweeps: dz = gamma * invstd * (g' - sum_g/n - xhat * sum_gx/n)   (training);  dz = gamma * invstd * g'  (frozen stats)
template <int N>
__device__ __forceinline__ float bn_dz(const BnChan<N>& q, int j, float z, float g, int act, float mg, float mgx) {
  const BnGrad e = bn_grad(q, j, z, g, act);
  return q.sc[j] * (e.ge - mg - e.xh * mgx);
}

// Partial rows [rows][C][2], rows = images * workgroups per plane (the *_rows queries): the pair of channel c in this workgroup's row
__device__ __forceinline__ float* bn_part_row(float* part, int b, int C, int c) {
  return part + ((size_t)(b * gridDim.x + blockIdx.x) * C + c) * 2;
}
// The tail of a reduce sweep, after every wavefront's block_put of its W / 2 channels' pairs into red[wave]: thread e < W adds the four
// wavefronts' entry e (common.h: left to right) and stores it, sum e & 1 of channel c0 + e / 2.
template <int W>
__device__ __forceinline__ void bn_part_store(const float (&red)[4][W], float* part, int b, int C, int c0) {
  __syncthreads();
  const int e = threadIdx.x, c = c0 + (e >> 1);
  if (e < W && c < C) bn_part_row(part, b, C, c)[e & 1] = block_sum4(red, e);
}

// ---- finalize: partial rows -> mean, invstd, running stats ---------------------------------------------------
// One workgroup per 8 channels: lane t sums the rows t / 8, t / 8 + 32, ... of channel 8 * blockIdx.x + t % 8 (8 adjacent
// channels = 64 contiguous bytes of a row), then the 32 row slices are folded in a fixed order through LDS.
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int rows, int row_stride, int C,
                                                          double count, float eps, float momentum,
                                                          float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                          float* __restrict__ running_mean, float* __restrict__ running_var,
                                                          long long* __restrict__ num_batches_tracked) {
  __shared__ double sh[2][32][8];
  const int cl = threadIdx.x & 7, slice = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;
  double s = 0.0, q = 0.0;
  if (c < C) {
    // (eight loads in flight, added in the same order: the chain of dependent load -> add steps was what the 24 us of this
    //  16-workgroup kernel were)
    int r = slice;
    for (; r + 7 * 32 < rows; r += 8 * 32) {
      float2 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float2*>(part + ((size_t)(r + j * 32) * row_stride + c) * 2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s += (double)v[j].x;
        q += (double)v[j].y;
      }
    }
    for (; r < rows; r += 32) {
      const float2 v = *reinterpret_cast<const float2*>(part + ((size_t)r * row_stride + c) * 2);
      s += (double)v.x;
      q += (double)v.y;
    }
  }
  sh[0][slice][cl] = s;
  sh[1][slice][cl] = q;
  __syncthreads();
  if (threadIdx.x < 8 && c < C) {
    s = 0.0;
    q = 0.0;
    for (int k = 0; k < 32; ++k) {
      s += sh[0][k][cl];
      q += sh[1][k][cl];
    }
    const double mean = s / count;
    double var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean != nullptr) {
      const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
      running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
      running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
    }
    if (c == 0 && num_batches_tracked != nullptr) *num_batches_tracked += 1;
  }
}

// ---- apply: y = act((z - mean) * (invstd * gamma) + beta) ------------------------------------------------------
template <bool VEC4>
__global__ __launch_bounds__(256) void bn_apply_act_kernel(const float* __restrict__ z, float* __restrict__ y,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd_or_var,
                                                           int stat_is_var, float eps, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int C, int HW, int act) {
  const int plane = blockIdx.y;
  BnChan<1> q;
  bn_chan_load(q, plane % C, C, mean, invstd_or_var, stat_is_var, eps, gamma, beta);
  const float* zp = z + (size_t)plane * HW;
  float* yp = y + (size_t)plane * HW;
  const auto fwd = [&](float v) { return act_fwd(fmaf(v - q.mu[0], q.sc[0], q.be[0]), act); };
  if (VEC4) {
    PLANE_WALK(i, HW >> 2) {
      float4 v = reinterpret_cast<const float4*>(zp)[i];
      v.x = fwd(v.x);
      v.y = fwd(v.y);
      v.z = fwd(v.z);
      v.w = fwd(v.w);
      reinterpret_cast<float4*>(yp)[i] = v;
    }
  } else {
    PLANE_WALK(i, HW) yp[i] = fwd(zp[i]);
  }
}

// ---- backward reduce: per (plane chunk) partial sums of g' and g' * xhat ----------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            int act, float* __restrict__ part, int C, int HW) {
  __shared__ float sh[4][2];
  const int plane = blockIdx.y;  // b*C + c
  const int c = plane % C;
  BnChan<1> q;
  bn_chan_load(q, c, C, mean, invstd, 0, 0.f, gamma, beta);
  const float* gp = g + (size_t)plane * HW;
  const float* zp = z + (size_t)plane * HW;
  float s = 0.f, t = 0.f;
  PLANE_WALK(i, HW) {
    const BnGrad e = bn_grad(q, 0, zp[i], gp[i], act);
    s += e.ge;
    t += e.ge * e.xh;
  }
  block_put2(sh[threadIdx.x >> 6], threadIdx.x & 63, 0, s, t);
  bn_part_store(sh, part, plane / C, C, c);
}

// dbeta = sum g, dgamma = sum g*xhat (fp64, fixed order), optionally clamped (the reference's per-parameter hook)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ part, int rows, int C, float clip,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ sum_g, float* __restrict__ sum_gx) {
  __shared__ double sh[4][2];
  const int c = blockIdx.x;
  double s = 0.0, q = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* src = part + ((size_t)r * C + c) * 2;
    s += (double)src[0];
    q += (double)src[1];
  }
  block_put2(sh[threadIdx.x >> 6], threadIdx.x & 63, 0, s, q);
  __syncthreads();
  if (threadIdx.x == 0) {
    s = block_sum4(sh, 0);
    q = block_sum4(sh, 1);
    sum_g[c] = (float)s;
    sum_gx[c] = (float)q;
    float db = (float)s, dg = (float)q;
    if (clip > 0.f) {
      db = fminf(fmaxf(db, -clip), clip);
      dg = fminf(fmaxf(dg, -clip), clip);
    }
    dbeta[c] = db;
    dgamma[c] = dg;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                           float* __restrict__ dz, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int act,
                                                           const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
                                                           float inv_count, int training, int C, int HW) {
  const int plane = blockIdx.y;
  const int c = plane % C;
  BnChan<1> q;
  bn_chan_load(q, c, C, mean, invstd, 0, 0.f, gamma, beta);
  const float mg = bn_mean_term(sum_g, c, inv_count, training), mgx = bn_mean_term(sum_gx, c, inv_count, training);
  const float* gp = g + (size_t)plane * HW;
  const float* zp = z + (size_t)plane * HW;
  float* dp = dz + (size_t)plane * HW;
  PLANE_WALK(i, HW) dp[i] = bn_dz(q, 0, zp[i], gp[i], act, mg, mgx);
}

// eval-mode helper: invstd = 1/sqrt(var + eps)
__global__ void bn_invstd_kernel(const float* __restrict__ var, float eps, float* __restrict__ invstd, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) invstd[c] = 1.0f / sqrtf(var[c] + eps);
}

// ---- generic deterministic reductions --------------------------------------------------------------------------
// out[j] = clamp(sum_r part[r][j]) for j < N  (fp64 accumulate, fixed order)
__global__ __launch_bounds__(256) void partials_reduce_kernel(const float* __restrict__ part, int rows, int N, float clip,
                                                              float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  double s = 0.0;
  int r = 0;   // (eight loads in flight, added in the same order)
  for (; r + 8 <= rows; r += 8) {
    float v8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v8[k] = part[(size_t)(r + k) * N + j];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (double)v8[k];
  }
  for (; r < rows; ++r) s += (double)part[(size_t)r * N + j];
  float v = (float)s;
  if (clip > 0.f) v = fminf(fmaxf(v, -clip), clip);
  out[j] = v;
}

// per-channel sum over (b, h, w) of an NCHW tensor (bias gradients): one workgroup per channel, fixed order
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ g, int B, int C, int HW, float clip,
                                                          float* __restrict__ out) {
  __shared__ double sh[4][1];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* gp = g + ((size_t)b * C + c) * HW;
    float ps = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) ps += gp[i];
    s += (double)ps;
  }
  block_put(sh[threadIdx.x >> 6], threadIdx.x & 63, 0, s);
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = (float)block_sum4(sh, 0);
    if (clip > 0.f) v = fminf(fmaxf(v, -clip), clip);
    out[c] = v;
  }
}

// =========================================================================================================
// Launch geometry.  grid = (workgroups per plane, planes): a plane is (image, channel) in fp32 and (image, channel block) in NCHW8c.
// Workgroups per plane, by family: 256 threads x the pixels a thread takes, 64 at the most.  The *_rows queries report images x this, and
// the launchers that write those rows call the same function.
// =========================================================================================================
static inline int plane_blocks(int HW, int per_thread) { return max(1, min(64, cdiv(HW, 256 * per_thread))); }
static inline int f32_blocks(int HW) { return plane_blocks(HW, 8); }
static inline int c8_blocks(int HW) { return plane_blocks(HW, 4); }
static inline int convert_blocks(int HW) { return plane_blocks(HW, 2); }
static inline int cb_of(int C) { return ((C + 15) / 16) * 2; }  // channel blocks: C padded to a multiple of 16

// gridDim.y holds the planes: the hardware's limit, refused before any launch
static int check_planes(const char* entry, int B, int per_image, const char* unit) {
  const long long limit = 65535;
  YOGO_CHECK_ARG((long long)B * per_image <= limit, "%s: batch * %s exceeds %lld", entry, unit, limit);
  return YOGO_OK;
}

// What the three backward entry points share.  Each runs bn_bwd_check, its reduce sweep, bn_bwd_finalize, its apply sweep.
struct BnBwdArgs {
  const float *mean, *invstd, *gamma, *beta;
  float *dgamma, *dbeta, *part, *sums;
  int B, C, HW;
  float clip;
  hipStream_t stream;
};
// io: the entry point's own tensors are there; shape: its further conditions on the shape
static int bn_bwd_check(const char* entry, bool io, bool shape, int planes_per_image, const char* unit, const BnBwdArgs& a) {
  YOGO_CHECK_ARG(io && a.mean && a.invstd && a.gamma && a.beta && a.dgamma && a.dbeta && a.part && a.sums, "%s: null pointer", entry);
  YOGO_CHECK_ARG(shape && a.B > 0 && a.C > 0 && a.HW > 0, "%s: bad shape", entry);
  return check_planes(entry, a.B, planes_per_image, unit);
}
// the fp64 sums of the B * nb partial rows -> sums (sum_g, then sum_gx), dgamma, dbeta; returns the apply sweep's 1 / (B HW)
static float bn_bwd_finalize(const BnBwdArgs& a, int nb) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(a.C), dim3(256), 0, a.stream, a.part, a.B * nb, a.C, a.clip, a.dgamma, a.dbeta, a.sums,
                     a.sums + a.C);
  return 1.0f / ((float)a.B * (float)a.HW);
}

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" int yogo_bn_finalize(const float* part, int rows, int row_stride, int C, long long count, float eps,
                                float momentum, float* mean_out, float* invstd_out, float* running_mean,
                                float* running_var, long long* num_batches_tracked, hipStream_t stream) {
  YOGO_CHECK_ARG(part && mean_out && invstd_out && C > 0 && rows > 0 && row_stride >= C && count > 0,
                 "bn_finalize: bad arguments");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 8)), dim3(256), 0, stream, part, rows, row_stride, C, (double)count, eps,
                     momentum, mean_out, invstd_out, running_mean, running_var, num_batches_tracked);
  YOGO_CHECK_LAUNCH("bn_finalize");
  return YOGO_OK;
}

extern "C" int yogo_bn_apply_act(const float* z, float* y, const float* mean, const float* invstd_or_var, int stat_is_var,
                                 float eps, const float* gamma, const float* beta, int B, int C, int HW, int act,
                                 hipStream_t stream) {
  YOGO_CHECK_ARG(z && y && mean && invstd_or_var && gamma && beta && C > 0 && HW > 0 && B >= 0, "bn_apply_act: bad arguments");
  if (B == 0) return YOGO_OK;
  if (int rc = check_planes("bn_apply_act", B, C, "channels")) return rc;
  if ((HW & 3) == 0) {
    dim3 grid(f32_blocks(HW), B * C);
    hipLaunchKernelGGL((bn_apply_act_kernel<true>), grid, dim3(256), 0, stream, z, y, mean, invstd_or_var, stat_is_var, eps,
                       gamma, beta, C, HW, act);
  } else {
    dim3 grid(plane_blocks(HW, 4), B * C);   // (the scalar walk: 4 pixels per thread; no partial rows depend on it)
    hipLaunchKernelGGL((bn_apply_act_kernel<false>), grid, dim3(256), 0, stream, z, y, mean, invstd_or_var, stat_is_var, eps,
                       gamma, beta, C, HW, act);
  }
  YOGO_CHECK_LAUNCH("bn_apply_act");
  return YOGO_OK;
}

extern "C" int yogo_bn_invstd(const float* var, float eps, float* invstd, int C, hipStream_t stream) {
  YOGO_CHECK_ARG(var && invstd && C > 0, "bn_invstd: bad arguments");
  hipLaunchKernelGGL(bn_invstd_kernel, dim3(cdiv(C, 256)), dim3(256), 0, stream, var, eps, invstd, C);
  YOGO_CHECK_LAUNCH("bn_invstd");
  return YOGO_OK;
}

extern "C" int yogo_bn_bwd_rows(int B, int HW, int* rows) {
  YOGO_CHECK_ARG(rows != nullptr, "bn_bwd_rows: null");
  *rows = B * f32_blocks(HW);
  return YOGO_OK;
}

// g: grad w.r.t. BN output; z: saved conv output; part: workspace rows*C*2 floats (rows from yogo_bn_bwd_rows).
// Writes dz (may alias g), dgamma, dbeta (clamped to +-clip when clip > 0).  sums: workspace 2*C floats.
extern "C" int yogo_bn_bwd(const float* g, const float* z, float* dz, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, int act, float* dgamma, float* dbeta, float* part,
                           float* sums, int B, int C, int HW, int training, float clip, hipStream_t stream) {
  const BnBwdArgs a{mean, invstd, gamma, beta, dgamma, dbeta, part, sums, B, C, HW, clip, stream};
  if (int rc = bn_bwd_check("bn_bwd", g && z && dz, true, C, "channels", a)) return rc;
  const int nb = f32_blocks(HW);
  const dim3 grid(nb, B * C);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, grid, dim3(256), 0, stream, g, z, mean, invstd, gamma, beta, act, part, C, HW);
  const float inv_count = bn_bwd_finalize(a, nb);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, stream, g, z, dz, mean, invstd, gamma, beta, act, sums, sums + C, inv_count,
                     training, C, HW);
  YOGO_CHECK_LAUNCH("bn_bwd");
  return YOGO_OK;
}

// in-place fold: row s (s < S) <- sum of rows s, s+S, s+2S, ...; each element is read and written by one thread only
__global__ __launch_bounds__(256) void partials_fold_kernel(float* __restrict__ part, int rows, int N, int S) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int s = blockIdx.y;
  if (j >= N) return;
  double acc = 0.0;
  int r = s;   // (eight loads in flight, added in the same order)
  for (; r + 7 * S < rows; r += 8 * S) {
    float v8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v8[k] = part[(size_t)(r + k * S) * N + j];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (double)v8[k];
  }
  for (; r < rows; r += S) acc += (double)part[(size_t)r * N + j];
  part[(size_t)s * N + j] = (float)acc;
}

// out[j] = clamp(sum_r part[r][j]).  NOTE: `part` is used as scratch (folded in place) when rows > 64.
extern "C" int yogo_partials_reduce(float* part, int rows, int N, float clip, float* out, hipStream_t stream) {
  YOGO_CHECK_ARG(part && out && rows > 0 && N > 0, "partials_reduce: bad arguments");
  if (rows > 64) {
    const int S = 64;
    hipLaunchKernelGGL(partials_fold_kernel, dim3(cdiv(N, 256), S), dim3(256), 0, stream, part, rows, N, S);
    rows = S;
  }
  hipLaunchKernelGGL(partials_reduce_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, part, rows, N, clip, out);
  YOGO_CHECK_LAUNCH("partials_reduce");
  return YOGO_OK;
}

extern "C" int yogo_channel_sum(const float* g, int B, int C, int HW, float clip, float* out, hipStream_t stream) {
  YOGO_CHECK_ARG(g && out && B > 0 && C > 0 && HW > 0, "channel_sum: bad arguments");
  hipLaunchKernelGGL(channel_sum_kernel, dim3(C), dim3(256), 0, stream, g, B, C, HW, clip, out);
  YOGO_CHECK_LAUNCH("channel_sum");
  return YOGO_OK;
}

// =========================================================================================================
// bf16 NCHW8c variants (training in bf16 storage): one 16-byte unit = 8 consecutive channels of one pixel.
// A "plane" is (image, channel block); statistics stay fp32 / fp64.
// =========================================================================================================
// this workgroup's plane: image, channel block, index of the plane's first unit
struct Plane8c {
  int b, cb;
  size_t at;
};
__device__ __forceinline__ Plane8c plane_8c(int Cb, int HW) {
  const int plane = blockIdx.y;  // b*Cb + cb
  return {plane / Cb, plane % Cb, (size_t)plane * HW};
}
__device__ __forceinline__ bf16x8 unit_load(const u32x4* p) { return __builtin_bit_cast(bf16x8, *p); }
// lane j of the unit of channel block cb: the result, or zero in a padding channel (>= C)
__device__ __forceinline__ __bf16 unit_lane(float r, int cb, int j, int C) { return (cb * 8 + j < C) ? (__bf16)r : (__bf16)0.f; }

__global__ __launch_bounds__(256) void bn_apply_act_8c_kernel(const u32x4* __restrict__ z, u32x4* __restrict__ y,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd_or_var, int stat_is_var, float eps,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              int C, int Cb, int HW, int act) {
  const Plane8c p = plane_8c(Cb, HW);
  BnChan<8> q;
  bn_chan_load(q, p.cb * 8, C, mean, invstd_or_var, stat_is_var, eps, gamma, beta);
  float sh2[8];  // y = z * sc + (beta - mean * sc): one FMA per value (conv_first_mfma_kernel applies the same form)
#pragma unroll
  for (int j = 0; j < 8; ++j) sh2[j] = fmaf(-q.mu[j], q.sc[j], q.be[j]);
  PLANE_WALK(i, HW) {
    const bf16x8 v = unit_load(z + p.at + i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = unit_lane(act_fwd(fmaf((float)v[j], q.sc[j], sh2[j]), act), p.cb, j, C);
    y[p.at + i] = __builtin_bit_cast(u32x4, o);
  }
}

// A reduce sweep over the planes of an 8c tensor: add(i, s, t) adds pixel i of plane p into the two running sums of its eight channels,
// then the block reduction and the partial row.  rows = B * gridDim.x.
template <class F>
__device__ __forceinline__ void reduce_8c(const Plane8c& p, float* part, int C, int HW, F&& add) {
  __shared__ float sh[4][16];
  float s[8], t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = t[j] = 0.f;
  PLANE_WALK(i, HW) add(i, s, t);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) block_put2(sh[wave], lane, 2 * j, s[j], t[j]);
  bn_part_store(sh, part, p.b, C, p.cb * 8);
}

// batch statistics of a stored bf16 tensor: partial (sum, sum of squares) per channel
__global__ __launch_bounds__(256) void bn_stats_8c_kernel(const u32x4* __restrict__ z, float* __restrict__ part, int C, int Cb,
                                                          int HW) {
  const Plane8c p = plane_8c(Cb, HW);
  reduce_8c(p, part, C, HW, [&](int i, float (&s)[8], float (&t)[8]) {
    const bf16x8 zv = unit_load(z + p.at + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = (float)zv[j];
      s[j] += v;
      t[j] = fmaf(v, v, t[j]);
    }
  });
}

// partial sums of g' and g' * xhat per channel
__global__ __launch_bounds__(256) void bn_bwd_reduce_8c_kernel(const u32x4* __restrict__ g, const u32x4* __restrict__ z,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               int act, float* __restrict__ part, int C, int Cb, int HW) {
  const Plane8c p = plane_8c(Cb, HW);
  BnChan<8> q;
  bn_chan_load(q, p.cb * 8, C, mean, invstd, 0, 0.f, gamma, beta);
  reduce_8c(p, part, C, HW, [&](int i, float (&s)[8], float (&t)[8]) {
    const bf16x8 gv = unit_load(g + p.at + i), zv = unit_load(z + p.at + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const BnGrad e = bn_grad(q, j, (float)zv[j], (float)gv[j], act);
      s[j] += e.ge;
      t[j] += e.ge * e.xh;
    }
  });
}

__global__ __launch_bounds__(256) void bn_bwd_apply_8c_kernel(const u32x4* __restrict__ g, const u32x4* __restrict__ z,
                                                              u32x4* __restrict__ dz, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int act,
                                                              const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
                                                              float inv_count, int training, int C, int Cb, int HW) {
  const Plane8c p = plane_8c(Cb, HW);
  BnChan<8> q;
  bn_chan_load(q, p.cb * 8, C, mean, invstd, 0, 0.f, gamma, beta);
  float mg[8], mgx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = min(p.cb * 8 + j, C - 1);   // (a padding lane: bn_chan_load's rule)
    mg[j] = bn_mean_term(sum_g, c, inv_count, training);
    mgx[j] = bn_mean_term(sum_gx, c, inv_count, training);
  }
  PLANE_WALK(i, HW) {
    const bf16x8 gv = unit_load(g + p.at + i), zv = unit_load(z + p.at + i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = unit_lane(bn_dz(q, j, (float)zv[j], (float)gv[j], act, mg[j], mgx[j]), p.cb, j, C);
    dz[p.at + i] = __builtin_bit_cast(u32x4, o);
  }
}

// fp32 NCHW -> bf16 NCHW8c (Cb channel blocks, padding channels zero) and back
__global__ __launch_bounds__(256) void nchw_f32_to_8c_kernel(const float* __restrict__ in, u32x4* __restrict__ out, int C, int Cb,
                                                             int HW) {
  const Plane8c p = plane_8c(Cb, HW);
  PLANE_WALK(i, HW) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = p.cb * 8 + j;
      o[j] = (c < C) ? (__bf16)in[((size_t)p.b * C + c) * HW + i] : (__bf16)0.f;   // (unit_lane's test, in front of the load)
    }
    out[p.at + i] = __builtin_bit_cast(u32x4, o);
  }
}

__global__ __launch_bounds__(256) void nchw8c_to_f32_kernel(const u32x4* __restrict__ in, float* __restrict__ out, int C, int Cb,
                                                            int HW) {
  const Plane8c p = plane_8c(Cb, HW);
  PLANE_WALK(i, HW) {
    const bf16x8 v = unit_load(in + p.at + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = p.cb * 8 + j;
      if (c < C) out[((size_t)p.b * C + c) * HW + i] = (float)v[j];
    }
  }
}

extern "C" int yogo_bn_apply_act_bf16(const void* z, void* y, const float* mean, const float* invstd_or_var, int stat_is_var,
                                      float eps, const float* gamma, const float* beta, int B, int C, int HW, int act,
                                      hipStream_t stream) {
  YOGO_CHECK_ARG(z && y && mean && invstd_or_var && gamma && beta && C > 0 && HW > 0 && B >= 0, "bn_apply_act_bf16: bad arguments");
  if (B == 0) return YOGO_OK;
  const int Cb = cb_of(C);
  if (int rc = check_planes("bn_apply_act_bf16", B, Cb, "channel blocks")) return rc;
  hipLaunchKernelGGL(bn_apply_act_8c_kernel, dim3(c8_blocks(HW), B * Cb), dim3(256), 0, stream, reinterpret_cast<const u32x4*>(z),
                     reinterpret_cast<u32x4*>(y), mean, invstd_or_var, stat_is_var, eps, gamma, beta, C, Cb, HW, act);
  YOGO_CHECK_LAUNCH("bn_apply_act_bf16");
  return YOGO_OK;
}

extern "C" int yogo_bn_bwd_bf16_rows(int B, int HW, int* rows) {
  YOGO_CHECK_ARG(rows != nullptr, "bn_bwd_bf16_rows: null");
  *rows = B * c8_blocks(HW);
  return YOGO_OK;
}

// bf16 NCHW8c g (gradient w.r.t. the block output), z (saved conv output) -> dz (may alias g), dgamma, dbeta
extern "C" int yogo_bn_bwd_bf16(const void* g, const void* z, void* dz, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, int act, float* dgamma, float* dbeta, float* part,
                                float* sums, int B, int C, int HW, int training, float clip, hipStream_t stream) {
  const BnBwdArgs a{mean, invstd, gamma, beta, dgamma, dbeta, part, sums, B, C, HW, clip, stream};
  const int Cb = cb_of(C), nb = c8_blocks(HW);
  if (int rc = bn_bwd_check("bn_bwd_bf16", g && z && dz, true, Cb, "channel blocks", a)) return rc;
  const dim3 grid(nb, B * Cb);
  const u32x4* g4 = reinterpret_cast<const u32x4*>(g);
  const u32x4* z4 = reinterpret_cast<const u32x4*>(z);
  hipLaunchKernelGGL(bn_bwd_reduce_8c_kernel, grid, dim3(256), 0, stream, g4, z4, mean, invstd, gamma, beta, act, part, C, Cb, HW);
  const float inv_count = bn_bwd_finalize(a, nb);
  hipLaunchKernelGGL(bn_bwd_apply_8c_kernel, grid, dim3(256), 0, stream, g4, z4, reinterpret_cast<u32x4*>(dz), mean, invstd, gamma, beta, act,
                     sums, sums + C, inv_count, training, C, Cb, HW);
  YOGO_CHECK_LAUNCH("bn_bwd_bf16");
  return YOGO_OK;
}

// ---- BatchNorm backward of the block UNDER a 1x1 convolution with P <= 16 outputs (the detection head, yogo/model.py:150-155) without that
// convolution's data gradient in memory.  g[c][pixel] = sum_k gh[k][pixel] * w[k][c] is one v_mfma_f32_16x16x32_bf16 per 16 pixels x 16 channels:
// A = the weights (row = channel, K = the head's outputs), B = the head's output gradient (column = pixel; its 16-byte units are the operand
// as they lie in memory), so lane (c16, g4) gets channels 4 g4 .. 4 g4 + 3 of pixel c16 -- the half of a 16-byte unit of z it then works on.
// Both sweeps compute the same g (rounded to bf16 as the data-gradient kernel's output would have been): the 128-channel gradient tensor is
// never written or read (-0.41 GB written, -0.82 GB read per step of base_model at batch 128).
// The pair keeps its own lane set-up, parameter loop and stripe loop (every channel 16 cp + 4 g4 + i exists: no clamp): with the set-up
// behind one struct, the walk behind a macro and bn_chan_load's clamped loop, yogo_bn_bwd_bf16_head at 128 x 128 x 97*129 took 356.6 against
// 354.6 us (LeakyReLU, frozen statistics) and 444.7 against 437.8 us (SiLU, batch statistics), outside the earlier text's own spread (profiles/bn_one_definition.log, 3a).
struct BnHeadLane {
  bf16x8 wop;     // A operand: channel 16 cp + c16, head outputs 8 g4 .. 8 g4 + 7
  BnChan<4> q;    // channels 16 cp + 4 g4 + i
};
__device__ __forceinline__ void bn_head_lane(BnHeadLane& L, const float* __restrict__ hw, int P, int C, int cp, int c16, int g4, const float* mean,
                                             const float* invstd, const float* gamma, const float* beta) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * g4 + j;
    L.wop[j] = (k < P) ? (__bf16)hw[(size_t)k * C + 16 * cp + c16] : (__bf16)0.f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 16 * cp + 4 * g4 + i;
    L.q.mu[i] = mean[c]; L.q.is[i] = invstd[c]; L.q.ga[i] = gamma[c]; L.q.be[i] = beta[c]; L.q.sc[i] = invstd[c] * gamma[c];
  }
}
// this lane's four gradients (bf16-rounded, widened) and pre-activations of pixel px (nothing beyond the plane: zeros)
__device__ __forceinline__ void bn_head_fetch(const BnHeadLane& L, const u32x4* __restrict__ ghp, const u32x2* __restrict__ zp2, int HW, int px, int g4,
                                              float (&gb)[4], float (&zf)[4]) {
  const bool valid = px < HW;
  u32x4 gop = {0u, 0u, 0u, 0u};
  if (valid && g4 < 2) gop = ghp[(size_t)g4 * HW + px];
  u32x2 zr = {0u, 0u};
  if (valid) zr = zp2[(size_t)px * 2];
  const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(L.wop, __builtin_bit_cast(bf16x8, gop), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  const bf16x4 zv = __builtin_bit_cast(bf16x4, zr);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gb[i] = (float)(__bf16)d[i];
    zf[i] = (float)zv[i];
  }
}
__global__ __launch_bounds__(256) void bn_bwd_reduce_head_kernel(const u32x4* __restrict__ gh, const float* __restrict__ hw, int P,
                                                                 const u32x4* __restrict__ z, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int act, float* __restrict__ part, int C, int Cb, int HW) {
  __shared__ float sh[4][32];
  const int cp = blockIdx.y % (Cb / 2), b = blockIdx.y / (Cb / 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c16 = lane & 15, g4 = lane >> 4;
  BnHeadLane L;
  bn_head_lane(L, hw, P, C, cp, c16, g4, mean, invstd, gamma, beta);
  const u32x4* ghp = gh + (size_t)b * 2 * HW;
  const u32x2* zp2 = reinterpret_cast<const u32x2*>(z + ((size_t)b * Cb + 2 * cp + (g4 >> 1)) * HW) + (g4 & 1);
  float s[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};
  for (int px0 = (blockIdx.x * 4 + wave) * 16; px0 < HW; px0 += gridDim.x * 64) {
    float gb[4], zf[4];
    bn_head_fetch(L, ghp, zp2, HW, px0 + c16, g4, gb, zf);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const BnGrad e = bn_grad(L.q, i, zf[i], gb[i], act);
      s[i] += e.ge;
      t[i] += e.ge * e.xh;
    }
  }
  // sums over the 16 pixels of a lane group (not block_put's whole wavefront: its four groups hold different channels); the four
  // wavefronts' entries then meet as everywhere
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a = s[i], c = t[i];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      c += __shfl_xor(c, o, 64);
    }
    if (c16 == 0) {
      sh[wave][2 * (4 * g4 + i)] = a;
      sh[wave][2 * (4 * g4 + i) + 1] = c;
    }
  }
  bn_part_store(sh, part, b, C, 16 * cp);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_head_kernel(const u32x4* __restrict__ gh, const float* __restrict__ hw, int P,
                                                                const u32x4* __restrict__ z, u32x4* __restrict__ dz, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int act, const float* __restrict__ sum_g,
                                                                const float* __restrict__ sum_gx, float inv_count, int training, int C, int Cb, int HW) {
  const int cp = blockIdx.y % (Cb / 2), b = blockIdx.y / (Cb / 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c16 = lane & 15, g4 = lane >> 4;
  BnHeadLane L;
  bn_head_lane(L, hw, P, C, cp, c16, g4, mean, invstd, gamma, beta);
  float mg[4], mgx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mg[i] = bn_mean_term(sum_g, 16 * cp + 4 * g4 + i, inv_count, training);
    mgx[i] = bn_mean_term(sum_gx, 16 * cp + 4 * g4 + i, inv_count, training);
  }
  const u32x4* ghp = gh + (size_t)b * 2 * HW;
  const size_t plane_u = ((size_t)b * Cb + 2 * cp + (g4 >> 1)) * HW;
  const u32x2* zp2 = reinterpret_cast<const u32x2*>(z + plane_u) + (g4 & 1);
  u32x2* dp2 = reinterpret_cast<u32x2*>(dz + plane_u) + (g4 & 1);
  for (int px0 = (blockIdx.x * 4 + wave) * 16; px0 < HW; px0 += gridDim.x * 64) {
    const int px = px0 + c16;
    float gb[4], zf[4];
    bn_head_fetch(L, ghp, zp2, HW, px, g4, gb, zf);
    bf16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (__bf16)bn_dz(L.q, i, zf[i], gb[i], act, mg[i], mgx[i]);
    if (px < HW) dp2[(size_t)px * 2] = __builtin_bit_cast(u32x2, o);
  }
}
// yogo_bn_bwd_bf16 with g computed from the head's output gradient gh (bf16 NCHW8c [B][2][HW], channels >= P zero) and the head's weights
// head_w ([P][C] fp32, OIHW of a 1x1 convolution; rounded to bf16 here as the packed operand of the head's data gradient is).  C a multiple of
// 16.  dz must not alias gh.
extern "C" int yogo_bn_bwd_bf16_head(const void* gh, const float* head_w, int P, const void* z, void* dz, const float* mean, const float* invstd,
                                     const float* gamma, const float* beta, int act, float* dgamma, float* dbeta, float* part, float* sums,
                                     int B, int C, int HW, int training, float clip, hipStream_t stream) {
  const BnBwdArgs a{mean, invstd, gamma, beta, dgamma, dbeta, part, sums, B, C, HW, clip, stream};
  const int Cb = cb_of(C), nb = c8_blocks(HW);
  if (int rc = bn_bwd_check("bn_bwd_bf16_head", gh && head_w && z && dz, (C % 16) == 0 && P > 0 && P <= 16, Cb, "channel blocks", a)) return rc;
  const dim3 grid(nb, B * (Cb / 2));   // a workgroup takes a PAIR of channel blocks
  const u32x4* g4 = reinterpret_cast<const u32x4*>(gh);
  const u32x4* z4 = reinterpret_cast<const u32x4*>(z);
  if (yogo_launch_log_enabled()) {
    yogo_launch_log("bn_bwd_reduce_head_kernel | B=%d C=%d HW=%d P=%d act=%d grid=%dx%d", B, C, HW, P, act, nb, B * (Cb / 2));
    yogo_launch_log("bn_bwd_apply_head_kernel | B=%d C=%d HW=%d P=%d act=%d training=%d grid=%dx%d", B, C, HW, P, act, training, nb, B * (Cb / 2));
  }
  hipLaunchKernelGGL(bn_bwd_reduce_head_kernel, grid, dim3(256), 0, stream, g4, head_w, P, z4, mean, invstd, gamma, beta, act, part, C, Cb, HW);
  const float inv_count = bn_bwd_finalize(a, nb);
  hipLaunchKernelGGL(bn_bwd_apply_head_kernel, grid, dim3(256), 0, stream, g4, head_w, P, z4, reinterpret_cast<u32x4*>(dz), mean, invstd, gamma, beta,
                     act, sums, sums + C, inv_count, training, C, Cb, HW);
  YOGO_CHECK_LAUNCH("bn_bwd_bf16_head");
  return YOGO_OK;
}

// batch statistics of a bf16 NCHW8c tensor (the stored convolution output) as partial rows for yogo_bn_finalize:
// part [rows][C][2] with rows from yogo_bn_bwd_bf16_rows(B, HW).  Cheaper than carrying the sums through the convolution's
// epilogue when that epilogue is on the critical path of a one-workgroup-per-CU kernel.
extern "C" int yogo_bn_stats_bf16(const void* z, float* part, int B, int C, int HW, hipStream_t stream) {
  YOGO_CHECK_ARG(z && part && B > 0 && C > 0 && HW > 0, "bn_stats_bf16: bad arguments");
  const int Cb = cb_of(C);
  if (int rc = check_planes("bn_stats_bf16", B, Cb, "channel blocks")) return rc;
  hipLaunchKernelGGL(bn_stats_8c_kernel, dim3(c8_blocks(HW), B * Cb), dim3(256), 0, stream, reinterpret_cast<const u32x4*>(z), part, C, Cb, HW);
  YOGO_CHECK_LAUNCH("bn_stats_bf16");
  return YOGO_OK;
}

extern "C" int yogo_nchw_f32_to_bf16_8c(const float* in, void* out, int B, int C, int HW, hipStream_t stream) {
  YOGO_CHECK_ARG(in && out && B > 0 && C > 0 && HW > 0, "nchw_f32_to_bf16_8c: bad arguments");
  const int Cb = cb_of(C);
  if (int rc = check_planes("nchw_f32_to_bf16_8c", B, Cb, "channel blocks")) return rc;
  hipLaunchKernelGGL(nchw_f32_to_8c_kernel, dim3(convert_blocks(HW), B * Cb), dim3(256), 0, stream, in, reinterpret_cast<u32x4*>(out), C, Cb,
                     HW);
  YOGO_CHECK_LAUNCH("nchw_f32_to_bf16_8c");
  return YOGO_OK;
}

extern "C" int yogo_bf16_8c_to_nchw_f32(const void* in, float* out, int B, int C, int HW, hipStream_t stream) {
  YOGO_CHECK_ARG(in && out && B > 0 && C > 0 && HW > 0, "bf16_8c_to_nchw_f32: bad arguments");
  const int Cb = cb_of(C);
  if (int rc = check_planes("bf16_8c_to_nchw_f32", B, Cb, "channel blocks")) return rc;
  hipLaunchKernelGGL(nchw8c_to_f32_kernel, dim3(convert_blocks(HW), B * Cb), dim3(256), 0, stream, reinterpret_cast<const u32x4*>(in), out, C, Cb,
                     HW);
  YOGO_CHECK_LAUNCH("bf16_8c_to_nchw_f32");
  return YOGO_OK;
}

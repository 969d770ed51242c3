// The output stage of `yogo infer --device-outputs` (yogo_amd/pred_sink.py): the kept rows that the threshold + NMS launch left at
// fixed strides (rows [B][cap][P], counts [B]) are compacted, transformed and counted into buffers that stay in HBM, so that the
// host reads kept rows only, once, instead of B * cap * P padded floats per batch.
//
//   mode 0 ("npy")   record = the 8 + C columns of format_to_numpy (yogo/utils/prediction_formatting.py:96-156):
//                    image id, x1*img_w, y1*img_h, x2*img_w, y2*img_h, objectness, first-argmax class, its score, the C scores
//   mode 1 ("rows")  record = the row itself (P floats)
//   arena == null    nothing is compacted; only the class histogram is updated
//
// Two launches, both stream-ordered, neither read by the host:
//   pred_sink_scan_kernel   ONE workgroup: clamps counts[b] to [0, cap], turns them into the arena row every image starts at (running
//                           total + exclusive prefix, into the workspace), appends them to img_counts at the running image total and
//                           advances the state.  Each lane sums a contiguous chunk of images, the chunk sums are scanned in LDS: any B.
//   pred_sink_copy_kernel   one workgroup per image, TILE rows at a time: a lane per row finds the first-argmax class (LDS), then the
//                           tile's records are written with consecutive lanes on consecutive floats (reads of the kept rows are
//                           consecutive too; the entries past counts[b] are never read).  Class counts go to an LDS histogram and
//                           from there to the state with one integer atomic per class and workgroup.
// Traffic per batch at the production geometry is 1-2 MB; the kernel exists to remove the padded read-back, not to win a roofline.
#include "common.h"
#include <climits>

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int COPY_THREADS = 256;
constexpr int TILE = COPY_THREADS;   // rows per step of the copy kernel: one lane per row in the argmax phase
constexpr int MAX_CLASSES = 1024;    // LDS histogram

// int64 state block (yogo_pred_sink_state_layout)
constexpr int ST_ROWS = 0;           // records in the arena
constexpr int ST_IMAGES = 1;         // entries in img_counts
constexpr int ST_DROPPED_ROWS = 2;   // records that did not fit in arena_cap
constexpr int ST_DROPPED_IMAGES = 3; // image entries that did not fit in img_cap
constexpr int ST_CLASS_COUNTS = 4;   // [C]

__device__ __forceinline__ int clamp_count(int c, int cap) { return c < 0 ? 0 : (c > cap ? cap : c); }

__global__ __launch_bounds__(SCAN_THREADS) void pred_sink_scan_kernel(const int* __restrict__ counts, int B, int cap,
                                                                      long long* state, long long arena_cap,
                                                                      int* __restrict__ img_counts, long long img_cap,
                                                                      long long* __restrict__ dst_row) {
  __shared__ long long sum_s[SCAN_THREADS];
  const int tid = threadIdx.x;
  // read by every lane before lane 0 advances it (behind the barriers below)
  const long long row_base = state[ST_ROWS];
  const long long img_base = state[ST_IMAGES];
  const int per = (B + SCAN_THREADS - 1) / SCAN_THREADS;
  const long long b0 = (long long)tid * per;
  long long own = 0;
  for (int k = 0; k < per; ++k) {
    const long long b = b0 + k;
    if (b < B) own += clamp_count(counts[b], cap);
  }
  sum_s[tid] = own;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {   // inclusive scan of the chunk sums
    const long long add = tid >= o ? sum_s[tid - o] : 0;
    __syncthreads();
    sum_s[tid] += add;
    __syncthreads();
  }
  long long run = row_base + sum_s[tid] - own;
  for (int k = 0; k < per; ++k) {
    const long long b = b0 + k;
    if (b < B) {
      const int c = clamp_count(counts[b], cap);
      dst_row[b] = run;
      if (img_base + b < img_cap) img_counts[img_base + b] = c;
      run += c;
    }
  }
  if (tid == 0) {
    const long long total = sum_s[SCAN_THREADS - 1];
    long long room = arena_cap - row_base;
    room = room < 0 ? 0 : room;
    const long long written = total < room ? total : room;
    long long iroom = img_cap - img_base;
    iroom = iroom < 0 ? 0 : iroom;
    const long long iwritten = B < iroom ? B : iroom;
    state[ST_ROWS] = row_base + written;
    state[ST_IMAGES] = img_base + iwritten;
    state[ST_DROPPED_ROWS] += total - written;
    state[ST_DROPPED_IMAGES] += B - iwritten;
  }
}

// first maximum, a NaN counting as the maximum (torch.max / np.argmax)
__device__ __forceinline__ int argmax_first(const float* __restrict__ v, int C, float& best) {
  best = v[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float x = v[c];
    if (best == best && (x > best || x != x)) {
      best = x;
      arg = c;
    }
  }
  return arg;
}

// MODE 0 npy records, 1 row records, 2 no records.  grid (B)
template <int MODE>
__global__ __launch_bounds__(COPY_THREADS) void pred_sink_copy_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int cap,
                                                                      int P, int count_classes, long long first_img_id, float img_h,
                                                                      float img_w, long long* __restrict__ state, float* __restrict__ arena,
                                                                      long long arena_cap, const long long* __restrict__ dst_row) {
  __shared__ int hist_s[MAX_CLASSES];
  __shared__ int arg_s[TILE];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int C = P - 5;
  const int n = clamp_count(counts[b], cap);
  if (n == 0) return;   // (uniform)
  const float* rows_b = rows + (size_t)b * cap * P;
  if (count_classes)
    for (int k = tid; k < C; k += COPY_THREADS) hist_s[k] = 0;
  const long long dst = MODE == 2 ? 0 : dst_row[b];
  const int reclen = MODE == 0 ? P + 3 : P;
  const float id = (float)(first_img_id + b);
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += TILE) {
    const int tn = n - r0 < TILE ? n - r0 : TILE;
    if ((MODE == 0 || count_classes) && tid < tn) {
      float best;
      const int arg = argmax_first(rows_b + (size_t)(r0 + tid) * P + 5, C, best);
      arg_s[tid] = arg;
      if (count_classes && best > 0.f) atomicAdd(&hist_s[arg], 1);
    }
    if (MODE == 0) __syncthreads();
    if (MODE != 2) {
      const float* src = rows_b + (size_t)r0 * P;
      for (int i = tid; i < tn * reclen; i += COPY_THREADS) {
        const int r = i / reclen;
        if ((unsigned long long)(dst + r0 + r) >= (unsigned long long)arena_cap) break;   // (rows ascend with i: the rest is past the arena too)
        float v;
        if (MODE == 1) {
          v = src[i];
        } else {
          const int j = i - r * reclen;
          const float* row = src + (size_t)r * P;
          if (j == 0) v = id;
          else if (j <= 4) v = __fmul_rn(row[j - 1], (j & 1) ? img_w : img_h);   // one fp32 multiply, as numpy's float32 * int
          else if (j == 5) v = row[4];
          else if (j == 6) v = (float)arg_s[r];
          else if (j == 7) v = row[5 + arg_s[r]];
          else v = row[j - 3];
        }
        arena[(size_t)(dst + r0) * reclen + i] = v;
      }
    }
    if (MODE == 0) __syncthreads();   // arg_s is rewritten by the next tile
  }
  if (count_classes) {
    __syncthreads();
    unsigned long long* cc = reinterpret_cast<unsigned long long*>(state + ST_CLASS_COUNTS);
    for (int k = tid; k < C; k += COPY_THREADS)
      if (hist_s[k]) atomicAdd(&cc[k], (unsigned long long)hist_s[k]);
  }
}

}  // namespace

extern "C" int yogo_pred_sink_state_layout(int C, long long* offsets) {
  YOGO_CHECK_ARG(offsets && C > 0, "pred_sink_state_layout: bad arguments");
  const long long o[6] = {ST_ROWS, ST_IMAGES, ST_DROPPED_ROWS, ST_DROPPED_IMAGES, ST_CLASS_COUNTS, ST_CLASS_COUNTS + (long long)C};
  for (int k = 0; k < 6; ++k) offsets[k] = o[k];
  return YOGO_OK;
}

extern "C" int yogo_pred_sink_workspace_bytes(int B, size_t* bytes) {
  YOGO_CHECK_ARG(bytes && B >= 0, "pred_sink_workspace_bytes: bad arguments");
  *bytes = (size_t)(B > 0 ? B : 1) * sizeof(long long);
  return YOGO_OK;
}

extern "C" int yogo_pred_sink_append(const float* rows, const int* counts, int B, int cap, int P, int mode, int count_classes,
                                     long long first_img_id, int img_h, int img_w, long long* state, float* arena, long long arena_cap,
                                     int* img_counts, long long img_cap, void* workspace, hipStream_t stream) {
  YOGO_CHECK_ARG(rows && counts && state, "pred_sink_append: null pointer");
  YOGO_CHECK_ARG(B >= 0 && cap > 0, "pred_sink_append: bad batch (B = %d, cap = %d)", B, cap);
  YOGO_CHECK_ARG(P >= 6, "pred_sink_append: P = %d, a row holds a box, objectness and at least one class score", P);
  YOGO_CHECK_ARG(P - 5 <= MAX_CLASSES, "pred_sink_append: %d classes, at most %d", P - 5, MAX_CLASSES);
  YOGO_CHECK_ARG((long long)cap * (P + 3) <= INT_MAX, "pred_sink_append: cap * (P + 3) = %lld does not fit an int", (long long)cap * (P + 3));
  YOGO_CHECK_ARG(count_classes == 0 || count_classes == 1, "pred_sink_append: count_classes must be 0 or 1");
  if (arena) {
    YOGO_CHECK_ARG(mode == 0 || mode == 1, "pred_sink_append: mode must be 0 (npy records) or 1 (rows)");
    YOGO_CHECK_ARG(mode != 0 || P - 5 <= 255, "pred_sink_append: %d classes, npy records hold the class in a uint8 (at most 255)", P - 5);
    YOGO_CHECK_ARG(mode != 0 || (img_h > 0 && img_w > 0), "pred_sink_append: bad image size %d x %d", img_h, img_w);
    YOGO_CHECK_ARG(img_counts && workspace, "pred_sink_append: null pointer (img_counts / workspace)");
    YOGO_CHECK_ARG(arena_cap >= 0 && img_cap >= 0, "pred_sink_append: negative capacity");
  } else {
    YOGO_CHECK_ARG(count_classes == 1, "pred_sink_append: no arena and no class counting: nothing to do");
  }
  if (B == 0) return YOGO_OK;
  if (arena) {
    long long* dst_row = static_cast<long long*>(workspace);
    hipLaunchKernelGGL(pred_sink_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, counts, B, cap, state, arena_cap, img_counts, img_cap,
                       dst_row);
    YOGO_CHECK_LAUNCH("pred_sink_scan");
    if (mode == 0)
      hipLaunchKernelGGL(pred_sink_copy_kernel<0>, dim3(B), dim3(COPY_THREADS), 0, stream, rows, counts, cap, P, count_classes, first_img_id,
                         (float)img_h, (float)img_w, state, arena, arena_cap, dst_row);
    else
      hipLaunchKernelGGL(pred_sink_copy_kernel<1>, dim3(B), dim3(COPY_THREADS), 0, stream, rows, counts, cap, P, count_classes, first_img_id,
                         0.f, 0.f, state, arena, arena_cap, dst_row);
  } else {
    hipLaunchKernelGGL(pred_sink_copy_kernel<2>, dim3(B), dim3(COPY_THREADS), 0, stream, rows, counts, cap, P, 1, 0ll, 0.f, 0.f, state,
                       static_cast<float*>(nullptr), 0ll, static_cast<const long long*>(nullptr));
  }
  YOGO_CHECK_LAUNCH("pred_sink_copy");
  if (yogo_launch_log_enabled())
    yogo_launch_log("pred_sink_copy_kernel<%d> | B=%d cap=%d P=%d count=%d", arena ? mode : 2, B, cap, P, count_classes);
  return YOGO_OK;
}

// match.hip -- the evaluation half after threshold + NMS, on the device:
//   match_kernel        prediction <-> label assignment of every image of a batch (yogo/utils/prediction_formatting.py:254-330:
//                       label compaction, cost = 1 - box_iou, scipy.optimize.linear_sum_assignment, the unmatched sets)
//   match_gather_kernel the batch-concatenated tensors PredictionLabelMatch.concat gives (prediction_formatting.py:183-204)
//   metrics_*_kernel    the class statistics Metrics.update adds per batch (yogo/metrics.py:113-158), into device accumulators
//
// The assignment is scipy's shortest-augmenting-path solver (rectangular_lsap) restated with its arithmetic order and its
// tie-breaking, in fp64: with mostly disjoint boxes most costs are exactly 1.0, and which zero-IoU pairs get matched decides the
// confusion matrix.  One workgroup per image.  The scan over the remaining columns and the arg-min are the parallel part; the
// outer loops are serial and every loop has a bound known on entry.  When the column count is small one wavefront works alone
// (cross-lane reductions, no workgroup barrier) and the other wavefronts of the workgroup leave; the whole workgroup works for
// the dense case.  The solver state lives in LDS when rows and columns fit, otherwise in the image's slice of the workspace.
//
// Compiled with -ffp-contract=off: (a1 + a2) - wh.x * wh.y must not contract into an FMA, or costs differ from the reference's in
// the last bit.  The fp32 division is the correctly rounded one (-fhip-fp32-correctly-rounded-divide-sqrt).
#include "common.h"
#include <cmath>
#include <cstring>

#define MATCH_THREADS 1024
#define MATCH_WAVES (MATCH_THREADS / 64)
#define MATCH_NARROW_COLS 1024              // up to this many columns one wavefront solves the image alone
#define MATCH_LDS_BYTES (160 * 1024 - 1024)  // dynamic LDS of the launch (the static part stays under 1 KB)
#define MATCH_META 8                         // ints per image: N, M, n_pairs, n_missed, n_extra, status, scores_in_unit, 0

struct MatchParams {
  const float* rows;    // [B][cap][P] xyxy rows of format_preds_batched
  const int* counts;    // [B]
  const float* labels;  // [B][6][cells]
  int* meta;            // [B][MATCH_META]
  int* pair_label;      // [B][cap]
  int* pair_pred;       // [B][cap]
  int* un_label;        // [B][cap]
  int* un_pred;         // [B][cap]
  float* lab_out;       // [B][cap][6]
  unsigned char* ws;    // [B][match_ws_per_image(cap)]
  size_t ws_per_image;
  int B, P, cells, cap;
};

// bytes of the solver state of an nr x nc problem (the layout of solve_image); one expression for the kernel's "fits the LDS" and
// the host's workspace size
__host__ __device__ inline size_t match_state_bytes(size_t nr, size_t nc, bool boxes) {
  return (boxes ? 16 * (nr + nc) : 0) + 8 * (nr + 2 * nc) + 4 * (2 * nr + 3 * nc);
}

template <bool WIDE>
__device__ __forceinline__ void bsync() {
  if constexpr (WIDE) {
    __syncthreads();
  } else {  // one wavefront: its LDS operations complete in order; wait for them and keep the compiler from moving code across
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// positions j < n with pred(j), in ascending j: emit(j, rank).  Returns the count.  Every working thread calls it.
template <bool WIDE, class Pred, class Emit>
__device__ __forceinline__ int ordered_compact(int n, int tid, int* s_wsum, Pred pred, Emit emit) {
  constexpr int T = WIDE ? MATCH_THREADS : 64;
  const int lane = tid & 63, w = tid >> 6;
  int out = 0;
  for (int base = 0; base < n; base += T) {
    const int j = base + tid;
    const bool f = j < n && pred(j);
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    int woff = 0, tot = __popcll(m);
    if constexpr (WIDE) {
      if (lane == 0) s_wsum[w] = tot;
      __syncthreads();
      tot = 0;
      for (int k = 0; k < MATCH_WAVES; ++k) {
        const int c = s_wsum[k];
        if (k < w) woff += c;
        tot += c;
      }
      __syncthreads();
    }
    if (f) emit(j, out + woff + pre);
    out += tot;
  }
  return out;
}

// torchvision.ops.box_iou's operations in fp32, operation for operation (prediction_formatting.py:217 in this package)
__device__ __forceinline__ float iou_f32(const float4 l, const float4 p) {
  const float a1 = (l.z - l.x) * (l.w - l.y);
  const float a2 = (p.z - p.x) * (p.w - p.y);
  const float w = fmaxf(fminf(l.z, p.z) - fmaxf(l.x, p.x), 0.0f);
  const float h = fmaxf(fminf(l.w, p.w) - fmaxf(l.y, p.y), 0.0f);
  const float inter = w * h;
  return inter / ((a1 + a2) - inter);
}

__device__ __forceinline__ float4 load_label_box(const float* lab_out_b, int i) {
  const float* q = lab_out_b + (size_t)i * 6;
  return make_float4(q[1], q[2], q[3], q[4]);
}
__device__ __forceinline__ float4 load_pred_box(const float* rows_b, int P, int j) {
  const float* q = rows_b + (size_t)j * P;
  return make_float4(q[0], q[1], q[2], q[3]);
}

// the solver of one image.  rows = the smaller side (nr <= nc); transposed: rows are predictions, columns labels.
// Returns the status; on 0, col4row / row4col hold the assignment.
template <bool WIDE, bool LDS>
__device__ __forceinline__ int solve_image(const float* rows_b, const float* lab_out_b, int P, int N, int M, unsigned char* state,
                                           int tid, double* red_s, unsigned* red_k, int* s_flag, int** col4row_out, int** row4col_out) {
  constexpr int T = WIDE ? MATCH_THREADS : 64;
  const bool transposed = N > M;
  const int nr = transposed ? M : N, nc = transposed ? N : M;
  // layout: [boxes of the rows, boxes of the columns (LDS only)] u[nr] v[nc] spc[nc] | col4row[nr] vis[nr] path[nc] row4col[nc] remaining[nc]
  float4* rb = reinterpret_cast<float4*>(state);
  float4* cb = rb + nr;
  double* u = reinterpret_cast<double*>(state + (LDS ? (size_t)16 * (nr + nc) : 0));
  double* v = u + nr;
  double* spc = v + nc;
  int* col4row = reinterpret_cast<int*>(spc + nc);
  int* vis = col4row + nr;
  int* path = vis + nr;
  int* row4col = path + nc;
  int* remaining = row4col + nc;
  *col4row_out = col4row;
  *row4col_out = row4col;

  auto row_box = [&](int i) -> float4 {
    if constexpr (LDS) return rb[i];
    return transposed ? load_pred_box(rows_b, P, i) : load_label_box(lab_out_b, i);
  };
  auto col_box = [&](int j) -> float4 {
    if constexpr (LDS) return cb[j];
    return transposed ? load_label_box(lab_out_b, j) : load_pred_box(rows_b, P, j);
  };
  auto cost = [&](const float4 r, const float4 c) -> float { return 1.0f - (transposed ? iou_f32(c, r) : iou_f32(r, c)); };

  for (int i = tid; i < nr; i += T) {
    if constexpr (LDS) rb[i] = transposed ? load_pred_box(rows_b, P, i) : load_label_box(lab_out_b, i);
    u[i] = 0.0;
    col4row[i] = -1;
  }
  for (int j = tid; j < nc; j += T) {
    if constexpr (LDS) cb[j] = transposed ? load_label_box(lab_out_b, j) : load_pred_box(rows_b, P, j);
    v[j] = 0.0;
    row4col[j] = -1;
  }
  bsync<WIDE>();

  // scipy rejects a matrix with a NaN or -inf entry before it solves ("matrix contains invalid numeric entries")
  {
    bool bad = false;
    for (int i = 0; i < nr; ++i) {
      const float4 rbox = row_box(i);
#pragma unroll 1
      for (int j = tid; j < nc; j += T) {
        const float c = cost(rbox, col_box(j));
        bad |= (c != c) || (c == -INFINITY);
      }
    }
    if (bad) *s_flag = 1;
    bsync<WIDE>();
    if (*s_flag) return 1;
  }

  int status = 0;
  for (int cur = 0; cur < nr && status == 0; ++cur) {
    for (int it = tid; it < nc; it += T) {
      remaining[it] = nc - 1 - it;
      spc[it] = INFINITY;
    }
    bsync<WIDE>();
    double minVal = 0.0;
    int i = cur, num = nc, nvis = 0, sink = -1;
    for (int step = 0; step < nc; ++step) {  // num strictly decreases: at most nc steps
      const double ui = u[i];
      const float4 rbox = row_box(i);
      double bs = INFINITY;
      unsigned bk = 0u;
      for (int it = tid; it < num; it += T) {
        const int j = remaining[it];
        const double r = ((minVal + (double)cost(rbox, col_box(j))) - ui) - v[j];
        double sj = spc[j];
        if (r < sj) {
          path[j] = i;
          spc[j] = r;
          sj = r;
        }
        // among equal minima: the LAST position whose column is unassigned if there is one, otherwise the FIRST position
        const unsigned k = row4col[j] < 0 ? (0x80000000u | (unsigned)it) : (0x7fffffffu - (unsigned)it);
        if (sj < bs || (sj == bs && k > bk)) {
          bs = sj;
          bk = k;
        }
      }
      for (int off = 32; off; off >>= 1) {
        const double s2 = __shfl_xor(bs, off);
        const unsigned k2 = __shfl_xor(bk, off);
        if (s2 < bs || (s2 == bs && k2 > bk)) {
          bs = s2;
          bk = k2;
        }
      }
      if constexpr (WIDE) {
        if ((tid & 63) == 0) {
          red_s[tid >> 6] = bs;
          red_k[tid >> 6] = bk;
        }
        __syncthreads();
        bs = red_s[0];
        bk = red_k[0];
        for (int w = 1; w < MATCH_WAVES; ++w) {
          const double s2 = red_s[w];
          const unsigned k2 = red_k[w];
          if (s2 < bs || (s2 == bs && k2 > bk)) {
            bs = s2;
            bk = k2;
          }
        }
      } else {
        bsync<WIDE>();
      }
      if (bk == 0u || bs == INFINITY) {  // (bk == 0: no candidate at all -- cannot happen while num > 0)
        status = 2;                      // scipy: "cost matrix is infeasible"
        break;
      }
      const int index = (bk & 0x80000000u) ? (int)(bk & 0x7fffffffu) : (int)(0x7fffffffu - bk);
      const int j = remaining[index];
      minVal = spc[j];
      const int r4 = row4col[j];
      const int last = remaining[num - 1];
      bsync<WIDE>();  // everybody has read remaining[] / the reduction slots
      if (tid == 0) {
        remaining[index] = last;
        vis[nvis] = j;
      }
      ++nvis;
      --num;
      if (r4 < 0) {
        sink = j;
        break;
      }
      i = r4;
      bsync<WIDE>();
    }
    if (status == 0 && sink < 0) status = 2;
    if (status) break;
    bsync<WIDE>();
    // dual variables: the visited rows are cur and the rows the visited columns were assigned to
    if (tid == 0) u[cur] += minVal;
    for (int k = tid; k < nvis; k += T) {
      const int j = vis[k];
      const double d = minVal - spc[j];
      v[j] -= d;
      if (j != sink) u[row4col[j]] += d;
    }
    bsync<WIDE>();
    if (tid == 0) {  // augment along the path back from the sink (at most cur + 1 swaps)
      int j = sink;
      for (int k = 0; k <= cur; ++k) {
        const int i2 = path[j];
        row4col[j] = i2;
        const int t = col4row[i2];
        col4row[i2] = j;
        j = t;
        if (i2 == cur) break;
      }
    }
    bsync<WIDE>();
  }
  return status;
}

// everything after the label compaction, by the threads that stay (all of them, or the first wavefront)
template <bool WIDE, bool LDS>
__device__ __forceinline__ void match_image(const MatchParams& p, int b, int N, int M, unsigned char* state, int tid, int* s_wsum,
                                            double* red_s, unsigned* red_k, int* s_flag) {
  constexpr int T = WIDE ? MATCH_THREADS : 64;
  const float* rows_b = p.rows + (size_t)b * p.cap * p.P;
  const float* lab_out_b = p.lab_out + (size_t)b * p.cap * 6;
  int* pl = p.pair_label + (size_t)b * p.cap;
  int* pp = p.pair_pred + (size_t)b * p.cap;
  int* ul = p.un_label + (size_t)b * p.cap;
  int* up = p.un_pred + (size_t)b * p.cap;
  int* meta = p.meta + (size_t)b * MATCH_META;
  int status = 0, n_pairs = 0, n_missed = N, n_extra = M;
  if (N > 0 && M > 0) {
    int *col4row, *row4col;
    status = solve_image<WIDE, LDS>(rows_b, lab_out_b, p.P, N, M, state, tid, red_s, red_k, s_flag, &col4row, &row4col);
    if (status == 0) {
      if (N <= M) {  // every label is matched; pairs in label order
        for (int i = tid; i < N; i += T) {
          pl[i] = i;
          pp[i] = col4row[i];
        }
        n_pairs = N;
        n_missed = 0;
        n_extra = ordered_compact<WIDE>(M, tid, s_wsum, [&](int j) { return row4col[j] < 0; }, [&](int j, int r) { up[r] = j; });
      } else {  // columns are labels: pairs in ascending label index (scipy sorts the transposed answer)
        n_pairs = ordered_compact<WIDE>(N, tid, s_wsum, [&](int j) { return row4col[j] >= 0; },
                                        [&](int j, int r) { pl[r] = j; pp[r] = row4col[j]; });
        n_missed = ordered_compact<WIDE>(N, tid, s_wsum, [&](int j) { return row4col[j] < 0; }, [&](int j, int r) { ul[r] = j; });
        n_extra = 0;
      }
    } else {
      n_missed = 0;
      n_extra = 0;
    }
  } else {
    for (int i = tid; i < N; i += T) ul[i] = i;
    for (int j = tid; j < M; j += T) up[j] = j;
  }
  bsync<WIDE>();  // the pair lists written above are read below
  // torchmetrics' normalisation switch is a property of every class score handed to one update: this image's share of it
  bool unit = true;
  const int C = p.P - 5;
  for (int e = tid; e < n_pairs * C; e += T) {
    const float s = rows_b[(size_t)pp[e / C] * p.P + 5 + e % C];
    unit &= (s >= 0.0f) && (s <= 1.0f);
  }
  if (!unit) s_flag[1] = 0;
  bsync<WIDE>();
  if (tid == 0) {
    meta[0] = N;
    meta[1] = M;
    meta[2] = n_pairs;
    meta[3] = n_missed;
    meta[4] = n_extra;
    meta[5] = status;
    meta[6] = s_flag[1];
    meta[7] = 0;
  }
}

__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(MatchParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int s_wsum[MATCH_WAVES];
  __shared__ double red_s[MATCH_WAVES];
  __shared__ unsigned red_k[MATCH_WAVES];
  __shared__ int s_flag[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    s_flag[0] = 0;  // an invalid cost was seen
    s_flag[1] = 1;  // every class score of the matched rows lies in [0, 1]
  }
  // label compaction: the cells with label[0] != 0 in ascending flat index (label.view(6, Sy*Sx).T[mask])
  const float* lab = p.labels + (size_t)b * 6 * p.cells;
  float* lab_out_b = p.lab_out + (size_t)b * p.cap * 6;
  const int cap = p.cap;
  const int N = ordered_compact<true>(
      p.cells, tid, s_wsum, [&](int c) { return lab[c] != 0.0f; },
      [&](int c, int r) {
        if (r < cap)
          for (int k = 0; k < 6; ++k) lab_out_b[(size_t)r * 6 + k] = lab[(size_t)k * p.cells + c];
      });
  int M = p.counts[b];
  M = M < 0 ? 0 : (M > cap ? cap : M);
  __syncthreads();  // the compacted label rows are read back by other threads
  const size_t nr = N < M ? N : M, nc = N < M ? M : N;
  const bool fits = match_state_bytes(nr, nc, true) <= (size_t)MATCH_LDS_BYTES;
  if (nc <= MATCH_NARROW_COLS) {  // (always fits: 76 B per column at most)
    if (tid >= 64) return;        // no workgroup barrier is executed after this point
    match_image<false, true>(p, b, N, M, smem, tid, s_wsum, red_s, red_k, s_flag);
  } else if (fits) {
    match_image<true, true>(p, b, N, M, smem, tid, s_wsum, red_s, red_k, s_flag);
  } else {
    match_image<true, false>(p, b, N, M, p.ws + (size_t)b * p.ws_per_image, tid, s_wsum, red_s, red_k, s_flag);
  }
}

// ---- gather: the tensors PredictionLabelMatch.concat over the images gives ---------------------------------------------------------
struct GatherParams {
  const float *rows, *lab_out;
  const int *meta, *pair_label, *pair_pred, *un_label, *un_pred;
  float *preds, *labels, *missed, *extra;
  long long K, Km, Ke;
  int B, P, cap;
};

__global__ __launch_bounds__(256) void match_gather_kernel(GatherParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  long long o_pair = 0, o_miss = 0, o_extra = 0;
  for (int k = 0; k < b; ++k) {  // (B is a batch size: a few hundred small loads at most)
    o_pair += p.meta[k * MATCH_META + 2];
    o_miss += p.meta[k * MATCH_META + 3];
    o_extra += p.meta[k * MATCH_META + 4];
  }
  const int* m = p.meta + (size_t)b * MATCH_META;
  const int n_pairs = m[2], n_miss = m[3], n_extra = m[4], P = p.P;
  const float* rows_b = p.rows + (size_t)b * p.cap * P;
  const float* lab_b = p.lab_out + (size_t)b * p.cap * 6;
  const int* pl = p.pair_label + (size_t)b * p.cap;
  const int* pp = p.pair_pred + (size_t)b * p.cap;
  const int* ul = p.un_label + (size_t)b * p.cap;
  const int* up = p.un_pred + (size_t)b * p.cap;
  for (int e = tid; e < n_pairs * P; e += blockDim.x) {
    const int r = e / P, c = e - r * P;
    if (o_pair + r < p.K) p.preds[(o_pair + r) * P + c] = rows_b[(size_t)pp[r] * P + c];
  }
  for (int e = tid; e < n_pairs * 6; e += blockDim.x) {
    const int r = e / 6, c = e - r * 6;
    if (o_pair + r < p.K) p.labels[(o_pair + r) * 6 + c] = lab_b[(size_t)pl[r] * 6 + c];
  }
  for (int e = tid; e < n_miss * 6; e += blockDim.x) {
    const int r = e / 6, c = e - r * 6;
    if (o_miss + r < p.Km) p.missed[(o_miss + r) * 6 + c] = lab_b[(size_t)ul[r] * 6 + c];
  }
  for (int e = tid; e < n_extra * P; e += blockDim.x) {
    const int r = e / P, c = e - r * P;
    if (o_extra + r < p.Ke) p.extra[(o_extra + r) * P + c] = rows_b[(size_t)up[r] * P + c];
  }
}

// ---- class statistics of a batch (Metrics.update / _ClassStats.update) --------------------------------------------------------------
#define ACC_THREADS 128
#define ACC_LDS_MAX (160 * 1024 - 256)  // dynamic LDS the accumulate kernel may ask for (its static part is one word)
#define MAP_ROW 11  // detection box, score, detection class, ground-truth box, ground-truth class

struct AccParams {
  const float *rows, *lab_out;
  const int *meta, *pair_label, *pair_pred, *un_label, *un_pred;
  const double* roc_thr;    // [T]   the doubles of torch.linspace(0, 1, T, dtype=float64)
  const double* cal_edges;  // [nbins + 1]
  unsigned long long* acc;  // the integer state, layout below
  double* bin_conf;         // [nbins]
  double* partial;          // [B][nbins] per-image sums of this batch
  float* map_rows;          // [map_cap][MAP_ROW] or null
  long long map_cap;
  int B, P, cap, T, nbins;
};
// integer state: confmat[C*C] pos[C] n missed[C] extra[C] total bin_count[nbins] bin_acc[nbins] hist[(T+1)*C*2] map_count status1 status2
__host__ __device__ inline long long acc_off_pos(int C) { return (long long)C * C; }
__host__ __device__ inline long long acc_off_n(int C) { return acc_off_pos(C) + C; }
__host__ __device__ inline long long acc_off_missed(int C) { return acc_off_n(C) + 1; }
__host__ __device__ inline long long acc_off_extra(int C) { return acc_off_missed(C) + C; }
__host__ __device__ inline long long acc_off_total(int C) { return acc_off_extra(C) + C; }
__host__ __device__ inline long long acc_off_bin_count(int C) { return acc_off_total(C) + 1; }
__host__ __device__ inline long long acc_off_bin_acc(int C, int nb) { return acc_off_bin_count(C) + nb; }
__host__ __device__ inline long long acc_off_hist(int C, int nb) { return acc_off_bin_acc(C, nb) + nb; }
__host__ __device__ inline long long acc_off_map_count(int C, int nb, int T) { return acc_off_hist(C, nb) + (long long)(T + 1) * C * 2; }
__host__ __device__ inline long long acc_off_status(int C, int nb, int T) { return acc_off_map_count(C, nb, T) + 1; }
__host__ __device__ inline long long acc_words(int C, int nb, int T) { return acc_off_status(C, nb, T) + 2; }

// #{table[k] <= x}: `>= threshold` counts for the ROC, bucketize(right=True) for the calibration bins
__device__ __forceinline__ int count_le(const double* table, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// torch's argmax / max on the CPU: the first maximum, a NaN counts as larger than everything
__device__ __forceinline__ bool torch_gt(double a, double b) { return a > b || (a != a && b == b); }

__global__ __launch_bounds__(ACC_THREADS) void metrics_accumulate_kernel(AccParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int s_unit;
  const int b = blockIdx.x, tid = threadIdx.x, P = p.P, C = P - 5, T = p.T, nb = p.nbins;
  double* binconf_s = reinterpret_cast<double*>(smem);                 // [nb][ACC_THREADS]
  int* hist_s = reinterpret_cast<int*>(binconf_s + nb * ACC_THREADS);  // [(T+1)][C][2]
  int* small_s = hist_s + (T + 1) * C * 2;                             // confmat[C*C] pos[C] missed[C] extra[C] bin_count[nb] bin_acc[nb]
  const int n_hist = (T + 1) * C * 2, n_small = C * C + 3 * C + 2 * nb;
  for (int k = tid; k < nb * ACC_THREADS; k += ACC_THREADS) binconf_s[k] = 0.0;
  for (int k = tid; k < n_hist + n_small; k += ACC_THREADS) hist_s[k] = 0;
  if (tid == 0) s_unit = 1;
  __syncthreads();
  {
    bool unit = true;
    for (int k = tid; k < p.B; k += ACC_THREADS) unit &= p.meta[k * MATCH_META + 6] != 0;
    if (!unit) s_unit = 0;
  }
  long long o_pair = 0;
  for (int k = 0; k < b; ++k) o_pair += p.meta[k * MATCH_META + 2];
  __syncthreads();
  const bool softmax = s_unit == 0;
  int* confmat_s = small_s;
  int* pos_s = confmat_s + C * C;
  int* missed_s = pos_s + C;
  int* extra_s = missed_s + C;
  int* binc_s = extra_s + C;
  int* bina_s = binc_s + nb;
  const int* m = p.meta + (size_t)b * MATCH_META;
  const int n_pairs = m[2], n_miss = m[3], n_extra = m[4], status = m[5];
  const float* rows_b = p.rows + (size_t)b * p.cap * P;
  const float* lab_b = p.lab_out + (size_t)b * p.cap * 6;
  const int* pl = p.pair_label + (size_t)b * p.cap;
  const int* pp = p.pair_pred + (size_t)b * p.cap;
  const int* ul = p.un_label + (size_t)b * p.cap;
  const int* up = p.un_pred + (size_t)b * p.cap;
  const long long map_base = p.map_rows ? (long long)p.acc[acc_off_map_count(C, nb, T)] + o_pair : 0;

  for (int r = tid; r < n_pairs; r += ACC_THREADS) {
    const float* row = rows_b + (size_t)pp[r] * P;
    const float* lab = lab_b + (size_t)pl[r] * 6;
    const long long target = (long long)lab[5];
    const bool valid = target >= 0 && target < C;
    // raw scores: first argmax, maximum
    int arg_raw = 0;
    double mx = (double)row[5];
    for (int c = 1; c < C; ++c) {
      const double s = (double)row[5 + c];
      if (torch_gt(s, mx)) { mx = s; arg_raw = c; }
    }
    if (valid) atomicAdd(&confmat_s[(int)target * C + arg_raw], 1);
    if (valid) atomicAdd(&pos_s[(int)target], 1);
    double denom = 1.0;
    if (softmax) {
      denom = 0.0;
      for (int c = 0; c < C; ++c) denom += exp((double)row[5 + c] - mx);
    }
    int arg = 0;
    double conf = 0.0;
    for (int c = 0; c < C; ++c) {
      const double s = (double)row[5 + c];
      const double pr = softmax ? exp(s - mx) / denom : s;
      if (c == 0 || torch_gt(pr, conf)) { conf = pr; arg = c; }
      const int k = count_le(p.roc_thr, T, pr);
      atomicAdd(&hist_s[(k * C + c) * 2 + ((valid && c == (int)target) ? 1 : 0)], 1);
    }
    int bin = count_le(p.cal_edges, nb + 1, conf) - 1;
    bin = bin < 0 ? 0 : (bin > nb - 1 ? nb - 1 : bin);
    atomicAdd(&binc_s[bin], 1);
    if ((long long)arg == target) atomicAdd(&bina_s[bin], 1);
    binconf_s[bin * ACC_THREADS + tid] += conf;  // this thread's own slot: summed below in a fixed order
    if (p.map_rows && map_base + r < p.map_cap) {
      float* o = p.map_rows + (map_base + r) * MAP_ROW;
      o[0] = row[0]; o[1] = row[1]; o[2] = row[2]; o[3] = row[3]; o[4] = row[4];
      o[5] = (float)arg_raw;
      o[6] = lab[1]; o[7] = lab[2]; o[8] = lab[3]; o[9] = lab[4];
      o[10] = (float)target;
    }
  }
  for (int r = tid; r < n_miss; r += ACC_THREADS) {
    const long long cls = (long long)lab_b[(size_t)ul[r] * 6 + 5];
    if (cls >= 0 && cls < C) atomicAdd(&missed_s[(int)cls], 1);
  }
  for (int r = tid; r < n_extra; r += ACC_THREADS) {
    const float* row = rows_b + (size_t)up[r] * P;
    int arg = 0;
    double mx = (double)row[5];
    for (int c = 1; c < C; ++c) {
      const double s = (double)row[5 + c];
      if (torch_gt(s, mx)) { mx = s; arg = c; }
    }
    atomicAdd(&extra_s[arg], 1);
  }
  __syncthreads();
  // integers: the order of additions does not matter
  unsigned long long* acc = p.acc;
  for (int k = tid; k < C * C; k += ACC_THREADS) if (confmat_s[k]) atomicAdd(&acc[k], (unsigned long long)confmat_s[k]);
  for (int k = tid; k < C; k += ACC_THREADS) {
    if (pos_s[k]) atomicAdd(&acc[acc_off_pos(C) + k], (unsigned long long)pos_s[k]);
    if (missed_s[k]) atomicAdd(&acc[acc_off_missed(C) + k], (unsigned long long)missed_s[k]);
    if (extra_s[k]) atomicAdd(&acc[acc_off_extra(C) + k], (unsigned long long)extra_s[k]);
  }
  for (int k = tid; k < nb; k += ACC_THREADS) {
    if (binc_s[k]) atomicAdd(&acc[acc_off_bin_count(C) + k], (unsigned long long)binc_s[k]);
    if (bina_s[k]) atomicAdd(&acc[acc_off_bin_acc(C, nb) + k], (unsigned long long)bina_s[k]);
  }
  for (int k = tid; k < n_hist; k += ACC_THREADS) if (hist_s[k]) atomicAdd(&acc[acc_off_hist(C, nb) + k], (unsigned long long)hist_s[k]);
  if (tid == 0) {
    if (n_pairs) {
      atomicAdd(&acc[acc_off_n(C)], (unsigned long long)n_pairs);
      atomicAdd(&acc[acc_off_total(C)], (unsigned long long)n_pairs);
    }
    if (status == 1 || status == 2) atomicAdd(&acc[acc_off_status(C, nb, T) + status - 1], 1ull);
  }
  // the fp64 confidence sums of this image, thread slots in ascending order
  for (int k = tid; k < nb; k += ACC_THREADS) {
    double s = 0.0;
    for (int t = 0; t < ACC_THREADS; ++t) s += binconf_s[k * ACC_THREADS + t];
    p.partial[(size_t)b * nb + k] = s;
  }
}

// one ordered pass over the per-image partial rows (the way bn_bwd_reduce takes its fixed-order partials), and the mAP row count
__global__ __launch_bounds__(64) void metrics_finalize_kernel(AccParams p) {
  const int C = p.P - 5;
  for (int k = threadIdx.x; k < p.nbins; k += 64) {
    double s = p.bin_conf[k];
    for (int b0 = 0; b0 < p.B; b0 += 16) {  // sixteen loads in flight, added in image order
      double t[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) t[i] = b0 + i < p.B ? p.partial[(size_t)(b0 + i) * p.nbins + k] : 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (b0 + i < p.B) s += t[i];
    }
    p.bin_conf[k] = s;
  }
  if (threadIdx.x == 0 && p.map_rows) {
    long long tot = 0;
    for (int b = 0; b < p.B; ++b) tot += p.meta[b * MATCH_META + 2];
    p.acc[acc_off_map_count(C, p.nbins, p.T)] += (unsigned long long)tot;
  }
}

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" int yogo_match_workspace_bytes(int B, int Sy, int Sx, int cap, size_t* bytes) {
  YOGO_CHECK_ARG(bytes && B > 0 && Sy > 0 && Sx > 0 && cap > 0, "match_workspace_bytes: bad arguments");
  const size_t side = (size_t)cap > (size_t)Sy * Sx ? (size_t)cap : (size_t)Sy * Sx;
  const size_t per = (match_state_bytes(side, side, false) + 15) & ~(size_t)15;
  *bytes = (size_t)B * per + 16;
  return YOGO_OK;
}

extern "C" int yogo_match_preds_labels_batched(const float* rows, const int* counts, const float* labels, int* meta, int* pair_label,
                                               int* pair_pred, int* un_label, int* un_pred, float* lab_out, void* workspace, int B,
                                               int P, int Sy, int Sx, int cap, hipStream_t stream) {
  YOGO_CHECK_ARG(rows && counts && labels && meta && pair_label && pair_pred && un_label && un_pred && lab_out && workspace,
                 "match_preds_labels_batched: null pointer");
  YOGO_CHECK_ARG(B > 0 && P > 5 && Sy > 0 && Sx > 0, "match_preds_labels_batched: bad shape");
  const long long cells = (long long)Sy * Sx;
  YOGO_CHECK_ARG(cap >= cells && cells < (1ll << 30), "match_preds_labels_batched: cap = %d must hold the %lld grid cells", cap, cells);
  MatchParams p{};
  p.rows = rows; p.counts = counts; p.labels = labels; p.meta = meta; p.pair_label = pair_label; p.pair_pred = pair_pred;
  p.un_label = un_label; p.un_pred = un_pred; p.lab_out = lab_out;
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  p.ws = ws + ((16 - (reinterpret_cast<uintptr_t>(ws) & 15)) & 15);
  p.ws_per_image = (match_state_bytes((size_t)cap, (size_t)cap, false) + 15) & ~(size_t)15;
  p.B = B; p.P = P; p.cells = (int)cells; p.cap = cap;
  if (int e = yogo_func_dynamic_lds(reinterpret_cast<const void*>(&match_kernel), MATCH_LDS_BYTES, "match_preds_labels_batched")) return e;
  yogo_launch_log("match_kernel | B=%d cells=%d P=%d lds=%d", B, (int)cells, P, MATCH_LDS_BYTES);
  hipLaunchKernelGGL(match_kernel, dim3(B), dim3(MATCH_THREADS), MATCH_LDS_BYTES, stream, p);
  YOGO_CHECK_LAUNCH("match_preds_labels_batched");
  return YOGO_OK;
}

extern "C" int yogo_match_gather(const float* rows, const float* lab_out, const int* meta, const int* pair_label, const int* pair_pred,
                                 const int* un_label, const int* un_pred, float* preds, float* labels, float* missed, float* extra,
                                 int B, int P, int cap, long long K, long long Km, long long Ke, hipStream_t stream) {
  YOGO_CHECK_ARG(rows && lab_out && meta && pair_label && pair_pred && un_label && un_pred, "match_gather: null pointer");
  YOGO_CHECK_ARG((K == 0 || (preds && labels)) && (Km == 0 || missed) && (Ke == 0 || extra), "match_gather: null output");
  YOGO_CHECK_ARG(B > 0 && P > 5 && cap > 0 && K >= 0 && Km >= 0 && Ke >= 0, "match_gather: bad shape");
  GatherParams p{};
  p.rows = rows; p.lab_out = lab_out; p.meta = meta; p.pair_label = pair_label; p.pair_pred = pair_pred; p.un_label = un_label;
  p.un_pred = un_pred; p.preds = preds; p.labels = labels; p.missed = missed; p.extra = extra;
  p.K = K; p.Km = Km; p.Ke = Ke; p.B = B; p.P = P; p.cap = cap;
  yogo_launch_log("match_gather_kernel | B=%d P=%d K=%lld Km=%lld Ke=%lld", B, P, K, Km, Ke);
  hipLaunchKernelGGL(match_gather_kernel, dim3(B), dim3(256), 0, stream, p);
  YOGO_CHECK_LAUNCH("match_gather");
  return YOGO_OK;
}

// the one place the layout of the integer state is decided: the Python side reads the offsets from here
extern "C" int yogo_metrics_state_layout(int C, int T, int nbins, long long* offsets) {
  YOGO_CHECK_ARG(offsets && C > 0 && T > 0 && nbins > 0, "metrics_state_layout: bad arguments");
  const long long o[12] = {0, acc_off_pos(C), acc_off_n(C), acc_off_missed(C), acc_off_extra(C), acc_off_total(C), acc_off_bin_count(C),
                           acc_off_bin_acc(C, nbins), acc_off_hist(C, nbins), acc_off_map_count(C, nbins, T), acc_off_status(C, nbins, T),
                           acc_words(C, nbins, T)};
  memcpy(offsets, o, sizeof(o));
  return YOGO_OK;
}

extern "C" int yogo_metrics_accumulate(const float* rows, const float* lab_out, const int* meta, const int* pair_label,
                                       const int* pair_pred, const int* un_label, const int* un_pred, const double* roc_thresholds,
                                       int T, const double* cal_edges, int nbins, long long* acc, double* bin_conf, double* partial,
                                       float* map_rows, long long map_cap, int B, int P, int cap, hipStream_t stream) {
  YOGO_CHECK_ARG(rows && lab_out && meta && pair_label && pair_pred && un_label && un_pred && roc_thresholds && cal_edges && acc &&
                     bin_conf && partial, "metrics_accumulate: null pointer");
  YOGO_CHECK_ARG(B > 0 && P > 5 && cap > 0 && T > 0 && nbins > 0 && map_cap >= 0, "metrics_accumulate: bad shape");
  const int C = P - 5;
  const size_t lds = (size_t)nbins * ACC_THREADS * sizeof(double) +
                     ((size_t)(T + 1) * C * 2 + (size_t)C * C + 3 * (size_t)C + 2 * (size_t)nbins) * sizeof(int);
  YOGO_CHECK_ARG(lds <= (size_t)ACC_LDS_MAX,
                 "metrics_accumulate: %d classes x %d thresholds x %d bins need %zu bytes of LDS, %d are available (at 500 thresholds and 30 bins: "
                 "up to 31 classes)", C, T, nbins, lds, ACC_LDS_MAX);
  if (int e = yogo_func_dynamic_lds(reinterpret_cast<const void*>(&metrics_accumulate_kernel), ACC_LDS_MAX, "metrics_accumulate")) return e;
  AccParams p{};
  p.rows = rows; p.lab_out = lab_out; p.meta = meta; p.pair_label = pair_label; p.pair_pred = pair_pred; p.un_label = un_label;
  p.un_pred = un_pred; p.roc_thr = roc_thresholds; p.cal_edges = cal_edges; p.acc = reinterpret_cast<unsigned long long*>(acc);
  p.bin_conf = bin_conf; p.partial = partial; p.map_rows = map_rows; p.map_cap = map_cap;
  p.B = B; p.P = P; p.cap = cap; p.T = T; p.nbins = nbins;
  yogo_launch_log("metrics_accumulate_kernel | B=%d C=%d T=%d bins=%d mAP=%d", B, C, T, nbins, map_rows ? 1 : 0);
  hipLaunchKernelGGL(metrics_accumulate_kernel, dim3(B), dim3(ACC_THREADS), lds, stream, p);
  YOGO_CHECK_LAUNCH("metrics_accumulate");
  yogo_launch_log("metrics_finalize_kernel | B=%d bins=%d", B, nbins);
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(64), 0, stream, p);
  YOGO_CHECK_LAUNCH("metrics_accumulate (finalize)");
  return YOGO_OK;
}

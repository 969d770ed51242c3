// The text of the prediction files of `yogo infer --save-preds --device-outputs`, written on the device: what
// prediction_rows_to_text (yogo_amd/utils/prediction_formatting.py; the f-string of yogo/infer.py:52-55) makes of the rows of one image,
//
//     "<class> <cx> <cy> <w> <h>" per row, joined by "\n", no trailing newline, an image without rows an empty file,
//
// for every image of a drained "rows" sink (yogo_amd/pred_sink.py) at once: records [N][P] in image order and img_counts [images] in,
// one dense byte buffer with the images' texts back to back and img_offsets [images + 1] out, byte for byte what the host code gives.
// The numbers are printed by float_text.h (shortest round-trip decimals: integer arithmetic, the same definition the host test
// compiles); <class> mirrors max(range(C), key=scores.__getitem__): the first maximum under ">", so a NaN never displaces the current
// best and a leading NaN keeps index 0 -- NOT the argmax of pred_sink_copy_kernel, whose NaN rule is that of the class counts.
//
// A line is formatted twice, once into a counter and once into its place, so that no fixed-stride copy of the text exists; the
// separator belongs to the line it precedes (every record but the first of its image starts with "\n"), which makes an image's
// offset the position of its first record's line.  Five launches, stream-ordered, none read by the host:
//   pred_text_image_scan_kernel   ONE workgroup: img_start [images + 1] = exclusive prefix of img_counts (as pred_sink_scan_kernel: a chunk
//                                 per lane, the chunk sums scanned in LDS).  A negative count or a sum other than N sets total = -1
//                                 and every later kernel returns at once: the counts are not trusted with an address.
//   pred_text_length_kernel       a lane per record: finds its image (binary search in img_start), measures its line, stores the length
//                                 (<= 111, bit 7 = first record of its image) in one byte and the workgroup's sum in block_sum
//   pred_text_block_scan_kernel   ONE workgroup: block_sum -> exclusive prefix in place, total = the byte count
//   pred_text_write_kernel        a lane per record: its place = the workgroup's base + the prefix of the lengths within the workgroup
//                                 (LDS scan); formats the line there, every store checked against text_cap
//   pred_text_offsets_kernel      a lane per image (and one for the end): the place of its first record's line
// The work is divergent integer arithmetic on ~50 bytes per record; scratch is one byte per record plus 8 per 256 records and image.
#include "common.h"
#include "float_text.h"
#include <climits>

namespace {

constexpr int THREADS = 256;   // records per workgroup of the length / write kernels
constexpr int FIRST_BIT = 0x80;

struct BoundedOut {   // stores at text[pos] while pos < cap, counts on regardless
  char* text;
  long long pos, cap;
  __device__ void put(char c) {
    if ((unsigned long long)pos < (unsigned long long)cap) text[pos] = c;
    ++pos;
  }
};

// max(range(C), key=s.__getitem__)
__device__ __forceinline__ int first_max_python(const float* __restrict__ s, int C) {
  int idx = 0;
  for (int k = 1; k < C; ++k)
    if (s[k] > s[idx]) idx = k;
  return idx;
}

template <class Out>
__device__ void put_line(const float* __restrict__ rec, int P, bool first, Out& o) {
  if (!first) o.put('\n');
  float_text::put_u32((unsigned)first_max_python(rec + 5, P - 5), o);
  for (int f = 0; f < 4; ++f) {
    o.put(' ');
    float_text::format_f32_repr_to(rec[f], o);
  }
}

// inclusive scan of one int per lane over the workgroup (s: THREADS ints of LDS, free to reuse after the call's last barrier)
__device__ __forceinline__ int block_inclusive_scan(int v, int* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const int add = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

__global__ __launch_bounds__(THREADS) void pred_text_image_scan_kernel(const int* __restrict__ img_counts, long long images, long long n,
                                                                       long long* __restrict__ img_start, long long* __restrict__ total) {
  __shared__ long long sum_s[THREADS];
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  const long long per = (images + THREADS - 1) / THREADS;
  const long long b0 = (long long)tid * per;
  long long own = 0;
  bool bad = false;
  for (long long k = 0; k < per; ++k) {
    const long long b = b0 + k;
    if (b < images) {
      const int c = img_counts[b];
      bad = bad || c < 0;
      own += c;
    }
  }
  if (bad) bad_s = 1;
  sum_s[tid] = own;
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const long long add = tid >= o ? sum_s[tid - o] : 0;
    __syncthreads();
    sum_s[tid] += add;
    __syncthreads();
  }
  const bool ok = !bad_s && sum_s[THREADS - 1] == n;
  if (tid == 0) {
    total[0] = ok ? 0 : -1;
    img_start[images] = n;
  }
  if (!ok) return;   // (uniform) img_start is not written: nothing reads it
  long long run = sum_s[tid] - own;
  for (long long k = 0; k < per; ++k) {
    const long long b = b0 + k;
    if (b < images) {
      img_start[b] = run;
      run += img_counts[b];
    }
  }
}

__global__ __launch_bounds__(THREADS) void pred_text_length_kernel(const float* __restrict__ records, long long n, int P,
                                                                   const long long* __restrict__ img_start, long long images,
                                                                   const long long* __restrict__ total, unsigned char* __restrict__ lens,
                                                                   long long* __restrict__ block_sum) {
  __shared__ int scan_s[THREADS];
  if (total[0] < 0) return;   // (uniform) the counts did not match
  const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
  int len = 0;
  if (r < n) {
    // the image of record r: the last i with img_start[i] <= r (img_start[0] = 0 <= r < n = img_start[images]); the empty images in
    // front of it share its start and come earlier
    long long lo = 0, hi = images;
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (img_start[mid] <= r) lo = mid; else hi = mid;
    }
    const bool first = img_start[lo] == r;
    float_text::CountOut o;
    put_line(records + (size_t)r * P, P, first, o);
    len = o.n;
    lens[r] = (unsigned char)(len | (first ? FIRST_BIT : 0));
  }
  const int incl = block_inclusive_scan(len, scan_s);
  if (threadIdx.x == THREADS - 1) block_sum[blockIdx.x] = incl;
}

__global__ __launch_bounds__(THREADS) void pred_text_block_scan_kernel(long long* __restrict__ block_sum, long long nblocks,
                                                                       long long* __restrict__ total) {
  __shared__ long long sum_s[THREADS];
  if (total[0] < 0) return;   // (uniform)
  const int tid = threadIdx.x;
  const long long per = (nblocks + THREADS - 1) / THREADS;
  const long long b0 = (long long)tid * per;
  long long own = 0;
  for (long long k = 0; k < per; ++k)
    if (b0 + k < nblocks) own += block_sum[b0 + k];
  sum_s[tid] = own;
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const long long add = tid >= o ? sum_s[tid - o] : 0;
    __syncthreads();
    sum_s[tid] += add;
    __syncthreads();
  }
  long long run = sum_s[tid] - own;
  for (long long k = 0; k < per; ++k)
    if (b0 + k < nblocks) {
      const long long v = block_sum[b0 + k];
      block_sum[b0 + k] = run;
      run += v;
    }
  if (tid == 0) total[0] = sum_s[THREADS - 1];
}

__global__ __launch_bounds__(THREADS) void pred_text_write_kernel(const float* __restrict__ records, long long n, int P,
                                                                  const unsigned char* __restrict__ lens,
                                                                  const long long* __restrict__ block_base,
                                                                  const long long* __restrict__ total, char* __restrict__ text,
                                                                  long long text_cap) {
  __shared__ int scan_s[THREADS];
  if (total[0] < 0) return;   // (uniform)
  const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
  const int packed = r < n ? lens[r] : 0;
  const int len = packed & (FIRST_BIT - 1);
  const int incl = block_inclusive_scan(len, scan_s);
  if (r >= n) return;
  BoundedOut o{text, block_base[blockIdx.x] + (incl - len), text_cap};
  put_line(records + (size_t)r * P, P, (packed & FIRST_BIT) != 0, o);
}

__global__ __launch_bounds__(THREADS) void pred_text_offsets_kernel(const long long* __restrict__ img_start, long long images, long long n,
                                                                    const unsigned char* __restrict__ lens,
                                                                    const long long* __restrict__ block_base,
                                                                    const long long* __restrict__ total, long long* __restrict__ img_offsets) {
  if (total[0] < 0) return;   // (uniform)
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i > images) return;
  const long long r = img_start[i];   // its first record, or that of the next image that has one
  long long off;
  if (r >= n) {
    off = total[0];
  } else {
    const long long blk = r / THREADS;
    off = block_base[blk];
    for (long long k = blk * THREADS; k < r; ++k) off += lens[k] & (FIRST_BIT - 1);
  }
  img_offsets[i] = off;
}

int class_digits(int P) {
  int d = 1;
  for (int v = P - 5 - 1; v >= 10; v /= 10) ++d;
  return d;
}

}  // namespace

extern "C" int yogo_pred_text_bound(long long n_records, long long images, int P, size_t* text_bytes, size_t* workspace_bytes) {
  YOGO_CHECK_ARG(text_bytes && workspace_bytes, "pred_text_bound: null pointer");
  YOGO_CHECK_ARG(n_records >= 0 && n_records <= INT_MAX && images >= 0 && images <= INT_MAX,
                 "pred_text_bound: bad sizes (%lld records, %lld images)", n_records, images);
  YOGO_CHECK_ARG(P >= 6, "pred_text_bound: P = %d, a row holds a box, objectness and at least one class score", P);
  // "\n", the class, four times " " and a number
  const size_t line = 1 + (size_t)class_digits(P) + 4 * (1 + (size_t)float_text::kMaxF32Chars);
  *text_bytes = (size_t)n_records * line;
  const size_t nblocks = ((size_t)n_records + THREADS - 1) / THREADS;
  *workspace_bytes = ((size_t)images + 1 + nblocks) * sizeof(long long) + (size_t)n_records;
  return YOGO_OK;
}

extern "C" int yogo_pred_text_format(const float* records, long long n, int P, const int* img_counts, long long images, char* text,
                                     long long text_cap, long long* img_offsets, long long* total, void* workspace, hipStream_t stream) {
  YOGO_CHECK_ARG(n >= 0 && n <= INT_MAX && images >= 0 && images <= INT_MAX, "pred_text_format: bad sizes (%lld records, %lld images)", n,
                 images);
  YOGO_CHECK_ARG(P >= 6, "pred_text_format: P = %d, a row holds a box, objectness and at least one class score", P);
  YOGO_CHECK_ARG(text_cap >= 0, "pred_text_format: negative text capacity");
  YOGO_CHECK_ARG(img_offsets && total, "pred_text_format: null pointer (img_offsets / total)");
  YOGO_CHECK_ARG(images > 0 || n == 0, "pred_text_format: %lld records of no image", n);
  YOGO_CHECK_ARG(n == 0 || (records && img_counts && workspace), "pred_text_format: null pointer (records / img_counts / workspace)");
  YOGO_CHECK_ARG(n == 0 || text || text_cap == 0, "pred_text_format: null text buffer of capacity %lld", text_cap);
  if (n == 0) {   // no text: every offset and the total are 0 (no launch; img_counts is not read)
    hipError_t e = hipMemsetAsync(img_offsets, 0, ((size_t)images + 1) * sizeof(long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(total, 0, sizeof(long long), stream);
    if (e != hipSuccess) {
      yogo_set_error("pred_text_format: hipMemsetAsync failed: %s", hipGetErrorString(e));
      return YOGO_ERR_HIP;
    }
    return YOGO_OK;
  }
  const long long nblocks = (n + THREADS - 1) / THREADS;
  long long* img_start = static_cast<long long*>(workspace);
  long long* block_sum = img_start + images + 1;
  unsigned char* lens = reinterpret_cast<unsigned char*>(block_sum + nblocks);
  hipLaunchKernelGGL(pred_text_image_scan_kernel, dim3(1), dim3(THREADS), 0, stream, img_counts, images, n, img_start, total);
  YOGO_CHECK_LAUNCH("pred_text_image_scan");
  hipLaunchKernelGGL(pred_text_length_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, stream, records, n, P, img_start, images, total, lens,
                     block_sum);
  YOGO_CHECK_LAUNCH("pred_text_length");
  hipLaunchKernelGGL(pred_text_block_scan_kernel, dim3(1), dim3(THREADS), 0, stream, block_sum, nblocks, total);
  YOGO_CHECK_LAUNCH("pred_text_block_scan");
  hipLaunchKernelGGL(pred_text_write_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, stream, records, n, P, lens, block_sum, total, text,
                     text_cap);
  YOGO_CHECK_LAUNCH("pred_text_write");
  hipLaunchKernelGGL(pred_text_offsets_kernel, dim3((unsigned)((images + 1 + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, img_start,
                     images, n, lens, block_sum, total, img_offsets);
  YOGO_CHECK_LAUNCH("pred_text_offsets");
  if (yogo_launch_log_enabled()) yogo_launch_log("pred_text_write_kernel | n=%lld images=%lld P=%d", n, images, P);
  return YOGO_OK;
}

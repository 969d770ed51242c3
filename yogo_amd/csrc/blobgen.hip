// Thumbnail ("blob") augmentation on the device: yogo/data/blobgen.py:208-263 (BlobDataset.__getitem__), which the reference
// runs per image in DataLoader workers.  A synthetic image is a flat background plus up to n thumbnails pasted at
// non-overlapping positions; here a batch of them is three launches:
//   blob_place_kernel        one wavefront per image: draws, background value, the placement search, label rows
//   blob_compose_kernel      (row band, image): background + flipped thumbnails -> the caller's batch rows, uint8 or fp32 / 255
//   blob_label_rows_kernel   placed rows -> one flat [N][5] list + offsets, for yogo_labels_rasterize (data_aug.hip)
//
// Randomness contract.  Every draw is a pure function of (seed, epoch, dataset index, slot, kind, try):
//   mix64(z)  = splitmix64's output function: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
//               z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31              (all arithmetic mod 2^64)
//   key       = mix64((u32)seed << 32 | (u32)epoch)
//   ctr       = index << 24 | slot << 16 | kind << 8 | try                  (index < 2^31, slot < 256, try < 100)
//   draw      = high 32 bits of mix64(key ^ ctr)
//   uniform m = (draw * m) >> 32                                             (an integer in [0, m))
// kinds: 0 thumbnail of the slot (over all thumbnails, try 0), 1 horizontal flip, 2 vertical flip (draw >> 31, try 0),
// 3 y of a try (m = H - h), 4 x of a try (m = W - w).  tests/_blobgen_ref.py restates it in numpy.
#include "common.h"

namespace {

constexpr int BLOB_MAX_N = 256;   // accepted boxes held in LDS by the placement kernel (and the slot field of the counter)
constexpr int BLOB_TRIES = 100;   // propose_non_intersecting_coords(num_tries=100), blobgen.py:181-206
constexpr int BAND_ROWS = 16;     // image rows per compose workgroup
constexpr int MAX_W = 4096;       // BAND_ROWS * W bytes of LDS per compose workgroup

enum { KIND_THUMB = 0, KIND_HFLIP = 1, KIND_VFLIP = 2, KIND_Y = 3, KIND_X = 4 };

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned draw32(unsigned long long key, unsigned long long ctr) { return (unsigned)(mix64(key ^ ctr) >> 32); }
__device__ __forceinline__ int uniform(unsigned d, int m) { return (int)(((unsigned long long)d * (unsigned)m) >> 32); }

// table: [T][5] int32 (atlas offset, h, w, class, shade).  One 64-lane wavefront per image s:
//  * background = floor(sum of the n drawn shades / n): the reference's uint8(float32(np.mean(shades))) -- the mean of at most
//    256 integers is k + j / n with j / n <= 255 / 256, far enough from k + 1 that neither rounding reaches it, and the cast
//    truncates;
//  * slots in draw order; each evaluates its tries 64 at a time, one lane per try, against the boxes accepted so far (LDS,
//    broadcast reads); the accepted try is the lowest set bit of the ballot, tries 64..99 run only when 0..63 all collide.
//    The reference's `box_iou(...).sum() == 0` on the normalised boxes is the integer half-open test used here (k / W is
//    correctly rounded and strictly increasing in k < W; two distinct floats never differ by 0).
// Outputs, rows [count, n) zeroed: boxes [S][n][4] (thumbnail, x, y, flips: bit 0 horizontal, bit 1 vertical),
// rows [S][n][5] fp32 (class, x / W, y / H, (x + w) / W, (y + h) / H), counts [S], background [S].
__global__ __launch_bounds__(64) void blob_place_kernel(const int* __restrict__ table, int T, const int* __restrict__ indices, int n,
                                                        int H, int W, unsigned long long key, int* __restrict__ boxes,
                                                        float* __restrict__ rows, int* __restrict__ counts, int* __restrict__ background) {
  __shared__ int4 acc[BLOB_MAX_N];   // accepted boxes (x0, y0, x1, y1), half-open
  const int s = blockIdx.x, lane = threadIdx.x;
  const unsigned long long ctr0 = (unsigned long long)(unsigned)indices[s] << 24;
  int sum = 0;
  for (int k = lane; k < n; k += 64) sum += table[uniform(draw32(key, ctr0 | (unsigned long long)k << 16), T) * 5 + 4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  const int bg = sum / n;
  int* bs = boxes + (size_t)s * n * 4;
  float* rs = rows + (size_t)s * n * 5;
  int count = 0;
  for (int k = 0; k < n; ++k) {
    const unsigned long long cs = ctr0 | (unsigned long long)k << 16;
    const int t = uniform(draw32(key, cs), T);
    const int h = table[t * 5 + 1], w = table[t * 5 + 2];
    if (h >= H || w >= W || h <= 0 || w <= 0) continue;   // refused at construction; never index past the image
    for (int c = 0; c < BLOB_TRIES; c += 64) {
      const int tr = c + lane;
      const int y = uniform(draw32(key, cs | KIND_Y << 8 | (unsigned)tr), H - h);
      const int x = uniform(draw32(key, cs | KIND_X << 8 | (unsigned)tr), W - w);
      int hit = 0;
      for (int j = 0; j < count; ++j) {
        const int4 b = acc[j];
        hit |= (x < b.z) & (b.x < x + w) & (y < b.w) & (b.y < y + h);
      }
      const unsigned long long ok = __ballot(tr < BLOB_TRIES && !hit);
      if (ok) {
        if (lane == __ffsll((long long)ok) - 1) {
          const int fl = (int)(draw32(key, cs | KIND_HFLIP << 8) >> 31) | (int)(draw32(key, cs | KIND_VFLIP << 8) >> 31) << 1;
          acc[count] = make_int4(x, y, x + w, y + h);
          int* bo = bs + count * 4;
          bo[0] = t; bo[1] = x; bo[2] = y; bo[3] = fl;
          float* ro = rs + count * 5;
          ro[0] = (float)table[t * 5 + 3];
          ro[1] = (float)x / (float)W;
          ro[2] = (float)y / (float)H;
          ro[3] = (float)(x + w) / (float)W;
          ro[4] = (float)(y + h) / (float)H;
        }
        __syncthreads();   // (one wavefront: orders the LDS write before the next slot's reads)
        ++count;
        break;
      }
    }
  }
  for (int e = count * 4 + lane; e < n * 4; e += 64) bs[e] = 0;
  for (int e = count * 5 + lane; e < n * 5; e += 64) rs[e] = 0.f;
  if (lane == 0) {
    counts[s] = count;
    background[s] = bg;
  }
}

// grid (row bands, images).  The band is built in LDS -- background, then every placed thumbnail that crosses it, flipped
// (boxes never overlap, so the order of the pastes does not matter) -- and leaves with one store per output byte / float:
// 8-byte stores for uint8 rows of a multiple of 8 bytes (772 x 1032), 16-byte stores of four fp32 / 255 otherwise.
template <bool F32>
__global__ __launch_bounds__(256) void blob_compose_kernel(const unsigned char* __restrict__ atlas, long long atlas_bytes,
                                                           const int* __restrict__ table, const int* __restrict__ boxes,
                                                           const int* __restrict__ counts, const int* __restrict__ background,
                                                           const int* __restrict__ positions, int n, int H, int W, int vec,
                                                           void* __restrict__ out) {
  extern __shared__ unsigned char band[];
  const int s = blockIdx.y, y0 = blockIdx.x * BAND_ROWS, tid = threadIdx.x;
  const int nrows = min(BAND_ROWS, H - y0), nb = nrows * W;
  const unsigned bg = (unsigned)background[s] & 0xffu;
  const unsigned bg4 = bg * 0x01010101u;
  for (int e = tid; e < (nb >> 2); e += 256) reinterpret_cast<unsigned*>(band)[e] = bg4;
  for (int e = (nb & ~3) + tid; e < nb; e += 256) band[e] = (unsigned char)bg;
  __syncthreads();
  const int cnt = counts[s];
  const int* bs = boxes + (size_t)s * n * 4;
  for (int k = 0; k < cnt; ++k) {
    const int t = bs[k * 4], x = bs[k * 4 + 1], y = bs[k * 4 + 2], fl = bs[k * 4 + 3];
    const int off = table[t * 5], h = table[t * 5 + 1], w = table[t * 5 + 2];
    const int r0 = max(y, y0), r1 = min(y + h, y0 + nrows);
    if (r0 >= r1 || x < 0 || x + w > W || off < 0 || (long long)off + (long long)h * w > atlas_bytes) continue;
    const int cells = (r1 - r0) * w;
    for (int e = tid; e < cells; e += 256) {
      const int rr = e / w, c = e - rr * w;
      const int ty = r0 + rr - y;
      const int sy = (fl & 2) ? h - 1 - ty : ty, sx = (fl & 1) ? w - 1 - c : c;
      band[(r0 + rr - y0) * W + x + c] = atlas[off + sy * w + sx];
    }
  }
  __syncthreads();
  const size_t base = ((size_t)positions[s] * H + y0) * W;
  if (!F32) {
    unsigned char* o = static_cast<unsigned char*>(out) + base;
    if (vec) {
      for (int e = tid; e < (nb >> 3); e += 256)
        reinterpret_cast<unsigned long long*>(o)[e] = reinterpret_cast<const unsigned long long*>(band)[e];
    } else {
      for (int e = tid; e < nb; e += 256) o[e] = band[e];
    }
  } else {
    float* o = static_cast<float*>(out) + base;
    if (vec) {
      for (int e = tid; e < (nb >> 2); e += 256) {
        const unsigned v = reinterpret_cast<const unsigned*>(band)[e];
        reinterpret_cast<float4*>(o)[e] = make_float4((float)(v & 0xffu) / 255.f, (float)((v >> 8) & 0xffu) / 255.f,
                                                      (float)((v >> 16) & 0xffu) / 255.f, (float)(v >> 24) / 255.f);
      }
    } else {
      for (int e = tid; e < nb; e += 256) o[e] = (float)band[e] / 255.f;
    }
  }
}

// one workgroup per image: its rows go to flat[offsets[s] ...] (offsets[s] = counts[0] + ... + counts[s - 1])
__global__ __launch_bounds__(256) void blob_label_rows_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int n,
                                                              float* __restrict__ flat, int* __restrict__ offsets) {
  const int s = blockIdx.x, tid = threadIdx.x;
  int off = 0;
  for (int k = 0; k < s; ++k) off += counts[k];
  const int c = counts[s];
  if (tid == 0) {
    offsets[s + 1] = off + c;
    if (s == 0) offsets[0] = 0;
  }
  for (int e = tid; e < c * 5; e += 256) flat[(size_t)off * 5 + e] = rows[(size_t)s * n * 5 + e];
}

}  // namespace

extern "C" int yogo_blobgen_max_n(int* n) {
  YOGO_CHECK_ARG(n, "blobgen_max_n: NULL output");
  *n = BLOB_MAX_N;
  return YOGO_OK;
}

// BlobDataset.__getitem__'s draws and placement (blobgen.py:140-160 get_random_thumbnails, :181-206 propose_non_intersecting_coords,
// :208-249) for S images at once.  See the header for the arguments.
extern "C" int yogo_blobgen_place(const int* table, int num_thumbnails, const int* indices, int S, int n, int H, int W, long long seed,
                                  long long epoch, int* boxes, float* rows, int* counts, int* background, hipStream_t stream) {
  YOGO_CHECK_ARG(table && indices && boxes && rows && counts && background && num_thumbnails > 0 && S >= 0,
                 "blobgen_place: bad arguments");
  YOGO_CHECK_ARG(n >= 1 && n <= BLOB_MAX_N, "blobgen_place: n = %d outside [1, %d]", n, BLOB_MAX_N);
  YOGO_CHECK_ARG(H >= 2 && W >= 2, "blobgen_place: bad image size %d x %d", H, W);
  if (S == 0) return YOGO_OK;
  const unsigned long long key = mix64((unsigned long long)(unsigned)seed << 32 | (unsigned)epoch);
  hipLaunchKernelGGL(blob_place_kernel, dim3(S), dim3(64), 0, stream, table, num_thumbnails, indices, n, H, W, key, boxes, rows, counts,
                     background);
  YOGO_CHECK_LAUNCH("blobgen_place");
  return YOGO_OK;
}

// blobgen.py:216-220 (background fill), :243 (paste), :261-262 (/ 255) into rows positions[0 .. S) of out [B][1][H][W].
extern "C" int yogo_blobgen_compose(const unsigned char* atlas, long long atlas_bytes, const int* table, const int* boxes,
                                    const int* counts, const int* background, const int* positions, int S, int n, int H, int W,
                                    void* out, int elem_bytes, hipStream_t stream) {
  YOGO_CHECK_ARG(atlas && table && boxes && counts && background && positions && out && S >= 0 && atlas_bytes > 0,
                 "blobgen_compose: bad arguments");
  YOGO_CHECK_ARG(elem_bytes == 1 || elem_bytes == 4, "blobgen_compose: elem_bytes must be 1 (uint8) or 4 (float32)");
  YOGO_CHECK_ARG(n >= 1 && n <= BLOB_MAX_N && H >= 2 && W >= 2 && W <= MAX_W, "blobgen_compose: bad n / image size (W <= %d)", MAX_W);
  if (S == 0) return YOGO_OK;
  const size_t lds = (size_t)round_up(BAND_ROWS * W, 16);
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const dim3 grid(cdiv(H, BAND_ROWS), S);
  if (elem_bytes == 1)
    hipLaunchKernelGGL(blob_compose_kernel<false>, grid, dim3(256), lds, stream, atlas, atlas_bytes, table, boxes, counts, background,
                       positions, n, H, W, (int)(aligned && W % 8 == 0), out);
  else
    hipLaunchKernelGGL(blob_compose_kernel<true>, grid, dim3(256), lds, stream, atlas, atlas_bytes, table, boxes, counts, background,
                       positions, n, H, W, (int)(aligned && W % 4 == 0), out);
  YOGO_CHECK_LAUNCH("blobgen_compose");
  return YOGO_OK;
}

extern "C" int yogo_blobgen_label_rows(const float* rows, const int* counts, int S, int n, float* flat, int* offsets, hipStream_t stream) {
  YOGO_CHECK_ARG(rows && counts && flat && offsets && S >= 0 && n >= 1 && n <= BLOB_MAX_N, "blobgen_label_rows: bad arguments");
  if (S == 0) return YOGO_OK;
  hipLaunchKernelGGL(blob_label_rows_kernel, dim3(S), dim3(256), 0, stream, rows, counts, n, flat, offsets);
  YOGO_CHECK_LAUNCH("blobgen_label_rows");
  return YOGO_OK;
}

// PNG files written on the device: the encoder behind `yogo infer --draw-boxes --device-draw` (yogo_amd/draw.py), the first of the
// codec family that writes.  yogo_amd/png_encode.py states the format choices and is the same encoder on the host, byte for byte:
//   filter   per scanline the type 0 .. 4 with the smallest sum of |filtered byte read as signed|, ties to the lowest type
//   bands    BAND_ROWS scanlines = one dynamic-Huffman DEFLATE block of literals only (257 literal codes, one distance code of
//            length zero), closed with an empty stored block; the last band's closing block carries BFINAL
//   lengths  two-queue Huffman over the used symbols sorted by (count, symbol), a leaf wins a tie; lengths over the limit (15; 7 for
//            the code-length alphabet) folded into it and the Kraft sum repaired one unit at a time; longest lengths to the rarest
//   header   all 19 code-length code lengths, each of the 258 lengths as its own symbol (no repeat codes)
//   stored   a band that does not come out smaller than stored blocks (<= 65 535 bytes each) is stored blocks
//   chunks   one IDAT chunk per band; the zlib header opens the first, the Adler-32 closes the last
// Two launches.  png_band_kernel, one workgroup per (band, image): filter choice per row (a wave per row), the histogram and the
// band's Adler sums, the code lengths (rank sort by all lanes, the tree by lane 0), then the bit stream -- every lane codes 16
// consecutive bytes at the bit offset a workgroup prefix sum gives it, OR-ing into an LDS buffer whose complete words go to the
// band's part of the work buffer -- and the chunk's CRC-32: per-lane CRCs of equal pieces (an LDS table), combined pairwise by
// multiplying with x^(8 n) mod P.  png_assemble_kernel, one workgroup per image: the bands' offsets, the Adler-32 from the bands'
// (a, b, n) in closed form, signature / IHDR / lengths / CRCs / IEND, and the bands copied into the file (wave_copy.h).
// Every store is held to the band's part of the work buffer or to the file's slot.
// Level 1 (literals and matches) is png_encode_matches.hip: another band kernel, this file's assembly; what both share is png_deflate.h.
#include "common.h"
#include "png_deflate.h"
#include "wave_copy.h"

namespace {

using namespace yogo_png;

constexpr int LIT = 257;            // literals and end-of-block
constexpr int PER_LANE = 16;        // bytes a lane codes per chunk
constexpr int CHUNK = THREADS * PER_LANE;
constexpr int OUTW = CHUNK * 15 / 32 + 72;   // words of the LDS bit buffer: a chunk at 15 bits per byte, the header, the carry

struct BandShared {
  unsigned hist[LIT + 3];
  unsigned cl_hist[20];
  unsigned crc_tab[256];
  unsigned out[OUTW];
  unsigned part[THREADS];
  unsigned long long red[2 * WAVES];
  unsigned wave_bits[WAVES];
  unsigned short lit_code[LIT + 1], cl_code[20];
  unsigned char lit_len[LIT + 3], cl_len[20];
  unsigned char ftype[BAND_ROWS];
  int use_huff, overflow;
  long long data_bytes;
  HuffScratch<LIT> huff;
};

__global__ __launch_bounds__(THREADS) void png_band_kernel(const unsigned char* __restrict__ pixels, int H, int W, int bpp,
                                                           unsigned char* __restrict__ work, long long work_per_image) {
  __shared__ BandShared S;
  const int band = blockIdx.x, img_i = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int rb = W * bpp, rowlen = rb + 1, nb = band_count(H);
  const int y_first = band * BAND_ROWS, rows = min(BAND_ROWS, H - y_first);
  const int n = rows * rowlen;
  const bool first = band == 0, last = band == nb - 1;
  const unsigned char* img = pixels + (long long)img_i * H * rb;
  unsigned char* image_work = work + (long long)img_i * work_per_image;
  unsigned* meta = reinterpret_cast<unsigned*>(image_work) + (long long)band * META_WORDS;
  const long long stride = band_stride(rb);
  unsigned char* stage = image_work + (long long)nb * META_WORDS * 4 + (long long)band * stride;
  unsigned char* dst = stage + 8;
  const long long dst_cap = stride - 8;

  for (int t = tid; t < LIT + 3; t += THREADS) S.hist[t] = 0;
  for (int t = tid; t < OUTW; t += THREADS) S.out[t] = 0;
  {
    unsigned c = tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    S.crc_tab[tid] = c;
  }
  if (tid == 0) S.overflow = 0;
  __syncthreads();

  // ---- the filter of every row, the histogram, the band's Adler sums --------------------------------------------------------
  unsigned long long s1 = 0, s2 = 0;
  for (int r = wave; r < rows; r += WAVES) {
    const int y = y_first + r;
    const unsigned char* cur = img + (long long)y * rb;
    unsigned sum[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < rb; i += WAVE) {
      const int x = cur[i], a = i >= bpp ? cur[i - bpp] : 0, b = y > 0 ? cur[i - rb] : 0, c = (y > 0 && i >= bpp) ? cur[i - rb - bpp] : 0;
      const int f[5] = {x, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth(a, b, c)) & 255};
#pragma unroll
      for (int k = 0; k < 5; ++k) sum[k] += f[k] >= 128 ? 256 - f[k] : f[k];
    }
    int ft = 0;
    unsigned best = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      unsigned v = sum[k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
      if (k == 0 || v < best) best = v, ft = k;
    }
    if (lane == 0) {
      S.ftype[r] = (unsigned char)ft;
      atomicAdd(&S.hist[ft], 1u);
      s1 += ft;
      s2 += (unsigned long long)(n - r * rowlen) * ft;
    }
    for (int i = lane; i < rb; i += WAVE) {
      const unsigned d = filtered(img, y, i, rb, bpp, ft);
      atomicAdd(&S.hist[d], 1u);
      s1 += d;
      s2 += (unsigned long long)(n - (r * rowlen + 1 + i)) * d;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, WAVE);
    s2 += __shfl_xor(s2, o, WAVE);
  }
  if (lane == 0) S.red[wave] = s1, S.red[WAVES + wave] = s2;
  if (tid == 0) S.hist[256] = 1;
  __syncthreads();

  // ---- code lengths, codes, and whether the band is coded or stored ---------------------------------------------------------
  huffman_lengths(S.hist, LIT, 15, S.lit_len, S.huff, tid);
  if (tid == 0) S.lit_len[LIT] = 0;   // the one distance code
  if (tid < 20) S.cl_hist[tid] = 0;
  __syncthreads();
  for (int t = tid; t < LIT + 1; t += THREADS) atomicAdd(&S.cl_hist[S.lit_len[t]], 1u);
  __syncthreads();
  huffman_lengths(S.cl_hist, 19, 7, S.cl_len, S.huff, tid);
  if (tid == 0) {
    canonical_codes(S.lit_len, LIT, 15, S.lit_code);
    canonical_codes(S.cl_len, 19, 7, S.cl_code);
    long long bits = 17 + 3 * 19 + 3;
    for (int t = 0; t < LIT + 1; ++t) bits += S.cl_len[S.lit_len[t]];
    for (int t = 0; t < LIT; ++t) bits += (long long)S.hist[t] * S.lit_len[t];
    S.use_huff = (bits + 7) / 8 + 4 < stored_bytes(n) ? 1 : 0;
  }
  __syncthreads();

  long long data_bytes = 0;
  if (S.use_huff) {
    // ---- the block header (lane 0), then the literals, PER_LANE consecutive bytes per lane ---------------------------------
    if (tid == 0) {
      int pos = 0;
      if (first) put_bits(S.out, pos, 0x0178u, 16);   // the zlib header 78 01
      put_bits(S.out, pos, 0u | (2u << 1) | (0u << 3) | (0u << 8) | (15u << 13), 17);   // BFINAL 0, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15
      const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      for (int k = 0; k < 19; ++k) put_bits(S.out, pos, S.cl_len[order[k]], 3);
      for (int t = 0; t < LIT + 1; ++t) put_bits(S.out, pos, S.cl_code[S.lit_len[t]], S.cl_len[S.lit_len[t]]);
      S.data_bytes = pos;   // (bits, for now)
    }
    __syncthreads();
    int bitpos = (int)S.data_bytes;
    long long gw = 0;   // words of dst written
    {   // the header's complete words
      const int cw = bitpos >> 5;
      if ((gw + cw) * 4 <= dst_cap) {
        for (int t = tid; t < cw; t += THREADS) reinterpret_cast<unsigned*>(dst)[gw + t] = S.out[t];
      } else if (tid == 0) S.overflow = 1;
      const unsigned carry = S.out[cw];
      __syncthreads();
      for (int t = tid; t <= cw; t += THREADS) S.out[t] = 0;
      __syncthreads();
      if (tid == 0) S.out[0] = carry;
      gw += cw;
      bitpos &= 31;
      __syncthreads();
    }
    for (int c0 = 0; c0 < n; c0 += CHUNK) {
      const int j0 = c0 + tid * PER_LANE;
      unsigned char sym[PER_LANE];
      unsigned my_bits = 0;
      int r = j0 < n ? j0 / rowlen : 0, col = j0 < n ? j0 - r * rowlen : 0;
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) {
        sym[k] = 0;
        if (j0 + k < n) {
          sym[k] = col == 0 ? S.ftype[r] : (unsigned char)filtered(img, y_first + r, col - 1, rb, bpp, S.ftype[r]);
          my_bits += S.lit_len[sym[k]];
          if (++col == rowlen) col = 0, ++r;
        }
      }
      unsigned incl = my_bits;
      for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += v;
      }
      if (lane == WAVE - 1) S.wave_bits[wave] = incl;
      __syncthreads();
      unsigned before = 0, chunk_bits = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += S.wave_bits[w];
        chunk_bits += S.wave_bits[w];
      }
      {
        const unsigned pos = bitpos + before + incl - my_bits;
        unsigned wi = pos >> 5;
        int nbits = pos & 31;
        unsigned long long acc = 0;
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
          if (j0 + k < n) {
            acc |= (unsigned long long)S.lit_code[sym[k]] << nbits;
            nbits += S.lit_len[sym[k]];
            if (nbits >= 32) {
              atomicOr(&S.out[wi++], (unsigned)acc);
              acc >>= 32;
              nbits -= 32;
            }
          }
        }
        if (nbits > 0 && acc != 0) atomicOr(&S.out[wi], (unsigned)acc);
      }
      __syncthreads();
      const int total = bitpos + (int)chunk_bits, cw = total >> 5;
      if ((gw + cw) * 4 <= dst_cap) {
        for (int t = tid; t < cw; t += THREADS) reinterpret_cast<unsigned*>(dst)[gw + t] = S.out[t];
      } else if (tid == 0) S.overflow = 1;
      const unsigned carry = S.out[cw];
      __syncthreads();
      for (int t = tid; t <= cw; t += THREADS) S.out[t] = 0;
      __syncthreads();
      if (tid == 0) S.out[0] = carry;
      gw += cw;
      bitpos = total & 31;
      __syncthreads();
    }
    if (tid == 0) {   // end of block, the closing empty stored block
      int pos = bitpos;
      put_bits(S.out, pos, S.lit_code[256], S.lit_len[256]);
      put_bits(S.out, pos, last ? 1u : 0u, 3);
      pos = (pos + 7) & ~7;
      put_bits(S.out, pos, 0u, 16);
      put_bits(S.out, pos, 0xFFFFu, 16);
      S.data_bytes = pos >> 3;   // the tail's bytes
    }
    __syncthreads();
    const int tail = (int)S.data_bytes;
    if (gw * 4 + tail <= dst_cap) {
      for (int t = tid; t < tail; t += THREADS) dst[gw * 4 + t] = (unsigned char)(S.out[t >> 2] >> (8 * (t & 3)));
    } else if (tid == 0) S.overflow = 1;
    data_bytes = gw * 4 + tail;
  } else {
    // ---- stored blocks ---------------------------------------------------------------------------------------------------
    const int zh = first ? 2 : 0, nblk = (n + MAX_STORED - 1) / MAX_STORED;
    data_bytes = zh + stored_bytes(n);
    if (data_bytes <= dst_cap) {
      if (first && tid < 2) dst[tid] = tid == 0 ? 0x78 : 0x01;
      for (int k = tid; k < nblk; k += THREADS) {
        unsigned char* h = dst + zh + (long long)k * (MAX_STORED + 5);
        const unsigned len = (unsigned)min(MAX_STORED, n - k * MAX_STORED);
        h[0] = (last && k == nblk - 1) ? 1 : 0;
        h[1] = (unsigned char)len, h[2] = (unsigned char)(len >> 8), h[3] = (unsigned char)~len, h[4] = (unsigned char)(~len >> 8);
      }
      for (int c0 = 0; c0 < n; c0 += CHUNK) {
        const int j0 = c0 + tid * PER_LANE;
        int r = j0 < n ? j0 / rowlen : 0, col = j0 < n ? j0 - r * rowlen : 0;
        for (int k = 0; k < PER_LANE && j0 + k < n; ++k) {
          const int j = j0 + k;
          dst[zh + 5 * (j / MAX_STORED + 1) + j] = col == 0 ? S.ftype[r] : (unsigned char)filtered(img, y_first + r, col - 1, rb, bpp, S.ftype[r]);
          if (++col == rowlen) col = 0, ++r;
        }
      }
    } else if (tid == 0) S.overflow = 1;
  }
  __syncthreads();   // the band's bytes are written: every lane may read them back
  const bool overflow = S.overflow != 0;

  // ---- the chunk's CRC-32 over its type and data: equal pieces per lane, zero bytes in front of the first ------------------------
  unsigned crc_state = 0;
  if (!overflow) {
    if (tid < 4) stage[4 + tid] = "IDAT"[tid];
    __syncthreads();
    const long long m = 4 + data_bytes, piece = (m + THREADS - 1) / THREADS, pad = piece * THREADS - m;
    const unsigned char* msg = stage + 4;
    unsigned c = 0;
    for (long long p = (long long)tid * piece; p < (long long)(tid + 1) * piece; ++p)
      if (p >= pad) c = S.crc_tab[(c ^ msg[p - pad]) & 255u] ^ (c >> 8);
    S.part[tid] = c;
    unsigned X = xpow8((unsigned long long)piece);
    __syncthreads();
    for (int s = 1; s < THREADS; s <<= 1) {
      if ((tid & (2 * s - 1)) == 0) S.part[tid] = mulmod(S.part[tid], X) ^ S.part[tid + s];
      X = mulmod(X, X);
      __syncthreads();
    }
    if (tid == 0) crc_state = S.part[0] ^ mulmod(0xFFFFFFFFu, xpow8((unsigned long long)m));
  }
  if (tid == 0) {
    unsigned long long a = 0, b = 0;
    for (int w = 0; w < WAVES; ++w) a += S.red[w] % ADLER_MOD, b += S.red[WAVES + w] % ADLER_MOD;
    meta[0] = (unsigned)data_bytes;
    meta[1] = crc_state;
    meta[2] = (unsigned)(a % ADLER_MOD);
    meta[3] = (unsigned)(b % ADLER_MOD);
    meta[4] = (unsigned)n;
    meta[5] = overflow ? 1u : 0u;
    meta[6] = meta[7] = 0;
  }
}

__device__ __forceinline__ void put_be32(unsigned char* p, unsigned v) {
  p[0] = (unsigned char)(v >> 24), p[1] = (unsigned char)(v >> 16), p[2] = (unsigned char)(v >> 8), p[3] = (unsigned char)v;
}

// the length of image i's file and its status, from its bands' records
__device__ __forceinline__ long long file_length(const unsigned char* work, long long work_per_image, int i, int nb, long long slot_bytes,
                                                 int* status) {
  const unsigned* meta = reinterpret_cast<const unsigned*>(work + (long long)i * work_per_image);
  long long len = 8 + 25 + 12 + 4;
  bool overflow = false;
  for (int k = 0; k < nb; ++k) {
    len += 12 + (long long)meta[k * META_WORDS];
    overflow = overflow || meta[k * META_WORDS + 5] != 0;
  }
  *status = overflow ? ST_BAND : (len > slot_bytes ? ST_SLOT : 0);
  return *status ? 0 : len;
}

__global__ __launch_bounds__(THREADS) void png_assemble_kernel(const unsigned char* __restrict__ work, long long work_per_image, int B, int H,
                                                               int W, int bpp, unsigned char* __restrict__ files, long long slot_bytes,
                                                               int packed, long long* __restrict__ offsets, int* __restrict__ status) {
  __shared__ unsigned long long before;
  __shared__ unsigned band_at[MAX_BANDS];
  __shared__ unsigned adler;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nb = band_count(H), rb = W * bpp;
  if (tid == 0) before = 0;
  __syncthreads();
  unsigned long long mine = 0;
  int st_any;
  for (int i = tid; i < b; i += THREADS) mine += (unsigned long long)file_length(work, work_per_image, i, nb, slot_bytes, &st_any);
  if (mine) atomicAdd(&before, mine);
  __syncthreads();
  int st;
  const long long flen = file_length(work, work_per_image, b, nb, slot_bytes, &st);
  const long long start = (long long)before;
  if (tid == 0) {
    offsets[b] = start;
    if (b == B - 1) offsets[B] = start + flen;
    status[b] = st;
  }
  if (st) return;
  unsigned char* file = files + (packed ? start : (long long)b * slot_bytes);
  const unsigned char* image_work = work + (long long)b * work_per_image;
  const unsigned* meta = reinterpret_cast<const unsigned*>(image_work);
  const unsigned char* stages = image_work + (long long)nb * META_WORDS * 4;
  const long long stride = band_stride(rb);
  if (tid == 0) {
    // where every band's chunk starts; the Adler-32 of the whole stream from the bands' sums:
    // over a band of n bytes, a += s1 and b += n * a_before + s2
    unsigned long long at = 33, a = 1, bsum = 0;
    for (int k = 0; k < nb; ++k) {
      band_at[k] = (unsigned)at;
      at += 12 + meta[k * META_WORDS] + (k == nb - 1 ? 4 : 0);
      bsum = (bsum + (unsigned long long)meta[k * META_WORDS + 4] % ADLER_MOD * a + meta[k * META_WORDS + 3]) % ADLER_MOD;
      a = (a + meta[k * META_WORDS + 2]) % ADLER_MOD;
    }
    adler = (unsigned)((bsum << 16) | a);
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int k = 0; k < 8; ++k) file[k] = sig[k];
    unsigned char* h = file + 8;
    put_be32(h, 13);
    h[4] = 'I', h[5] = 'H', h[6] = 'D', h[7] = 'R';
    put_be32(h + 8, (unsigned)W);
    put_be32(h + 12, (unsigned)H);
    h[16] = 8, h[17] = bpp == 1 ? 0 : bpp == 2 ? 4 : bpp == 3 ? 2 : 6, h[18] = 0, h[19] = 0, h[20] = 0;
    unsigned c = 0xFFFFFFFFu;
    for (int k = 4; k < 21; ++k) c = crc_byte_bitwise(c, h[k]);
    put_be32(h + 21, ~c);
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int k = 0; k < 12; ++k) file[at + k] = iend[k];
  }
  __syncthreads();
  for (int k = tid; k < nb; k += THREADS) {   // a band's length and CRC; the last one's data go on with the Adler-32
    unsigned char* chunk = file + band_at[k];
    const unsigned data = meta[k * META_WORDS];
    unsigned c = meta[k * META_WORDS + 1];
    if (k == nb - 1) {
      put_be32(chunk, data + 4);
      put_be32(chunk + 8 + data, adler);
      for (int q = 0; q < 4; ++q) c = crc_byte_bitwise(c, (adler >> (24 - 8 * q)) & 255u);
      put_be32(chunk + 12 + data, ~c);
    } else {
      put_be32(chunk, data);
      put_be32(chunk + 8 + data, ~c);
    }
  }
  for (int k = wave; k < nb; k += WAVES)   // type and data
    yogo_wave::wave_copy(file + band_at[k] + 4, stages + (long long)k * stride + 4, 4 + (long long)meta[k * META_WORDS], lane);
}

}  // namespace

// (png_encode_matches.hip) the band launch of level 1
int yogo_png_band_matches_launch(const unsigned char* pixels, int B, int H, int W, int bpp, unsigned char* work, long long work_per,
                                 hipStream_t stream);

extern "C" int yogo_png_encode_bound_level(int H, int W, int bpp, int level, size_t* slot_bytes, size_t* work_bytes) {
  YOGO_CHECK_ARG(slot_bytes && work_bytes, "png_encode_bound: null argument");
  YOGO_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && bpp >= 1 && bpp <= 4, "png_encode_bound: bad image shape %d x %d x %d", H, W, bpp);
  YOGO_CHECK_ARG(level == 0 || level == 1, "png_encode_bound: level %d (0: literals only, 1: literals and matches)", level);
  const int rb = W * bpp, nb = band_count(H);
  long long total = 8 + 25 + 12;
  for (int k = 0; k < nb; ++k) {
    const int rows = H - k * BAND_ROWS < BAND_ROWS ? H - k * BAND_ROWS : BAND_ROWS;
    total += 12 + stored_bytes((long long)rows * (rb + 1)) + (k == 0 ? 2 : 0) + (k == nb - 1 ? 4 : 0);
  }
  YOGO_CHECK_ARG(total < (1LL << 31), "png_encode_bound: an image of %d x %d x %d bytes (files below 2 GiB)", H, W, bpp);
  *slot_bytes = (size_t)total;
  *work_bytes = (size_t)work_per_image(H, rb, level);
  return YOGO_OK;
}

extern "C" int yogo_png_encode_bound(int H, int W, int bpp, size_t* slot_bytes, size_t* work_bytes) {
  return yogo_png_encode_bound_level(H, W, bpp, 0, slot_bytes, work_bytes);
}

extern "C" int yogo_png_encode_level(const unsigned char* pixels, int B, int H, int W, int bpp, int level, unsigned char* files,
                                     long long slot_bytes, int packed, long long* offsets, int* status, unsigned char* work,
                                     long long work_bytes, hipStream_t stream) {
  YOGO_CHECK_ARG(pixels && files && offsets && status && work, "png_encode: null argument");
  YOGO_CHECK_ARG(B >= 0 && B <= 65535, "png_encode: B = %d images, at most 65535 per call", B);
  size_t bound = 0, per_image = 0;
  if (int rc = yogo_png_encode_bound_level(H, W, bpp, level, &bound, &per_image)) return rc;
  YOGO_CHECK_ARG(slot_bytes >= 0 && (packed == 0 || packed == 1), "png_encode: bad slot size or packed flag");
  YOGO_CHECK_ARG(work_bytes >= (long long)B * (long long)per_image, "png_encode: %lld bytes of work space, %d images need %lld at level %d",
                 work_bytes, B, (long long)B * (long long)per_image, level);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 15) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "png_encode: the work space must be 16-byte, the offsets 8-byte, the status 4-byte aligned");
  if (B == 0) return YOGO_OK;
  const int nb = band_count(H);
  if (level == 0) {
    hipLaunchKernelGGL(png_band_kernel, dim3(nb, B), dim3(THREADS), 0, stream, pixels, H, W, bpp, work, (long long)per_image);
    YOGO_CHECK_LAUNCH("png_encode (bands)");
  } else if (int rc = yogo_png_band_matches_launch(pixels, B, H, W, bpp, work, (long long)per_image, stream)) {
    return rc;
  }
  hipLaunchKernelGGL(png_assemble_kernel, dim3(B), dim3(THREADS), 0, stream, work, (long long)per_image, B, H, W, bpp, files, slot_bytes,
                     packed, offsets, status);
  YOGO_CHECK_LAUNCH("png_encode (assembly)");
  if (yogo_launch_log_enabled()) {
    if (level == 0) yogo_launch_log("png_band_kernel | B=%d image=%dx%dx%d bands=%d", B, H, W, bpp, nb);
    yogo_launch_log("png_assemble_kernel | B=%d slot=%lld packed=%d", B, slot_bytes, packed);
  }
  return YOGO_OK;
}

extern "C" int yogo_png_encode(const unsigned char* pixels, int B, int H, int W, int bpp, unsigned char* files, long long slot_bytes,
                               int packed, long long* offsets, int* status, unsigned char* work, long long work_bytes,
                               hipStream_t stream) {
  return yogo_png_encode_level(pixels, B, H, W, bpp, 0, files, slot_bytes, packed, offsets, status, work, work_bytes, stream);
}

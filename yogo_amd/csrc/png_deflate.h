// What the PNG band kernels share: png_encode.hip (level 0, literals only) and png_encode_matches.hip (level 1, literals and matches).
// The geometry of the work buffer, the CRC-32 arithmetic, the scanline filters, the code-length rule of yogo_amd/png_encode.py and
// the bit buffer's store.  Nothing here checks a bound: the kernels hold every store to their part of the work buffer.
#pragma once
#include "common.h"
#include "wave_copy.h"

namespace yogo_png {

using yogo_wave::WAVE;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int BAND_ROWS = 16;
constexpr int MAX_STORED = 65535;
constexpr int META_WORDS = 8;       // per band: data bytes, CRC register, Adler s1, s2, n, overflow
constexpr unsigned ADLER_MOD = 65521u;
constexpr unsigned CRC_POLY = 0xEDB88320u;
constexpr int MAX_BANDS = 4096;     // H <= 65535
constexpr int ST_SLOT = 1, ST_BAND = 2;

__host__ __device__ inline long long stored_bytes(long long n) { return n + 5 * ((n + MAX_STORED - 1) / MAX_STORED); }
__host__ __device__ inline long long band_stride(int rb) { return (8 + stored_bytes((long long)BAND_ROWS * (rb + 1)) + 2 + 4 + 15) & ~15LL; }
__host__ __device__ inline int band_count(int H) { return (H + BAND_ROWS - 1) / BAND_ROWS; }

// a * b mod P, polynomials over GF(2) in the CRC's reflected order (bit 31 is x^0)
__device__ __forceinline__ unsigned mulmod(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
// x^(8 n) mod P
__device__ __forceinline__ unsigned xpow8(unsigned long long n) {
  unsigned r = 0x80000000u, base = 0x00800000u;   // 1, x^8
  for (; n; n >>= 1) {
    if (n & 1ull) r = mulmod(r, base);
    base = mulmod(base, base);
  }
  return r;
}
__device__ __forceinline__ unsigned crc_byte_bitwise(unsigned c, unsigned byte) {
  c ^= byte;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
  return c;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// byte i of row y of the image at img, filtered with type ft
__device__ __forceinline__ unsigned filtered(const unsigned char* __restrict__ img, int y, int i, int rb, int bpp, int ft) {
  const unsigned char* cur = img + (long long)y * rb;
  const int x = cur[i];
  if (ft == 0) return x;
  const int a = i >= bpp ? cur[i - bpp] : 0;
  if (ft == 1) return (x - a) & 255;
  const int b = y > 0 ? cur[i - rb] : 0;
  if (ft == 2) return (x - b) & 255;
  if (ft == 3) return (x - ((a + b) >> 1)) & 255;
  const int c = (y > 0 && i >= bpp) ? cur[i - rb - bpp] : 0;
  return (x - paeth(a, b, c)) & 255;
}

template <int N>   // N: the most symbols of an alphabet it serves
struct HuffScratch {
  unsigned leaf_f[N], node_f[N];
  unsigned short sym[N], leaf_parent[N], node_parent[N], depth[N];
  int used;
};

// code lengths of at most `limit` bits for the nsym counts at freq -> len (0 for an unused symbol); called by the whole workgroup
template <int N>
__device__ void huffman_lengths(const unsigned* freq, int nsym, int limit, unsigned char* len, HuffScratch<N>& s, int tid) {
  if (tid == 0) s.used = 0;
  __syncthreads();
  for (int t = tid; t < nsym; t += THREADS) {
    len[t] = 0;
    const unsigned f = freq[t];
    if (f == 0) continue;
    int rank = 0;
    for (int u = 0; u < nsym; ++u) {
      const unsigned g = freq[u];
      rank += (g != 0 && (g < f || (g == f && u < t))) ? 1 : 0;
    }
    s.sym[rank] = (unsigned short)t;
    s.leaf_f[rank] = f;
    atomicAdd(&s.used, 1);
  }
  __syncthreads();
  if (tid == 0) {
    const int n = s.used;
    if (n == 1) {
      len[s.sym[0]] = 1;
    } else if (n > 1) {
      int li = 0, ni = 0;
      for (int k = 0; k < n - 1; ++k) {   // the two smallest of the leaves left and the internal nodes made so far
        unsigned total = 0;
        for (int two = 0; two < 2; ++two) {
          if (li < n && (ni >= k || s.leaf_f[li] <= s.node_f[ni])) {
            total += s.leaf_f[li];
            s.leaf_parent[li++] = (unsigned short)k;
          } else {
            total += s.node_f[ni];
            s.node_parent[ni++] = (unsigned short)k;
          }
        }
        s.node_f[k] = total;
      }
      s.depth[n - 2] = 0;
      for (int k = n - 3; k >= 0; --k) s.depth[k] = s.depth[s.node_parent[k]] + 1;
      int count[16];
      for (int b = 0; b < 16; ++b) count[b] = 0;
      for (int i = 0; i < n; ++i) {
        const int d = s.depth[s.leaf_parent[i]] + 1;
        ++count[d < limit ? d : limit];
      }
      unsigned kraft = 0;
      for (int b = 1; b <= limit; ++b) kraft += (unsigned)count[b] << (limit - b);
      while (kraft > (1u << limit)) {
        --count[limit];
        int b = limit - 1;
        while (count[b] == 0) --b;
        --count[b];
        count[b + 1] += 2;
        --kraft;
      }
      int i = 0;
      for (int b = limit; b >= 1; --b)
        for (int c = 0; c < count[b]; ++c) len[s.sym[i++]] = (unsigned char)b;
    }
  }
  __syncthreads();
}

// canonical codes, bit-reversed (the stream fills bytes from the least significant bit); lane 0
__device__ inline void canonical_codes(const unsigned char* len, int nsym, int limit, unsigned short* code) {
  int count[17], next[17];
  for (int b = 0; b <= 16; ++b) count[b] = 0;
  for (int t = 0; t < nsym; ++t) ++count[len[t]];
  count[0] = 0;
  int c = 0;
  next[0] = 0;
  for (int b = 1; b <= limit; ++b) {
    c = (c + count[b - 1]) << 1;
    next[b] = c;
  }
  for (int t = 0; t < nsym; ++t) {
    const int b = len[t];
    code[t] = b ? (unsigned short)(__brev((unsigned)next[b]++) >> (32 - b)) : 0;
  }
}

// `bits` bits of v at bit `pos` of the LDS buffer (one lane, plain stores)
__device__ __forceinline__ void put_bits(unsigned* buf, int& pos, unsigned v, int bits) {
  const int w = pos >> 5, sh = pos & 31;
  buf[w] |= v << sh;
  if (sh + bits > 32) buf[w + 1] |= v >> (32 - sh);
  pos += bits;
}

// The chunk's CRC-32 over its type and the data_bytes bytes the workgroup has written behind stage + 8 (equal pieces per lane, zero
// bytes in front of the first, combined pairwise by multiplying with x^(8 n) mod P), then the band's record for png_assemble_kernel.
// Called by the whole workgroup behind a barrier; crc_tab [256] and part [THREADS] are LDS, red the waves' Adler sums (s1, then s2).
__device__ inline void band_crc_and_record(unsigned char* stage, long long data_bytes, bool overflow, int n, const unsigned* crc_tab,
                                           unsigned* part, const unsigned long long* red, unsigned* meta, int tid) {
  unsigned crc_state = 0;
  if (!overflow) {
    if (tid < 4) stage[4 + tid] = "IDAT"[tid];
    __syncthreads();
    const long long m = 4 + data_bytes, piece = (m + THREADS - 1) / THREADS, pad = piece * THREADS - m;
    const unsigned char* msg = stage + 4;
    unsigned c = 0;
    for (long long p = (long long)tid * piece; p < (long long)(tid + 1) * piece; ++p)
      if (p >= pad) c = crc_tab[(c ^ msg[p - pad]) & 255u] ^ (c >> 8);
    part[tid] = c;
    unsigned X = xpow8((unsigned long long)piece);
    __syncthreads();
    for (int s = 1; s < THREADS; s <<= 1) {
      if ((tid & (2 * s - 1)) == 0) part[tid] = mulmod(part[tid], X) ^ part[tid + s];
      X = mulmod(X, X);
      __syncthreads();
    }
    if (tid == 0) crc_state = part[0] ^ mulmod(0xFFFFFFFFu, xpow8((unsigned long long)m));
  }
  if (tid == 0) {
    unsigned long long a = 0, b = 0;
    for (int w = 0; w < WAVES; ++w) a += red[w] % ADLER_MOD, b += red[WAVES + w] % ADLER_MOD;
    meta[0] = (unsigned)data_bytes;
    meta[1] = crc_state;
    meta[2] = (unsigned)(a % ADLER_MOD);
    meta[3] = (unsigned)(b % ADLER_MOD);
    meta[4] = (unsigned)n;
    meta[5] = overflow ? 1u : 0u;
    meta[6] = meta[7] = 0;
  }
}

// ---- level 1 (png_encode_matches.hip): its part of the work buffer lies behind level 0's, so png_assemble_kernel serves both ------
constexpr int MATCH_PIECE = 512, MATCH_WINDOW = 64, MIN_MATCH = 3, MAX_MATCH = 258;   // PIECE, WINDOW, ... of yogo_amd/png_encode.py
// a band's filtered bytes, and as much twice for its tokens (16 bits per position)
__host__ __device__ inline long long filtered_stride(int rb) { return ((long long)BAND_ROWS * (rb + 1) + 15) & ~15LL; }
__host__ __device__ inline long long work_per_image(int H, int rb, int level) {
  const long long nb = band_count(H);
  return nb * META_WORDS * 4 + nb * band_stride(rb) + (level ? 3 * nb * filtered_stride(rb) : 0);
}

}  // namespace yogo_png

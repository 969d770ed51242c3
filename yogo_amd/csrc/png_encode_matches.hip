// Level 1 of the PNG encoder (`--device-draw-level 1`): a band is ONE dynamic-Huffman DEFLATE block of literals and matches.
// yogo_amd/png_encode.py states the rules and is the same encoder on the host, byte for byte; png_encode.hip is level 0, whose
// filter choice, bands, chunks, stored fallback and assembly launch (png_assemble_kernel) this level keeps.
//   pieces      the band's filtered bytes in pieces of MATCH_PIECE bytes; no match passes its piece's end or the band's first byte
//   candidates  at a position the distances bpp * k, k = 1 .. MATCH_WINDOW; the length is the run of bytes equal to the byte
//               `distance` before them (overlapping copies allowed), at most MAX_MATCH and up to the piece's end; the longest wins,
//               ties to the nearest; below MIN_MATCH there is no match
//   parse       greedy from a piece's first byte, pieces independent of each other
//   block       286 literal/length and 30 distance code lengths spelled out (one distance code of length zero in a band without a
//               match); stored blocks when the exact bit count does not come out smaller
// png_band_matches_kernel, one workgroup per (band, image).  The filtered bytes are needed at random earlier positions, so they are
// written ONCE to the band's part of the work buffer (behind level 0's parts) and staged from there, a chunk of CHUNK positions and
// the 4 * MATCH_WINDOW bytes before it at a time, into an LDS window: a band may be 16 x 262 141 bytes, nothing assumes it fits LDS.
// Pass 1 per chunk: every lane finds the winner of its positions in the window, one lane per piece walks the parse and marks the
// token starts, all lanes count the tokens into the two histograms and keep them (16 bits per position) in the work buffer.  Then
// the code lengths and the exact bit count.  Pass 2 per chunk: every lane codes the tokens that start in its PER_LANE consecutive
// positions at the bit offset a workgroup prefix sum gives it, OR-ing into an LDS bit buffer whose complete words go to the band's
// stage.  A token costs at most 15 bits as a literal and 15 + 5 + 15 + 6 = 41 as a match of >= 3 bytes (distances <= 256 have at
// most 6 extra bits), so a chunk is at most 16 bits per byte: OUTW.  Every store is held to the band's parts of the work buffer.
// LDS per workgroup: 31 KiB (BandShared below), five workgroups of four waves per CU.
#include "common.h"
#include "png_deflate.h"

namespace {

using namespace yogo_png;

constexpr int NLEN = 286, NDIST = 30;   // literal/length and distance symbols
constexpr int PER_LANE = 16;            // positions a lane codes per chunk
constexpr int CHUNK = THREADS * PER_LANE;
constexpr int PIECES = CHUNK / MATCH_PIECE;
constexpr int BACK = 4 * MATCH_WINDOW;  // the farthest candidate
constexpr int OUTW = CHUNK * 16 / 32 + 80;   // words of the LDS bit buffer: a chunk at 16 bits per byte; the header (2302 bits); the carry
constexpr unsigned TOKEN = 0x8000u;     // a position's 16 bits: length (9 bits, 0: a literal), k - 1 (6 bits), "a token starts here"
static_assert(CHUNK % MATCH_PIECE == 0 && MATCH_PIECE > MAX_MATCH && PIECES <= THREADS, "pieces tile a chunk; a match of 258 fits one");
static_assert(MIN_MATCH == 3, "the first test of a candidate compares three bytes of a four-byte read");
static_assert(MATCH_WINDOW <= 64 && BACK <= 256, "k - 1 in 6 bits; distances with at most 6 extra bits");

__device__ const unsigned short LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const unsigned char LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const unsigned short DIST_BASE[16] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193};
__device__ const unsigned char DIST_EXTRA[16] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6};

struct BandShared {
  unsigned hist[NLEN + 2];
  unsigned dhist[NDIST + 2];
  unsigned cl_hist[20];
  unsigned crc_tab[256];
  unsigned out[OUTW];
  unsigned part[THREADS];
  unsigned long long red[2 * WAVES];
  unsigned wave_bits[WAVES];
  unsigned extra_bits;
  unsigned short lit_code[NLEN], dist_code[NDIST], cl_code[20];
  unsigned short tok[CHUNK];
  unsigned short len_base[29], dist_base[16];
  unsigned char len_extra[29], dist_extra[16];
  unsigned char len_sym[MAX_MATCH + 2], dist_sym[BACK + 4];   // by length / distance
  unsigned char hl[NLEN + NDIST + 4], cl_len[20];             // the header's lengths: literal/length, then distance
  unsigned char win[BACK + CHUNK + 4];   // (+ 4: the four-byte read at a chunk's last positions)
  unsigned char ftype[BAND_ROWS];
  int use_huff, overflow, ndist;
  long long data_bytes;
  HuffScratch<NLEN> huff;
};

__global__ __launch_bounds__(THREADS) void png_band_matches_kernel(const unsigned char* __restrict__ pixels, int H, int W, int bpp,
                                                                   unsigned char* __restrict__ work, long long work_per) {
  __shared__ BandShared S;
  const int band = blockIdx.x, img_i = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int rb = W * bpp, rowlen = rb + 1, nb = band_count(H);
  const int y_first = band * BAND_ROWS, rows = min(BAND_ROWS, H - y_first);
  const int n = rows * rowlen;
  const bool first = band == 0, last = band == nb - 1;
  const unsigned char* img = pixels + (long long)img_i * H * rb;
  unsigned char* image_work = work + (long long)img_i * work_per;
  unsigned* meta = reinterpret_cast<unsigned*>(image_work) + (long long)band * META_WORDS;
  const long long stride = band_stride(rb), fstride = filtered_stride(rb);   // n <= fstride
  unsigned char* stage = image_work + (long long)nb * META_WORDS * 4 + (long long)band * stride;
  unsigned char* dst = stage + 8;
  const long long dst_cap = stride - 8;
  unsigned char* level1 = image_work + (long long)nb * META_WORDS * 4 + (long long)nb * stride;
  unsigned char* fb = level1 + (long long)band * fstride;                                          // [n] the filtered bytes
  unsigned short* tokens = reinterpret_cast<unsigned short*>(level1 + (long long)nb * fstride + 2 * (long long)band * fstride);   // [n]

  for (int t = tid; t < NLEN + 2; t += THREADS) S.hist[t] = 0;
  for (int t = tid; t < OUTW; t += THREADS) S.out[t] = 0;
  if (tid < NDIST + 2) S.dhist[tid] = 0;
  {
    unsigned c = tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    S.crc_tab[tid] = c;
  }
  if (tid < 29) S.len_base[tid] = LEN_BASE[tid], S.len_extra[tid] = LEN_EXTRA[tid];
  if (tid < 16) S.dist_base[tid] = DIST_BASE[tid], S.dist_extra[tid] = DIST_EXTRA[tid];
  for (int t = tid; t <= MAX_MATCH; t += THREADS) {   // the last symbol whose base is at most the length (258 has its own)
    int s = 0;
    for (int k = 1; k < 29; ++k) s = LEN_BASE[k] <= t ? k : s;
    S.len_sym[t] = (unsigned char)s;
  }
  for (int t = tid; t <= BACK; t += THREADS) {
    int s = 0;
    for (int k = 1; k < 16; ++k) s = DIST_BASE[k] <= t ? k : s;
    S.dist_sym[t] = (unsigned char)s;
  }
  if (tid == 0) S.overflow = 0, S.extra_bits = 0;
  __syncthreads();

  // ---- the filter of every row; the filtered bytes to the work buffer; the band's Adler sums --------------------------------
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
    unsigned char* frow = fb + (long long)r * rowlen;   // r * rowlen + rowlen <= n
    if (lane == 0) {
      S.ftype[r] = (unsigned char)ft;
      frow[0] = (unsigned char)ft;
      s1 += ft;
      s2 += (unsigned long long)(n - r * rowlen) * ft;
    }
    for (int i = lane; i < rb; i += WAVE) {
      const unsigned d = filtered(img, y, i, rb, bpp, ft);
      frow[1 + i] = (unsigned char)d;
      s1 += d;
      s2 += (unsigned long long)(n - (r * rowlen + 1 + i)) * d;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, WAVE);
    s2 += __shfl_xor(s2, o, WAVE);
  }
  if (lane == 0) S.red[wave] = s1, S.red[WAVES + wave] = s2;
  __syncthreads();   // the band's filtered bytes are written: every lane may read them back

  // ---- pass 1: winners, parse, histograms; the tokens to the work buffer ----------------------------------------------------
  unsigned my_extra = 0;
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const int cn = min(CHUNK, n - c0);
    for (int t = tid; t < BACK + cn; t += THREADS) {
      const int p = c0 - BACK + t;
      S.win[t] = p >= 0 ? fb[p] : 0;
    }
    __syncthreads();
    for (int i = tid; i < cn; i += THREADS) {
      const int p = c0 + i;
      const int room = min(MAX_MATCH, min(cn, (i / MATCH_PIECE + 1) * MATCH_PIECE) - i);   // up to the piece's (the band's) end
      const unsigned char* at = S.win + BACK + i;
      int best = 0, best_k = 0;
      if (room >= MIN_MATCH) {
        unsigned head;   // the position's first four bytes; only MIN_MATCH of them are compared (room: they lie inside the chunk)
        __builtin_memcpy(&head, at, 4);
        for (int k = 1, d = bpp; k <= MATCH_WINDOW && d <= p; ++k, d += bpp) {
          unsigned cand;
          __builtin_memcpy(&cand, at - d, 4);
          if ((cand ^ head) & 0xFFFFFFu) continue;   // fewer than MIN_MATCH equal bytes: no match, and no bar to a farther one
          int l = MIN_MATCH;
          while (l < room && at[l] == at[l - d]) ++l;
          if (l > best) {   // strictly: a tie stays with the nearer one
            best = l, best_k = k;
            if (best == room) break;
          }
        }
      }
      S.tok[i] = best >= MIN_MATCH ? (unsigned short)(best | ((best_k - 1) << 9)) : 0;
    }
    __syncthreads();
    if (tid < PIECES && tid * MATCH_PIECE < cn) {   // greedy from the piece's first byte
      const int end = min(cn, (tid + 1) * MATCH_PIECE);
      for (int i = tid * MATCH_PIECE; i < end;) {
        const unsigned v = S.tok[i];
        S.tok[i] = (unsigned short)(v | TOKEN);
        i += (v & 511u) ? (int)(v & 511u) : 1;
      }
    }
    __syncthreads();
    for (int i = tid; i < cn; i += THREADS) {
      const unsigned v = S.tok[i];
      tokens[c0 + i] = (unsigned short)v;   // c0 + i < n
      if (!(v & TOKEN)) continue;
      const int l = v & 511u;
      if (l == 0) {
        atomicAdd(&S.hist[S.win[BACK + i]], 1u);
      } else {
        const int ls = S.len_sym[l], ds = S.dist_sym[bpp * (int)(((v >> 9) & 63u) + 1)];
        atomicAdd(&S.hist[257 + ls], 1u);
        atomicAdd(&S.dhist[ds], 1u);
        my_extra += S.len_extra[ls] + S.dist_extra[ds];
      }
    }
    __syncthreads();
  }
  if (my_extra) atomicAdd(&S.extra_bits, my_extra);
  if (tid == 0) S.hist[256] = 1;
  __syncthreads();

  // ---- code lengths, codes, and whether the band is coded or stored ---------------------------------------------------------
  unsigned char* lit_len = S.hl;
  unsigned char* dist_len = S.hl + NLEN;
  huffman_lengths(S.hist, NLEN, 15, lit_len, S.huff, tid);
  huffman_lengths(S.dhist, NDIST, 15, dist_len, S.huff, tid);
  if (tid == 0) {
    unsigned matches = 0;
    for (int t = 0; t < NDIST; ++t) matches += S.dhist[t];
    S.ndist = matches ? NDIST : 1;   // no match: one distance code of length zero
  }
  if (tid < 20) S.cl_hist[tid] = 0;
  __syncthreads();
  const int nhl = NLEN + S.ndist;
  for (int t = tid; t < nhl; t += THREADS) atomicAdd(&S.cl_hist[S.hl[t]], 1u);
  __syncthreads();
  huffman_lengths(S.cl_hist, 19, 7, S.cl_len, S.huff, tid);
  if (tid == 0) {
    canonical_codes(lit_len, NLEN, 15, S.lit_code);
    canonical_codes(dist_len, NDIST, 15, S.dist_code);
    canonical_codes(S.cl_len, 19, 7, S.cl_code);
    long long bits = 17 + 3 * 19 + 3 + (long long)S.extra_bits;
    for (int t = 0; t < nhl; ++t) bits += S.cl_len[S.hl[t]];
    for (int t = 0; t < NLEN; ++t) bits += (long long)S.hist[t] * lit_len[t];
    for (int t = 0; t < NDIST; ++t) bits += (long long)S.dhist[t] * dist_len[t];
    S.use_huff = (bits + 7) / 8 + 4 < stored_bytes(n) ? 1 : 0;
  }
  __syncthreads();

  long long data_bytes = 0;
  if (S.use_huff) {
    // ---- the block header (lane 0), then the tokens that start in PER_LANE consecutive positions per lane --------------------
    if (tid == 0) {
      int pos = 0;
      if (first) put_bits(S.out, pos, 0x0178u, 16);   // the zlib header 78 01
      put_bits(S.out, pos, 0u | (2u << 1) | ((unsigned)(NLEN - 257) << 3) | ((unsigned)(S.ndist - 1) << 8) | (15u << 13), 17);   // BFINAL 0, BTYPE 2, HLIT, HDIST, HCLEN 15
      const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      for (int k = 0; k < 19; ++k) put_bits(S.out, pos, S.cl_len[order[k]], 3);
      for (int t = 0; t < nhl; ++t) put_bits(S.out, pos, S.cl_code[S.hl[t]], S.cl_len[S.hl[t]]);   // at most 16 + 17 + 57 + 316 * 7 bits: 72 words
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
      unsigned code[PER_LANE];        // the literal or length code with the length's extra bits, then (<< 21) its bit count
      unsigned dcode[PER_LANE];       // the distance code with its extra bits, then (<< 21) its bit count; 0 for a literal
      unsigned my_bits = 0;
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) {
        code[k] = dcode[k] = 0;
        if (j0 + k < n) {
          const unsigned v = tokens[j0 + k];
          if (v & TOKEN) {
            const int l = v & 511u;
            if (l == 0) {
              const int s = fb[j0 + k];
              code[k] = S.lit_code[s] | ((unsigned)lit_len[s] << 21);
              my_bits += lit_len[s];
            } else {
              const int d = bpp * (int)(((v >> 9) & 63u) + 1);
              const int ls = S.len_sym[l], ds = S.dist_sym[d];
              const unsigned lb = lit_len[257 + ls], db = dist_len[ds];
              code[k] = (S.lit_code[257 + ls] | ((unsigned)(l - S.len_base[ls]) << lb)) | ((lb + S.len_extra[ls]) << 21);
              dcode[k] = (S.dist_code[ds] | ((unsigned)(d - S.dist_base[ds]) << db)) | ((db + S.dist_extra[ds]) << 21);
              my_bits += lb + S.len_extra[ls] + db + S.dist_extra[ds];
            }
          }
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
      {   // (chunk_bits <= 16 * CHUNK: every word index below stays under OUTW)
        const unsigned pos = bitpos + before + incl - my_bits;
        unsigned wi = pos >> 5;
        int nbits = pos & 31;
        unsigned long long acc = 0;
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const unsigned c = half ? dcode[k] : code[k];
            if (c >> 21) {   // at most 21 bits behind fewer than 32 pending ones
              acc |= (unsigned long long)(c & 0x1FFFFFu) << nbits;
              nbits += (int)(c >> 21);
              if (nbits >= 32) {
                atomicOr(&S.out[wi++], (unsigned)acc);
                acc >>= 32;
                nbits -= 32;
              }
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
      put_bits(S.out, pos, S.lit_code[256], lit_len[256]);
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
    // ---- stored blocks: the filtered bytes as they are ------------------------------------------------------------------------
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
      for (int j = tid; j < n; j += THREADS) dst[zh + 5 * (j / MAX_STORED + 1) + j] = fb[j];
    } else if (tid == 0) S.overflow = 1;
  }
  __syncthreads();   // the band's bytes are written: every lane may read them back
  band_crc_and_record(stage, data_bytes, S.overflow != 0, n, S.crc_tab, S.part, S.red, meta, tid);
}

}  // namespace

// the band launch of level 1 (yogo_png_encode_level in png_encode.hip checks the arguments and runs the assembly behind it)
int yogo_png_band_matches_launch(const unsigned char* pixels, int B, int H, int W, int bpp, unsigned char* work, long long work_per,
                                 hipStream_t stream) {
  const int nb = band_count(H);
  hipLaunchKernelGGL(png_band_matches_kernel, dim3(nb, B), dim3(THREADS), 0, stream, pixels, H, W, bpp, work, work_per);
  YOGO_CHECK_LAUNCH("png_encode (bands, level 1)");
  if (yogo_launch_log_enabled()) yogo_launch_log("png_band_matches_kernel | B=%d image=%dx%dx%d bands=%d", B, H, W, bpp, nb);
  return YOGO_OK;
}

// DEFLATE streams (RFC 1951) inflated on the device: what zarr's `zlib` codec stores per chunk (yogo_amd/zarr_feed.py).
// The host takes the zlib wrapper (RFC 1950) off -- yogo_amd/inflate.py: split_zlib checks the 2-byte header and reads the 4-byte
// trailer -- and hands over the stored bytes as they came off the disk plus one table row per stream:
//   table[e] = { src_off, src_len, dst_off, dst_len, adler32 }   (int64 each)
// src_off / src_len: the raw DEFLATE bytes in `src`; dst_off / dst_len: where exactly dst_len inflated bytes belong in `dst`;
// adler32: the trailer's value.  status[e] = 0, or the code of the check that ended the row (the INF_* numbers of
// yogo_amd/inflate.py, whose inflate_status makes the same checks in the same order).
//
// One wavefront (a 64-thread workgroup) per row.  The bit position, the block state and every decoded token are wave-uniform:
// each lane holds one dword of a 256-byte window of the source, three v_readlane fetch the 64 bits at the bit position, and one
// such fetch holds a whole token (15 + 5 + 15 + 13 bits at most).  Runs of literals are decoded several per fetch: every lane looks up the code that
// would start at its own bit offset into the fetch, and the wave follows the chain of code lengths from offset 0 with one
// v_readlane per literal.  A literal goes to the lane of its place in a pending run of up to 64, which the wave
// stores together; a match is copied by the 64 lanes together (wave_copy.h; a distance below the length
// is periodic); a stored block is one wave_copy.
//
// Huffman codes live in LDS, 2.4 KB per wavefront: a primary table of the first 9 bits (literal / length) or 7 bits (distance,
// and the code-length code while a dynamic header is read), entry = symbol << 4 | code length; an entry of 0 sends the lookup to
// the overflow -- the canonical walk over the per-length counts (one lane each) and the symbols sorted by code, which resolves
// codes up to 15 bits and finds the patterns that no code owns.  The wave builds them together: counts by LDS atomics, each
// symbol's place among those of its length by ballots, each primary entry by the same walk on its own bit pattern.  A fixed
// block builds its tables the same way from the fixed lengths.
//
// Code-length sets are held to zlib's rule: an over-subscribed set is refused; an incomplete one too, except a literal / length
// or distance set whose only code has length 1, and a distance set with no code at all (a pattern without a code is then a bad
// symbol when it is met).  The code-length code itself must be complete.
//
// Bounds: every source bit is checked against src_len before it is used -- the window's loads are held to src_len and read as
// zero beyond it, and a token whose bits pass 8 * src_len ends the row; every destination byte is checked against dst_len
// BEFORE it is written, whatever the stream says; a row that does not lie inside the buffers is refused before its first access.
// Every loop consumes at least one source bit per trip or ends the row.
//
// Visibility: as in blosc_lz4.hip -- between a match's loads and the earlier stores of other lanes stands __syncthreads(), the
// workgroup-scope release / acquire pair, which in a workgroup of one wavefront is an ordering constraint alone.  The same
// holds for the Adler-32 pass, which reads the dst_len bytes back once the stream has ended well.
#include "common.h"
#include "wave_copy.h"

namespace {

using yogo_wave::WAVE;
using yogo_wave::wave_copy;
using yogo_wave::wave_copy_periodic;

enum : int { ST_OK = 0, ST_BAD_ROW = 1, ST_BAD_BLOCK_TYPE = 2, ST_STORED_LEN = 3, ST_SOURCE_ENDS = 4, ST_BAD_LENGTHS = 5,
             ST_BAD_SYMBOL = 6, ST_BAD_DISTANCE = 7, ST_PAST_DESTINATION = 8, ST_ENDS_EARLY = 9, ST_ADLER = 10 };

constexpr int LIT_BITS = 9, DIST_BITS = 7, MAX_BITS = 15;
constexpr int MAX_LIT = 288, MAX_DIST = 32, N_CL = 19;
constexpr unsigned ADLER_MOD = 65521;

struct Tables {
  unsigned short lit_tab[1 << LIT_BITS];
  unsigned short dist_tab[1 << DIST_BITS];   // (the code-length code's while a dynamic header is read)
  unsigned short lit_sorted[MAX_LIT];
  unsigned short dist_sorted[MAX_DIST];
  unsigned char lens[MAX_LIT + MAX_DIST];    // literal / length code lengths, then the distance code lengths
  unsigned char cl_lens[32];
  int cnt[16], offs[16];
};

__device__ const unsigned char CL_ORDER[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Source {
  const unsigned char* s;
  long long n, wbase;
  unsigned w;   // this lane's dword of the window: bytes wbase + 4 * lane ..., zero from n on
};

__device__ __forceinline__ int lane_value(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the 64 bits from bit position bp (wave-uniform) on; bits past the end of the source read as zero
__device__ __forceinline__ unsigned long long peek(Source& b, long long bp, int lane) {
  const long long byte = bp >> 3;
  if (byte < b.wbase || byte - b.wbase > 4 * WAVE - 12) {
    b.wbase = byte;
    const long long p = byte + 4 * lane;
    unsigned v = 0;
    if (p + 4 <= b.n) {
      __builtin_memcpy(&v, b.s + p, 4);
    } else {
      for (int k = 0; k < 4; ++k)
        if (p + k < b.n) v |= (unsigned)b.s[p + k] << (8 * k);
    }
    b.w = v;
  }
  const int rel = (int)(byte - b.wbase), i = rel >> 2, sh = ((rel & 3) << 3) | (int)(bp & 7);   // i <= 61, sh <= 31
  const unsigned long long lo = (unsigned)lane_value((int)b.w, i) | ((unsigned long long)(unsigned)lane_value((int)b.w, i + 1) << 32);
  const unsigned long long hi = (unsigned)lane_value((int)b.w, i + 2);
  return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// One code off the low bits of `bits` (wave-uniform) -> its length; sym = its symbol, or -1 (length 15) where no code owns the pattern.
// cv: lane l holds how many codes have length l.
__device__ __forceinline__ int decode(unsigned bits, const unsigned short* tab, int P, const unsigned short* sorted, int cv, int& sym) {
  const int e = uniform(tab[bits & ((1u << P) - 1)]);
  if (e & 15) {
    sym = e >> 4;
    return e & 15;
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= MAX_BITS; ++len) {
    code |= (bits >> (len - 1)) & 1;
    const int c = lane_value(cv, len);
    if (code - c < first) {
      sym = uniform(sorted[index + code - first]);
      return len;
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  sym = -1;
  return MAX_BITS;
}

// The tables of the n code lengths at `lens` (LDS, written before the call) -> false where zlib refuses the set.  codes: this is
// the code-length code (an incomplete one is refused whatever its shape).  cv: see decode.
__device__ bool build(Tables& T, const unsigned char* lens, int n, unsigned short* tab, int P, unsigned short* sorted, bool codes,
                      int& cv, int lane) {
  if (lane < 16) T.cnt[lane] = 0;
  __syncthreads();   // the lengths and the zeroed counts are in place; nobody still reads the tables of the block before
  for (int i = lane; i < n; i += WAVE) {
    const int l = lens[i];
    if (l) atomicAdd(&T.cnt[l], 1);
  }
  __syncthreads();
  cv = lane < 16 ? T.cnt[lane] : 0;
  int left = 1, longest = 0, start = 0;
  for (int len = 1; len <= MAX_BITS; ++len) {
    const int c = lane_value(cv, len);
    left = (left << 1) - c;
    if (left < 0) return false;   // over-subscribed
    if (c) longest = len;
    if (len < lane) start += c;   // lane l: the place in `sorted` of the first symbol of length l
  }
  if (codes ? left > 0 : (left > 0 && longest > 1)) return false;   // incomplete
  if (lane < 16) T.offs[lane] = start;
  __syncthreads();
  for (int base = 0; base < n; base += WAVE) {
    const int i = base + lane, l = i < n ? lens[i] : 0;
    const int o = T.offs[l];
    int rank = 0, total = 0;
    for (int len = 1; len <= MAX_BITS; ++len) {
      if (lane_value(cv, len) == 0) continue;
      const unsigned long long m = __ballot(l == len);
      if (l == len) {
        rank = __popcll(m & ((1ull << lane) - 1));
        total = __popcll(m);
      }
    }
    if (l) sorted[o + rank] = (unsigned short)i;
    if (l && rank == 0) T.offs[l] = o + total;
    __syncthreads();   // the next 64 symbols go behind these
  }
  for (int e = lane; e < (1 << P); e += WAVE) {   // (every lane makes the same number of trips)
    int code = 0, first = 0, index = 0, v = 0;
    for (int len = 1; len <= P; ++len) {
      code |= (e >> (len - 1)) & 1;
      const int c = lane_value(cv, len);
      if (v == 0 && code - c < first) v = ((int)sorted[index + code - first] << 4) | len;
      index += c;
      first = (first + c) << 1;
      code <<= 1;
    }
    tab[e] = (unsigned short)v;
  }
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(WAVE) void inflate_zlib_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                            const long long* __restrict__ table, unsigned char* dst,
                                                            long long dst_bytes, int* __restrict__ status) {
  __shared__ Tables T;
  const int row = blockIdx.x, lane = threadIdx.x;
  const long long* t = table + 5LL * row;
  const long long src_off = t[0], n = t[1], dst_off = t[2], dst_len = t[3], adler = t[4];
  int st = ST_OK;
  if (src_off < 0 || n < 0 || src_off > src_bytes || n > src_bytes - src_off || dst_off < 0 || dst_len < 0 || dst_off > dst_bytes ||
      dst_len > dst_bytes - dst_off) {
    if (lane == 0) status[row] = ST_BAD_ROW;
    return;
  }
  Source B{src + src_off, n, -(1LL << 20), 0u};
  unsigned char* d = dst + dst_off;
  const long long nbits = 8 * n;
  long long bp = 0, dp = 0;   // the source bit position; the destination bytes stored so far
  int nlit = 0, litv = 0;     // the pending literals: lane k holds the one that belongs at d[dp + k]
  int lcv = 0, dcv = 0, ccv = 0;

#define FAIL(code) { st = (code); break; }
#define FLUSH_LITERALS()                        \
  {                                             \
    if (lane < nlit) d[dp + lane] = (unsigned char)litv; \
    dp += nlit;                                 \
    nlit = 0;                                   \
  }

  for (;;) {   // blocks
    if (bp + 3 > nbits) FAIL(ST_SOURCE_ENDS);
    const unsigned hdr = (unsigned)peek(B, bp, lane);
    const int bfinal = hdr & 1, type = (hdr >> 1) & 3;
    bp += 3;
    if (type == 3) FAIL(ST_BAD_BLOCK_TYPE);
    if (type == 0) {
      FLUSH_LITERALS();
      bp = (bp + 7) & ~7LL;
      if (bp + 32 > nbits) FAIL(ST_SOURCE_ENDS);
      const unsigned v = (unsigned)peek(B, bp, lane);
      const long long len = v & 0xFFFF;
      bp += 32;
      if (len != ((v >> 16) ^ 0xFFFF)) FAIL(ST_STORED_LEN);
      if (len > n - (bp >> 3)) FAIL(ST_SOURCE_ENDS);
      if (len > dst_len - dp) FAIL(ST_PAST_DESTINATION);
      wave_copy(d + dp, B.s + (bp >> 3), len, lane);
      dp += len;
      bp += 8 * len;
    } else {
      int nl, nd;
      if (type == 1) {
        nl = MAX_LIT;
        nd = MAX_DIST;
        for (int i = lane; i < MAX_LIT + MAX_DIST; i += WAVE) T.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
      } else {
        if (bp + 14 > nbits) FAIL(ST_SOURCE_ENDS);
        unsigned long long v = peek(B, bp, lane);
        nl = (int)(v & 31) + 257;
        nd = (int)((v >> 5) & 31) + 1;
        const int nc = (int)((v >> 10) & 15) + 4;
        bp += 14;
        if (nl > 286 || nd > 30) FAIL(ST_BAD_LENGTHS);
        if (bp + 3 * nc > nbits) FAIL(ST_SOURCE_ENDS);
        v = peek(B, bp, lane);   // 57 bits at most
        bp += 3 * nc;
        if (lane < 32) T.cl_lens[lane] = 0;
        __syncthreads();
        if (lane < nc) T.cl_lens[CL_ORDER[lane]] = (unsigned char)((v >> (3 * lane)) & 7);
        if (!build(T, T.cl_lens, N_CL, T.dist_tab, DIST_BITS, T.dist_sorted, true, ccv, lane)) FAIL(ST_BAD_LENGTHS);
        const int total = nl + nd;
        int i = 0, prev = 0;
        while (i < total) {
          v = peek(B, bp, lane);
          int sym;
          const int l = decode((unsigned)v, T.dist_tab, DIST_BITS, T.dist_sorted, ccv, sym);
          if (bp + l > nbits) FAIL(ST_SOURCE_ENDS);
          if (sym < 0) FAIL(ST_BAD_LENGTHS);   // (a complete code owns every pattern)
          bp += l;
          v >>= l;
          if (sym < 16) {
            if (lane == 0) T.lens[i] = (unsigned char)sym;
            prev = sym;
            ++i;
            continue;
          }
          if (sym == 16 && i == 0) FAIL(ST_BAD_LENGTHS);
          const int eb = sym == 16 ? 2 : sym == 17 ? 3 : 7, val = sym == 16 ? prev : 0;
          if (bp + eb > nbits) FAIL(ST_SOURCE_ENDS);
          const int rep = (sym == 18 ? 11 : 3) + (int)(v & ((1u << eb) - 1));
          bp += eb;
          if (i + rep > total) FAIL(ST_BAD_LENGTHS);
          for (int j = lane; j < rep; j += WAVE) T.lens[i + j] = (unsigned char)val;
          i += rep;
          prev = val;
        }
        if (st) break;
        __syncthreads();
        if (uniform(T.lens[256]) == 0) FAIL(ST_BAD_LENGTHS);   // no end-of-block code
      }
      if (!build(T, T.lens, nl, T.lit_tab, LIT_BITS, T.lit_sorted, false, lcv, lane)) FAIL(ST_BAD_LENGTHS);
      if (!build(T, T.lens + nl, nd, T.dist_tab, DIST_BITS, T.dist_sorted, false, dcv, lane)) FAIL(ST_BAD_LENGTHS);
      for (;;) {   // tokens
        unsigned long long v = peek(B, bp, lane);
        {
          // A run of literals out of one fetch: lane i looks up the primary entry of the bits from bp + i on -- one LDS access for 56
          // candidate positions -- and the wave follows the chain from position 0, one v_readlane per literal.  Every literal
          // passes the checks of the one-token path below; the first position that is no literal with a primary entry, or fails
          // a check, is left to that path, which names the defect.
          const int ev = T.lit_tab[(unsigned)(v >> lane) & ((1u << LIT_BITS) - 1)];   // (lanes past 64 - LIT_BITS are not consulted)
          int pos = 0;
          while (pos <= 64 - LIT_BITS) {
            const int e = lane_value(ev, pos), el = e & 15;
            if (el == 0 || (e >> 4) >= 256 || bp + pos + el > nbits || dp + nlit >= dst_len) break;
            if (lane == nlit) litv = e >> 4;
            pos += el;
            if (++nlit == WAVE) FLUSH_LITERALS();
          }
          if (pos) {
            bp += pos;
            v = peek(B, bp, lane);
          }
        }
        int sym;
        int l = decode((unsigned)v, T.lit_tab, LIT_BITS, T.lit_sorted, lcv, sym);
        if (bp + l > nbits) FAIL(ST_SOURCE_ENDS);
        if (sym < 0) FAIL(ST_BAD_SYMBOL);
        bp += l;
        v >>= l;
        if (sym < 256) {
          if (dp + nlit >= dst_len) FAIL(ST_PAST_DESTINATION);
          if (lane == nlit) litv = sym;
          if (++nlit == WAVE) FLUSH_LITERALS();
          continue;
        }
        if (sym == 256) break;
        if (sym >= 286) FAIL(ST_BAD_SYMBOL);
        sym -= 257;
        int eb = sym < 8 || sym == 28 ? 0 : (sym >> 2) - 1;
        if (bp + eb > nbits) FAIL(ST_SOURCE_ENDS);
        const long long len = (sym < 8 ? 3 + sym : sym == 28 ? 258 : 3 + ((4 + (sym & 3)) << eb)) + (long long)(v & ((1u << eb) - 1));
        bp += eb;
        v >>= eb;
        l = decode((unsigned)v, T.dist_tab, DIST_BITS, T.dist_sorted, dcv, sym);
        if (bp + l > nbits) FAIL(ST_SOURCE_ENDS);
        if (sym < 0 || sym >= 30) FAIL(ST_BAD_SYMBOL);
        bp += l;
        v >>= l;
        eb = sym < 4 ? 0 : (sym >> 1) - 1;
        if (bp + eb > nbits) FAIL(ST_SOURCE_ENDS);
        const long long dist = (sym < 4 ? 1 + sym : 1 + ((2 + (sym & 1)) << eb)) + (long long)(v & ((1u << eb) - 1));
        bp += eb;
        FLUSH_LITERALS();
        if (dist > dp) FAIL(ST_BAD_DISTANCE);
        if (len > dst_len - dp) FAIL(ST_PAST_DESTINATION);
        __syncthreads();   // everything stored so far (these literals, every earlier token) is visible to the loads below
        if (dist >= len) {
          for (int j = lane; j < len; j += WAVE) d[dp + j] = d[dp - dist + j];   // (at most 258 bytes: five trips)
        } else {
          wave_copy_periodic(d + dp, dist, len, lane);
        }
        dp += len;   // (the next match's barrier stands between these stores and its loads)
      }
      if (st) break;
    }
    if (bfinal) break;
  }
  FLUSH_LITERALS();   // (what came before a defect is stored as well)
#undef FAIL
#undef FLUSH_LITERALS
  if (st == ST_OK && dp != dst_len) st = ST_ENDS_EARLY;
  if (st == ST_OK) {
    // Adler-32 of the dst_len bytes: a = 1 + sum d[i], b = dst_len + sum (dst_len - i) * d[i], both mod 65521
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    unsigned wt = (unsigned)((dst_len - lane) % ADLER_MOD);   // (dst_len - i) mod 65521 for this lane's i (not used where lane >= dst_len)
    for (long long i = lane; i < dst_len; i += WAVE) {
      const unsigned x = d[i];
      s1 += x;
      s2 += (unsigned long long)wt * x;
      wt = wt >= WAVE ? wt - WAVE : wt + ADLER_MOD - WAVE;
    }
    for (int o = WAVE / 2; o; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    const unsigned a = (unsigned)((1 + s1) % ADLER_MOD), b = (unsigned)((dst_len % ADLER_MOD + s2 % ADLER_MOD) % ADLER_MOD);
    if ((((unsigned long long)b << 16) | a) != (unsigned long long)adler) st = ST_ADLER;
  }
  if (lane == 0) status[row] = st;
}

}  // namespace

extern "C" int yogo_inflate_zlib(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                                 long long dst_bytes, int* status, hipStream_t stream) {
  YOGO_CHECK_ARG(src && table && dst && status && src_bytes > 0 && dst_bytes > 0 && n >= 0, "inflate_zlib: bad arguments");
  YOGO_CHECK_ARG(n <= (1 << 24), "inflate_zlib: %d table rows, at most %d per call", n, 1 << 24);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "inflate_zlib: the table must be 8-byte and the status 4-byte aligned");
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(dst) & 15) == 0, "inflate_zlib: the destination must be 16-byte aligned");
  YOGO_CHECK_ARG(src + src_bytes <= dst || dst + dst_bytes <= src, "inflate_zlib: the source and the destination overlap");
  if (n == 0) return YOGO_OK;
  hipLaunchKernelGGL(inflate_zlib_kernel, dim3(n), dim3(WAVE), 0, stream, src, src_bytes, table, dst, dst_bytes, status);
  YOGO_CHECK_LAUNCH("inflate_zlib");
  if (yogo_launch_log_enabled()) yogo_launch_log("inflate_zlib_kernel | rows=%d src=%lld dst=%lld", n, src_bytes, dst_bytes);
  return YOGO_OK;
}

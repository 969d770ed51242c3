// Zstandard frames decoded on the device (yogo_amd/zarr_feed.py, yogo_amd/zstd.py): the blocks of Blosc chunks whose inner codec is
// zstd -- one frame per block -- and the chunks of zarr's `zstd` codec -- one frame per chunk.  The host hands over the stored bytes
// as they came off the disk plus one table row per frame:
//   table[e] = { src_off, src_len, dst_off, dst_len, raw }   (int64 each)
// as yogo_blosc_lz4_decode takes them; raw != 0: the bytes are copied, else they are one frame that decodes to exactly dst_len bytes.
// status[e] = 0, or the code of the check that ended the row (the ZSTD_* numbers of yogo_amd/zstd.py, whose zstd_frame_status makes
// the same checks in the same order).
//
// One wavefront (a 64-thread workgroup) per row.  Everything that steers the decode is wave-uniform: the frame and block headers,
// the bit position of the sequences' backward bitstream, the three FSE states and every decoded sequence; every lane computes
// them, the copies -- literal runs and matches (wave_copy.h, periodic matches included), raw and RLE blocks, RLE literals -- are
// done by the 64 lanes together.  The tables of a wavefront live in LDS and persist from block to block, so that repeat mode and
// treeless literals just keep them: the Huffman decoding table (2^11 entries of 2 bytes), the FSE tables of literal lengths, match
// lengths and offsets (512 / 512 / 256 entries of 4 bytes), the table of the Huffman weights (64 entries) and 1.25 KB of scratch
// for the builders: 10 752 bytes per wavefront.  The 64 lanes build the tables together: a Huffman symbol's first entry comes from
// ballots over the weights (symbols of one weight in symbol order, weights ascending), the entries are filled symbol by symbol by
// all lanes; an FSE table's symbols are spread by rank (lane s owns symbol s: its run of ranks by a prefix sum, the positions
// below the "less than one" symbols by ballots over the walk (j * step) & mask), then every lane walks the table once and numbers
// the states of its symbol.  Huffman-coded literals go to the row's 128 KB of workspace: one lane per stream (four lanes with
// four streams) decodes through a 64-bit container of its backward bitstream, refilled 32 bits at a time; the sequences then
// copy from there.
//
// Bounds: every source bit is checked against the row's src_len (a section's end, which was checked against it) before it is used
// -- a window load never leaves the stream it belongs to, bits below a backward stream's start read as zeros and end the row where
// the format does not expect them; every destination byte is checked against dst_len and every workspace byte against 128 KB before
// it is written, whatever the stream says; a row that does not lie inside the buffers is refused before its first access.  Every
// loop consumes source bits, or counts down a number checked before, or ends the row.
//
// Visibility: as in blosc_lz4.hip, __syncthreads() (one wavefront: an ordering constraint) stands between the stores of one step
// (a table in LDS, literals in the workspace, a sequence's bytes) and the loads of the next.
#include "common.h"
#include "wave_copy.h"

namespace {

using yogo_wave::WAVE;
using yogo_wave::wave_copy;
using yogo_wave::wave_fill;
typedef unsigned char u8;
typedef long long i64;
typedef unsigned long long u64;
// The source, the destination and the workspace are global memory; where a pointer has travelled through a struct the compiler
// no longer knows it and would use FLAT instructions, whose completion the LDS counter waits for as well -- every table lookup
// would wait for the stores before it.  The Huffman loop and the window loads say it.
typedef __attribute__((address_space(1))) const u8 gc8;
typedef __attribute__((address_space(1))) u8 g8;

enum : int { ST_OK = 0, ST_BAD_ROW = 1, ST_SOURCE_ENDS = 2, ST_BAD_MAGIC = 3, ST_UNSUPPORTED_HEADER = 4, ST_CONTENT_SIZE = 5, ST_BAD_BLOCK = 6,
             ST_BAD_LITERALS = 7, ST_BAD_HUFFMAN = 8, ST_BAD_FSE_TABLE = 9, ST_BAD_BITSTREAM = 10, ST_BAD_SEQUENCES = 11, ST_BAD_OFFSET = 12,
             ST_PAST_DESTINATION = 13, ST_ENDS_EARLY = 14, ST_TRAILING = 15 };
constexpr i64 BLOCK_MAX = 1 << 17;
constexpr int HUF_MAX_BITS = 11;

struct FseEntry { unsigned short base; u8 sym, nb; };
struct Tables {
  unsigned short huf[1 << HUF_MAX_BITS];   // symbol | bits << 8
  FseEntry ll[512], ml[512], of[256], hw[64];
  unsigned int symp[128];                  // (builder) the symbol at each table position, 4 per word
  u8 symr[512];                            // (builder) the symbol of each rank
  u8 weights[256];
};

__constant__ signed char LL_DEFAULT[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ signed char ML_DEFAULT[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                           1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ signed char OF_DEFAULT[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
__constant__ unsigned int LL_BASE[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
                                         1024, 2048, 4096, 8192, 16384, 32768, 65536};
__constant__ u8 LL_BITS[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__constant__ unsigned int ML_BASE[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
                                         33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
__constant__ u8 ML_BITS[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                               1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

__device__ __forceinline__ u64 lanes_below(int lane) { return (1ull << lane) - 1; }
__device__ __forceinline__ int popc64(u64 v) { return __popcll(v); }
__device__ __forceinline__ int bit_length(unsigned v) { return 32 - __clz((int)v); }   // v > 0

// the bytes [b, b + 8) of the stream s[0, n), little-endian, zeros outside it
__device__ __forceinline__ u64 window(const u8* s, i64 n, i64 b) {
  gc8* g = (gc8*)s;
  u64 v = 0;
  if (b >= 0 && b + 8 <= n) {
    __builtin_memcpy(&v, g + b, 8);
  } else {
    for (int i = 0; i < 8; ++i)
      if (b + i >= 0 && b + i < n) v |= (u64)g[b + i] << (8 * i);
  }
  return v;
}

// A backward bitstream s[0, n): pos bits are left to read, the next ones just below bit pos.  cont holds the 64 bits from bit cbase.
struct Back {
  const u8* s;
  i64 n, pos, cbase;
  u64 cont;
};

// n > 0 and s[n - 1] != 0 (the caller has checked both)
__device__ __forceinline__ void back_open(Back& b, const u8* s, i64 n) {
  b.s = s;
  b.n = n;
  b.pos = 8 * (n - 1) + bit_length(s[n - 1]) - 1;
  b.cbase = 8 * (n - 8);
  b.cont = window(s, n, n - 8);
}

// the k bits (0 <= k <= 32) below bit `top` of the stream, zeros below its start
__device__ __forceinline__ unsigned back_bits(Back& b, i64 top, int k) {
  if (k == 0) return 0;
  const i64 lo = top - k;
  if (lo < b.cbase || top > b.cbase + 64) {
    const i64 byte0 = ((top + 7) >> 3) - 8;
    b.cbase = 8 * byte0;
    b.cont = window(b.s, b.n, byte0);
  }
  return (unsigned)((b.cont >> (lo - b.cbase)) & ((1ull << k) - 1));
}

// read k bits; below the start zeros are read and pos goes negative (the caller's to judge)
__device__ __forceinline__ unsigned back_read(Back& b, int k) {
  const unsigned v = back_bits(b, b.pos, k);
  b.pos -= k;
  return v;
}

// k <= 24 bits from bit `pos` of the forward bit stream s[lo, hi), zeros past its end
__device__ __forceinline__ unsigned fwd_peek(const u8* s, i64 lo, i64 hi, i64 pos, int k) {
  const i64 b = lo + (pos >> 3);
  unsigned v = 0;
  for (int i = 0; i < 4; ++i)
    if (b + i < hi) v |= (unsigned)s[b + i] << (8 * i);
  return (v >> (pos & 7)) & ((1u << k) - 1);
}

// The decoding table of normalised counts (lane s holds the count of symbol s in f, -1: "less than one"; they sum to 1 << log).
__device__ void fse_build(FseEntry* table, Tables& T, int f, int log, int lane) {
  const int size = 1 << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
  u8* symp = reinterpret_cast<u8*>(T.symp);
  const u64 neg = __ballot(f == -1);
  const int high = size - popc64(neg);
  if (f == -1) symp[size - 1 - popc64(neg & lanes_below(lane))] = (u8)lane;
  const int fp = f > 0 ? f : 0;
  int rank = fp;   // inclusive prefix sum over the lanes
  for (int d = 1; d < WAVE; d <<= 1) {
    const int o = __shfl_up(rank, d);
    if (lane >= d) rank += o;
  }
  rank -= fp;
  for (int i = 0; i < fp && rank + i < 512; ++i) T.symr[rank + i] = (u8)lane;
  __syncthreads();
  int running = 0;
  for (int c = 0; c < size; c += WAVE) {
    const int j = c + lane, p = (j * step) & mask;
    const bool valid = j < size && p < high;
    const u64 m = __ballot(valid);
    if (valid) {
      const int r = running + popc64(m & lanes_below(lane));
      symp[p] = T.symr[r & 511];
    }
    running += popc64(m);
  }
  __syncthreads();
  unsigned nxt = f == -1 ? 1u : (unsigned)fp;
  for (int w = 0; w < (size + 3) / 4; ++w) {
    const unsigned four = T.symp[w];
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * w + k;
      if (i < size && ((four >> (8 * k)) & 255u) == (unsigned)lane && nxt) {
        const unsigned x = nxt++;
        const int nb = log - (bit_length(x) - 1);
        FseEntry e;
        e.base = (unsigned short)((x << nb) - size);
        e.sym = (u8)lane;
        e.nb = (u8)nb;
        table[i] = e;
      }
    }
  }
  __syncthreads();
}

// An FSE table description at s[lo, hi) -> status; the table is built, its accuracy log and the byte after the description given.
__device__ int fse_read(const u8* s, i64 lo, i64 hi, int max_log, int max_sym, FseEntry* table, Tables& T, int lane, int& log_out, i64& end_out) {
  const i64 nbits = 8 * (hi - lo);
  i64 pos = 4;
  if (pos > nbits) return ST_SOURCE_ENDS;
  const int log = 5 + (int)fwd_peek(s, lo, hi, 0, 4);
  if (log > max_log) return ST_BAD_FSE_TABLE;
  int remaining = 1 << log, nsym = 0, mine = 0;
  while (remaining > 0) {
    if (nsym > max_sym) return ST_BAD_FSE_TABLE;
    const int bits = bit_length((unsigned)remaining + 1);
    int val = (int)fwd_peek(s, lo, hi, pos, bits);
    const int lower = (1 << (bits - 1)) - 1, threshold = (1 << bits) - 1 - (remaining + 1);
    if ((val & lower) < threshold) {
      pos += bits - 1;
      val &= lower;
    } else {
      pos += bits;
      if (val > lower) val -= threshold;
    }
    if (pos > nbits) return ST_SOURCE_ENDS;
    const int p = val - 1;
    remaining -= p < 0 ? -p : p;
    if (remaining < 0) return ST_BAD_FSE_TABLE;
    if (lane == nsym) mine = p;
    ++nsym;
    if (p == 0) {
      for (;;) {
        const int rep = (int)fwd_peek(s, lo, hi, pos, 2);
        pos += 2;
        if (pos > nbits) return ST_SOURCE_ENDS;
        nsym += rep;
        if (rep != 3) break;
        if (nsym > max_sym + 1) return ST_BAD_FSE_TABLE;
      }
    }
  }
  if (nsym > max_sym + 1) return ST_BAD_FSE_TABLE;
  fse_build(table, T, mine, log, lane);
  log_out = log;
  end_out = lo + ((pos + 7) >> 3);
  return ST_OK;
}

// The Huffman decoding table from T.weights[0, nsym) (the last weight still to be implied) -> status, the table's log
__device__ int huf_build(Tables& T, int nsym, int lane, int& log_out) {
  int w[4], st[4];
  unsigned total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int sidx = k * WAVE + lane;
    w[k] = sidx < nsym ? T.weights[sidx] : 0;
    st[k] = 0;
    total += w[k] ? 1u << (w[k] - 1) : 0u;
  }
  for (int d = 1; d < WAVE; d <<= 1) total += __shfl_xor(total, d);
  if (total == 0) return ST_BAD_HUFFMAN;
  const int log = bit_length(total);
  if (log > HUF_MAX_BITS) return ST_BAD_HUFFMAN;
  const unsigned left = (1u << log) - total;
  if (left & (left - 1)) return ST_BAD_HUFFMAN;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k * WAVE + lane == nsym) w[k] = bit_length(left);
  int run = 0;
  for (int ww = 1; ww <= log; ++ww) {
    int before = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u64 m = __ballot(w[k] == ww);
      if (w[k] == ww) st[k] = run + ((before + popc64(m & lanes_below(lane))) << (ww - 1));
      before += popc64(m);
    }
    run += before << (ww - 1);
  }
  // (run == 1 << log: the weights' sum; every symbol's entries lie inside the table)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    u64 m = __ballot(w[k] > 0);
    while (m) {
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int ws = __shfl(w[k], l), start = __shfl(st[k], l);
      const int len = 1 << (ws - 1);
      const unsigned short val = (unsigned short)((k * WAVE + l) | ((log + 1 - ws) << 8));
      for (int i = lane; i < len && start + i < (1 << HUF_MAX_BITS); i += WAVE) T.huf[start + i] = val;
    }
  }
  __syncthreads();
  log_out = log;
  return ST_OK;
}

// A Huffman tree description at s[lo, hi) -> status; the table is built, the byte after the description given.
__device__ int huf_read(const u8* s, i64 lo, i64 hi, Tables& T, int lane, int& log_out, i64& end_out) {
  if (lo >= hi) return ST_SOURCE_ENDS;
  const int hb = s[lo];
  int nsym;
  i64 end;
  if (hb >= 128) {
    nsym = hb - 127;
    end = lo + 1 + (nsym + 1) / 2;
    if (end > hi) return ST_SOURCE_ENDS;
    bool big = false;
    for (int i = lane; i < nsym; i += WAVE) {
      const int b = s[lo + 1 + i / 2];
      const int wt = i % 2 == 0 ? b >> 4 : b & 15;
      T.weights[i] = (u8)wt;
      big |= wt > HUF_MAX_BITS;
    }
    if (__ballot(big)) return ST_BAD_HUFFMAN;
  } else {
    end = lo + 1 + hb;
    if (end > hi) return ST_SOURCE_ENDS;
    int log;
    i64 at;
    const int st = fse_read(s, lo + 1, end, 6, 11, T.hw, T, lane, log, at);
    if (st) return st;
    if (at >= end || s[end - 1] == 0) return ST_BAD_BITSTREAM;
    Back b;
    back_open(b, s + at, end - at);
    unsigned s1 = back_read(b, log), s2 = back_read(b, log);
    if (b.pos < 0) return ST_BAD_BITSTREAM;
    nsym = 0;
    for (;;) {   // the two states take turns until one's update passes the start of the stream
      if (nsym >= 254) return ST_BAD_HUFFMAN;
      const FseEntry e1 = T.hw[s1 & 63];
      if (lane == 0) T.weights[nsym] = e1.sym;
      ++nsym;
      s1 = e1.base + back_read(b, e1.nb);
      if (b.pos < 0) {
        if (lane == 0) T.weights[nsym] = T.hw[s2 & 63].sym;
        ++nsym;
        break;
      }
      const FseEntry e2 = T.hw[s2 & 63];
      if (lane == 0) T.weights[nsym] = e2.sym;
      ++nsym;
      s2 = e2.base + back_read(b, e2.nb);
      if (b.pos < 0) {
        if (lane == 0) T.weights[nsym] = T.hw[s1 & 63].sym;
        ++nsym;
        break;
      }
    }
  }
  __syncthreads();
  const int st = huf_build(T, nsym, lane, log_out);
  end_out = end;
  return st;
}

// the bytes [b, b + 4) of the stream s[0, n), little-endian, zeros outside it
__device__ __forceinline__ unsigned window32(gc8* g, int n, int b) {
  unsigned v = 0;
  if (b >= 0 && b + 4 <= n) {
    __builtin_memcpy(&v, g + b, 4);
  } else {
    for (int i = 0; i < 4; ++i)
      if (b + i >= 0 && b + i < n) v |= (unsigned)g[b + i] << (8 * i);
  }
  return v;
}

// One Huffman stream s[0, n) (n <= 128 KB) of `count` symbols into out (this lane alone) -> true when it ends exactly.  One wave
// issues an instruction every few cycles whatever the number of its active lanes, so the loop is kept short: the unread bits stand
// at the top of a 64-bit container (a table index is one shift of its high half, a code is consumed by one shift), 32 bits are
// added below them whenever 32 or fewer are left -- loaded one refill ahead --, and eight symbols go out in one store.
__device__ bool huf_stream(const u8* s, i64 n64, int count, const Tables& T, int log, u8* out) {
  gc8* g = (gc8*)s;
  g8* o = (g8*)out;
  const int n = (int)n64;
  if (n <= 0 || g[n - 1] == 0) return false;
  const int hb = bit_length(g[n - 1]) - 1;         // the marker's place in the last byte
  int pos = 8 * (n - 1) + hb;                      // bits left to read
  u64 cont = window(s, n64, n64 - 8) << (8 - hb);  // the marker and what lies above it are shifted out
  int avail = 56 + hb;                             // bits of the stream in cont (zeros stand in below a stream shorter than that)
  int bp = n - 8;                                  // the bytes below bp are not in cont yet
  unsigned nx = window32(g, n, bp - 4);
  u64 acc = 0;
  int i = 0;
  for (; i < count; ++i) {
    const unsigned e = T.huf[(unsigned)(cont >> 32) >> (32 - log)];
    acc = (acc >> 8) | ((u64)(e & 255u) << 56);
    if ((i & 7) == 7) __builtin_memcpy(o + i - 7, &acc, 8);
    const int nb = (int)(e >> 8);
    cont <<= nb;
    avail -= nb;
    pos -= nb;
    if (pos < 0) break;
    if (avail <= 32) {
      cont |= (u64)nx << (32 - avail);
      avail += 32;
      bp -= 4;
      nx = window32(g, n, bp - 4);
    }
  }
  if (pos != 0 || i != count) return false;
  const int left = count & 7;
  acc >>= 8 * (8 - left) & 63;
  for (int j = 0; j < left; ++j) o[count - left + j] = (u8)(acc >> (8 * j));
  return true;
}

struct Frame {
  const u8* s;   // the row's source
  i64 n;
  u8* d;         // the row's destination
  i64 dst_len, dp;
  u8* work;      // BLOCK_MAX bytes
  int huf_log, ll_log, of_log, ml_log;   // -1: no table yet
  i64 rep0, rep1, rep2;
};

// One compressed block s[lo, hi) -> status
__device__ int block(Frame& F, Tables& T, i64 lo, i64 hi, int lane) {
  const u8* s = F.s;
  // ---- the literals section
  if (lo >= hi) return ST_SOURCE_ENDS;
  const int b0 = s[lo];
  const int ltype = b0 & 3, sf = (b0 >> 2) & 3;
  const u8* lits = F.work;
  i64 regen, q;
  int rle_byte = -1;
  if (ltype < 2) {
    const int hdr = sf == 1 ? 2 : sf == 3 ? 3 : 1;
    if (hdr > hi - lo) return ST_SOURCE_ENDS;
    unsigned v = b0;
    if (hdr > 1) v |= (unsigned)s[lo + 1] << 8;
    if (hdr > 2) v |= (unsigned)s[lo + 2] << 16;
    regen = v >> (hdr == 1 ? 3 : 4);
    if (regen > BLOCK_MAX) return ST_BAD_LITERALS;
    const i64 at = lo + hdr;
    if (ltype == 0) {
      if (regen > hi - at) return ST_SOURCE_ENDS;
      lits = s + at;
      q = at + regen;
    } else {
      if (hi - at < 1) return ST_SOURCE_ENDS;
      rle_byte = s[at];
      q = at + 1;
    }
  } else {
    const int hdr = sf < 2 ? 3 : sf + 2, bits = sf < 2 ? 10 : sf == 2 ? 14 : 18;
    if (hdr > hi - lo) return ST_SOURCE_ENDS;
    u64 v = 0;
    for (int i = 0; i < hdr; ++i) v |= (u64)s[lo + i] << (8 * i);
    regen = (i64)((v >> 4) & ((1u << bits) - 1));
    const i64 comp = (i64)((v >> (4 + bits)) & ((1u << bits) - 1));
    if (regen > BLOCK_MAX) return ST_BAD_LITERALS;
    i64 at = lo + hdr;
    if (comp > hi - at) return ST_SOURCE_ENDS;
    const i64 end = at + comp;
    if (ltype == 2) {
      const int st = huf_read(s, at, end, T, lane, F.huf_log, at);
      if (st) return st;
    } else if (F.huf_log < 0) {
      return ST_BAD_LITERALS;
    }
    bool ok = true;
    if (sf == 0) {
      if (lane == 0) ok = huf_stream(s + at, end - at, (int)regen, T, F.huf_log, F.work);
    } else {
      if (end - at < 6) return ST_SOURCE_ENDS;
      const i64 z0 = s[at] | (s[at + 1] << 8), z1 = s[at + 2] | (s[at + 3] << 8), z2 = s[at + 4] | (s[at + 5] << 8);
      at += 6;
      if (z0 + z1 + z2 > end - at) return ST_BAD_LITERALS;
      const i64 seg = (regen + 3) / 4;
      if (regen < 3 * seg) return ST_BAD_LITERALS;
      if (lane < 4) {
        const i64 from = lane == 0 ? 0 : lane == 1 ? z0 : lane == 2 ? z0 + z1 : z0 + z1 + z2;
        const i64 len = lane == 0 ? z0 : lane == 1 ? z1 : lane == 2 ? z2 : end - at - z0 - z1 - z2;
        ok = huf_stream(s + at + from, len, (int)(lane < 3 ? seg : regen - 3 * seg), T, F.huf_log, F.work + lane * seg);
      }
    }
    if (__ballot(!ok)) return ST_BAD_BITSTREAM;
    q = end;
  }
  __syncthreads();   // the literals in the workspace are visible to the copies below
  // ---- the sequences section
  if (q >= hi) return ST_SOURCE_ENDS;
  const int n0 = s[q];
  int nseq;
  if (n0 == 0) {
    nseq = 0;
    q += 1;
    if (q != hi) return ST_BAD_SEQUENCES;
  } else if (n0 < 128) {
    nseq = n0;
    q += 1;
  } else if (n0 < 255) {
    if (hi - q < 2) return ST_SOURCE_ENDS;
    nseq = ((n0 - 128) << 8) + s[q + 1];
    q += 2;
  } else {
    if (hi - q < 3) return ST_SOURCE_ENDS;
    nseq = s[q + 1] + (s[q + 2] << 8) + 0x7F00;
    q += 3;
  }
  i64 lp = 0;
  u8* d = F.d;
  if (nseq) {
    if (q >= hi) return ST_SOURCE_ENDS;
    const int modes = s[q];
    q += 1;
    if (modes & 3) return ST_BAD_SEQUENCES;
    for (int t = 0; t < 3; ++t) {   // literal lengths, offsets, match lengths
      const int mode = (modes >> (6 - 2 * t)) & 3;
      FseEntry* table = t == 0 ? T.ll : t == 1 ? T.of : T.ml;
      int& log = t == 0 ? F.ll_log : t == 1 ? F.of_log : F.ml_log;
      const int max_log = t == 1 ? 8 : 9, max_sym = t == 0 ? 35 : t == 1 ? 31 : 52;
      if (mode == 0) {
        const int cnt = t == 0 ? 36 : t == 1 ? 29 : 53;
        const signed char* def = t == 0 ? LL_DEFAULT : t == 1 ? OF_DEFAULT : ML_DEFAULT;
        log = t == 1 ? 5 : 6;
        fse_build(table, T, lane < cnt ? def[lane] : 0, log, lane);
      } else if (mode == 1) {
        if (q >= hi) return ST_SOURCE_ENDS;
        const int sym = s[q];
        if (sym > max_sym) return ST_BAD_FSE_TABLE;
        if (lane == 0) {
          FseEntry e;
          e.base = 0;
          e.sym = (u8)sym;
          e.nb = 0;
          table[0] = e;
        }
        __syncthreads();
        log = 0;
        q += 1;
      } else if (mode == 2) {
        const int st = fse_read(s, q, hi, max_log, max_sym, table, T, lane, log, q);
        if (st) return st;
      } else if (log < 0) {
        return ST_BAD_FSE_TABLE;
      }
    }
    if (q >= hi || s[hi - 1] == 0) return ST_BAD_BITSTREAM;
    Back b;
    back_open(b, s + q, hi - q);
    unsigned ll_s = back_read(b, F.ll_log), of_s = back_read(b, F.of_log), ml_s = back_read(b, F.ml_log);
    if (b.pos < 0) return ST_BAD_BITSTREAM;
    for (int i = 0; i < nseq; ++i) {
      const FseEntry le = T.ll[ll_s & 511], oe = T.of[of_s & 255], me = T.ml[ml_s & 511];
      const int ofc = oe.sym & 31, mlc = me.sym < 53 ? me.sym : 52, llc = le.sym < 36 ? le.sym : 35;   // (the builders hold the symbols to these limits)
      const u64 ofv = (1ull << ofc) + back_read(b, ofc);
      const i64 ml = (i64)ML_BASE[mlc] + back_read(b, ML_BITS[mlc]);
      const i64 ll = (i64)LL_BASE[llc] + back_read(b, LL_BITS[llc]);
      if (i != nseq - 1) {
        ll_s = le.base + back_read(b, le.nb);
        ml_s = me.base + back_read(b, me.nb);
        of_s = oe.base + back_read(b, oe.nb);
      }
      if (b.pos < 0) return ST_BAD_BITSTREAM;
      i64 off;
      if (ofv > 3) {
        off = (i64)ofv - 3;
        F.rep2 = F.rep1;
        F.rep1 = F.rep0;
        F.rep0 = off;
      } else {
        const int idx = (int)ofv - 1 + (ll == 0 ? 1 : 0);
        if (idx == 0) {
          off = F.rep0;
        } else if (idx == 1) {
          off = F.rep1;
          F.rep1 = F.rep0;
          F.rep0 = off;
        } else if (idx == 2) {
          off = F.rep2;
          F.rep2 = F.rep1;
          F.rep1 = F.rep0;
          F.rep0 = off;
        } else {
          off = F.rep0 - 1;
          F.rep2 = F.rep1;
          F.rep1 = F.rep0;
          F.rep0 = off;
        }
      }
      if (ll > regen - lp) return ST_BAD_SEQUENCES;
      if (ll > F.dst_len - F.dp) return ST_PAST_DESTINATION;
      if (rle_byte >= 0) wave_fill(d + F.dp, (u8)rle_byte, ll, lane);
      else wave_copy(d + F.dp, lits + lp, ll, lane);
      lp += ll;
      F.dp += ll;
      if (off <= 0 || off > F.dp) return ST_BAD_OFFSET;
      if (ml > F.dst_len - F.dp) return ST_PAST_DESTINATION;
      __syncthreads();   // everything stored so far (these literals, every earlier sequence and block) is visible to the loads below
      if (off >= ml) wave_copy(d + F.dp, d + F.dp - off, ml, lane);
      else yogo_wave::wave_copy_periodic(d + F.dp, off, ml, lane);
      F.dp += ml;
    }
    if (b.pos != 0) return ST_BAD_BITSTREAM;
  }
  const i64 rest = regen - lp;
  if (rest > F.dst_len - F.dp) return ST_PAST_DESTINATION;
  if (rle_byte >= 0) wave_fill(d + F.dp, (u8)rle_byte, rest, lane);
  else wave_copy(d + F.dp, lits + lp, rest, lane);
  F.dp += rest;
  return ST_OK;
}

// One frame -> status
__device__ int frame(Frame& F, Tables& T, int lane) {
  const u8* s = F.s;
  const i64 n = F.n;
  if (n < 4) return ST_SOURCE_ENDS;
  if ((s[0] | (s[1] << 8) | (s[2] << 16) | ((unsigned)s[3] << 24)) != 0xFD2FB528u) return ST_BAD_MAGIC;
  if (n < 5) return ST_SOURCE_ENDS;
  const int fhd = s[4];
  i64 p = 5;
  if ((fhd & 0x08) || (fhd & 0x03)) return ST_UNSUPPORTED_HEADER;
  const int single = (fhd >> 5) & 1, checksum = (fhd >> 2) & 1, fcs_flag = fhd >> 6;
  if (!single) {
    if (p >= n) return ST_SOURCE_ENDS;
    p += 1;   // the window descriptor: not enforced
  }
  const int fcs_bytes = fcs_flag == 0 ? single : 1 << fcs_flag;
  if (fcs_bytes) {
    if (n - p < fcs_bytes) return ST_SOURCE_ENDS;
    u64 fcs = 0;
    for (int i = 0; i < fcs_bytes; ++i) fcs |= (u64)s[p + i] << (8 * i);
    if (fcs_bytes == 2) fcs += 256;
    p += fcs_bytes;
    if (fcs != (u64)F.dst_len) return ST_CONTENT_SIZE;
  }
  for (;;) {
    if (n - p < 3) return ST_SOURCE_ENDS;
    const unsigned bh = s[p] | (s[p + 1] << 8) | (s[p + 2] << 16);
    p += 3;
    const int last = bh & 1, btype = (bh >> 1) & 3;
    const i64 size = bh >> 3;
    if (btype == 3 || size > BLOCK_MAX) return ST_BAD_BLOCK;
    if (btype == 0) {
      if (size > n - p) return ST_SOURCE_ENDS;
      if (size > F.dst_len - F.dp) return ST_PAST_DESTINATION;
      wave_copy(F.d + F.dp, s + p, size, lane);
      F.dp += size;
      p += size;
    } else if (btype == 1) {
      if (n - p < 1) return ST_SOURCE_ENDS;
      if (size > F.dst_len - F.dp) return ST_PAST_DESTINATION;
      wave_fill(F.d + F.dp, s[p], size, lane);
      F.dp += size;
      p += 1;
    } else {
      if (size > n - p) return ST_SOURCE_ENDS;
      const int st = block(F, T, p, p + size, lane);
      if (st) return st;
      p += size;
    }
    if (last) break;
  }
  if (checksum) {
    if (n - p < 4) return ST_SOURCE_ENDS;
    p += 4;   // present, not verified
  }
  if (p != n) return ST_TRAILING;
  if (F.dp != F.dst_len) return ST_ENDS_EARLY;
  return ST_OK;
}

__global__ __launch_bounds__(WAVE) void zstd_decode_kernel(const u8* __restrict__ src, i64 src_bytes, const i64* __restrict__ table, u8* dst,
                                                           i64 dst_bytes, int* __restrict__ status, u8* work, i64 work_bytes) {
  __shared__ Tables T;
  const int e = blockIdx.x, lane = threadIdx.x;
  const i64* t = table + 5LL * e;
  const i64 src_off = t[0], n = t[1], dst_off = t[2], dst_len = t[3], raw = t[4];
  int st;
  if (src_off < 0 || n < 0 || src_off > src_bytes || n > src_bytes - src_off || dst_off < 0 || dst_len < 0 || dst_off > dst_bytes ||
      dst_len > dst_bytes - dst_off || (raw && n != dst_len) || (e + 1LL) * BLOCK_MAX > work_bytes) {
    st = ST_BAD_ROW;
  } else if (raw) {
    wave_copy(dst + dst_off, src + src_off, n, lane);
    st = ST_OK;
  } else {
    Frame F;
    F.s = src + src_off;
    F.n = n;
    F.d = dst + dst_off;
    F.dst_len = dst_len;
    F.dp = 0;
    F.work = work + e * BLOCK_MAX;
    F.huf_log = F.ll_log = F.of_log = F.ml_log = -1;
    F.rep0 = 1;
    F.rep1 = 4;
    F.rep2 = 8;
    st = frame(F, T, lane);
  }
  if (lane == 0) status[e] = st;
}

}  // namespace

extern "C" int yogo_zstd_work_bytes(int n, size_t* bytes) {
  YOGO_CHECK_ARG(bytes && n >= 0 && n <= (1 << 20), "zstd_work_bytes: bad arguments");
  *bytes = (size_t)(n > 0 ? n : 1) * (size_t)BLOCK_MAX;
  return YOGO_OK;
}

extern "C" int yogo_zstd_decode(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                                long long dst_bytes, int* status, unsigned char* work, long long work_bytes, hipStream_t stream) {
  YOGO_CHECK_ARG(src && table && dst && status && work && src_bytes > 0 && dst_bytes > 0 && n >= 0, "zstd_decode: bad arguments");
  YOGO_CHECK_ARG(n <= (1 << 20), "zstd_decode: %d table rows, at most %d per call", n, 1 << 20);
  YOGO_CHECK_ARG(work_bytes >= (long long)n * BLOCK_MAX, "zstd_decode: a workspace of %lld bytes for %d rows, %lld needed (yogo_zstd_work_bytes)",
                 work_bytes, n, (long long)n * BLOCK_MAX);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "zstd_decode: the table must be 8-byte and the status 4-byte aligned");
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(work) & 15) == 0,
                 "zstd_decode: the destination and the workspace must be 16-byte aligned");
  YOGO_CHECK_ARG(src + src_bytes <= dst || dst + dst_bytes <= src, "zstd_decode: the source and the destination overlap");
  YOGO_CHECK_ARG((work + work_bytes <= dst || dst + dst_bytes <= work) && (work + work_bytes <= src || src + src_bytes <= work),
                 "zstd_decode: the workspace overlaps the source or the destination");
  if (n == 0) return YOGO_OK;
  hipLaunchKernelGGL(zstd_decode_kernel, dim3(n), dim3(WAVE), 0, stream, src, src_bytes, table, dst, dst_bytes, status, work, work_bytes);
  YOGO_CHECK_LAUNCH("zstd_decode");
  if (yogo_launch_log_enabled()) yogo_launch_log("zstd_decode_kernel | rows=%d src=%lld dst=%lld", n, src_bytes, dst_bytes);
  return YOGO_OK;
}

// Baseline JPEG files (ITU-T T.81: SOF0 / SOF1, Huffman, 8 bits, one interleaved scan) decoded on the device to the planes
// `read_image` gives: what the PNG batch steps (yogo_amd/png_batch.py) launch over a chunk's JPEG files in front of the unpack kernel.
// The host parses the marker segments (yogo_amd/jpeg.py: parse_jpeg, table_row) and hands over the files as they came off the
// disk plus one table row per file, 18 int64:
//   { src_off, src_len, dst_off, dst_len, H, W, components | luma h << 8 | luma v << 16, restart interval, scan_off,
//     quant[3], dc[3], ac[3] }
// src_off / src_len: the file's bytes in `src`, any alignment; dst_off / dst_len: where its C_out * H * W output bytes belong in
// `dst`; scan_off: where the entropy-coded bytes start; quant[c]: 2 * (offset of component c's 64 quantiser entries) + (1 where
// they are 16-bit); dc[c] / ac[c]: the offsets of the 16 counts of component c's DHT tables; all offsets from the file's first
// byte, -1 for a table the file never defined.  THE KERNEL READS DQT / DHT FROM THE FILE at these offsets -- no descriptor blob is
// uploaded --, and trusts nothing: every offset is held to the file before it is used.
// status[e] = 0, or the code of the check that ended the row (the JPG_* numbers of yogo_amd/jpeg.py, whose jpeg_status makes the
// same checks in the same order).
//
// One wavefront (a 64-thread workgroup) per file, band by band; a band is one MCU row (8 image rows; 16 for 4:2:0).
//   serial part   -- bits, codes, extra bits, DC prediction, byte unstuffing, restart markers -- wave-uniform: every lane runs it on
//                 the same values, lane 0 stores.  The source passes through a 1 KB window in LDS that the 64 lanes load together.
//                 Huffman codes: a primary table of the first 9 bits in LDS (symbol << 5 | length), longer codes by libjpeg's
//                 maxcode walk; built by the lanes together, one symbol per lane.  A coefficient is dequantised as it is decoded
//                 and held to +-2047 (JPG_COEF_RANGE: more than 8-bit samples give; beyond it libjpeg's IDCTs part ways).
//   parallel part -- one block per lane: the 13-bit LLM IDCT of jidctint.c (columns, 16-bit saturation, rows, +128, clamp) in registers.
//                 Grey goes from the registers to dst; colour writes its samples over the block's coefficients in LDS, then one
//                 lane per pixel upsamples (jdsample.c's fancy h2v1 / h2v2, replication at two chroma columns or fewer, as
//                 jinit_upsampler chooses), converts (jdcolor.c, 16-bit fixed point) and stores R, G, B planes or PIL's luma of
//                 them.  4:2:0 needs the chroma row above / below: a band emits the last row of the band before it (kept in
//                 LDS: one luma row, one row of each chroma) and holds back its own last row unless it is the frame's last band.
// Two instantiations, launched one after the other over the same table: <1> serves the grey rows (16.3 KB of coefficients), <3> the
// colour rows (48.8 KB); each leaves the other's rows alone.  Frames wider than MAX_W = 1040 are refused (JPG_BAD_ROW): the host's
// predicate keeps them.
//
// Bounds: a row that does not lie inside src / dst, or whose frame the kernel does not take, is refused before its first access;
// every source byte is fetched through the window, whose loads are held to src_len; every destination byte is y < H, x < W of
// a frame with C_out * H * W == dst_len.  Every loop consumes source bits or ends the row.
#include "common.h"

namespace {

constexpr int WAVE = 64;
enum : int { ST_OK = 0, ST_BAD_ROW = 1, ST_NO_TABLE = 2, ST_BAD_HUFFMAN = 3, ST_SOURCE_ENDS = 4, ST_BAD_CODE = 5, ST_BAD_CATEGORY = 6,
             ST_RUN_PAST_63 = 7, ST_BAD_MARKER = 8, ST_NO_EOI = 9, ST_MCU_COUNT = 10, ST_COEF_RANGE = 11 };
constexpr int MAX_W = 1040, COEF_MAX = 2047, COLS = 18, WIN = 1024, LOOK_BITS = 9, STOP_END = -1;

__device__ const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huffman {
  unsigned short look[1 << LOOK_BITS];
  unsigned char vals[256];
  int maxcode[17], valoff[17];   // per code length: the largest code (-1: none), index of its first symbol minus its first code
};

template <int NC>
struct Shared {
  short coef[(NC == 1 ? MAX_W / 8 : 3 * MAX_W / 8) * 64];
  Huffman dc[NC], ac[NC];
  unsigned short quant[NC][64];   // zigzag order, as the file stores them
  unsigned win[WIN / 4];
  unsigned char keep_y[NC == 1 ? 4 : MAX_W], keep_c[2][NC == 1 ? 4 : MAX_W / 2];
};

__device__ __forceinline__ int lane_value(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

struct Reader {
  const unsigned char* s;   // the file
  long long n, pos, wbase;  // its length; the next byte to load; which bytes the window holds
  unsigned long long acc;   // the next bits, from bit 63 down
  int nb, stop;             // real bits in acc; 0, STOP_END (the source ended) or the marker the loads stopped in front of
};

// byte p < n of the file (wave-uniform p)
__device__ __forceinline__ int source_byte(Reader& R, unsigned* win, long long p, int lane) {
  if (p < R.wbase || p >= R.wbase + WIN) {
    __syncthreads();   // nobody still reads the window
    R.wbase = p & ~3LL;
#pragma unroll
    for (int k = 0; k < WIN / 4 / WAVE; ++k) {
      const long long q = R.wbase + 4 * (k * WAVE + lane);
      unsigned v = 0;
      if (q + 4 <= R.n) {
        __builtin_memcpy(&v, R.s + q, 4);
      } else {
        for (int j = 0; j < 4; ++j)
          if (q + j < R.n) v |= (unsigned)R.s[q + j] << (8 * j);
      }
      win[k * WAVE + lane] = v;
    }
    __syncthreads();
  }
  const int rel = (int)(p - R.wbase);
  return (win[rel >> 2] >> (8 * (rel & 3))) & 0xFF;
}

// at least 49 real bits in acc, unless the source ends or a marker stands in front of them
__device__ __forceinline__ void fill(Reader& R, unsigned* win, int lane) {
  while (R.nb <= 48 && R.stop == 0) {
    if (R.pos >= R.n) {
      R.stop = STOP_END;
      break;
    }
    const int b = source_byte(R, win, R.pos, lane);
    if (b == 0xFF) {
      if (R.pos + 1 >= R.n) {
        R.stop = STOP_END;
        break;
      }
      const int b2 = source_byte(R, win, R.pos + 1, lane);
      if (b2 != 0) {
        R.stop = b2;
        break;
      }
      R.pos += 2;
    } else {
      R.pos += 1;
    }
    R.acc |= (unsigned long long)b << (56 - R.nb);
    R.nb += 8;
  }
}

__device__ __forceinline__ int ended(const Reader& R) {
  return R.stop == STOP_END ? ST_SOURCE_ENDS : R.stop == 0xD9 ? ST_MCU_COUNT : ST_BAD_MARKER;
}

// one code off the front of acc -> its length (0: no code owns the pattern), sym = its symbol
__device__ __forceinline__ int huffman_decode(const Huffman& T, unsigned long long acc, int& sym) {
  const int peek = (int)(acc >> 48);
  const int e = T.look[peek >> (16 - LOOK_BITS)];
  if (e) {
    sym = e >> 5;
    return e & 31;
  }
  for (int l = LOOK_BITS + 1; l <= 16; ++l) {
    const int code = peek >> (16 - l);
    if (code <= T.maxcode[l]) {
      sym = T.vals[(code + T.valoff[l]) & 255];
      return l;
    }
  }
  sym = 0;
  return 0;
}

// the DHT table whose 16 counts stand at file offset `off` -> T; 0 or the status
__device__ int huffman_build(Huffman& T, const unsigned char* s, long long n, long long off, int lane) {
  if (off < 0 || off > n - 16) return ST_NO_TABLE;
  const int cnt = lane < 16 ? s[off + lane] : 0;
  int total = 0;
  for (int l = 0; l < 16; ++l) total += lane_value(cnt, l);
  if (off + 16 + total > n) return ST_NO_TABLE;
  if (total > 256) return ST_BAD_HUFFMAN;
  __syncthreads();   // nobody still reads the table of the file before
  int code = 0, k = 0, bad = 0;
  const int i = lane;   // (a table has at most 256 symbols: four per lane, below)
  int codes[4] = {0, 0, 0, 0}, lens[4] = {0, 0, 0, 0};
  for (int l = 1; l <= 16; ++l) {
    const int c = lane_value(cnt, l - 1);
    if (c && code + c >= (1 << l)) bad = 1;
    if (lane == 0) {
      T.maxcode[l] = c ? code + c - 1 : -1;
      T.valoff[l] = k - code;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = i + j * WAVE;
      if (idx >= k && idx < k + c) {
        codes[j] = code + (idx - k);
        lens[j] = l;
      }
    }
    k += c;
    code = (code + c) << 1;
  }
  if (bad) return ST_BAD_HUFFMAN;
  for (int e = lane; e < (1 << LOOK_BITS); e += WAVE) T.look[e] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = i + j * WAVE;
    if (idx < total) {
      const int sym = s[off + 16 + idx];
      T.vals[idx] = (unsigned char)sym;
      if (lens[j] <= LOOK_BITS) {
        const int sh = LOOK_BITS - lens[j];
        for (int f = 0; f < (1 << sh); ++f) T.look[(codes[j] << sh) + f] = (unsigned short)((sym << 5) | lens[j]);
      }
    }
  }
  __syncthreads();
  return ST_OK;
}

// jidctint.c's one-dimensional pass (13-bit constants) over eight values, descaled by `shift` with rounding; unsigned: the sums wrap
__device__ __forceinline__ void idct_pass(int (&v)[8], int shift) {
  const unsigned i0 = v[0], i1 = v[1], i2 = v[2], i3 = v[3], i4 = v[4], i5 = v[5], i6 = v[6], i7 = v[7];
  unsigned z1 = (i2 + i6) * 4433u;
  const unsigned t2 = z1 + i6 * (unsigned)-15137, t3 = z1 + i2 * 6270u;
  const unsigned t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  z1 = i7 + i1;
  unsigned z2 = i5 + i3, z3 = i7 + i3, z4 = i5 + i1;
  const unsigned z5 = (z3 + z4) * 9633u;
  unsigned o0 = i7 * 2446u, o1 = i5 * 16819u, o2 = i3 * 25172u, o3 = i1 * 12299u;
  z1 *= (unsigned)-7373;
  z2 *= (unsigned)-20995;
  z3 = z3 * (unsigned)-16069 + z5;
  z4 = z4 * (unsigned)-3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  const unsigned half = 1u << (shift - 1);
  v[0] = (int)(t10 + o3 + half) >> shift;
  v[7] = (int)(t10 - o3 + half) >> shift;
  v[1] = (int)(t11 + o2 + half) >> shift;
  v[6] = (int)(t11 - o2 + half) >> shift;
  v[2] = (int)(t12 + o1 + half) >> shift;
  v[5] = (int)(t12 - o1 + half) >> shift;
  v[3] = (int)(t13 + o0 + half) >> shift;
  v[4] = (int)(t13 - o0 + half) >> shift;
}

__device__ __forceinline__ int clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the block of 64 dequantised coefficients at c (natural order) -> x: its 64 samples, 0 .. 255
__device__ __forceinline__ void idct_block(const short* c, int (&x)[64]) {
  const int4* c4 = reinterpret_cast<const int4*>(c);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int4 q = c4[r];
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[r * 8 + 2 * j] = (short)(w[j] & 0xFFFF);
      x[r * 8 + 2 * j + 1] = w[j] >> 16;
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = x[r * 8 + col];
    idct_pass(v, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r * 8 + col] = clamp(v[r], -32768, 32767);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int v[8];
#pragma unroll
    for (int col = 0; col < 8; ++col) v[col] = x[r * 8 + col];
    idct_pass(v, 18);
#pragma unroll
    for (int col = 0; col < 8; ++col) x[r * 8 + col] = clamp(v[col] + 128, 0, 255);
  }
}

struct Frame {
  int H, W, hs, vs, mx, my, bpm, cw, ch, C_out;
  unsigned char* d;
};

// colour: the samples of the band as the IDCT left them, 64 bytes at the start of every block's 128
template <int NC>
__device__ __forceinline__ int luma_at(const Shared<NC>& S, const Frame& F, int r, int x) {   // r: row of the band
  const int m = x / (8 * F.hs), k = (r >> 3) * F.hs + ((x >> 3) & (F.hs - 1));
  return reinterpret_cast<const unsigned char*>(S.coef)[(m * F.bpm + k) * 128 + (r & 7) * 8 + (x & 7)];
}
// chroma c at row cy of the frame's chroma plane, column cx; band_c0: the band's first chroma row (the row above it is kept)
template <int NC>
__device__ __forceinline__ int chroma_at(const Shared<NC>& S, const Frame& F, int c, int cy, int cx, int band_c0) {
  if (cy < band_c0) return S.keep_c[c][cx];
  return reinterpret_cast<const unsigned char*>(S.coef)[((cx >> 3) * F.bpm + F.hs * F.vs + c) * 128 + (cy - band_c0) * 8 + (cx & 7)];
}

// chroma c upsampled at pixel (row y of the frame, column x), minus nothing: 0 .. 255
template <int NC>
__device__ __forceinline__ int chroma_up(const Shared<NC>& S, const Frame& F, int c, int y, int x, int band_c0) {
  if (F.hs == 1) return chroma_at(S, F, c, y, x, band_c0);
  const int cx = x >> 1;
  if (F.vs == 1) {
    const int v = chroma_at(S, F, c, y, cx, band_c0);
    if (F.cw <= 2) return v;
    if (x & 1) return cx == F.cw - 1 ? v : (3 * v + chroma_at(S, F, c, y, cx + 1, band_c0) + 2) >> 2;
    return cx == 0 ? v : (3 * v + chroma_at(S, F, c, y, cx - 1, band_c0) + 1) >> 2;
  }
  const int near = y >> 1, far = clamp((y & 1) ? near + 1 : near - 1, 0, F.ch - 1);
  if (F.cw <= 2) return chroma_at(S, F, c, near, cx, band_c0);
  const int s = 3 * chroma_at(S, F, c, near, cx, band_c0) + chroma_at(S, F, c, far, cx, band_c0);
  if (x & 1) {
    if (cx == F.cw - 1) return (4 * s + 7) >> 4;
    return (3 * s + 3 * chroma_at(S, F, c, near, cx + 1, band_c0) + chroma_at(S, F, c, far, cx + 1, band_c0) + 7) >> 4;
  }
  if (cx == 0) return (4 * s + 8) >> 4;
  return (3 * s + 3 * chroma_at(S, F, c, near, cx - 1, band_c0) + chroma_at(S, F, c, far, cx - 1, band_c0) + 8) >> 4;
}

// row y of the frame, its luma at row r of the band (r < 0: the kept row)
template <int NC>
__device__ __forceinline__ void emit_row(const Shared<NC>& S, const Frame& F, int y, int r, int band_c0, int lane) {
  const long long plane = (long long)F.H * F.W, at = (long long)y * F.W;
  for (int x = lane; x < F.W; x += WAVE) {
    const int yy = r < 0 ? S.keep_y[x] : luma_at(S, F, r, x);
    const int cb = chroma_up(S, F, 0, y, x, band_c0) - 128, cr = chroma_up(S, F, 1, y, x, band_c0) - 128;
    const int R = clamp(yy + ((91881 * cr + 32768) >> 16), 0, 255);
    const int G = clamp(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
    const int B = clamp(yy + ((116130 * cb + 32768) >> 16), 0, 255);
    if (F.C_out == 3) {
      F.d[at + x] = (unsigned char)R;
      F.d[plane + at + x] = (unsigned char)G;
      F.d[2 * plane + at + x] = (unsigned char)B;
    } else {
      F.d[at + x] = (unsigned char)((19595 * R + 38470 * G + 7471 * B + 0x8000) >> 16);
    }
  }
}

template <int NC>
__global__ __launch_bounds__(WAVE) void jpeg_decode_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                           const long long* __restrict__ table, unsigned char* dst, long long dst_bytes,
                                                           int C_out, int* __restrict__ status) {
  __shared__ Shared<NC> S;
  const int row = blockIdx.x, lane = threadIdx.x;
  const long long* t = table + (long long)COLS * row;
  const long long src_off = t[0], n = t[1], dst_off = t[2], dst_len = t[3], H64 = t[4], W64 = t[5], fmt = t[6], ri64 = t[7], scan_off = t[8];
  const int nc = (int)(fmt & 0xFF);
  if ((nc == 3) != (NC == 3)) return;   // the other instantiation's row
  const int hs = (int)((fmt >> 8) & 0xFF), vs = (int)((fmt >> 16) & 0xFF);
  if (src_off < 0 || n < 0 || src_off > src_bytes || n > src_bytes - src_off || dst_off < 0 || dst_len < 0 || dst_off > dst_bytes ||
      dst_len > dst_bytes - dst_off || (fmt >> 24) != 0 || (nc != 1 && nc != 3) || H64 < 1 || H64 > 65535 || W64 < 1 || W64 > MAX_W ||
      dst_len != C_out * H64 * W64 || ri64 < 0 || ri64 > 65535 || scan_off < 0 || scan_off > n ||
      (NC == 3 ? !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) : false)) {
    if (lane == 0) status[row] = ST_BAD_ROW;
    return;
  }
  const unsigned char* s = src + src_off;
  Frame F;
  F.H = (int)H64;
  F.W = (int)W64;
  F.hs = NC == 1 ? 1 : hs;
  F.vs = NC == 1 ? 1 : vs;
  F.mx = (F.W + 8 * F.hs - 1) / (8 * F.hs);
  F.my = (F.H + 8 * F.vs - 1) / (8 * F.vs);
  F.bpm = NC == 1 ? 1 : F.hs * F.vs + 2;
  F.cw = (F.W + F.hs - 1) / F.hs;
  F.ch = (F.H + F.vs - 1) / F.vs;
  F.C_out = C_out;
  F.d = dst + dst_off;
  const int ri = (int)ri64;
  int st = ST_OK;

  // the tables, from the file
  for (int c = 0; c < NC && st == ST_OK; ++c) {
    const long long q = t[9 + c];
    const long long qo = q >> 1;
    const int wide = (int)(q & 1);
    if (q < 0 || qo > n - (wide ? 128 : 64)) {
      st = ST_NO_TABLE;
      break;
    }
    S.quant[c][lane] = wide ? (unsigned short)((s[qo + 2 * lane] << 8) | s[qo + 2 * lane + 1]) : (unsigned short)s[qo + lane];
  }
  for (int c = 0; c < NC && st == ST_OK; ++c) {
    st = huffman_build(S.dc[c], s, n, t[12 + c], lane);
    if (st == ST_OK) st = huffman_build(S.ac[c], s, n, t[15 + c], lane);
  }
  if (st != ST_OK) {
    if (lane == 0) status[row] = st;
    return;
  }

  Reader R{s, n, scan_off, -(1LL << 40), 0ull, 0, 0};
  int pred[NC];
  for (int c = 0; c < NC; ++c) pred[c] = 0;
  int mcu = 0, togo = ri, expected = 0;
  const int band_blocks = F.mx * F.bpm;

#define FAIL(code) { st = (code); goto done; }
  for (int band = 0; band < F.my; ++band) {
    __syncthreads();   // the band before is stored
    {
      int4* z = reinterpret_cast<int4*>(S.coef);
      for (int i = lane; i < band_blocks * 8; i += WAVE) z[i] = make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    for (int m = 0; m < F.mx; ++m, ++mcu) {
      if (ri && mcu) {
        if (togo == 0) {   // a restart marker stands here
          fill(R, S.win, lane);
          if (R.nb >= 8) FAIL(ST_BAD_MARKER);
          if (R.stop == STOP_END) FAIL(ST_SOURCE_ENDS);
          if (R.stop != 0xD0 + expected) FAIL(ST_BAD_MARKER);
          expected = (expected + 1) & 7;
          R.pos += 2;
          R.acc = 0;
          R.nb = 0;
          R.stop = 0;
          for (int c = 0; c < NC; ++c) pred[c] = 0;
          togo = ri;
        }
      }
      --togo;
      int blk = m * F.bpm;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int nb_c = (NC == 3 && c == 0) ? F.hs * F.vs : 1;
        for (int b = 0; b < nb_c; ++b, ++blk) {
          short* out = S.coef + blk * 64;
          int k = 0;
          while (k < 64) {
            fill(R, S.win, lane);
            int sym;
            const int len = huffman_decode(k == 0 ? S.dc[c] : S.ac[c], R.acc, sym);
            if ((len ? len : 16) > R.nb) FAIL(ended(R));
            if (len == 0) FAIL(ST_BAD_CODE);
            R.acc <<= len;
            R.nb -= len;
            int r = sym >> 4, sz = sym & 15;
            if (k == 0) {
              if (sym > 11) FAIL(ST_BAD_CATEGORY);
              r = 0;
            } else if (sz == 0) {
              if (r == 15) {
                if (k + 16 > 64) FAIL(ST_RUN_PAST_63);
                k += 16;
                continue;
              }
              if (r) FAIL(ST_BAD_CATEGORY);
              break;
            } else if (sz > 10) {
              FAIL(ST_BAD_CATEGORY);
            }
            k += r;
            if (k > 63) FAIL(ST_RUN_PAST_63);
            int val = 0;
            if (sz) {
              if (sz > R.nb) FAIL(ended(R));
              val = (int)(R.acc >> (64 - sz));
              R.acc <<= sz;
              R.nb -= sz;
              if (val < (1 << (sz - 1))) val -= (1 << sz) - 1;
            }
            if (k == 0) {
              pred[c] += val;
              val = pred[c];
            }
            val *= (int)S.quant[c][k];
            if (val < -COEF_MAX || val > COEF_MAX) FAIL(ST_COEF_RANGE);
            if (lane == 0) out[ZIGZAG[k]] = (short)val;
            ++k;
          }
        }
      }
    }
    __syncthreads();   // the band's coefficients are in place
    if (NC == 1) {
      for (int b = lane; b < band_blocks; b += WAVE) {
        int x[64];
        idct_block(S.coef + b * 64, x);
        const int x0 = b * 8;
        const bool whole = x0 + 8 <= F.W;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int y = band * 8 + r;
          if (y >= F.H) break;
          for (int p = 0; p < C_out; ++p) {
            unsigned char* o = F.d + ((long long)p * F.H + y) * F.W + x0;
            if (whole && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
              reinterpret_cast<unsigned*>(o)[0] = x[r * 8] | x[r * 8 + 1] << 8 | x[r * 8 + 2] << 16 | x[r * 8 + 3] << 24;
              reinterpret_cast<unsigned*>(o)[1] = x[r * 8 + 4] | x[r * 8 + 5] << 8 | x[r * 8 + 6] << 16 | x[r * 8 + 7] << 24;
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (x0 + j < F.W) o[j] = (unsigned char)x[r * 8 + j];
            }
          }
        }
      }
    } else {
      for (int b = lane; b < band_blocks; b += WAVE) {
        int x[64];
        idct_block(S.coef + b * 64, x);   // (the lane's own block: read whole before it is written)
        unsigned* o = reinterpret_cast<unsigned*>(S.coef + b * 64);
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = x[4 * j] | x[4 * j + 1] << 8 | x[4 * j + 2] << 16 | x[4 * j + 3] << 24;
      }
      __syncthreads();
      const int rows = 8 * F.vs, y0 = band * rows, c0 = band * 8;
      const bool context = F.vs == 2, last = band == F.my - 1;
      if (context && band > 0) emit_row(S, F, y0 - 1, -1, c0, lane);
      const int upto = (context && !last) ? rows - 1 : rows;   // 4:2:0 holds its last row back for the chroma row below it
      for (int r = 0; r < upto && y0 + r < F.H; ++r) emit_row(S, F, y0 + r, r, c0, lane);
      if (context && !last) {
        __syncthreads();   // the kept rows were read
        for (int x = lane; x < F.W; x += WAVE) S.keep_y[x] = (unsigned char)luma_at(S, F, rows - 1, x);
        for (int x = lane; x < F.cw; x += WAVE) {
          S.keep_c[0][x] = (unsigned char)chroma_at(S, F, 0, c0 + 7, x, c0);
          S.keep_c[1][x] = (unsigned char)chroma_at(S, F, 1, c0 + 7, x, c0);
        }
      }
    }
  }
  fill(R, S.win, lane);
  if (R.nb >= 8 || R.stop != 0xD9) st = ST_NO_EOI;
done:
#undef FAIL
  if (lane == 0) status[row] = st;
}

}  // namespace

extern "C" int yogo_jpeg_decode(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                                long long dst_bytes, int C_out, int* status, hipStream_t stream) {
  YOGO_CHECK_ARG(src && table && dst && status && src_bytes > 0 && dst_bytes > 0 && n >= 0, "jpeg_decode: bad arguments");
  YOGO_CHECK_ARG(C_out == 1 || C_out == 3, "jpeg_decode: %d output planes, 1 or 3 are written", C_out);
  YOGO_CHECK_ARG(n <= (1 << 24), "jpeg_decode: %d table rows, at most %d per call", n, 1 << 24);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "jpeg_decode: the table must be 8-byte and the status 4-byte aligned");
  YOGO_CHECK_ARG(src + src_bytes <= dst || dst + dst_bytes <= src, "jpeg_decode: the source and the destination overlap");
  if (n == 0) return YOGO_OK;
  hipLaunchKernelGGL(jpeg_decode_kernel<1>, dim3(n), dim3(WAVE), 0, stream, src, src_bytes, table, dst, dst_bytes, C_out, status);
  YOGO_CHECK_LAUNCH("jpeg_decode");
  hipLaunchKernelGGL(jpeg_decode_kernel<3>, dim3(n), dim3(WAVE), 0, stream, src, src_bytes, table, dst, dst_bytes, C_out, status);
  YOGO_CHECK_LAUNCH("jpeg_decode");
  if (yogo_launch_log_enabled()) yogo_launch_log("jpeg_decode_kernel | rows=%d src=%lld dst=%lld planes=%d", n, src_bytes, dst_bytes, C_out);
  return YOGO_OK;
}

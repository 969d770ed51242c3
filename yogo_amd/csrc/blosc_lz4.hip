// The blocks of Blosc-compressed zarr chunks, decoded on the device (yogo_amd/zarr_feed.py, yogo_amd/blosc.py): zarr's default
// compressor is Blosc(cname="lz4", shuffle=1), and a Blosc chunk of uint8 data is a header, a table of block starts and
// independent blocks, each either one LZ4 block or the raw bytes.  The host parses the headers (blosc.parse_chunk) and hands over
// the stored bytes as they came off the disk plus one table entry per block:
//   table[e] = { src_off, src_len, dst_off, dst_len, raw }   (int64 each)
// src_off / src_len: the block's bytes in `src`; dst_off / dst_len: where its decoded bytes belong in `dst` -- the staging layout
// yogo_zarr_unpack reads; raw != 0: the bytes are copied, else they are one LZ4 block.  status[e] = 0, or the code of the check
// that ended the entry (the LZ4_* numbers of yogo_amd/blosc.py, whose lz4_block_status makes the same checks in the same order).
//
// One wavefront (a 64-thread workgroup) per entry.  A raw entry is a copy in 16-byte pieces on the destination's alignment (the
// loads are unaligned 16-byte global loads where the source sits differently -- a block's bytes follow a 4-byte size wherever
// the previous block ended), bytes at both edges.  An LZ4 entry is decoded sequence by sequence: token, lengths and offset are
// wave-uniform (every lane holds one byte of a 64-byte window of the source, v_readlane fetches from it), the literal and the
// match copy are done by the 64 lanes together.  A match whose offset is smaller than its length is periodic: byte i of it is
// byte i % offset of the `offset` bytes before it, all written before this sequence -- no dependency inside one copy.
//
// Bounds: every source access is checked against src_len and every destination access against dst_len BEFORE it is made,
// whatever the bytes say; an entry that does not lie inside the buffers is refused before its first access.  Every loop
// consumes at least one source byte per trip.
//
// Visibility: a match reads bytes that other lanes of this wavefront stored to global memory in an earlier sequence.  Between a
// sequence's stores and the next sequence's loads stands __syncthreads(), the workgroup-scope release / acquire pair.  In a
// workgroup of one wavefront the compiler lowers it to an ordering constraint alone (no s_barrier, no cache maintenance): a
// wavefront's vector memory instructions reach the CU's write-through vector cache in program order, which is all that
// workgroup scope asks for here.  It costs no LDS; a 64 KiB history window in LDS would hold two blocks per CU, and this loop,
// latency-bound per sequence, wants many wavefronts per CU.
#include "common.h"
#include "wave_copy.h"

namespace {

using yogo_wave::WAVE;
using yogo_wave::wave_copy;
enum : int { ST_OK = 0, ST_LITERALS_PAST_SOURCE = 1, ST_SOURCE_ENDS_IN_SEQUENCE = 2, ST_BAD_OFFSET = 3, ST_PAST_DESTINATION = 4,
             ST_ENDS_EARLY = 5, ST_BAD_ENTRY = 6 };

// the source byte at p (0 <= p < n, wave-uniform) out of the wave's 64-byte window, which is refilled when p lies outside it
__device__ __forceinline__ unsigned src_byte(const unsigned char* s, long long n, long long p, long long& wbase, unsigned& w, int lane) {
  if (p < wbase || p >= wbase + WAVE) {
    wbase = p;
    w = p + lane < n ? s[p + lane] : 0u;
  }
  return (unsigned)__builtin_amdgcn_readlane((int)w, (int)(p - wbase));
}

__global__ __launch_bounds__(WAVE) void blosc_lz4_decode_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                                const long long* __restrict__ table, unsigned char* dst,
                                                                long long dst_bytes, int* __restrict__ status) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const long long* t = table + 5LL * e;
  const long long src_off = t[0], n = t[1], dst_off = t[2], dst_len = t[3], raw = t[4];
  int st = ST_OK;
  if (src_off < 0 || n < 0 || src_off > src_bytes || n > src_bytes - src_off || dst_off < 0 || dst_len < 0 || dst_off > dst_bytes ||
      dst_len > dst_bytes - dst_off || (raw && n != dst_len)) {
    st = ST_BAD_ENTRY;
  } else if (raw) {
    wave_copy(dst + dst_off, src + src_off, n, lane);
  } else {
    const unsigned char* s = src + src_off;
    unsigned char* d = dst + dst_off;
    long long sp = 0, dp = 0, wbase = -WAVE;
    unsigned w = 0;
    for (;;) {
      if (sp >= n) { st = ST_SOURCE_ENDS_IN_SEQUENCE; break; }
      const unsigned token = src_byte(s, n, sp++, wbase, w, lane);
      long long lit = token >> 4;
      if (lit == 15) {
        unsigned b;
        do {
          if (sp >= n) { st = ST_SOURCE_ENDS_IN_SEQUENCE; break; }
          b = src_byte(s, n, sp++, wbase, w, lane);
          lit += b;
        } while (b == 255);
        if (st) break;
      }
      if (lit > n - sp) { st = ST_LITERALS_PAST_SOURCE; break; }
      if (lit > dst_len - dp) { st = ST_PAST_DESTINATION; break; }
      wave_copy(d + dp, s + sp, lit, lane);
      sp += lit;
      dp += lit;
      if (sp == n) { st = dp == dst_len ? ST_OK : ST_ENDS_EARLY; break; }
      if (n - sp < 2) { st = ST_SOURCE_ENDS_IN_SEQUENCE; break; }
      const unsigned lo = src_byte(s, n, sp++, wbase, w, lane);
      const unsigned hi = src_byte(s, n, sp++, wbase, w, lane);
      const long long off = lo | (hi << 8);
      long long ml = token & 15;
      if (ml == 15) {
        unsigned b;
        do {
          if (sp >= n) { st = ST_SOURCE_ENDS_IN_SEQUENCE; break; }
          b = src_byte(s, n, sp++, wbase, w, lane);
          ml += b;
        } while (b == 255);
        if (st) break;
      }
      ml += 4;
      if (off == 0 || off > dp) { st = ST_BAD_OFFSET; break; }
      if (ml > dst_len - dp) { st = ST_PAST_DESTINATION; break; }
      __syncthreads();   // everything stored so far (these literals, every earlier sequence) is visible to the loads below
      if (off >= ml) {
        wave_copy(d + dp, d + dp - off, ml, lane);
      } else {
        yogo_wave::wave_copy_periodic(d + dp, off, ml, lane);
      }
      dp += ml;   // (the next sequence's barrier stands between these stores and its loads)
    }
  }
  if (lane == 0) status[e] = st;
}

}  // namespace

extern "C" int yogo_blosc_lz4_decode(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                                     long long dst_bytes, int* status, hipStream_t stream) {
  YOGO_CHECK_ARG(src && table && dst && status && src_bytes > 0 && dst_bytes > 0 && n >= 0, "blosc_lz4_decode: bad arguments");
  YOGO_CHECK_ARG(n <= (1 << 24), "blosc_lz4_decode: %d table entries, at most %d per call", n, 1 << 24);
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "blosc_lz4_decode: the table must be 8-byte and the status 4-byte aligned");
  YOGO_CHECK_ARG((reinterpret_cast<uintptr_t>(dst) & 15) == 0, "blosc_lz4_decode: the destination must be 16-byte aligned");
  YOGO_CHECK_ARG(src + src_bytes <= dst || dst + dst_bytes <= src, "blosc_lz4_decode: the source and the destination overlap");
  if (n == 0) return YOGO_OK;
  hipLaunchKernelGGL(blosc_lz4_decode_kernel, dim3(n), dim3(WAVE), 0, stream, src, src_bytes, table, dst, dst_bytes, status);
  YOGO_CHECK_LAUNCH("blosc_lz4_decode");
  if (yogo_launch_log_enabled())
    yogo_launch_log("blosc_lz4_decode_kernel | entries=%d src=%lld dst=%lld", n, src_bytes, dst_bytes);
  return YOGO_OK;
}

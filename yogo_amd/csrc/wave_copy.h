// Copies and fills done by the 64 lanes of one wavefront together: what the device decoders (blosc_lz4.hip, inflate.hip, zstd.hip) move
// bytes with.  None checks a bound: the caller has held both ranges to its buffers before it calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace yogo_wave {

constexpr int WAVE = 64;

// n bytes from s to d by the whole wave; the ranges do not overlap.  Aligned 16-byte stores, 16-byte loads at the source's alignment.
__device__ __forceinline__ void wave_copy(unsigned char* d, const unsigned char* s, long long n, int lane) {
  if (n < 4 * WAVE) {
    for (long long i = lane; i < n; i += WAVE) d[i] = s[i];
    return;
  }
  const long long head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;   // < n
  const long long pieces = (n - head) >> 4;
  if (lane < head) d[lane] = s[lane];
  long long p = lane;
  for (; p + 3 * WAVE < pieces; p += 4 * WAVE) {   // four loads in flight before the first store (d may alias s for the compiler)
    // (named, not `uint4 v[4]`: inlined into inflate.hip the array kept a stack slot -- 80 bytes of scratch per lane and three
    // scratch stores of the loaded values in this loop, by the compiler's resource remarks and the ISA; named, both kernels use no
    // scratch, and blosc_lz4_decode_kernel, which had none either way, goes from 50 to 46 VGPRs)
    uint4 v0, v1, v2, v3;
    const unsigned char* sp = s + head + 16 * p;
    unsigned char* dq = d + head + 16 * p;
    __builtin_memcpy(&v0, sp, 16);
    __builtin_memcpy(&v1, sp + 16 * WAVE, 16);
    __builtin_memcpy(&v2, sp + 32 * WAVE, 16);
    __builtin_memcpy(&v3, sp + 48 * WAVE, 16);
    *reinterpret_cast<uint4*>(dq) = v0;
    *reinterpret_cast<uint4*>(dq + 16 * WAVE) = v1;
    *reinterpret_cast<uint4*>(dq + 32 * WAVE) = v2;
    *reinterpret_cast<uint4*>(dq + 48 * WAVE) = v3;
  }
  for (; p < pieces; p += WAVE) {
    uint4 v;
    __builtin_memcpy(&v, s + head + 16 * p, 16);
    *reinterpret_cast<uint4*>(d + head + 16 * p) = v;
  }
  const long long done = head + 16 * pieces;
  if (done + lane < n) d[done + lane] = s[done + lane];   // < 16 bytes are left
}

// A match of ml bytes at d whose source starts off bytes before d, 1 <= off < ml: periodic, byte j is byte j % off of the `off`
// bytes before d, all written before this call -- no dependency inside the copy.  Lane i serves bytes i, i + 64, ...; r follows
// j % off without a division per trip.
__device__ __forceinline__ void wave_copy_periodic(unsigned char* d, long long off, long long ml, int lane) {
  const unsigned char* m = d - off;
  const int o = (int)off, step = WAVE % o;
  int r = lane % o;
  for (long long j = lane; j < ml; j += WAVE) {
    d[j] = m[r];
    r += step;
    if (r >= o) r -= o;
  }
}

// n bytes of value v at d by the whole wave (a run-length block, run-length literals).  Aligned 16-byte stores, bytes at both edges.
__device__ __forceinline__ void wave_fill(unsigned char* d, unsigned char v, long long n, int lane) {
  if (n < 4 * WAVE) {
    for (long long i = lane; i < n; i += WAVE) d[i] = v;
    return;
  }
  const long long head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;   // < n
  const long long pieces = (n - head) >> 4;
  if (lane < head) d[lane] = v;
  const unsigned w = v * 0x01010101u;
  const uint4 q = make_uint4(w, w, w, w);
  for (long long p = lane; p < pieces; p += WAVE) *reinterpret_cast<uint4*>(d + head + 16 * p) = q;
  const long long done = head + 16 * pieces;
  if (done + lane < n) d[done + lane] = v;   // < 16 bytes are left
}

}  // namespace yogo_wave

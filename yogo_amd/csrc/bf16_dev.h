// Device-side primitives shared by the hand-written bf16 kernels (gfx950 / CDNA4 only): the hardware idioms every kernel file of the
// conv family needs, each with the hazard rule that goes with it, defined once.  A primitive used by two kernel files lives here
// (DESIGN.md 3.0); what only one kernel uses -- its K-step bodies, its multi-piece DMA statements -- stays in that kernel's file.
// Host code goes to common.h, not here.
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>

// native vector types (HIP's uint4 / uint2 are structs and get spilled to scratch when selected / stored through pointers)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- division by a run-time constant.  n / d = __umulhi(n, m) with m = ceil(2^32 / d): the host computes m with magic_u32(d) and
// proves the quotient exact for the launch's largest dividend with magic_div_exact(nmax, d) (common.h) -- a kernel that divides this
// way has a planner or an eligibility check that made both calls.  d = 1 has no 32-bit multiplier (magic_u32 gives all ones): udivm is
// for divisors known to be > 1, udivm1 tests for d == 1.
__device__ __forceinline__ int udivm(int n, unsigned m) { return (int)__umulhi((unsigned)n, m); }
__device__ __forceinline__ int udivm1(int n, int d, unsigned m) { return d == 1 ? n : (int)__umulhi((unsigned)n, m); }

// ---- buffer resource descriptors.  Word 3 of a raw (untyped, stride 0) buffer: DATA_FORMAT (bits 18:15) = 4 = 32 bits, everything
// else zero -- no swizzle, no index / thread-id addressing -- so that word 2 counts BYTES and the range check is "offset >= bytes":
// such a lane loads zeros (into registers or through LDS-DMA into LDS) and its stores are dropped.
constexpr int RSRC_WORD3 = 0x00020000;
// A per-lane byte offset with bit 31 set is out of range of every descriptor (their sizes stay below 2^31: the eligibility checks):
// the way a lane opts out of a load or a store without a branch.
constexpr unsigned OOB = 0x80000000u;
// The descriptor has to be wave-uniform (it travels in four SGPRs); build it from uniform values only, or pass it through uniform4().
__device__ __forceinline__ i32x4 rsrc(const void* ptr, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(ptr);
  return i32x4{(int)(unsigned)a, (int)((unsigned)(a >> 32) & 0xFFFFu), (int)bytes, RSRC_WORD3};
}

// ---- wave-uniform values the compiler cannot prove uniform -> SGPRs.  HAZARD: a buffer instruction inside an asm statement whose
// descriptor or scalar offset was written by v_readfirstlane needs 4 wait states in front ("s_nop 4": hipcc does not look inside asm
// statements); every helper below that takes a descriptor carries it.
__device__ __forceinline__ unsigned uniform(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ i32x4 uniform4(i32x4 r) {
  return i32x4{__builtin_amdgcn_readfirstlane(r.x), __builtin_amdgcn_readfirstlane(r.y), __builtin_amdgcn_readfirstlane(r.z), __builtin_amdgcn_readfirstlane(r.w)};
}

// ---- lane index, re-derived at every use (volatile: never merged with an earlier copy that would have to stay live across a tile
// loop or the other role's code -- or be spilled; the register-bound persistent kernels have none to spare)
__device__ __forceinline__ int lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// ---- f(integral_constant<int, I>) for every I of the sequence: a loop whose index is a template argument of the asm statements inside
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

// ---- accumulator registers owned by asm statements: named literally in the statements and listed as clobbers, so that the kernel
// descriptor allocates them (conv_bf16_ws.hip has the story).  A kernel file composes its list from these blocks.
#define ACC_A0_63 "a0","a1","a2","a3","a4","a5","a6","a7","a8","a9","a10","a11","a12","a13","a14","a15","a16","a17","a18","a19","a20","a21","a22","a23","a24","a25","a26","a27","a28","a29","a30","a31","a32","a33","a34","a35","a36","a37","a38","a39","a40","a41","a42","a43","a44","a45","a46","a47","a48","a49","a50","a51","a52","a53","a54","a55","a56","a57","a58","a59","a60","a61","a62","a63"
#define ACC_A64_127 "a64","a65","a66","a67","a68","a69","a70","a71","a72","a73","a74","a75","a76","a77","a78","a79","a80","a81","a82","a83","a84","a85","a86","a87","a88","a89","a90","a91","a92","a93","a94","a95","a96","a97","a98","a99","a100","a101","a102","a103","a104","a105","a106","a107","a108","a109","a110","a111","a112","a113","a114","a115","a116","a117","a118","a119","a120","a121","a122","a123","a124","a125","a126","a127"
#define ACC_A128_159 "a128","a129","a130","a131","a132","a133","a134","a135","a136","a137","a138","a139","a140","a141","a142","a143","a144","a145","a146","a147","a148","a149","a150","a151","a152","a153","a154","a155","a156","a157","a158","a159"
// acc_read8<R>(r): the eight consecutive accumulator registers a[R : R + 7] -> VGPRs in ONE statement (hipcc pads every asm statement
// with a wait state).  The statement CLOBBERS the file's whole accumulator list (a clobber list is not a function argument, hence a
// macro that defines the function): hipcc then cannot keep a value of its own in an AGPR across any part of an epilogue -- a clobbered
// register holds nothing live across the statement.  The caller has put the wait states behind the last MFMA (16 passes: "s_nop 15" twice).
#define DEFINE_ACC_READ8(...)                                                                                                             \
  template <int R>                                                                                                                        \
  __device__ __forceinline__ void acc_read8(float (&r)[8]) {                                                                              \
    asm volatile(                                                                                                                         \
        "v_accvgpr_read_b32 %0, a[%8]\n\tv_accvgpr_read_b32 %1, a[%8+1]\n\tv_accvgpr_read_b32 %2, a[%8+2]\n\tv_accvgpr_read_b32 %3, a[%8+3]\n\t" \
        "v_accvgpr_read_b32 %4, a[%8+4]\n\tv_accvgpr_read_b32 %5, a[%8+5]\n\tv_accvgpr_read_b32 %6, a[%8+6]\n\tv_accvgpr_read_b32 %7, a[%8+7]"   \
        : "=v"(r[0]), "=v"(r[1]), "=v"(r[2]), "=v"(r[3]), "=v"(r[4]), "=v"(r[5]), "=v"(r[6]), "=v"(r[7])                                  \
        : "n"(R)                                                                                                                          \
        : __VA_ARGS__);                                                                                                                   \
  }

// ---- tile walk of the persistent kernels: virtual workgroup lin of nwg (hardware workgroup i runs on XCD i % 8) -> the tile it
// takes, so that the workgroups of one XCD share a CONTIGUOUS run of tiles (neighbouring tiles share halo rows and weights in that
// XCD's L2): XCD x owns nwg / 8 tiles, the first nwg % 8 XCDs one more, and workgroup lin takes tile lin / 8 of XCD lin % 8's run.
__device__ __forceinline__ unsigned xcd_remap(unsigned lin, unsigned nwg) {
  const unsigned xq = nwg >> 3, xr = nwg & 7;
  const unsigned xcd = lin & 7;
  return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
}

// ---- LDS-DMA (buffer_load ... lds: 64 lanes x 4 or 16 bytes land at LDS address m0 + lane * size, out-of-range lanes as zeros) and
// 16-byte stores.  The descriptor, the LDS address and the scalar offset are "s" operands: the caller has made them uniform (the
// *_uniform forms do it here).  Every statement starts with the wait states of the v_readfirstlane hazard above.
// four pieces (64 lanes x 16 bytes each) of one descriptor with one scalar offset and their own per-lane offsets: LDS destinations
// lds + k * 4 KB (m0 is stepped in place; "s_nop 0": one wait state between a write of m0 and the LDS-DMA that reads it)
__device__ __forceinline__ void dma4(i32x4 rs, unsigned lds, int v0, int v1, int v2, int v3, unsigned soff) {
  asm volatile(
      "s_mov_b32 m0, %5\n\ts_nop 4\n\tbuffer_load_dwordx4 %0, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 4096\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 4096\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 4096\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %6 offen lds"
      ::"v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(rs), "s"(lds), "s"(soff) : "memory", "scc");
}
// ONE piece, 64 lanes x 16 bytes -> LDS bytes [lds, lds + 1024), with m0 saved and restored around it: for code the compiler schedules
// LDS instructions of its own around (they read m0).  Issued from inline asm on purpose: hipcc (ROCm 7.2) makes every later LDS read wait
// for ALL of its own LDS-DMA loads (vmcnt(0)), which would serialise a ring; these loads are invisible to it and the caller retires them
// with a counted s_waitcnt vmcnt.  (conv_bf16_tiled.hip's bf_dma16 is this with a scalar offset register in place of the literal 0.)
__device__ __forceinline__ void dma16(i32x4 rs, unsigned lds, int voff) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(lds), "s"(rs)
               : "memory");
}
__device__ __forceinline__ void dma16_uniform(i32x4 rs, unsigned lds, int voff) { dma16(rs, uniform(lds), voff); }
// 64 lanes x 4 bytes -> LDS bytes [lds, lds + 256)
__device__ __forceinline__ void dma_dword(i32x4 rs, unsigned lds, int voff, unsigned soff) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 4\n\tbuffer_load_dword %0, %2, %3 offen lds" ::"v"(voff), "s"(lds), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma_dword_uniform(i32x4 rs, unsigned lds, int voff, unsigned soff) {
  dma_dword(uniform4(rs), uniform(lds), voff, uniform(soff));
}
// one 16-byte unit per lane.  Two forms, named for what differs:
//   store16          the operands are uniform already, and the caller's next vector instruction does not write `data`;
//   store16_uniform  descriptor and scalar offset are made uniform here, and "s_nop 1" follows the store: a 16-byte store reads its
//                    data registers over several cycles and the next vector instruction must not overwrite them -- hipcc, which would
//                    insert that wait state itself, does not look inside asm statements.  For a caller whose following code is
//                    compiler-scheduled arithmetic on the same registers (an epilogue that stores straight from its accumulators'
//                    VGPR copies); store16's callers store from a register FIFO that is refilled by LDS reads much later.
__device__ __forceinline__ void store16(u32x4 data, int voff, i32x4 rs, unsigned soff) {
  asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen" ::"v"(data), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ void store16_uniform(u32x4 data, int voff, i32x4 rs, unsigned soff) {
  rs = uniform4(rs); soff = uniform(soff);
  asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" ::"v"(data), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// ---- the transposed LDS fetch of an MFMA operand staged as [pixel][channels] bf16: two ds_read_b64_tr_b16, each handing the lane 4
// pixels of "its" channel, from the LDS bytes at lo and hi (generic pointers into the dynamic LDS block) -> 8 pixels
__device__ __forceinline__ bf16x8 lds_tr8(const unsigned char* lo_addr, const unsigned char* hi_addr) {
  typedef bf16x4 __attribute__((address_space(3))) * lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4)lo_addr);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4)hi_addr);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- epilogue idioms of the MFMA kernels.  After a 32x32 MFMA a lane holds, per group of eight accumulator registers, channels
// 4 h .. 4 h + 3 of channel block cb and of block cb + 1 of its pixel (h = lane >> 5): half a 16-byte unit of each block.
// pack_unit_swap: eight fp32 -> bf16 (round to nearest even), then the two half-waves trade one 8-byte group (lanes 32-63 hand their
// block-cb half down, lanes 0-31 hand their block-(cb + 1) half up): lanes 0-31 end up with the whole unit of block cb, lanes 32-63 with
// that of block cb + 1 -- one 16-byte store per lane, 512 contiguous bytes per half-wave.
__device__ __forceinline__ u32x4 pack_unit_swap(const float (&v)[8]) {
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i];
  const u32x4 w = __builtin_bit_cast(u32x4, o);   // (x, y) = this lane's 4 channels of block cb, (z, w) = of block cb + 1
  const auto r0 = __builtin_amdgcn_permlane32_swap(w.x, w.z, false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(w.y, w.w, false, false);
  return u32x4{r0[0], r1[0], r0[1], r1[1]};
}
// sign_byte: bit i = (v[i] > 0) -- the LeakyReLU sign map the data gradient reads in place of the activation.  The compare leaves its
// result in vcc and an add-with-carry shifts it into the byte (m = 2 m + carry), values taken from 7 down to 0: two vector instructions
// per value where compare / select / shift-or takes three (these epilogues are bound by vector-instruction issue).  ONE statement: the
// sixteen instructions stay together.
__device__ __forceinline__ unsigned sign_byte(const float (&v)[8]) {
  unsigned m = 0;
#define BF16_DEV_SGN(I) "v_cmp_lt_f32_e32 vcc, 0, %" #I "\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
  asm(BF16_DEV_SGN(8) BF16_DEV_SGN(7) BF16_DEV_SGN(6) BF16_DEV_SGN(5) BF16_DEV_SGN(4) BF16_DEV_SGN(3) BF16_DEV_SGN(2)
      "v_cmp_lt_f32_e32 vcc, 0, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc"
      : "+v"(m)
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7])
      : "vcc");
#undef BF16_DEV_SGN
  return m;
}

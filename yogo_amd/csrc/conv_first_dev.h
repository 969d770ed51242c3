// What the VALU kernels of layer 0 share (conv_first.hip, conv_first_infer_bf16.hip): the zero-padded 3x3 gather, the bf16 unpacking of
// the backward sweeps, and the host's choice of a <TIn, CIN> instantiation -- each defined once (the block reduction of per-lane sums
// into a partial row is common.h's block_put / block_sum4).  The rule of bf16_dev.h holds here too: a primitive used by two kernels lives here, what one kernel
// alone uses stays in its file.  conv_first_bn_wgrad_kernel keeps its own text of both gathers and of the reduction (measured: see there),
// so cf_gather_u8s2 has one caller today, the packed sweep.  conv_first_mfma.hip and conv_first_fused_bwd.hip (the benched step's layer 0)
// keep their own copies of the 16-bit row load and the sign decode, and their reductions add in another order: not to be merged with these.
#pragma once
#include "bf16_dev.h"

// ---- the input patch.  p is the kernel's parameter struct (IH, IW, stride), taken by reference so that its fields stay the scalar
// loads they are in the kernel.  One tap, branch-free: the address is clamped to element 0 and the value selected, so a lane outside
// the image (or with ok = false: beyond the tile's tail) loads in[0] and gets 0 -- the image holds at least one element.
template <typename TIn, typename P>
__device__ __forceinline__ float cf_tap(const TIn* inb, const P& p, bool ok, int oy, int ox, int ci, int kh, int kw) {
  const int iy = oy * p.stride + kh - 1, ix = ox * p.stride + kw - 1;
  const bool in = ok && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW;
  const float v = (float)inb[in ? ((size_t)ci * p.IH + iy) * p.IW + ix : 0];
  return in ? v : 0.f;
}
// the 9 * CIN values of output pixel (oy, ox), x[(ci * 3 + kh) * 3 + kw]
template <int CIN, typename TIn, typename P>
__device__ __forceinline__ void cf_gather(float (&x)[CIN * 9], const TIn* inb, const P& p, bool ok, int oy, int ox) {
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) x[(ci * 3 + kh) * 3 + kw] = cf_tap(inb, p, ok, oy, ox, ci, kh, kw);
}
// The branch form of cf_gather: a lane outside the image skips the load.  Same values; kept for conv_first_kernel on fp32 images.
template <int CIN, typename TIn, typename P>
__device__ __forceinline__ void cf_gather_branch(float (&x)[CIN * 9], const TIn* inb, const P& p, bool ok, int oy, int ox) {
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iy = oy * p.stride + kh - 1, ix = ox * p.stride + kw - 1;
        float v = 0.f;
        if (ok && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) v = (float)inb[((size_t)ci * p.IH + iy) * p.IW + ix];
        x[(ci * 3 + kh) * 3 + kw] = v;
      }
}
// The same patch for a uint8 one-channel image at stride 2 with even IH and IW: the three bytes of a patch row come from two 16-bit
// loads, bytes [o - 2, o) for the left tap and [o, o + 2) for the other two with o = iy * IW + 2 * ox, and only the top row and the left
// column can fall outside the image (iy <= IH - 1, 2 * ox + 1 <= IW - 1) -- a third of the per-byte bounds arithmetic.
// PRECONDITION: ib is 2-byte aligned (o is even, so every load then is); the launcher sends a less aligned image to cf_gather.
__device__ __forceinline__ void cf_gather_u8s2(float (&x)[9], const unsigned char* ib, int IW, bool ok, int oy, int ox) {
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int iy = 2 * oy + kh - 1;
    const bool rok = ok && iy >= 0;
    const int o_ = rok ? iy * IW + 2 * ox : 0;
    const unsigned hi_ = *reinterpret_cast<const unsigned short*>(ib + o_);
    const unsigned lo_ = *reinterpret_cast<const unsigned short*>(ib + ((rok && ox > 0) ? o_ - 2 : o_));
    x[kh * 3 + 0] = (rok && ox > 0) ? (float)(lo_ >> 8) : 0.f;
    x[kh * 3 + 1] = rok ? (float)(hi_ & 0xFFu) : 0.f;
    x[kh * 3 + 2] = rok ? (float)(hi_ >> 8) : 0.f;
  }
}

// ---- bf16 NCHW8c units in the backward kernels.  The two bf16 of a dword, widened: low half << 16, high half masked
__device__ __forceinline__ f32x2 cf_widen(unsigned w) {
  return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xFFFF0000u)};
}
// LeakyReLU derivative of channel pair q (channels 2q, 2q + 1 of an 8-channel unit) from the pixel's sign word of the forward pass.
// Its 16 bits are two bytes in the forward kernel's lane order: channel c < 4 or >= 12 at bit c, 4..7 at c + 4, 8..11 at c - 4; the
// caller has shifted the word right by 4 for the second unit, so that unit's pairs sit where the first unit's do.
__device__ __forceinline__ f32x2 cf_leaky_pair(unsigned sgn, int q) {
  const int pos = q < 2 ? 2 * q : 8 + 2 * (q - 2);   // (a constant of the caller's unrolled loop)
  return f32x2{(sgn >> pos) & 1u ? 1.f : LEAKY_SLOPE, (sgn >> (pos + 1)) & 1u ? 1.f : LEAKY_SLOPE};
}

// ---- the launchers' half (kept beside the kernels it instantiates, unlike bf16_dev.h: it is these two files' alone).
// output size of the 3x3, pad 1 convolution
static inline int cf_out_dim(int I, int stride) { return (I - 1) / stride + 1; }
// f(TIn{}, integral_constant<int, CIN>{}) for the image type (in_dtype 0 = uint8, 1 = float32) and channel count (1 | 3) of a launch;
// the launcher has checked both
template <class F>
static inline void cf_dispatch(int in_dtype, int Cin, F&& f) {
  if (in_dtype == 0 && Cin == 1) f(uint8_t{}, std::integral_constant<int, 1>{});
  else if (in_dtype == 0) f(uint8_t{}, std::integral_constant<int, 3>{});
  else if (Cin == 1) f(float{}, std::integral_constant<int, 1>{});
  else f(float{}, std::integral_constant<int, 3>{});
}

// Layer 0's inference forward of the bf16 path (the training step's layer 0 is conv_first_mfma.hip).
#include "conv_first_dev.h"
#include "conv_bf16_plan.h"

// ---- first convolution, bf16 NCHW8c output: Cin = 1|3, uint8 or fp32 input (weights fp32, BatchNorm pre-folded) -----------
struct ConvFirstBf16Params {
  const void* in;
  const float* w;     // [Cout][Cin*9] (already scaled)
  const float* bias;  // [Cout] or null
  u32x4* out;         // [B][Mb][OH][OW] units
  int B, Cin, Cout, Mb, IH, IW, OH, OW, stride, act;
};

template <typename TIn, int CIN>
__global__ __launch_bounds__(256) void conv_first_bf16_kernel(const ConvFirstBf16Params p) {
  const int b = blockIdx.y;
  const int npix = p.OH * p.OW;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const int oy = pix / p.OW, ox = pix - oy * p.OW;
  const TIn* inb = reinterpret_cast<const TIn*>(p.in) + (size_t)b * CIN * p.IH * p.IW;
  const float* __restrict__ w = p.w;
  float x[CIN * 9];
  cf_gather<CIN>(x, inb, p, true, oy, ox);
  for (int cb = 0; cb < p.Mb; ++cb) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int co = cb * 8 + j;
      float acc = 0.f;
      if (co < p.Cout) {  // uniform
#pragma unroll
        for (int q = 0; q < CIN * 9; ++q) acc = fmaf(w[co * CIN * 9 + q], x[q], acc);
        if (p.bias != nullptr) acc += p.bias[co];
        acc = act_fwd(acc, p.act);
      }
      o[j] = (__bf16)acc;
    }
    p.out[((size_t)b * p.Mb + cb) * npix + pix] = __builtin_bit_cast(u32x4, o);
  }
}

// first conv (Cin 1|3; in_dtype 0 = uint8, 1 = float32), fp32 weights [Cout][Cin][3][3] with BatchNorm already folded;
// out: bf16 NCHW8c with kb(Cout) channel blocks (padding channels are written as zeros)
extern "C" int yogo_conv_first_fwd_bf16(const void* in, int in_dtype, const float* w, const float* bias, void* out, int B,
                                        int Cin, int Cout, int IH, int IW, int stride, int act, hipStream_t stream) {
  YOGO_CHECK_ARG(in && w && out, "conv_first_fwd_bf16: null pointer");
  YOGO_CHECK_ARG((Cin == 1 || Cin == 3) && Cout > 0 && (stride == 1 || stride == 2) && (in_dtype == 0 || in_dtype == 1) && B >= 0,
                 "conv_first_fwd_bf16: unsupported shape");
  ConvFirstBf16Params p{};
  p.in = in; p.w = w; p.bias = bias; p.out = reinterpret_cast<u32x4*>(out);
  p.B = B; p.Cin = Cin; p.Cout = Cout; p.Mb = bf_kb_of(Cout); p.IH = IH; p.IW = IW; p.stride = stride; p.act = act;
  p.OH = cf_out_dim(IH, stride); p.OW = cf_out_dim(IW, stride);
  if (B == 0) return YOGO_OK;
  dim3 grid(cdiv(p.OH * p.OW, 256), B);
  cf_dispatch(in_dtype, Cin, [&](auto tin, auto cin) {
    hipLaunchKernelGGL((conv_first_bf16_kernel<decltype(tin), decltype(cin)::value>), grid, dim3(256), 0, stream, p);
  });
  YOGO_CHECK_LAUNCH("conv_first_fwd_bf16");
  if (yogo_launch_log_enabled())
    yogo_launch_log("conv_first_bf16_kernel<%s, %d> | B=%d Cout=%d in=%dx%d out=%dx%d stride=%d act=%d bias=%d", in_dtype == 0 ? "uint8_t" : "float", Cin, B, Cout, IH, IW,
                    p.OH, p.OW, stride, act, bias != nullptr);
  return YOGO_OK;
}

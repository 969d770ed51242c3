// The fixed-order split-K reduction every weight-gradient kernel file ends with (wgrad_reduce.hip): slabs [nslab][T][Mpad][Npad] and
// bias partial rows [nbias][Mpad] -> dw (OIHW) and db, clamped to +-clip when clip > 0.  Kernels cannot be launched across translation
// units without RDC, hence host entry points.  Users: wgrad_f32.hip, wgrad_bf16.hip, conv_first_fused_bwd.hip.
#pragma once
#include "common.h"

extern "C" int yogo_internal_wgrad_reduce(const float* slab, int nslab, int T, int M, int N, int Mpad, int Npad, float clip, float* dw,
                                          const float* bias_part, int nbias, float* db, hipStream_t stream);
// queue != NULL (a yogo_wgrad_reduce_queue): the reduction is only recorded; yogo_wgrad_reduce_flush launches everything recorded in
// one kernel.  Same summation order, same bits as the immediate form.
extern "C" int yogo_internal_wgrad_reduce_q(void* queue, const float* slab, int nslab, int T, int M, int N, int Mpad, int Npad, float clip, float* dw,
                                            const float* bias_part, int nbias, float* db, hipStream_t stream);

// blend_contrib.h — launcher of the contribution pass (blend_contrib.hip): per-(view, Gaussian) reductions of the blend weight
// w = α·T over the (pixel, list entry) pairs the colour blend composited.
#pragma once
#include "ggr_common.h"

namespace ggr {

// The list ids are (view, Gaussian) pair indices v·P1 + g, so every output is a flat [V·P1] array indexed by the id.
// Each output may be null (not computed); the others must have been cleared on the stream before the launch:
//   weight_sum   float  Σ_pixels w      added atomically: reproducible only up to the order of the float additions;
//   weight_max   float  max_pixels w    an integer atomic max on the bit pattern (w >= 0): bit-reproducible from run to run;
//   pixel_count  int32  pixels with the entry live: an integer atomic add: bit-reproducible from run to run.
void launch_blend_contrib(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                          float* weight_sum, float* weight_max, int32_t* pixel_count, int views, int scissored, hipStream_t s);

}  // namespace ggr

// blend_dist.h — launchers of the distortion pass (blend_dist.hip): the depth-distortion plane over a forward's tile lists.
#pragma once
#include "ggr_common.h"

namespace ggr {

// out_distortion [V, H, W]: every pixel is written.  totals [V, 2, H, W] or NULL: per pixel Σ w and the origin-relative Σ w·d,
// what the backward needs beside the plane.
void launch_blend_dist_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           float* out_distortion, float* totals, int views, int scissored, hipStream_t s);

// out_distortion / totals: what the forward wrote; dL_dout [V, H, W]; grad2d [V·P1][16], zeroed or holding other terms of the
// same frame (the sums are added atomically: the six geometric slots and GGR_G2D_Z).
void launch_blend_dist_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           const float* out_distortion, const float* totals, const float* dL_dout, float* grad2d, int views,
                           hipStream_t s);

}  // namespace ggr

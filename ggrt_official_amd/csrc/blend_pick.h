// blend_pick.h — launcher of the pick pass (blend_pick.hip): per-PIXEL picks over the list entries the colour blend composited —
// the median-depth Gaussian, the Gaussian of the largest blend weight, and the number of composited entries.
#pragma once
#include "ggr_common.h"

namespace ggr {

// The list ids are (view, Gaussian) pair indices v·P1 + g; the index planes hold g (the id minus view·P1), −1 for a pixel
// without a live entry.  Every plane is [V,H,W]; each may be null (not computed).  The kernel writes every pixel of every
// plane it is given — nothing has to be cleared — with plain stores: all five are bit-reproducible from run to run.
//   median_index  int32  the last live entry with T_before > 0.5         median_depth  float  its depth value (splat[2·id+1].z)
//   max_index     int32  the live entry of the largest w (earliest wins)   max_weight    float  that w
//   count         int32  the number of live entries
void launch_blend_pick(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                       int32_t* median_index, float* median_depth, int32_t* max_index, float* max_weight, int32_t* count,
                       int views, int P1, int scissored, hipStream_t s);

}  // namespace ggr

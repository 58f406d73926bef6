// blend_feat.h — launchers of the feature pass (blend_feat.hip): K per-Gaussian channels composited over a forward's tile lists.
#pragma once
#include "ggr_common.h"

#define GGR_MAX_FEATURES 32

namespace ggr {

// features [sets·P1, K]; the list ids are (view, Gaussian) pair indices v·P1 + g, view v renders set v / vps.
// out_features [V, K, H, W].
void launch_blend_feat_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           const float* features, int K, int P1, int vps, float* out_features, int views, int scissored,
                           hipStream_t s);

// out_features: what the forward wrote; dL_dout [V, K, H, W]; dL_dfeatures [sets·P1, K], zeroed; grad2d [V·P1][16], zeroed or
// holding other terms of the same frame (the sums are added atomically).
void launch_blend_feat_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           const float* features, int K, int P1, int vps, const float* out_features, const float* dL_dout,
                           float* dL_dfeatures, float* grad2d, int views, hipStream_t s);

}  // namespace ggr

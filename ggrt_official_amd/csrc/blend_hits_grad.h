// blend_hits_grad.h — launcher of the hit pass's backward (blend_hits_grad.hip): the gradient of a loss over the per-pixel hit
// weights and the rest (blend_hits.hip's `weight` / `rest`) w.r.t. the 2D mean, conic and opacity of every Gaussian, added into
// the per-(view, Gaussian) records of the backward scratch.
#pragma once
#include "blend_hits.h"

namespace ggr {

// `weight` [V,K,H,W] and `count` [V,H,W]: what launch_blend_hits wrote over the same lists; `final_T` [V,H,W]: the colour
// forward's final transmittance (its image buffer).  `dL_dweight` [V,K,H,W] and `dL_drest` [V,H,W]: the upstream gradients;
// either may be null (zeros).  Slots k >= count are never read, in `weight` or `dL_dweight`, nor is dL_drest where count <= K.
// The sums are added with float atomics into slots GGR_G2D_MEAN … GGR_G2D_OPACITY of grad2d's records, as the feature backward
// adds its own.
void launch_blend_hits_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat, const float* final_T,
                           int K, const float* weight, const int32_t* count, const float* dL_dweight, const float* dL_drest,
                           float* grad2d, int views, hipStream_t s);

}  // namespace ggr

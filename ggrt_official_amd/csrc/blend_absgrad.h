// blend_absgrad.h — launcher of the absgrad pass (blend_absgrad.hip): per-Gaussian ABSOLUTE screen-space positional gradients
// over a forward's tile lists.
#pragma once
#include "ggr_common.h"

namespace ggr {

// Per (view, Gaussian) row gid of the launch set, over the pixels p where the colour blend composited the Gaussian:
//     out_absgrad[gid·2 + c] += Σ_p |∂L_p/∂mean2D_c|        out_grad[gid·2 + c] += Σ_p ∂L_p/∂mean2D_c      (c = x, y; NDC-scaled)
// for the loss that reaches the pixel through the colour, depth and alpha planes (dL_dcolor [V,3,H,W]; dL_ddepth, dL_dalpha
// [V,H,W] or NULL).  Terms of a feature or a distortion loss are NOT included.  out_color [V,3,H,W] / out_depth [V,H,W] (NULL iff
// dL_ddepth is NULL) / final_T: what the forward wrote.  out_absgrad, out_grad (or NULL) [V·P1][2]: zeroed by the caller, the
// sums are added with float atomics.
void launch_blend_absgrad(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat, const float4* colour,
                          const float* final_T, const float* out_color, const float* out_depth,
                          const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, float* out_absgrad,
                          float* out_grad, int views, hipStream_t s);

}  // namespace ggr

// projection.h — launchers of the projection pass (projection.hip): the per-(view, Gaussian) quantities preprocess_fwd left in the
// geometry buffer as six plain arrays, and the seeding of a loss's gradient w.r.t. them into the records of the backward scratch.
#pragma once
#include "ggr_common.h"

namespace ggr {

// `pairs` = V·P (view, Gaussian) pairs; splat [pairs][2], colour [pairs], radii [pairs]: the forward's.  Every output may be null;
// each one given has EVERY element written: the record's own bits where radii > 0, zero elsewhere.
// means2d [pairs,2], depth [pairs], conic [pairs,3] = (xx, xy, yy), opacity [pairs], color [pairs,3], valid [pairs] (bytes 0 / 1).
void launch_projection_unpack(size_t pairs, const float4* splat, const float4* colour, const int32_t* radii, float* means2d,
                              float* depth, float* conic, float* opacity, float* color, uint8_t* valid, hipStream_t s);

// The upstream gradients (shapes as above; each may be null = zeros) go into floats 0..9 of every pair's record of grad2d
// ([pairs][GGR_G2D_STRIDE]) in the records' units: the mean's × (W/2, H/2) (pixels → NDC), the conic's xy × 1/2 (the half
// convention preprocess_bwd doubles again), colour, opacity and depth value as they are.  Rows with radii <= 0 contribute nothing,
// whatever their gradients hold.  `add` = 1: plain read-modify-write of the rows with radii > 0 (the scratch holds other passes'
// terms; each record belongs to one thread, the launch is stream-ordered against the other writers).  `add` = 0: every record is
// WRITTEN whole (16 floats), so the launch is also the clearing of grad2d.
void launch_projection_seed(size_t pairs, int W, int H, const int32_t* radii, const float* dL_dmeans2d, const float* dL_ddepth,
                            const float* dL_dconic, const float* dL_dopacity, const float* dL_dcolor, float* grad2d, int add,
                            hipStream_t s);

}  // namespace ggr

// depth_head.h — launchers of the depth-head pass (depth_head.hip): GGRt's DepthPredictorMonocular tail and the lines around it
// in EncoderEpipolar.forward (softmax over depth buckets, bucket choice, disparity → depth, pdf → opacity, pixel-offset
// coordinates) in one launch, and its backward in one launch.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kDepthHeadTile = 64;         // heads (c, r, j) per tile = lanes per workgroup (one wave)
constexpr int kDepthHeadMaxChunks = 2048;  // workgroups over all cameras, about: the rest of a camera's tiles is strided over
constexpr int kDepthHeadMaxBuckets = 64;
constexpr int kDepthHeadMaxSamples = 16;

// C cameras × R rays × srf surfaces × spp samples; head h = r·srf + j of camera c owns the Gaussians p = c·G + h·spp + k,
// G = R·srf·spp.  All pointers are device pointers; float32 unless said otherwise:
//   logits [C,R,2·s·srf] dense, channel order (bucket, surface, {pdf, offset})
//   xy_raw: two floats per (c, h) at float offset (c·R·srf + h)·xy_stride      ray_xy [R,2]   near [C]   far [C]
//   u [C,G] (sampled mode only)
//   depth [C,G]  opacity [C,G]  coords [C,G,2]  index [C,G] int32           (forward: every element written; backward reads index)
//   g_depth [C,G] / g_opacity [C,G] / g_coords [C,G,2]: each may be null (taken as zero)
//   g_logits [C,R,2·s·srf] (written whole)   g_xy [C,R·srf,2] dense (written whole; may be null)
struct DepthHeadArgs {
    int C, R, s, srf, spp, deterministic, transmittance, xy_stride;
    float exponent, opacity_scale, inv_w, inv_h;
    const float *logits, *xy_raw, *ray_xy, *near, *far, *u;
    float *depth, *opacity, *coords;
    int* index;
    const float *g_depth, *g_opacity, *g_coords;
    float *g_logits, *g_xy;
};

void launch_depth_head_forward(const DepthHeadArgs& a, hipStream_t s);
void launch_depth_head_backward(const DepthHeadArgs& a, hipStream_t s);

}  // namespace ggr

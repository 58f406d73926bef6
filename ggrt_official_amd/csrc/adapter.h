// adapter.h — launchers of the Gaussian adapter pass (adapter.hip): GGRt's encoder tail (raw network output + depth + ray
// coordinates → means, scales, world-space quaternions, rotated harmonics) in one launch, and its backward in one launch.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kAdapterTile = 64;        // raw rows per tile = lanes per workgroup (one wave)
constexpr int kAdapterMaxChunks = 2048; // workgroups over all cameras, about: the rest of a camera's tiles is strided over

// C cameras × G Gaussians, row p = c·G + g; `spp` consecutive Gaussians share one raw row (G % spp == 0).
// d_sh ∈ {1, 4, 9, 16, 25}.  All pointers are device pointers to dense float32 arrays:
//   depth [C,G]  coords [C,G,2]  raw [C,G/spp,7+3·d_sh] = (scale logits 3, quaternion xyzw 4, harmonics (xyz d_sh))
//   c2w [C,3,4]  Kinv [C,3,3]  q_cam [C,4] wxyz  scale_mult [C]  sh_transform [C,d_sh,d_sh] (diagonal blocks read)  sh_mask [d_sh]
//   means [P,3]  scales [P,3]  quats [P,4] wxyz  harmonics [P,3,d_sh]                       (forward: every element written)
//   g_means … g_harmonics: the gradients w.r.t. those four (backward: all four required)
//   g_raw [C,G/spp,7+3·d_sh] (written whole)  g_depth [C,G] / g_coords [C,G,2] (written whole; may be null)
//   g_c2w [C,3,4]  g_Kinv [C,3,3]  g_q_cam [C,4]  g_scale_mult [C]  g_sh_transform [C,d_sh,d_sh]: each may be null (skipped);
//   the launch ADDS into them with float atomics, one add per workgroup and element: the caller zero-initialises them.
struct AdapterArgs {
    int C, G, spp, d_sh;
    float scale_min, scale_max, eps;
    const float *depth, *coords, *raw, *c2w, *Kinv, *q_cam, *scale_mult, *sh_transform, *sh_mask;
    float *means, *scales, *quats, *harmonics;
    const float *g_means, *g_scales, *g_quats, *g_harmonics;
    float *g_raw, *g_depth, *g_coords, *g_c2w, *g_Kinv, *g_q_cam, *g_scale_mult, *g_sh_transform;
};

void launch_adapter_forward(const AdapterArgs& a, hipStream_t s);
void launch_adapter_backward(const AdapterArgs& a, hipStream_t s);

}  // namespace ggr

// upsample_depth.h — launchers of the convex depth upsampling pass (upsample_depth.hip): GGRt's DepthPoseNet.upsample_depth
// (ggrt/depth_pose_network.py) — a softmax over the 9 taps of a [N, 9 r r, h, w] mask, the convex combination of each cell's 3 x 3
// neighbourhood into r x r sub-pixels, a bilinear resize (align_corners) to the image size and, optionally, disp_to_depth's affine
// map — for a whole stacked batch in two launches forward and two backward.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kUpsampleTilePixels = 64;     // a workgroup owns 64 consecutive cells of the flattened h x w plane: one wave along x
constexpr int kUpsampleWaves = 4;           // ... and four waves, each on its own sub-pixels (sub-pixel i r + j belongs to wave (i r + j) % 4)
constexpr int kUpsampleThreads = kUpsampleTilePixels * kUpsampleWaves;
constexpr int kUpsampleMaxRatio = 8;        // r
constexpr int kUpsampleMaxSide = 1 << 16;   // r h, r w, Ho and Wo: a float source coordinate is exact to 2^-7 of a pixel up to here

// depth [N,h,w]; mask [N,9 r r,h,w]; out [N,Ho,Wo]; all device pointers, float32, dense.
struct UpsampleDepthArgs {
    int N, h, w, r, Ho, Wo, disp_on;
    float disp_a, disp_b;                   // out = disp_a + disp_b * resized when disp_on
    float sy, sx;                           // (r h - 1) / (Ho - 1) and (r w - 1) / (Wo - 1) in float, 0 where the output side is 1
    float inv_sy, inv_sx;                   // (Ho - 1) / (r h - 1) and (Wo - 1) / (r w - 1), 0 where sy or sx is 0 (backward: where to look)
    const float *depth, *mask;
    float* out;                 // forward
    float* workspace;           // forward: up [N, r h, r w] (unused at the identity size); backward: the tap sums [N,9,h,w]
    const float* g_out;         // backward: as out
    float *g_mask, *g_depth;    // backward: each may be NULL
};

int64_t upsample_depth_tiles(int h, int w);
int64_t upsample_depth_workspace_floats(int N, int h, int w, int r);

void launch_upsample_depth_forward(const UpsampleDepthArgs& a, hipStream_t s);
void launch_upsample_depth_backward(const UpsampleDepthArgs& a, hipStream_t s);

}  // namespace ggr

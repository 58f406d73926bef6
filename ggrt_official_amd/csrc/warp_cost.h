// warp_cost.h — launchers of the feature-metric cost map pass (warp_cost.hip): GGRt's DepthPoseNet.get_cost_each / depth_cost_calc
// (ggrt/depth_pose_network.py) — lift with the scaled K and 1/inv_depth, move by each view's pose, project with the view's scaled K,
// gather its feature map bilinearly, square the difference — for all V views in one launch forward and two backward.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kWarpTilePixels = 64;         // a workgroup owns 64 consecutive pixels of the flattened h x w plane: one wave along x
constexpr int kWarpGroups = 8;              // ... and eight waves, each on its own channels (channel c belongs to wave c % 8)
constexpr int kWarpThreads = kWarpTilePixels * kWarpGroups;
constexpr int kWarpChannelSlice = 32;       // forward: channels per workgroup (four per wave)
constexpr int kWarpMaxViews = 16;           // V
constexpr int kWarpMaxSide = 1 << 14;       // h and w
constexpr int kWarpMaxChannels = 1 << 16;   // C
constexpr int kWarpPosePartials = 12;       // doubles per (tile, view): dL/dR (9, row-major) and dL/dt (3)

// fmap [C,h,w]; fmaps_ref [V,C,h,w]; inv_depth [h,w]; K [9] and ref_Ks [V,9] at FULL resolution; poses [V,6] (t, then the Euler
// angles x, y, z); all device pointers, float32, dense.  cost [V,C,h,w], or [C,h,w] with `mean`.
struct WarpCostArgs {
    int V, C, h, w, mean, disp_on;
    float scale, disp_a, disp_b;            // d = disp_a + disp_b * inv_depth when disp_on
    const float *fmap, *fmaps_ref, *inv_depth, *K, *ref_Ks, *poses;
    float* cost;                // forward
    int* cells;                 // forward: [V,h,w,3] or NULL
    double* workspace;          // backward: [tiles][V][12]
    const float* g_cost;        // backward: as cost
    float *g_fmap, *g_fmaps_ref, *g_inv, *g_poses;      // backward: each may be NULL; g_fmaps_ref is ACCUMULATED into (zero on entry)
};

int64_t warp_cost_tiles(int h, int w);
int64_t warp_cost_workspace_doubles(int V, int h, int w);

void launch_warp_cost_forward(const WarpCostArgs& a, hipStream_t s);
void launch_warp_cost_backward(const WarpCostArgs& a, hipStream_t s);

}  // namespace ggr

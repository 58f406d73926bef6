// warp_cost.hip — GGRt's feature-metric cost map (ggrt/depth_pose_network.py: DepthPoseNet.get_cost_each, depth_cost_calc) with its
// geometry (ggrt/geometry/camera.py: Camera.scaled / reconstruct / project, depth.py: inv2depth, disp_to_depth; ggrt/pose_util.py:
// Pose.from_vec), for one target feature map [C,h,w], V reference maps, one inverse-depth map and one pose per view.
//
// A workgroup is 8 waves over 64 consecutive pixels of the flattened plane (lanes run along x: the maps are channel-planar): the
// sample coordinates of its pixels are computed ONCE per view, into LDS, and the waves split the channels (c % 8).
//
// Forward, one launch, grid (pixel tiles, channel slices of 32, V) — or (tiles, slices, 1) with `mean`, the views looped inside so
// that the mean is one register sum in the order of the views: cost = (fmap - bilinear(fmaps_ref[v]; u, v))^2.
//
// Backward, two launches:
//   1 grid (pixel tiles), the views looped inside, every channel: per (pixel, channel) the thread forms dL/dfmap (summed over the
//     views in its own output element, which no other thread touches), scatters dL/dfmaps_ref through the four taps with float
//     atomics, and adds its channels' share of dL/du, dL/dv; the eight waves' shares meet in LDS in a fixed order, and wave 0 takes
//     them through the projection into the pose (12 double sums per workgroup and view: dL/dR, dL/dt) and the pixel's inverse depth
//     (summed over the views in a register, written once).
//   2 one workgroup per view: adds the 12 sums over the tiles in a fixed order and chains them into the six numbers.
// Everything but dL/dfmaps_ref has a fixed order of summation: two runs give the same bits.  The backward calls the forward's own
// `project` and `taps_at` (warp_geometry.h, shared with photometric_loss.hip), compiled without contraction, so it makes the
// forward's floor and clamp decisions without storing them.  This file keeps what is the cost map's own: `scaled_K`, the folded
// disparity, `tile_coordinates`, the channel split, the scatter with atomics and the LDS meeting of the eight waves.
#include "warp_cost.h"
#include "block_reduce.h"
#include "warp_geometry.h"
#include <math.h>

namespace ggr {

int64_t warp_cost_tiles(int h, int w) { return ((int64_t)h * w + kWarpTilePixels - 1) / kWarpTilePixels; }
int64_t warp_cost_workspace_doubles(int V, int h, int w) { return warp_cost_tiles(h, w) * V * kWarpPosePartials; }

namespace {

constexpr int TP = kWarpTilePixels, G = kWarpGroups, NT = kWarpThreads, MV = kWarpMaxViews, CS = kWarpChannelSlice;
constexpr int KPT = CS / G;     // forward: channels per thread

// scale_intrinsics (Camera.scaled returns the camera itself for a factor of exactly 1)
__device__ __forceinline__ void scaled_K(const float* K, float s, float* out) {
#pragma clang fp contract(off)
    for (int k = 0; k < 9; ++k) out[k] = K[k];
    if (s == 1.f) return;
    out[0] = K[0] * s;
    out[4] = K[4] * s;
    out[2] = (K[2] + 0.5f) * s - 0.5f;
    out[5] = (K[5] + 0.5f) * s - 0.5f;
}

// Camera.Kinv of the scaled target camera, the pose of view j and the view's scaled intrinsics
__device__ void setup_cam(const WarpCostArgs& a, int j, Cam* c) {
    float K[9];
    scaled_K(a.K, a.scale, K);
    kinv_closed_form(K, c->Kinv);
    pose_from_vec(a.poses + (int64_t)j * 6, c->R, c->t);
    scaled_K(a.ref_Ks + (int64_t)j * 9, a.scale, c->Kr);
}

// disp_to_depth's affine map (when folded) in front of inv2depth
__device__ __forceinline__ float inverse_depth(const WarpCostArgs& a, float inv) {
#pragma clang fp contract(off)
    return a.disp_on ? a.disp_a + a.disp_b * inv : inv;
}

// the sample coordinates of the tile's pixels for views v0 .. v0 + nv - 1, once per workgroup
__device__ __forceinline__ void tile_coordinates(const WarpCostArgs& a, int v0, int nv, int64_t hw, Cam* cam, float (*sU)[TP], float (*sV)[TP],
                                                 bool write_cells) {
    if ((int)threadIdx.x < nv) setup_cam(a, v0 + (int)threadIdx.x, &cam[threadIdx.x]);
    __syncthreads();
    for (int idx = threadIdx.x; idx < nv * TP; idx += NT) {
        const int vi = idx / TP, l = idx - vi * TP;
        const int64_t q = (int64_t)blockIdx.x * TP + l;
        float u = 0.f, v = 0.f;
        if (q < hw) {
            const int y = (int)(q / a.w), x = (int)(q - (int64_t)y * a.w);
            const Proj pr = project(cam[vi], inverse_depth(a, a.inv_depth[q]), x, y);
            u = pr.u;
            v = pr.v;
            if (write_cells) {
                const Taps t = taps_at(u, v, a.h, a.w);
                int* c = a.cells + ((int64_t)(v0 + vi) * hw + q) * 3;
                c[0] = t.ix;
                c[1] = t.iy;
                c[2] = pr.P2 >= 1e-5f ? 0 : 1;
            }
        }
        sU[vi][l] = u;
        sV[vi][l] = v;
    }
    __syncthreads();
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void warp_cost_fwd_kernel(const WarpCostArgs a) {
    __shared__ Cam cam[MV];
    __shared__ float sU[MV][TP], sV[MV][TP];
    const int lane = threadIdx.x & (TP - 1), g = threadIdx.x / TP;
    const int64_t hw = (int64_t)a.h * a.w, p = (int64_t)blockIdx.x * TP + lane;
    const int nv = a.mean ? a.V : 1, v0 = a.mean ? 0 : (int)blockIdx.z;
    tile_coordinates(a, v0, nv, hw, cam, sU, sV, a.cells != nullptr && blockIdx.y == 0);
    if (p >= hw) return;
    const int c0 = (int)blockIdx.y * CS + g;
    float f[KPT], acc[KPT];
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const int c = c0 + G * k;
        f[k] = c < a.C ? a.fmap[(int64_t)c * hw + p] : 0.f;
        acc[k] = 0.f;
    }
    for (int vi = 0; vi < nv; ++vi) {
        const Taps t = taps_at(sU[vi][lane], sV[vi][lane], a.h, a.w);
        const float* ref = a.fmaps_ref + (int64_t)(v0 + vi) * a.C * hw;
        const float w00 = t.wx0 * t.wy0, w01 = t.wx1 * t.wy0, w10 = t.wx0 * t.wy1, w11 = t.wx1 * t.wy1;
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int c = c0 + G * k;
            if (c >= a.C) continue;
            const float* pl = ref + (int64_t)c * hw;
            const float fw = tap(pl, t.o00) * w00 + tap(pl, t.o01) * w01 + tap(pl, t.o10) * w10 + tap(pl, t.o11) * w11;
            const float d = f[k] - fw;
            acc[k] += d * d;
        }
    }
    float* out = a.cost + (a.mean ? 0 : (int64_t)v0 * a.C * hw);
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const int c = c0 + G * k;
        if (c < a.C) out[(int64_t)c * hw + p] = a.mean ? acc[k] / (float)a.V : acc[k];
    }
}

// ---- backward 1 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void warp_cost_bwd_kernel(const WarpCostArgs a) {
    __shared__ Cam cam[MV];
    __shared__ float sU[MV][TP], sV[MV][TP], sGu[G][TP], sGv[G][TP];
    const int lane = threadIdx.x & (TP - 1), g = threadIdx.x / TP;
    const int64_t hw = (int64_t)a.h * a.w, p = (int64_t)blockIdx.x * TP + lane;
    const bool live = p < hw, geometry = a.g_inv != nullptr || a.g_poses != nullptr;
    tile_coordinates(a, 0, a.V, hw, cam, sU, sV, false);
    const int py = live ? (int)(p / a.w) : 0, px = live ? (int)(p - (int64_t)py * a.w) : 0;
    const float inv = (live && g == 0) ? a.inv_depth[p] : 0.f;
    float gd = 0.f;
    for (int v = 0; v < a.V; ++v) {
        float gu = 0.f, gv = 0.f;
        if (live) {
            const Taps t = taps_at(sU[v][lane], sV[v][lane], a.h, a.w);
            const float w00 = t.wx0 * t.wy0, w01 = t.wx1 * t.wy0, w10 = t.wx0 * t.wy1, w11 = t.wx1 * t.wy1;
            const float* ref = a.fmaps_ref + (int64_t)v * a.C * hw;
            float* gref = a.g_fmaps_ref ? a.g_fmaps_ref + (int64_t)v * a.C * hw : nullptr;
            const float* go = a.g_cost + (a.mean ? 0 : (int64_t)v * a.C * hw);
            for (int c = g; c < a.C; c += G) {
                const int64_t o = (int64_t)c * hw;
                const float* pl = ref + o;
                const float v00 = tap(pl, t.o00), v01 = tap(pl, t.o01), v10 = tap(pl, t.o10), v11 = tap(pl, t.o11);
                const float fw = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
                float up = go[o + p];
                if (a.mean) up = up / (float)a.V;
                const float df = 2.f * (a.fmap[o + p] - fw) * up;      // dL/dfmap of this view; dL/d(warped value) is its negative
                if (a.g_fmap) {
                    float* out = a.g_fmap + o + p;                     // (this thread's own element: the views add up in it)
                    *out = v == 0 ? df : *out + df;
                }
                const float gw = -df;
                gu += gw * (t.wy0 * (v01 - v00) + t.wy1 * (v11 - v10));
                gv += gw * (t.wx0 * (v10 - v00) + t.wx1 * (v11 - v01));
                if (gref && gw != 0.f) {
                    if (t.o00 >= 0) atomicAdd(gref + o + t.o00, gw * w00);
                    if (t.o01 >= 0) atomicAdd(gref + o + t.o01, gw * w01);
                    if (t.o10 >= 0) atomicAdd(gref + o + t.o10, gw * w10);
                    if (t.o11 >= 0) atomicAdd(gref + o + t.o11, gw * w11);
                }
            }
        }
        if (!geometry) continue;
        sGu[g][lane] = gu;
        sGv[g][lane] = gv;
        __syncthreads();
        if (g == 0) {
            double acc[kWarpPosePartials];
            for (int k = 0; k < kWarpPosePartials; ++k) acc[k] = 0.0;
            if (live) {
                gu = sGu[0][lane];
                gv = sGv[0][lane];
                for (int k = 1; k < G; ++k) { gu += sGu[k][lane]; gv += sGv[k][lane]; }
                if (gu != 0.f || gv != 0.f) {
                    const float d = inverse_depth(a, inv);
                    // u = P0 / Z, v = P1 / Z, Z = max(P2, 1e-5); P = Kr (R X + t); X = ray * depth  (written out, as in
                    // photometric_loss.hip: see there)
                    const Cam& c = cam[v];
                    const Proj pr = project(c, d, px, py);
                    float gP[3], gY[3], gX[3];
                    gP[0] = gu / pr.Z;
                    gP[1] = gv / pr.Z;
                    gP[2] = pr.P2 >= 1e-5f ? -(gu * pr.u + gv * pr.v) / pr.Z : 0.f;
                    for (int m = 0; m < 3; ++m) gY[m] = c.Kr[m] * gP[0] + c.Kr[3 + m] * gP[1] + c.Kr[6 + m] * gP[2];
                    for (int m = 0; m < 3; ++m) gX[m] = c.R[m] * gY[0] + c.R[3 + m] * gY[1] + c.R[6 + m] * gY[2];
                    for (int m = 0; m < 3; ++m) {
                        for (int l = 0; l < 3; ++l) acc[3 * m + l] = (double)(gY[m] * pr.X[l]);
                        acc[9 + m] = (double)gY[m];
                    }
                    const float gdepth = gX[0] * pr.ray[0] + gX[1] * pr.ray[1] + gX[2] * pr.ray[2];
                    if (d >= 1e-6f) gd += -gdepth * pr.depth * pr.depth;     // (below the clamp, and at or below zero, the depth is a constant)
                }
            }
            if (a.g_poses) {
                double* out = a.workspace + ((int64_t)blockIdx.x * a.V + v) * kWarpPosePartials;
                for (int k = 0; k < kWarpPosePartials; ++k) {
                    const double s = wave_sum(acc[k]);
                    if (lane == 0) out[k] = s;
                }
            }
        }
        __syncthreads();
    }
    if (g == 0 && live && a.g_inv) a.g_inv[p] = a.disp_on ? gd * a.disp_b : gd;
}

// ---- backward 2: dL/dposes from the workgroups' sums ------------------------------------------------------------------------------
__global__ __launch_bounds__(TP) void warp_cost_pose_kernel(const WarpCostArgs a, const int64_t tiles) {
    const int j = blockIdx.x;
    double v[kWarpPosePartials];
    for (int k = 0; k < kWarpPosePartials; ++k) v[k] = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += TP) {
        const double* p = a.workspace + (t * a.V + j) * kWarpPosePartials;
        for (int k = 0; k < kWarpPosePartials; ++k) v[k] += p[k];
    }
    for (int k = 0; k < kWarpPosePartials; ++k) v[k] = wave_sum(v[k]);
    if (threadIdx.x == 0) {
        pose_chain(v, a.poses + (int64_t)j * 6, a.g_poses + (int64_t)j * 6);
    }
}

}  // namespace

void launch_warp_cost_forward(const WarpCostArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)warp_cost_tiles(a.h, a.w), (unsigned)((a.C + CS - 1) / CS), (unsigned)(a.mean ? 1 : a.V));
    hipLaunchKernelGGL(warp_cost_fwd_kernel, grid, dim3(NT), 0, s, a);
}

void launch_warp_cost_backward(const WarpCostArgs& a, hipStream_t s) {
    const int64_t tiles = warp_cost_tiles(a.h, a.w);
    hipLaunchKernelGGL(warp_cost_bwd_kernel, dim3((unsigned)tiles), dim3(NT), 0, s, a);
    if (a.g_poses) hipLaunchKernelGGL(warp_cost_pose_kernel, dim3((unsigned)a.V), dim3(TP), 0, s, a, tiles);
}

}  // namespace ggr

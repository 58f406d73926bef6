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
// `project` and `taps_at`, compiled without contraction, so it makes the forward's floor and clamp decisions without storing them.
#include "warp_cost.h"
#include <math.h>

namespace ggr {

int64_t warp_cost_tiles(int h, int w) { return ((int64_t)h * w + kWarpTilePixels - 1) / kWarpTilePixels; }
int64_t warp_cost_workspace_doubles(int V, int h, int w) { return warp_cost_tiles(h, w) * V * kWarpPosePartials; }

namespace {

constexpr int TP = kWarpTilePixels, G = kWarpGroups, NT = kWarpThreads, MV = kWarpMaxViews, CS = kWarpChannelSlice;
constexpr int KPT = CS / G;     // forward: channels per thread

struct Cam { float Kinv[9], R[9], t[3], Kr[9]; };

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

// Camera.Kinv of the scaled target camera (a clone of K with four entries replaced), Pose.from_vec (R = Rx Ry Rz of the Euler angles,
// translation first) and the view's scaled intrinsics
__device__ void setup_cam(const WarpCostArgs& a, int j, Cam* c) {
#pragma clang fp contract(off)
    float K[9];
    scaled_K(a.K, a.scale, K);
    for (int k = 0; k < 9; ++k) c->Kinv[k] = K[k];
    c->Kinv[0] = 1.f / K[0];
    c->Kinv[4] = 1.f / K[4];
    c->Kinv[2] = -1.f * K[2] / K[0];
    c->Kinv[5] = -1.f * K[5] / K[4];
    const float* p = a.poses + (int64_t)j * 6;
    float sx, cx, sy, cy, sz, cz;
    sincosf(p[3], &sx, &cx);
    sincosf(p[4], &sy, &cy);
    sincosf(p[5], &sz, &cz);
    c->R[0] = cy * cz;                  c->R[1] = -cy * sz;                 c->R[2] = sy;
    c->R[3] = cx * sz + sx * sy * cz;   c->R[4] = cx * cz - sx * sy * sz;   c->R[5] = -sx * cy;
    c->R[6] = sx * sz - cx * sy * cz;   c->R[7] = sx * cz + cx * sy * sz;   c->R[8] = cx * cy;
    c->t[0] = p[0]; c->t[1] = p[1]; c->t[2] = p[2];
    scaled_K(a.ref_Ks + (int64_t)j * 9, a.scale, c->Kr);
}

struct Proj { float d, depth, ray[3], X[3], P2, Z, u, v; };

// disp_to_depth's affine map (when folded), inv2depth, Camera.reconstruct (the target camera's pose is the identity), Camera.project
// with its Z.clamp(min=1e-5); the normalisation 2x/(w-1) - 1 and grid_sample's align_corners=True undo each other: (u, v) is the
// sample position in pixels
__device__ __forceinline__ Proj project(const WarpCostArgs& a, const Cam& c, float inv, int qx, int qy) {
#pragma clang fp contract(off)
    Proj r;
    r.d = a.disp_on ? a.disp_a + a.disp_b * inv : inv;
    r.depth = r.d <= 0.f ? 0.f : 1.f / fmaxf(r.d, 1e-6f);
    const float x = (float)qx, y = (float)qy;
    for (int k = 0; k < 3; ++k) {
        r.ray[k] = c.Kinv[3 * k] * x + c.Kinv[3 * k + 1] * y + c.Kinv[3 * k + 2];
        r.X[k] = r.ray[k] * r.depth;
    }
    float Y[3], P[3];
    for (int k = 0; k < 3; ++k) Y[k] = c.R[3 * k] * r.X[0] + c.R[3 * k + 1] * r.X[1] + c.R[3 * k + 2] * r.X[2] + c.t[k];
    for (int k = 0; k < 3; ++k) P[k] = c.Kr[3 * k] * Y[0] + c.Kr[3 * k + 1] * Y[1] + c.Kr[3 * k + 2] * Y[2];
    r.P2 = P[2];
    r.Z = fmaxf(P[2], 1e-5f);
    r.u = P[0] / r.Z;
    r.v = P[1] / r.Z;
    return r;
}

// the four taps of grid_sample(bilinear, zeros, align_corners=True) at (u, v): the cell, offsets (-1 where the tap lies outside) and
// weights.  A sample that no tap of the map reaches (a NaN or an infinite coordinate too) has the cell (-2, -2).
struct Taps { int ix, iy; int64_t o00, o01, o10, o11; float wx0, wx1, wy0, wy1; };

__device__ __forceinline__ Taps taps_at(float u, float v, int H, int W) {
#pragma clang fp contract(off)
    Taps t;
    t.ix = t.iy = -2;
    t.o00 = t.o01 = t.o10 = t.o11 = -1;
    t.wx0 = t.wx1 = t.wy0 = t.wy1 = 0.f;
    if (!(u > -1.f && u < (float)W && v > -1.f && v < (float)H)) return t;
    const float fx = floorf(u), fy = floorf(v);
    const int ix = (int)fx, iy = (int)fy;
    t.ix = ix; t.iy = iy;
    t.wx0 = (fx + 1.f) - u; t.wx1 = u - fx;
    t.wy0 = (fy + 1.f) - v; t.wy1 = v - fy;
    const bool x0 = ix >= 0, x1 = ix + 1 < W, y0 = iy >= 0, y1 = iy + 1 < H;
    const int64_t base = (int64_t)iy * W + ix;
    if (x0 && y0) t.o00 = base;
    if (x1 && y0) t.o01 = base + 1;
    if (x0 && y1) t.o10 = base + W;
    if (x1 && y1) t.o11 = base + W + 1;
    return t;
}

__device__ __forceinline__ float tap(const float* __restrict__ p, int64_t o) { return o >= 0 ? p[o] : 0.f; }

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
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
            const Proj pr = project(a, cam[vi], a.inv_depth[q], x, y);
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
                    // u = P0 / Z, v = P1 / Z, Z = max(P2, 1e-5); P = Kr (R X + t); X = ray * depth
                    const Cam& c = cam[v];
                    const Proj pr = project(a, c, inv, px, py);
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
                    if (pr.d >= 1e-6f) gd += -gdepth * pr.depth * pr.depth;     // (below the clamp, and at or below zero, the depth is a constant)
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
        const float* p = a.poses + (int64_t)j * 6;
        float* g = a.g_poses + (int64_t)j * 6;
        const double sx = sin((double)p[3]), cx = cos((double)p[3]), sy = sin((double)p[4]), cy = cos((double)p[4]);
        const double sz = sin((double)p[5]), cz = cos((double)p[5]);
        const double R[9] = {cy * cz, -cy * sz, sy, cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy,
                             sx * sz - cx * sy * cz, sx * cz + cx * sy * sz, cx * cy};
        // dR/dx: row 1 becomes -row 2, row 2 becomes row 1
        const double gx = -(v[3] * R[6] + v[4] * R[7] + v[5] * R[8]) + (v[6] * R[3] + v[7] * R[4] + v[8] * R[5]);
        const double gy = v[0] * (-sy * cz) + v[1] * (sy * sz) + v[2] * cy + v[3] * (sx * cy * cz) + v[4] * (-sx * cy * sz) + v[5] * (sx * sy) +
                          v[6] * (-cx * cy * cz) + v[7] * (cx * cy * sz) + v[8] * (-cx * sy);
        const double gz = v[0] * (-cy * sz) + v[1] * (-cy * cz) + v[3] * (cx * cz - sx * sy * sz) + v[4] * (-cx * sz - sx * sy * cz) +
                          v[6] * (sx * cz + cx * sy * sz) + v[7] * (-sx * sz + cx * sy * cz);
        g[0] = (float)v[9]; g[1] = (float)v[10]; g[2] = (float)v[11];
        g[3] = (float)gx; g[4] = (float)gy; g[5] = (float)gz;
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

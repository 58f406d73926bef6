// warp_geometry.h — the reprojection of a target pixel into a reference view, shared by the photometric loss (photometric_loss.hip)
// and the feature-metric cost map (warp_cost.hip): GGRt's Camera.Kinv / reconstruct / project (ggrt/geometry/camera.py), inv2depth
// (depth.py), Pose.from_vec (ggrt/pose_util.py) and grid_sample(bilinear, zeros, align_corners=True), forward and backward.
//
// Everything that decides WHERE a pixel samples — kinv_closed_form, pose_from_vec, project, taps_at — is compiled with
// `fp contract(off)`: every product, sum and division is the same IEEE operation at every call site whatever the optimiser does
// around it, so a backward that calls them again gets the forward's (u, v), floor and clamp decisions without storing them.  The
// pose chain decides nothing and is left to the optimiser.  The twelve lines from (dL/du, dL/dv) back through the projection stay
// written out in the two backward kernels: as a function here they raised the photometric backward's registers past three
// workgroups a CU and changed which products the compiler fuses in the cost map's dL/dinv_depth.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace ggr {

struct Cam { float Kinv[9], R[9], t[3], Kr[9]; };

// Camera.Kinv: a clone of K with four entries replaced
__device__ __forceinline__ void kinv_closed_form(const float* K, float* Kinv) {
#pragma clang fp contract(off)
    for (int k = 0; k < 9; ++k) Kinv[k] = K[k];
    Kinv[0] = 1.f / K[0];
    Kinv[4] = 1.f / K[4];
    Kinv[2] = -1.f * K[2] / K[0];
    Kinv[5] = -1.f * K[5] / K[4];
}

// Pose.from_vec: the translation first, then R = Rx Ry Rz of the Euler angles
__device__ __forceinline__ void pose_from_vec(const float* six, float* R, float* t) {
#pragma clang fp contract(off)
    float sx, cx, sy, cy, sz, cz;
    sincosf(six[3], &sx, &cx);
    sincosf(six[4], &sy, &cy);
    sincosf(six[5], &sz, &cz);
    R[0] = cy * cz;                  R[1] = -cy * sz;                 R[2] = sy;
    R[3] = cx * sz + sx * sy * cz;   R[4] = cx * cz - sx * sy * sz;   R[5] = -sx * cy;
    R[6] = sx * sz - cx * sy * cz;   R[7] = sx * cz + cx * sy * sz;   R[8] = cx * cy;
    t[0] = six[0]; t[1] = six[1]; t[2] = six[2];
}

struct Proj { float depth, ray[3], X[3], P2, Z, u, v; };

// inv2depth of the inverse depth d, Camera.reconstruct (the target camera's pose is the identity), Camera.project with its
// Z.clamp(min=1e-5); the normalisation 2x/(W-1) - 1 and grid_sample's align_corners=True undo each other: (u, v) is the sample
// position in pixels
__device__ __forceinline__ Proj project(const Cam& c, float d, int qx, int qy) {
#pragma clang fp contract(off)
    Proj r;
    r.depth = d <= 0.f ? 0.f : 1.f / fmaxf(d, 1e-6f);
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
#pragma clang fp contract(off)      // (nothing here could fuse; the rule of the file header, made visible)
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

__device__ __forceinline__ float sample(const float* __restrict__ p, const Taps& t) {
    return tap(p, t.o00) * (t.wx0 * t.wy0) + tap(p, t.o01) * (t.wx1 * t.wy0) + tap(p, t.o10) * (t.wx0 * t.wy1) + tap(p, t.o11) * (t.wx1 * t.wy1);
}

// dL/dR (v[0..8], row-major) and dL/dt (v[9..11]) into the gradient of the six pose numbers of `six`
__device__ __forceinline__ void pose_chain(const double (&v)[12], const float* six, float* g) {
    const double sx = sin((double)six[3]), cx = cos((double)six[3]), sy = sin((double)six[4]), cy = cos((double)six[4]);
    const double sz = sin((double)six[5]), cz = cos((double)six[5]);
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

}  // namespace ggr

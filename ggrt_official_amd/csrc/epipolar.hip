// epipolar.hip — the epipolar-sampler pass: GGRt's EpipolarSampler.forward and the depth lines of EpipolarTransformer.forward.
//
// Per pair-ray (bi, vi, ov, ri) — a ray of view vi projected into the other view o = ov + (ov >= vi) — the contract is
// GgrEpipolarPass in include/ggr_raster.h:
//   ray:      xy = ((x+½)/w, (y+½)/h);  d = c2w_v · normalise(Kinv_v·(xy, 1));  origin = c2w_v's translation
//   segment:  project_rays with near_v, far_v: the point projections at t = near, far, the four frame intersections, the
//             reference's validity tests, min / max over the valid intersections (first index on ties), the four-way selection,
//             nan_to_num(·, 0) and the mask                                    → xy_min, xy_max, valid
//   samples:  xy_i = xy_min + (i+½)/s·(xy_max − xy_min), i < s;  features_i = valid · bilinear(images[bi, o], xy_i)
//   depth_i:  the least-squares intersection of the casting ray with view o's ray through xy_i (valid or not), its distance
//             to the origin clipped to [near_v, far_v], as relative disparity
//
// Launch shape.  The feature write is the bound (s·c floats per pair-ray, 16 KiB at 32 × 128, against 7·s floats of everything
// else), so it goes out as whole rows with the channel fastest: a WAVE owns one pair-ray, every lane computes the ray's segment
// (a few hundred flops, the same in all 64 lanes: cheaper than a broadcast), lane i < s owns sample i for the small outputs and
// the depth, and then the wave walks the s samples with its lanes across the channels — every load and store of a tap is one
// run of 256 contiguous bytes.  That needs the feature maps channel-last, which `images` [b,v,c,h,w] is not: one small launch
// lays them out as scratch [b·v, h·w, c] first (a tiled transpose through LDS; 1/32 of the output's bytes at s = 32, v = 2).
// Four waves share a workgroup and nothing else: no LDS, no barrier in the main kernel.
// The backward walks the same pair-rays, reads the saved segment (xy_min, xy_max, valid: 17 B per pair-ray), recomputes taps and
// weights, and adds dL/dfeatures·weight into a channel-last accumulator with float atomics (runs of 256 contiguous bytes per
// wave-instruction); a transpose launch then writes dL/dimages [b,v,c,h,w] whole.  The sum's order is the hardware's: two runs
// agree to rounding, not to the bit.
#include "epipolar.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

namespace ggr {

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = kEpipolarWaves;
constexpr int TT = 32;   // the layout kernels' tile: 32 pixels × 32 channels

struct Hit { float t, x, y; bool ok; };
struct Segment { float x0, y0, x1, y1; bool valid; };
struct PairRay { int cam_v, cam_o, ov, ri; };

__device__ __forceinline__ bool in_unit(float q) { return q >= -1e-6f && q <= 1.f + 1e-6f; }
__device__ __forceinline__ float clamp_nonfinite(float q) { return isnan(q) ? 0.f : (isinf(q) ? (q > 0.f ? 1e8f : -1e8f) : q); }
__device__ __forceinline__ float zero_nonfinite(float q) { return isfinite(q) ? q : 0.f; }

__device__ __forceinline__ PairRay decode(const EpipolarArgs& a, int p, int R) {
    PairRay q;
    q.ri = p % R;
    int t = p / R;
    q.ov = t % (a.v - 1);
    t /= (a.v - 1);
    const int vi = t % a.v, bi = t / a.v;
    q.cam_v = bi * a.v + vi;
    q.cam_o = bi * a.v + q.ov + (q.ov >= vi ? 1 : 0);
    return q;
}

// where the projected ray crosses the frame line (DIM, value): _intersect_image_coordinate
template <int DIM>
__device__ __forceinline__ Hit frame_hit(const float* K, const float* O, const float* D, float value) {
    constexpr int OD = 1 - DIM;
    const float fs = K[4 * DIM], fo = K[4 * OD], cs = K[3 * DIM + 2], co = K[3 * OD + 2];
    const float os = O[DIM], oo = O[OD], ds = D[DIM], dd = D[OD], oz = O[2], dz = D[2];
    const float c = (value - cs) / fs;
    Hit h;
    h.t = (c * oz - os) / (ds - c * dz);
    const float other = co + fo * (oo * (c * dz - ds) + dd * (os - c * oz)) / (dz * os - ds * oz);
    const float z = oz + h.t * dz;
    h.ok = in_unit(other) && z > -1e-6f && h.t > -1e-6f;
    h.x = DIM == 0 ? value : other;
    h.y = DIM == 0 ? other : value;
    return h;
}

// the projection of O + t·D: project_camera_space (epsilon, ±1e8) and the three tests
__device__ __forceinline__ Hit point_hit(const float* K, const float* O, const float* D, float t) {
    const float px = O[0] + t * D[0], py = O[1] + t * D[1], pz = O[2] + t * D[2];
    const float den = pz + FLT_EPSILON;
    const float qx = clamp_nonfinite(px / den), qy = clamp_nonfinite(py / den), qz = clamp_nonfinite(pz / den);
    Hit h;
    h.t = t;
    h.x = K[0] * qx + K[1] * qy + K[2] * qz;
    h.y = K[3] * qx + K[4] * qy + K[5] * qz;
    h.ok = in_unit(h.x) && in_unit(h.y) && pz > -1e-6f && t > -1e-6f;
    return h;
}

template <bool LARGEST>
__device__ __forceinline__ Hit reduce_hits(const Hit (&h)[4]) {
    const float lowest = LARGEST ? -INFINITY : INFINITY;
    Hit best = h[0];
    float bt = h[0].ok ? h[0].t : lowest;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const float t = h[i].ok ? h[i].t : lowest;
        if (LARGEST ? t > bt : t < bt) { bt = t; best = h[i]; }   // (strict: the first index keeps a tie)
    }
    return best;
}

__device__ __forceinline__ void load9(const float* p, float* m) {
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = p[i];
}

// rows 0..2 of a 4×4: R (9) and t (3)
__device__ __forceinline__ void load_rigid(const float* p, float* R, float* t) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = p[4 * i + j];
        t[i] = p[4 * i + 3];
    }
}

__device__ __forceinline__ void mat3_mul(const float* M, const float* x, float* y) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = M[3 * i] * x[0] + M[3 * i + 1] * x[1] + M[3 * i + 2] * x[2];
}

// get_world_rays' direction through the normalised image point (x, y)
__device__ __forceinline__ void world_direction(const float* Kinv, const float* R, float x, float y, float* d) {
    float c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = Kinv[3 * i] * x + Kinv[3 * i + 1] * y + Kinv[3 * i + 2];
    const float n = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    c[0] /= n; c[1] /= n; c[2] /= n;
    mat3_mul(R, c, d);
}

__device__ __forceinline__ float sample_pos(int i, int s) { return ((float)i + 0.5f) / (float)s; }
__device__ __forceinline__ float lerp_at(float lo, float hi, float pos) { return fmaf(pos, hi - lo, lo); }

__device__ __forceinline__ void cross3(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the four taps of grid_sample(bilinear, zeros, align_corners=False) at the normalised point (x, y): pixel offsets (−1: the tap
// lies outside and contributes nothing) and weights, in grid_sample's order nw, ne, sw, se and with its arithmetic
struct Taps { int at[4]; float w[4]; };

__device__ __forceinline__ Taps bilinear_taps(float x, float y, int w, int h) {
    const float ix = ((2.f * x - 1.f + 1.f) * (float)w - 1.f) * 0.5f, iy = ((2.f * y - 1.f + 1.f) * (float)h - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    const float wx0 = (fx + 1.f) - ix, wx1 = ix - fx, wy0 = (fy + 1.f) - iy, wy1 = iy - fy;
    // (compared as floats first: a point far outside, or NaN, never reaches the conversion)
    const bool x0_in = fx >= 0.f && fx <= (float)(w - 1), x1_in = fx >= -1.f && fx <= (float)(w - 2);
    const bool y0_in = fy >= 0.f && fy <= (float)(h - 1), y1_in = fy >= -1.f && fy <= (float)(h - 2);
    const int px = (x0_in || x1_in) ? (int)fx : 0, py = (y0_in || y1_in) ? (int)fy : 0;
    Taps t;
    t.at[0] = (x0_in && y0_in) ? py * w + px : -1;
    t.at[1] = (x1_in && y0_in) ? py * w + px + 1 : -1;
    t.at[2] = (x0_in && y1_in) ? (py + 1) * w + px : -1;
    t.at[3] = (x1_in && y1_in) ? (py + 1) * w + px + 1 : -1;
    t.w[0] = wx0 * wy0; t.w[1] = wx1 * wy0; t.w[2] = wx0 * wy1; t.w[3] = wx1 * wy1;
    return t;
}

// images [b,v,c,h,w] (any strides) → out [b·v, h·w, c]: a 32 × 32 tile through LDS, read along x, written along c
__global__ void __launch_bounds__(TT * 8)
epipolar_to_channel_last_kernel(const EpipolarArgs a) {
    __shared__ float tile[TT][TT + 1];
    const int cam = blockIdx.z, bi = cam / a.v, vi = cam % a.v, hw = a.h * a.w;
    const int p0 = blockIdx.x * TT, c0 = blockIdx.y * TT, tx = threadIdx.x, ty = threadIdx.y;
    const float* src = a.images + (long long)bi * a.img_sb + (long long)vi * a.img_sv;
    const int p = p0 + tx;
    if (p < hw) {
        const int y = p / a.w, x = p - y * a.w;
        const long long off = (long long)y * a.img_sh + (long long)x * a.img_sw;
        for (int k = ty; k < TT; k += 8)
            if (c0 + k < a.c) tile[k][tx] = src[(long long)(c0 + k) * a.img_sc + off];
    }
    __syncthreads();
    if (c0 + tx < a.c)
        for (int k = ty; k < TT; k += 8)
            if (p0 + k < hw) a.scratch[((size_t)cam * hw + p0 + k) * a.c + c0 + tx] = tile[tx][k];
}

// acc [b·v, h·w, c] → g_images [b,v,c,h,w] dense, every element written
__global__ void __launch_bounds__(TT * 8)
epipolar_from_channel_last_kernel(const EpipolarArgs a) {
    __shared__ float tile[TT][TT + 1];
    const int cam = blockIdx.z, hw = a.h * a.w;
    const int p0 = blockIdx.x * TT, c0 = blockIdx.y * TT, tx = threadIdx.x, ty = threadIdx.y;
    if (c0 + tx < a.c)
        for (int k = ty; k < TT; k += 8)
            if (p0 + k < hw) tile[k][tx] = a.scratch[((size_t)cam * hw + p0 + k) * a.c + c0 + tx];
    __syncthreads();
    if (p0 + tx < hw)
        for (int k = ty; k < TT; k += 8)
            if (c0 + k < a.c) a.g_images[((size_t)cam * a.c + c0 + k) * hw + p0 + tx] = tile[tx][k];
}

__global__ void __launch_bounds__(WAVE * WAVES)
epipolar_fwd_kernel(const EpipolarArgs a, const int total) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: the ray's math is the same in all lanes)
    const int ww = a.x1 - a.x0, R = ww * (a.y1 - a.y0), s = a.s, c = a.c, hw = a.h * a.w;
    const float* maps = a.scratch;

    for (int p = blockIdx.x * WAVES + wave; p < total; p += gridDim.x * WAVES) {
        const PairRay q = decode(a, p, R);
        // ---- the ray (generate_image_rays)
        const int ry = q.ri / ww, rx = q.ri - ry * ww;
        const float xr = ((float)(a.x0 + rx) + 0.5f) / (float)a.w, yr = ((float)(a.y0 + ry) + 0.5f) / (float)a.h;
        float Kinv_v[9], Rv[9], org[3], dir[3];
        load9(a.Kinv + 9 * q.cam_v, Kinv_v);
        load_rigid(a.c2w + 16 * q.cam_v, Rv, org);
        world_direction(Kinv_v, Rv, xr, yr, dir);
        const float near = a.near[q.cam_v], far = a.far[q.cam_v];
        if (q.ov == 0 && lane == 0) {
            const size_t at = (size_t)q.cam_v * R + q.ri;
            if (a.xy_ray) { a.xy_ray[2 * at] = xr; a.xy_ray[2 * at + 1] = yr; }
            if (a.origins) { a.origins[3 * at] = org[0]; a.origins[3 * at + 1] = org[1]; a.origins[3 * at + 2] = org[2]; }
            if (a.directions) { a.directions[3 * at] = dir[0]; a.directions[3 * at + 1] = dir[1]; a.directions[3 * at + 2] = dir[2]; }
        }
        // ---- its segment in view o (project_rays)
        float K[9], Rw[9], tw[3], O[3], D[3];
        load9(a.K + 9 * q.cam_o, K);
        load_rigid(a.w2c + 16 * q.cam_o, Rw, tw);
        mat3_mul(Rw, org, O);
        O[0] += tw[0]; O[1] += tw[1]; O[2] += tw[2];
        mat3_mul(Rw, dir, D);
        const Hit frame[4] = {frame_hit<0>(K, O, D, 0.f), frame_hit<0>(K, O, D, 1.f), frame_hit<1>(K, O, D, 0.f), frame_hit<1>(K, O, D, 1.f)};
        const Hit at_near = point_hit(K, O, D, near), at_far = point_hit(K, O, D, far);
        const Hit lo = at_near.ok ? at_near : reduce_hits<false>(frame), hi = at_far.ok ? at_far : reduce_hits<true>(frame);
        Segment g;
        g.valid = lo.ok && hi.ok;
        const float m = g.valid ? 1.f : 0.f;
        g.x0 = zero_nonfinite(lo.x) * m; g.y0 = zero_nonfinite(lo.y) * m;
        g.x1 = zero_nonfinite(hi.x) * m; g.y1 = zero_nonfinite(hi.y) * m;
        if (lane == 0) {
            if (a.valid) a.valid[p] = g.valid ? 1 : 0;
            if (a.seg) { a.seg[4 * (size_t)p] = g.x0; a.seg[4 * (size_t)p + 1] = g.y0; a.seg[4 * (size_t)p + 2] = g.x1; a.seg[4 * (size_t)p + 3] = g.y1; }
        }
        // ---- lane i: sample i's coordinates and depth
        if (lane < s) {
            const size_t at = (size_t)p * s + lane;
            const float pos = sample_pos(lane, s), half = 0.5f / (float)s;
            const float xs = lerp_at(g.x0, g.x1, pos), ys = lerp_at(g.y0, g.y1, pos);
            if (a.xy_sample) { a.xy_sample[2 * at] = xs; a.xy_sample[2 * at + 1] = ys; }
            if (a.xy_near) { a.xy_near[2 * at] = lerp_at(g.x0, g.x1, pos - half); a.xy_near[2 * at + 1] = lerp_at(g.y0, g.y1, pos - half); }
            if (a.xy_far) { a.xy_far[2 * at] = lerp_at(g.x0, g.x1, pos + half); a.xy_far[2 * at + 1] = lerp_at(g.y0, g.y1, pos + half); }
            if (a.depth) {
                float Kinv_o[9], Ro[9], oo[3], dy[3], r[3], n[3], c1[3], c2[3];
                load9(a.Kinv + 9 * q.cam_o, Kinv_o);
                load_rigid(a.c2w + 16 * q.cam_o, Ro, oo);
                world_direction(Kinv_o, Ro, xs, ys, dy);
                float raw;
                if (dot3(dir, dy) > 1.f - 1e-5f) {
                    const float e0 = 1e10f - org[0], e1 = 1e10f - org[1], e2 = 1e10f - org[2];
                    raw = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
                } else {
                    // the least-squares point of two lines is the midpoint of their common perpendicular; taken relative to the
                    // casting ray's origin:  p − o = ½(t1·d + r + t2·dy),  r = o_y − o,  n = d × dy,
                    // t1 = ((r × dy)·n)/|n|²,  t2 = ((r × d)·n)/|n|²   (the closed-form solution of the 3×3 normal system)
                    r[0] = oo[0] - org[0]; r[1] = oo[1] - org[1]; r[2] = oo[2] - org[2];
                    cross3(dir, dy, n);
                    cross3(r, dy, c1);
                    cross3(r, dir, c2);
                    const float nn = dot3(n, n), t1 = dot3(c1, n) / nn, t2 = dot3(c2, n) / nn;
                    const float e0 = 0.5f * (t1 * dir[0] + r[0] + t2 * dy[0]), e1 = 0.5f * (t1 * dir[1] + r[1] + t2 * dy[1]),
                                e2 = 0.5f * (t1 * dir[2] + r[2] + t2 * dy[2]);
                    raw = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
                }
                raw = fminf(fmaxf(raw, near), far);
                const float dn = 1.f / (near + 1e-10f), df = 1.f / (far + 1e-10f);
                a.depth[at] = 1.f - (1.f / (raw + 1e-10f) - df) / (dn - df + 1e-10f);
            }
        }
        // ---- the features: lanes across channels, one sample after the other
        if (a.features) {
            float* out = a.features + (size_t)p * s * c;
            if (!g.valid) {
                for (int i = lane; i < s * c; i += WAVE) out[i] = 0.f;
            } else {
                const float* map = maps + (size_t)q.cam_o * hw * c;
#pragma unroll 4
                for (int i = 0; i < s; ++i) {
                    const float pos = sample_pos(i, s);
                    const Taps t = bilinear_taps(lerp_at(g.x0, g.x1, pos), lerp_at(g.y0, g.y1, pos), a.w, a.h);
                    for (int ch = lane; ch < c; ch += WAVE) {
                        float acc = 0.f;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (t.at[k] >= 0) acc += map[(size_t)t.at[k] * c + ch] * t.w[k];
                        out[(size_t)i * c + ch] = acc;
                    }
                }
            }
        }
    }
}

// the accumulator's zeroes, as a kernel: a node like the others when the launches are captured into a graph
__global__ void __launch_bounds__(256)
epipolar_zero_kernel(float* __restrict__ p, const size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0.f;
}

__global__ void __launch_bounds__(WAVE * WAVES)
epipolar_bwd_kernel(const EpipolarArgs a, const int total) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ww = a.x1 - a.x0, R = ww * (a.y1 - a.y0), s = a.s, c = a.c, hw = a.h * a.w;

    for (int p = blockIdx.x * WAVES + wave; p < total; p += gridDim.x * WAVES) {
        if (!a.valid[p]) continue;
        const PairRay q = decode(a, p, R);
        const float x0 = a.seg[4 * (size_t)p], y0 = a.seg[4 * (size_t)p + 1], x1 = a.seg[4 * (size_t)p + 2], y1 = a.seg[4 * (size_t)p + 3];
        const float* g = a.g_features + (size_t)p * s * c;
        float* acc = a.scratch + (size_t)q.cam_o * hw * c;
#pragma unroll 2
        for (int i = 0; i < s; ++i) {
            const float pos = sample_pos(i, s);
            const Taps t = bilinear_taps(lerp_at(x0, x1, pos), lerp_at(y0, y1, pos), a.w, a.h);
            for (int ch = lane; ch < c; ch += WAVE) {
                const float gv = g[(size_t)i * c + ch];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (t.at[k] >= 0) atomicAdd(acc + (size_t)t.at[k] * c + ch, gv * t.w[k]);
            }
        }
    }
}

int pair_rays(const EpipolarArgs& a) { return a.b * a.v * (a.v - 1) * (a.y1 - a.y0) * (a.x1 - a.x0); }   // (checked < 2^31 by the caller)

dim3 layout_grid(const EpipolarArgs& a) {
    return dim3((unsigned)((a.h * a.w + TT - 1) / TT), (unsigned)((a.c + TT - 1) / TT), (unsigned)(a.b * a.v));
}

}  // namespace

void launch_epipolar_forward(const EpipolarArgs& a, hipStream_t s) {
    const int total = pair_rays(a);
    if (total <= 0) return;
    if (a.features) hipLaunchKernelGGL(epipolar_to_channel_last_kernel, layout_grid(a), dim3(TT, 8), 0, s, a);
    const int groups = std::min((total + WAVES - 1) / WAVES, kEpipolarMaxGroups);
    hipLaunchKernelGGL(epipolar_fwd_kernel, dim3((unsigned)groups), dim3(WAVE * WAVES), 0, s, a, total);
}

void launch_epipolar_backward(const EpipolarArgs& a, hipStream_t s) {
    const int total = pair_rays(a);
    if (total <= 0) return;
    const size_t cells = (size_t)a.b * a.v * a.h * a.w * a.c;
    hipLaunchKernelGGL(epipolar_zero_kernel, dim3((unsigned)std::min<size_t>((cells + 255) / 256, 4096)), dim3(256), 0, s, a.scratch, cells);
    const int groups = std::min((total + WAVES - 1) / WAVES, kEpipolarMaxGroups);
    hipLaunchKernelGGL(epipolar_bwd_kernel, dim3((unsigned)groups), dim3(WAVE * WAVES), 0, s, a, total);
    hipLaunchKernelGGL(epipolar_from_channel_last_kernel, layout_grid(a), dim3(TT, 8), 0, s, a);
}

}  // namespace ggr

// upsample_depth.hip — GGRt's convex depth upsampling (ggrt/depth_pose_network.py: DepthPoseNet.upsample_depth, with
// ggrt/geometry/depth.py: disp_to_depth folded) for a stacked batch of N maps: depth [N,h,w], mask [N,9 r r,h,w] -> out [N,Ho,Wo].
//
// The mask is the traffic (9 r r floats per cell against r r written), and for one channel it is contiguous along the flattened
// (y, x).  A workgroup is 4 waves over 64 consecutive cells of that flattened plane: lanes run along the cells, so each of the nine
// tap reads of a sub-pixel is one contiguous wave access, and the waves split the r r sub-pixels.  What is strided by r across those
// lanes — the writes of `up` forward, the reads of dL/dup backward — goes through LDS, and leaves or enters memory in runs of 64 r
// consecutive floats per sub-row.
//
// Forward, two launches (one at the identity size, where the first writes `out` itself):
//   1 grid (N x tiles): per cell the 9 zero-padded depth taps, per sub-pixel the softmax over its 9 logits (maximum subtracted) and
//     the convex sum -> LDS -> up [N, r h, r w] in the workspace.
//   2 one thread per output pixel: the bilinear resize with align_corners (source = scale * destination in float, as torch forms
//     it; weights (1 - l, l)) and the affine map.
// Backward, two launches, both gathers with a fixed order of summation (no atomics, nothing to zero):
//   1 grid (N x tiles): every up pixel of the tile gathers the output pixels whose taps reach it (the forward's own index
//     arithmetic decides which) -> LDS; per sub-pixel the softmax is recomputed from the mask, dL/dmask = p_k g (d_k - up) is written
//     whole, and the per-tap sums S_k = sum over sub-pixels of p_k g meet across the four waves in LDS in a fixed order and go to
//     the workspace [N,9,h,w].
//   2 one thread per cell: dL/ddepth = the 9 tap sums of the neighbouring cells that read this cell.  Skipped without dL/ddepth.
#include "upsample_depth.h"
#include <math.h>

namespace ggr {

int64_t upsample_depth_tiles(int h, int w) { return ((int64_t)h * w + kUpsampleTilePixels - 1) / kUpsampleTilePixels; }
int64_t upsample_depth_workspace_floats(int N, int h, int w, int r) { return (int64_t)N * h * w * (r * r > 9 ? r * r : 9); }

namespace {

constexpr int TP = kUpsampleTilePixels, G = kUpsampleWaves, NT = kUpsampleThreads, MR = kUpsampleMaxRatio;
constexpr int STR = TP + 8;     // LDS row of one sub-pixel: the transposed access (j fastest, then the cell) lands 2-way on the banks

// the 9 zero-padded taps of cell (y, x): F.unfold(depth, 3, padding=1), tap k = ky 3 + kx reads (y + ky - 1, x + kx - 1)
__device__ __forceinline__ void depth_taps(const float* __restrict__ d, int y, int x, int h, int w, float* t) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        t[k] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? d[yy * w + xx] : 0.f;
    }
}

// softmax over the 9 logits of one (cell, sub-pixel): channel k r r + ij of the cell's image, hw apart
__device__ __forceinline__ void tap_softmax(const float* __restrict__ m, int r2hw, float* p) {
    float mx = -INFINITY, sum = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        p[k] = m[k * r2hw];
        mx = fmaxf(mx, p[k]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        p[k] = expf(p[k] - mx);
        sum += p[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = p[k] / sum;
}

// ---- forward 1: the convex combination ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void upsample_convex_kernel(const UpsampleDepthArgs a, float* __restrict__ dst, const int affine, const int tiles) {
    __shared__ float sUp[MR * MR][STR];
    const int lane = threadIdx.x & (TP - 1), g = threadIdx.x / TP;
    const int n = blockIdx.x / tiles, q0 = (blockIdx.x - n * tiles) * TP;
    const int hw = a.h * a.w, r = a.r, r2 = r * r, q = q0 + lane;
    if (q < hw) {
        const int y = q / a.w, x = q - y * a.w;
        float d[9], p[9];
        depth_taps(a.depth + n * hw, y, x, a.h, a.w, d);
        for (int ij = g; ij < r2; ij += G) {
            tap_softmax(a.mask + (n * 9 * r2 + ij) * hw + q, r2 * hw, p);
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) v += p[k] * d[k];
            sUp[ij][lane] = v;
        }
    }
    __syncthreads();
    // sub-row i of the tile is 64 r consecutive floats of `up` wherever the cells share a row
    const int rw = a.w * r, run = TP * r;
    for (int idx = threadIdx.x; idx < TP * r2; idx += NT) {
        const int i = idx / run, rem = idx - i * run, l = rem / r, j = rem - l * r;
        const int qq = q0 + l;
        if (qq >= hw) continue;
        const int yy = qq / a.w, xx = qq - yy * a.w;
        const float v = sUp[i * r + j][l];
        dst[(n * a.h * r + yy * r + i) * rw + xx * r + j] = affine ? a.disp_a + a.disp_b * v : v;
    }
}

// the two taps of one axis of F.interpolate(bilinear, align_corners=True) for destination index o: source = scale * o
struct Axis { int i0, step; float l0, l1; };

__device__ __forceinline__ Axis axis_taps(int o, float scale, int in) {
#pragma clang fp contract(off)
    Axis t;
    const float src = scale * (float)o;
    t.i0 = min((int)src, in - 1);
    t.step = t.i0 < in - 1 ? 1 : 0;
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// ---- forward 2: the resize and the affine map --------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void upsample_resize_kernel(const UpsampleDepthArgs a, const int total) {
    const int64_t t64 = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t64 >= total) return;
    const int t = (int)t64, H = a.h * a.r, W = a.w * a.r;
    const int ox = t % a.Wo, rest = t / a.Wo, oy = rest % a.Ho, n = rest / a.Ho;
    const Axis ay = axis_taps(oy, a.sy, H), ax = axis_taps(ox, a.sx, W);
    const float* up = a.workspace + (n * H + ay.i0) * W + ax.i0;
    const float v00 = up[0], v01 = up[ax.step], v10 = up[ay.step * W], v11 = up[ay.step * W + ax.step];
    const float v = ay.l0 * (ax.l0 * v00 + ax.l1 * v01) + ay.l1 * (ax.l0 * v10 + ax.l1 * v11);
    a.out[t] = a.disp_on ? a.disp_a + a.disp_b * v : v;
}

// the destination indices that can reach source index I on one axis: a superset, the taps themselves decide.  The float source
// coordinate is within 2^-7 of the exact one for sides up to 65536, which moves a border by less than one destination index.
__device__ __forceinline__ void reach(int I, float inv_scale, int out, int* lo, int* hi) {
    if (inv_scale == 0.f) { *lo = 0; *hi = out - 1; return; }       // one source or one destination index: every destination is a candidate
    *lo = max((int)floorf((float)(I - 1) * inv_scale) - 2, 0);
    *hi = min((int)floorf((float)(I + 1) * inv_scale) + 2, out - 1);
}

// the weight with which destination o takes source I (both taps may fall on I at the last index); false where neither does
__device__ __forceinline__ bool axis_weight(int o, int I, float scale, int in, float* wgt) {
    const Axis t = axis_taps(o, scale, in);
    const bool first = t.i0 == I, second = t.i0 + t.step == I;
    *wgt = (first ? t.l0 : 0.f) + (second ? t.l1 : 0.f);
    return first || second;
}

// dL/dup at (Y, X) of one image: the output pixels whose taps reach it, rows then columns, ascending
__device__ float gather_up_gradient(const UpsampleDepthArgs& a, const float* __restrict__ go, int Y, int X, int H, int W) {
    int ylo, yhi, xlo, xhi;
    reach(Y, a.inv_sy, a.Ho, &ylo, &yhi);
    reach(X, a.inv_sx, a.Wo, &xlo, &xhi);
    float wx;
    while (xlo <= xhi && !axis_weight(xlo, X, a.sx, W, &wx)) ++xlo;     // (the reaching indices are one run: the source index grows with o)
    while (xhi >= xlo && !axis_weight(xhi, X, a.sx, W, &wx)) --xhi;
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        float wy;
        if (!axis_weight(oy, Y, a.sy, H, &wy)) continue;
        const float* row = go + oy * a.Wo;
        for (int ox = xlo; ox <= xhi; ++ox) {
            axis_weight(ox, X, a.sx, W, &wx);
            acc += (wy * wx) * row[ox];
        }
    }
    return a.disp_on ? acc * a.disp_b : acc;
}

// ---- backward 1: dL/dup, dL/dmask and the tap sums ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void upsample_cells_bwd_kernel(const UpsampleDepthArgs a, const int tiles) {
    __shared__ float sG[MR * MR][STR];
    __shared__ float sS[G][9][TP];
    const int lane = threadIdx.x & (TP - 1), g = threadIdx.x / TP;
    const int n = blockIdx.x / tiles, q0 = (blockIdx.x - n * tiles) * TP;
    const int hw = a.h * a.w, r = a.r, r2 = r * r, q = q0 + lane;
    const int H = a.h * r, W = a.w * r, run = TP * r;
    const float* go = a.g_out + n * a.Ho * a.Wo;
    for (int idx = threadIdx.x; idx < TP * r2; idx += NT) {
        const int i = idx / run, rem = idx - i * run, l = rem / r, j = rem - l * r;
        const int qq = q0 + l;
        if (qq >= hw) continue;
        const int yy = qq / a.w, xx = qq - yy * a.w;
        sG[i * r + j][l] = gather_up_gradient(a, go, yy * r + i, xx * r + j, H, W);
    }
    __syncthreads();
    float s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.f;
    if (q < hw) {
        const int y = q / a.w, x = q - y * a.w;
        float d[9], p[9];
        depth_taps(a.depth + n * hw, y, x, a.h, a.w, d);
        for (int ij = g; ij < r2; ij += G) {
            const int c0 = (n * 9 * r2 + ij) * hw + q;
            tap_softmax(a.mask + c0, r2 * hw, p);
            const float gu = sG[ij][lane];
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) v += p[k] * d[k];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float pg = p[k] * gu;
                if (a.g_mask) a.g_mask[c0 + k * r2 * hw] = pg * (d[k] - v);     // the softmax Jacobian applied to dL/dp_k = g d_k
                s[k] += pg;
            }
        }
    }
    if (!a.g_depth) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) sS[g][k][lane] = s[k];
    __syncthreads();
    if (g == 0 && q < hw) {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.workspace[(n * 9 + k) * hw + q] = ((sS[0][k][lane] + sS[1][k][lane]) + sS[2][k][lane]) + sS[3][k][lane];
    }
}

// ---- backward 2: dL/ddepth from the tap sums ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void upsample_depth_bwd_kernel(const UpsampleDepthArgs a, const int total) {
    const int64_t t64 = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t64 >= total) return;
    const int t = (int)t64, hw = a.h * a.w;
    const int n = t / hw, q = t - n * hw, y = q / a.w, x = q - y * a.w;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {       // tap k of cell (y - ky + 1, x - kx + 1) reads this cell
        const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
        if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) acc += a.workspace[(n * 9 + k) * hw + yy * a.w + xx];
    }
    a.g_depth[t] = acc;
}

}  // namespace

void launch_upsample_depth_forward(const UpsampleDepthArgs& a, hipStream_t s) {
    const int tiles = (int)upsample_depth_tiles(a.h, a.w);
    const bool identity = a.Ho == a.h * a.r && a.Wo == a.w * a.r;
    hipLaunchKernelGGL(upsample_convex_kernel, dim3((unsigned)(tiles * a.N)), dim3(NT), 0, s, a, identity ? a.out : a.workspace,
                       identity ? a.disp_on : 0, tiles);
    if (identity) return;
    const int total = a.N * a.Ho * a.Wo;
    hipLaunchKernelGGL(upsample_resize_kernel, dim3((unsigned)(((int64_t)total + NT - 1) / NT)), dim3(NT), 0, s, a, total);
}

void launch_upsample_depth_backward(const UpsampleDepthArgs& a, hipStream_t s) {
    const int tiles = (int)upsample_depth_tiles(a.h, a.w);
    hipLaunchKernelGGL(upsample_cells_bwd_kernel, dim3((unsigned)(tiles * a.N)), dim3(NT), 0, s, a, tiles);
    if (!a.g_depth) return;
    const int total = a.N * a.h * a.w;
    hipLaunchKernelGGL(upsample_depth_bwd_kernel, dim3((unsigned)(((int64_t)total + NT - 1) / NT)), dim3(NT), 0, s, a, total);
}

}  // namespace ggr

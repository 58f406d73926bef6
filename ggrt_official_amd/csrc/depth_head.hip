// depth_head.hip — the depth-head pass: what GGRt does between depth_predictor.projection and GaussianAdapter.forward, in one
// forward and one backward launch.
//
// Per head (c, r, j) — camera, ray, surface — with s depth buckets and spp samples (the contract: include/ggr_raster.h,
// GgrDepthHeadPass):
//   pdf = softmax(pdf logits),  npdf = pdf / (FLT_EPSILON + Σ pdf)
//   index_k = sampled:        min(#{d : cdf_d <= u_k}, s − 1), cdf the running float32 sum of npdf
//             deterministic:  the bucket of k-th largest pdf, ties to the lower bucket
//   depth_k = 1 / ((1 − rel)·(1/(near+ε) − 1/(far+ε)) + 1/(far+ε) + ε),  rel = (index_k + σ(offset logit at index_k)) / s
//   q_k = transmittance ? pdf_i / (1 − Σ_{d<i} pdf_d + 1e-10) : npdf_i;   opacity_k = scale·½·(1 − max(1−q, 0)^e + q^(1/e))
//   coords_k = ray_xy[r] + (σ(xy_raw) − ½)·(1/w, 1/h)
//
// Layout.  A head's logits are 2·s floats (256 B at s = 32); with srf = 1 the heads of a camera are one contiguous array.  A lane
// that walked its own head in global memory would touch 64 cache lines per wave-instruction, so the heads go through LDS as in
// adapter.hip: a workgroup is ONE wave and owns tiles of 64 consecutive heads of one camera, which it copies into LDS one dword per
// lane (256 contiguous bytes per wave-instruction; only a float's alignment is asked of any buffer) at an odd row pitch, so that
// lane i then walks head i without bank conflicts.  The softmax is computed IN PLACE in LDS (the pdf replaces its logit), so no
// per-lane array is indexed at run time; the per-sample quantities live in registers (arrays of KMAX, the kernel's template
// parameter, fully unrolled).  The backward recomputes the softmax, forms dL/dpdf per bucket in the offset slot, then overwrites
// both slots with the gradients and streams the tile out the way it came in: dL/dlogits is written whole and coalesced, without
// atomics — one lane owns one head, repeated indices of a head are summed in registers.  With srf > 1 a head's floats interleave
// with its ray's other surfaces: the tile's rays are then walked whole and each float finds its head by a division.
// The small per-Gaussian arrays (depth, opacity, index, u: 4 B per lane at a 4·spp B stride) are accessed directly: a wave's
// accesses cover whole lines between them.  xy_raw is read in place at the caller's row stride (8 B per head).
// The grid is (chunks, C): a workgroup never sees two cameras and strides over its camera's tiles.
#include "depth_head.h"
#include <algorithm>
#include <cfloat>

namespace ggr {

namespace {

constexpr int TILE = kDepthHeadTile;

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// heads [h0, h0 + n) of camera c between global memory and the LDS tile (row = head − h0, column = 2·bucket + channel).
// STORE = false: logits → tile;  true: tile → dL/dlogits.
template <bool STORE>
__device__ __forceinline__ void stage(const DepthHeadArgs& a, float* tile, const float* __restrict__ src, float* __restrict__ dst,
                                      int c, int h0, int n, int lane, int pitch) {
    const int S2 = 2 * a.s;
    if (a.srf == 1) {
        const size_t base = ((size_t)c * a.R + h0) * S2;
        const float inv = 1.f / (float)S2;
        const int count = n * S2;                              // <= 64·128
        for (int i = lane; i < count; i += TILE) {
            const int row = (int)(((float)i + 0.5f) * inv);    // i / S2: exact for i < 2^13, S2 <= 128
            const int at = row * pitch + (i - row * S2);
            if (STORE) dst[base + i] = tile[at]; else tile[at] = src[base + i];
        }
    } else {
        const int srf = a.srf, W = S2 * srf;
        const int r_lo = h0 / srf, r_hi = (h0 + n - 1) / srf;
        for (int r = r_lo; r <= r_hi; ++r) {
            const size_t base = ((size_t)c * a.R + r) * W;
            const int hr = r * srf - h0;                       // the ray's surface 0 as a row of the tile
            for (int o = lane; o < W; o += TILE) {
                const int pair = o >> 1, d = pair / srf, row = hr + (pair - d * srf);
                if (row >= 0 && row < n) {
                    const int at = row * pitch + 2 * d + (o & 1);
                    if (STORE) dst[base + o] = tile[at]; else tile[at] = src[base + o];
                }
            }
        }
    }
}

// pdf logits of one head → pdf, in place; returns FLT_EPSILON + Σ pdf
__device__ __forceinline__ float softmax_in_place(float* row, int s) {
    float m = row[0];
    for (int d = 1; d < s; ++d) m = fmaxf(m, row[2 * d]);
    float z = 0.f;
    for (int d = 0; d < s; ++d) { const float e = expf(row[2 * d] - m); row[2 * d] = e; z += e; }
    float sum = 0.f;
    for (int d = 0; d < s; ++d) { const float p = row[2 * d] / z; row[2 * d] = p; sum += p; }
    return FLT_EPSILON + sum;
}

// pre[k] = Σ_{d<idx[k]} pdf_d, in bucket order.  The sum is compensated (Kahan): 1 − pre is what the transmittance form divides by,
// and at a late bucket it is small beside the rounding a plain running sum of up to 63 terms collects (measured: a 2e-5 relative
// error of an opacity, five times the float32 torch route's, whose cumsum is a scan).
template <int KMAX>
__device__ __forceinline__ void prefix_sums(const float* row, int s, const int (&idx)[KMAX], float (&pre)[KMAX]) {
    float run = 0.f, lost = 0.f;
    for (int d = 0; d < s; ++d) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) pre[k] = d == idx[k] ? run : pre[k];
        const float y = row[2 * d] - lost, next = run + y;
        lost = (next - run) - y;
        run = next;
    }
}

struct Disparity { float range, far; };   // 1/(near+ε) − 1/(far+ε), 1/(far+ε)

__device__ __forceinline__ Disparity load_disparity(const DepthHeadArgs& a, int c) {
    const float dn = 1.f / (a.near[c] + 1e-10f), df = 1.f / (a.far[c] + 1e-10f);
    return {dn - df, df};
}

template <int KMAX>
__global__ void __launch_bounds__(TILE)
depth_head_fwd_kernel(const DepthHeadArgs a, const int tiles_per_cam, const int pitch) {
    extern __shared__ float tile[];
    const int c = blockIdx.y, lane = threadIdx.x, s = a.s, spp = a.spp, H = a.R * a.srf;
    const Disparity disp = load_disparity(a, c);
    const float inv_e = 1.f / a.exponent;

    for (int t = blockIdx.x; t < tiles_per_cam; t += gridDim.x) {
        const int h0 = t * TILE, n = min(TILE, H - h0);
        __syncthreads();   // (the previous tile's rows are read)
        stage<false>(a, tile, a.logits, nullptr, c, h0, n, lane, pitch);
        __syncthreads();
        if (lane < n) {
            float* row = tile + lane * pitch;
            const int h = h0 + lane;
            const size_t p0 = ((size_t)c * H + h) * spp;
            const float denom = softmax_in_place(row, s);

            int idx[KMAX];
            if (a.deterministic) {
                unsigned long long taken = 0ull;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) {
                    idx[k] = -1;
                    if (k < spp) {
                        float best = -1.f;
                        int bi = 0;
                        for (int d = 0; d < s; ++d) {
                            const float p = row[2 * d];
                            if (!((taken >> d) & 1ull) && p > best) { best = p; bi = d; }   // (strict: ties stay with the lower bucket)
                        }
                        idx[k] = bi;
                        taken |= 1ull << bi;
                    }
                }
            } else {
                float u[KMAX];
#pragma unroll
                for (int k = 0; k < KMAX; ++k) { u[k] = k < spp ? a.u[p0 + k] : -1.f; idx[k] = 0; }
                float cdf = 0.f;
                for (int d = 0; d < s; ++d) {
                    cdf += row[2 * d] / denom;
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) idx[k] += cdf <= u[k] ? 1 : 0;
                }
#pragma unroll
                for (int k = 0; k < KMAX; ++k) idx[k] = k < spp ? min(idx[k], s - 1) : -1;
            }
            float pre[KMAX];   // Σ_{d<i} pdf_d at i = idx[k]
#pragma unroll
            for (int k = 0; k < KMAX; ++k) pre[k] = 0.f;
            if (a.transmittance) prefix_sums<KMAX>(row, s, idx, pre);
            const float x0 = a.xy_raw[((size_t)c * H + h) * a.xy_stride], x1 = a.xy_raw[((size_t)c * H + h) * a.xy_stride + 1];
            const int r = h / a.srf;
            const float cx = a.ray_xy[2 * r] + (sigmoidf(x0) - 0.5f) * a.inv_w, cy = a.ray_xy[2 * r + 1] + (sigmoidf(x1) - 0.5f) * a.inv_h;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < spp) {
                    const int i = idx[k];
                    const float pi = row[2 * i];
                    const float rel = ((float)i + sigmoidf(row[2 * i + 1])) / (float)s;
                    const float q = a.transmittance ? pi / (1.f - pre[k] + 1e-10f) : pi / denom;
                    float o = q;
                    if (a.exponent != 1.f) o = 0.5f * (1.f - powf(fmaxf(1.f - q, 0.f), a.exponent) + powf(q, inv_e));
                    a.depth[p0 + k] = 1.f / ((1.f - rel) * disp.range + disp.far + 1e-10f);
                    a.opacity[p0 + k] = a.opacity_scale * o;
                    a.index[p0 + k] = i;
                    a.coords[2 * (p0 + k)] = cx;
                    a.coords[2 * (p0 + k) + 1] = cy;
                }
            }
        }
    }
}

template <int KMAX>
__global__ void __launch_bounds__(TILE)
depth_head_bwd_kernel(const DepthHeadArgs a, const int tiles_per_cam, const int pitch) {
    extern __shared__ float tile[];
    const int c = blockIdx.y, lane = threadIdx.x, s = a.s, spp = a.spp, H = a.R * a.srf;
    const Disparity disp = load_disparity(a, c);
    const float e = a.exponent, inv_e = 1.f / a.exponent;

    for (int t = blockIdx.x; t < tiles_per_cam; t += gridDim.x) {
        const int h0 = t * TILE, n = min(TILE, H - h0);
        __syncthreads();   // (the previous tile has left)
        stage<false>(a, tile, a.logits, nullptr, c, h0, n, lane, pitch);
        __syncthreads();
        if (lane < n) {
            float* row = tile + lane * pitch;
            const int h = h0 + lane;
            const size_t p0 = ((size_t)c * H + h) * spp;
            const float denom = softmax_in_place(row, s);

            int idx[KMAX];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) idx[k] = k < spp ? min(max(a.index[p0 + k], 0), s - 1) : -1;
            float pre[KMAX];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) pre[k] = 0.f;
            if (a.transmittance) prefix_sums<KMAX>(row, s, idx, pre);
            // per sample: dL/d(offset logit at its bucket) `goff`, dL/dpdf at its bucket `at`, dL/dpdf below its bucket `below`
            // (the transmittance's prefix sum); `all`: dL/dpdf of every bucket (npdf's normalisation)
            float goff[KMAX], at[KMAX], below[KMAX], all = 0.f, gx = 0.f, gy = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                goff[k] = at[k] = below[k] = 0.f;
                if (k < spp) {
                    const int i = idx[k];
                    const float pi = row[2 * i], sg = sigmoidf(row[2 * i + 1]);
                    const float rel = ((float)i + sg) / (float)s;
                    const float depth = 1.f / ((1.f - rel) * disp.range + disp.far + 1e-10f);
                    const float gd = a.g_depth ? a.g_depth[p0 + k] : 0.f;
                    goff[k] = gd * disp.range * depth * depth * sg * (1.f - sg) / (float)s;
                    const float T = 1.f - pre[k] + 1e-10f;
                    const float q = a.transmittance ? pi / T : pi / denom;
                    float dodq = a.opacity_scale;
                    if (e != 1.f) {
                        const float base = 1.f - q;
                        const float first = base < 0.f ? 0.f : e * powf(base, e - 1.f);
                        dodq = a.opacity_scale * 0.5f * (first + inv_e * powf(q, inv_e - 1.f));
                    }
                    const float gq = a.g_opacity ? a.g_opacity[p0 + k] * dodq : 0.f;
                    if (a.transmittance) { at[k] = gq / T; below[k] = gq * pi / (T * T); }
                    else { at[k] = gq / denom; all -= gq * pi / (denom * denom); }
                    if (a.g_coords) { gx += a.g_coords[2 * (p0 + k)]; gy += a.g_coords[2 * (p0 + k) + 1]; }
                }
            }
            // dL/dpdf_d into the offset slot (its logits are consumed), and Σ pdf·dL/dpdf
            float dot = 0.f;
            for (int d = 0; d < s; ++d) {
                float g = all;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) g += (d == idx[k] ? at[k] : 0.f) + (d < idx[k] ? below[k] : 0.f);
                row[2 * d + 1] = g;
                dot += row[2 * d] * g;
            }
            // the softmax's backward into the pdf slot, the offsets' gradient into theirs
            for (int d = 0; d < s; ++d) {
                row[2 * d] = row[2 * d] * (row[2 * d + 1] - dot);
                float o = 0.f;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) o += d == idx[k] ? goff[k] : 0.f;
                row[2 * d + 1] = o;
            }
            if (a.g_xy) {
                const float sx = sigmoidf(a.xy_raw[((size_t)c * H + h) * a.xy_stride]);
                const float sy = sigmoidf(a.xy_raw[((size_t)c * H + h) * a.xy_stride + 1]);
                a.g_xy[2 * ((size_t)c * H + h)] = gx * sx * (1.f - sx) * a.inv_w;
                a.g_xy[2 * ((size_t)c * H + h) + 1] = gy * sy * (1.f - sy) * a.inv_h;
            }
        }
        __syncthreads();
        stage<true>(a, tile, nullptr, a.g_logits, c, h0, n, lane, pitch);
    }
}

struct Launch { dim3 grid; int tiles, pitch; size_t lds; };

Launch depth_head_launch(const DepthHeadArgs& a) {
    Launch l;
    const int H = a.R * a.srf;
    l.tiles = (H + TILE - 1) / TILE;
    l.pitch = (2 * a.s) | 1;
    l.lds = (size_t)TILE * l.pitch * sizeof(float);   // <= 64·129·4 = 33 KiB
    const int chunks = std::max(1, std::min(l.tiles, kDepthHeadMaxChunks / a.C));
    l.grid = dim3((unsigned)chunks, (unsigned)a.C);
    return l;
}

}  // namespace

#define GGR_DEPTH_HEAD_DISPATCH(kernel)                                                                               \
    do {                                                                                                              \
        const Launch l = depth_head_launch(a);                                                                        \
        if (a.spp <= 1) hipLaunchKernelGGL(kernel<1>, l.grid, dim3(TILE), l.lds, s, a, l.tiles, l.pitch);             \
        else if (a.spp <= 2) hipLaunchKernelGGL(kernel<2>, l.grid, dim3(TILE), l.lds, s, a, l.tiles, l.pitch);        \
        else if (a.spp <= 4) hipLaunchKernelGGL(kernel<4>, l.grid, dim3(TILE), l.lds, s, a, l.tiles, l.pitch);        \
        else if (a.spp <= 8) hipLaunchKernelGGL(kernel<8>, l.grid, dim3(TILE), l.lds, s, a, l.tiles, l.pitch);        \
        else hipLaunchKernelGGL(kernel<16>, l.grid, dim3(TILE), l.lds, s, a, l.tiles, l.pitch);                       \
    } while (0)

void launch_depth_head_forward(const DepthHeadArgs& a, hipStream_t s) {
    if (a.C <= 0 || a.R <= 0) return;
    GGR_DEPTH_HEAD_DISPATCH(depth_head_fwd_kernel);
}

void launch_depth_head_backward(const DepthHeadArgs& a, hipStream_t s) {
    if (a.C <= 0 || a.R <= 0) return;
    GGR_DEPTH_HEAD_DISPATCH(depth_head_bwd_kernel);
}

}  // namespace ggr

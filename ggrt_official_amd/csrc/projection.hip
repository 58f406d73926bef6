// projection.hip — the projection pass: where every Gaussian lands on the screen, as plain arrays, and the way back.
//
// preprocess_fwd leaves, per (view, Gaussian) pair, the 2D mean, the conic, the opacity the pixels see, the depth value and the
// colour in the geometry buffer (ggr_common.h: splat[pair][2] and colour[pair]); preprocess_bwd turns a gradient w.r.t. exactly
// those quantities — floats 0..9 of the pair's 64-byte record of the backward scratch (GGR_G2D_*) — into the gradients of the
// caller's inputs.  The two kernels here are the missing ends: projection_unpack copies the quantities out (the same bits, zero
// where the Gaussian is culled), projection_seed puts a caller's gradient w.r.t. them into the records, ahead of ggr_backward*.
//
// Both are streaming kernels over the pairs: one thread per pair, 256-thread blocks, no LDS, no atomics, a handful of registers
// (occupancy is whatever the memory pipe wants).  Loads of the records are 16 B per lane; the outputs are arrays of 1, 2 and 3
// floats per pair in the layouts torch hands on, so their accesses are 4 B per lane at a stride of 4, 8 or 12 B: the caller's
// arrays need no more than a float's alignment (a view at an odd element offset is a valid [P,2] array), and a wave's accesses
// still cover whole cache lines between them.
//
// Units of the records (as blend_bwd.hip writes them and preprocess_bwd.hip reads them):
//   GGR_G2D_MEAN   dL/d(NDC x, y): the blend scales its pixel-space sums by W/2, H/2 — pixel = ((ndc + 1)·W − 1)/2;
//   GGR_G2D_CONIC  (xx, xy, yy) with xy in the HALF convention: the blend stores ½·dL/dconic.xy and preprocess_bwd's dL_db
//                  carries the factor 2 (upstream's convention);
//   GGR_G2D_RGB, GGR_G2D_OPACITY, GGR_G2D_Z  as they are (the opacity is the record's: compensated under anti-aliasing).
#include "projection.h"

namespace ggr {

namespace {

__global__ void __launch_bounds__(256)
projection_unpack_kernel(size_t pairs, const float4* __restrict__ splat, const float4* __restrict__ colour,
                         const int32_t* __restrict__ radii, float* __restrict__ means2d, float* __restrict__ depth,
                         float* __restrict__ conic, float* __restrict__ opacity, float* __restrict__ color,
                         uint8_t* __restrict__ valid) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    const bool ok = radii[i] > 0;
    // (a culled pair's record holds whatever preprocess_fwd left there: it is read — the loads stay unconditional and in
    //  flight together — and then replaced, never multiplied)
    const float4 s0 = splat[2 * i], s1 = splat[2 * i + 1], c = colour[i];
    if (means2d) { means2d[2 * i] = ok ? s0.x : 0.f; means2d[2 * i + 1] = ok ? s0.y : 0.f; }
    if (depth) depth[i] = ok ? s1.z : 0.f;
    if (conic) { conic[3 * i] = ok ? s0.z : 0.f; conic[3 * i + 1] = ok ? s0.w : 0.f; conic[3 * i + 2] = ok ? s1.x : 0.f; }
    if (opacity) opacity[i] = ok ? s1.y : 0.f;
    if (color) { color[3 * i] = ok ? c.x : 0.f; color[3 * i + 1] = ok ? c.y : 0.f; color[3 * i + 2] = ok ? c.z : 0.f; }
    if (valid) valid[i] = ok ? 1 : 0;
}

template <bool ADD>
__global__ void __launch_bounds__(256)
projection_seed_kernel(size_t pairs, float half_w, float half_h, const int32_t* __restrict__ radii,
                       const float* __restrict__ g_means2d, const float* __restrict__ g_depth, const float* __restrict__ g_conic,
                       const float* __restrict__ g_opacity, const float* __restrict__ g_color, float* __restrict__ grad2d) {
    static_assert(GGR_G2D_RGB == 0 && GGR_G2D_MEAN == 3 && GGR_G2D_CONIC == 5 && GGR_G2D_OPACITY == 8 && GGR_G2D_Z == 9 &&
                  GGR_G2D_STRIDE == 16, "the record is written as {rgb, mean.x | mean.y, conic | opacity, z}");
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    const bool ok = radii[i] > 0;
    float4* const rec = reinterpret_cast<float4*>(grad2d + GGR_G2D_STRIDE * i);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok) {   // a culled pair: its gradients are not read at all (a NaN there reaches nothing)
        if (!ADD) { rec[0] = zero; rec[1] = zero; rec[2] = zero; rec[3] = zero; }
        return;
    }
    float4 r0 = zero, r1 = zero;
    float2 r2 = make_float2(0.f, 0.f);
    if (g_color) { r0.x = g_color[3 * i]; r0.y = g_color[3 * i + 1]; r0.z = g_color[3 * i + 2]; }
    if (g_means2d) { r0.w = half_w * g_means2d[2 * i]; r1.x = half_h * g_means2d[2 * i + 1]; }
    if (g_conic) { r1.y = g_conic[3 * i]; r1.z = 0.5f * g_conic[3 * i + 1]; r1.w = g_conic[3 * i + 2]; }
    if (g_opacity) r2.x = g_opacity[i];
    if (g_depth) r2.y = g_depth[i];
    if (ADD) {   // floats 0..9 only: 10..15 are not this pass's
        const float4 o0 = rec[0], o1 = rec[1];
        const float2 o2 = *reinterpret_cast<const float2*>(rec + 2);
        rec[0] = make_float4(o0.x + r0.x, o0.y + r0.y, o0.z + r0.z, o0.w + r0.w);
        rec[1] = make_float4(o1.x + r1.x, o1.y + r1.y, o1.z + r1.z, o1.w + r1.w);
        *reinterpret_cast<float2*>(rec + 2) = make_float2(o2.x + r2.x, o2.y + r2.y);
    } else {
        rec[0] = r0; rec[1] = r1; rec[2] = make_float4(r2.x, r2.y, 0.f, 0.f); rec[3] = zero;
    }
}

}  // namespace

void launch_projection_unpack(size_t pairs, const float4* splat, const float4* colour, const int32_t* radii, float* means2d,
                              float* depth, float* conic, float* opacity, float* color, uint8_t* valid, hipStream_t s) {
    if (pairs == 0) return;
    hipLaunchKernelGGL(projection_unpack_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, pairs, splat, colour, radii,
                       means2d, depth, conic, opacity, color, valid);
}

void launch_projection_seed(size_t pairs, int W, int H, const int32_t* radii, const float* dL_dmeans2d, const float* dL_ddepth,
                            const float* dL_dconic, const float* dL_dopacity, const float* dL_dcolor, float* grad2d, int add,
                            hipStream_t s) {
    if (pairs == 0) return;
    const dim3 grid((unsigned)((pairs + 255) / 256)), block(256);
    const float half_w = 0.5f * (float)W, half_h = 0.5f * (float)H;
    if (add)
        hipLaunchKernelGGL(projection_seed_kernel<true>, grid, block, 0, s, pairs, half_w, half_h, radii, dL_dmeans2d, dL_ddepth,
                           dL_dconic, dL_dopacity, dL_dcolor, grad2d);
    else
        hipLaunchKernelGGL(projection_seed_kernel<false>, grid, block, 0, s, pairs, half_w, half_h, radii, dL_dmeans2d, dL_ddepth,
                           dL_dconic, dL_dopacity, dL_dcolor, grad2d);
}

}  // namespace ggr

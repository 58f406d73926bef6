// blend_absgrad.hip — the absgrad pass: per-Gaussian ABSOLUTE screen-space positional gradients over the tile lists of a forward,
// for gfx950.
//
// No counterpart in the reference.  A training loop densifies where a Gaussian's screen-space positional gradient is large.  The
// signed dL/dmean2D the backward returns under-reports it: the per-pixel terms ∂L_p/∂mean2D_i change sign across the footprint
// and cancel in the sum over pixels (AbsGS, GOF; gsplat's `absgrad`).  This pass accumulates their ABSOLUTE values:
//     absgrad[i] = ( Σ_p |gx_{i,p}| , Σ_p |gy_{i,p}| )          grad[i] = ( Σ_p gx_{i,p} , Σ_p gy_{i,p} )   (the signed cross-check)
// It is no function of any tensor a backward returns — the |·| stands in front of the sum over pixels — so it walks the lists.
//
// Per pixel p, over the entries i the colour blend composited there, in list order, w_i = α_i·T_i, with the loss reaching the
// pixel through C = Σ w_i c_i + T_f·bg, D = Σ w_i d_i (d the DEPTH VALUE the depth plane blends) and A = 1 − T_f = Σ w_i, whose
// upstream gradients are g_C, g_D, g_A (the last two zero when absent):
//     u_i = g_C·c_i + g_D·d_i + g_A         u_bg = g_C·bg
//     ∂L_p/∂α_i = T_i·u_i − R_i/(1 − α_i),  R_i = Σ_{j behind i} w_j·u_j + T_f·u_bg
//     gx = ½W·∂L_p/∂α_i·o_i·G_i·(−(cxx·dx + cxy·dy))     gy = ½H·∂L_p/∂α_i·o_i·G_i·(−(cyy·dy + cxy·dx))     (dx, dy) = mean2D_i − p
// — exactly what blend_bwd.hip sums into dL_dmeans2D (straight-through 0.99 clamp, the same NDC scaling, o the record's opacity:
// compensated under antialiasing).  The terms a FEATURE loss and a DISTORTION loss add to dL_dmeans2D (blend_feat.hip,
// blend_dist.hip) are NOT part of absgrad: it covers what ggr_backward*'s own blend differentiates.
//
// A FRONT-TO-BACK replay, as blend_dist_bwd_kernel (same mapping: one 256-thread workgroup per 16×16 tile, wave w owns the 8×8
// quadrant (w&1, w>>1), batches of 256 entries staged through LDS, every wave culls the batch against the box of its live pixels
// and walks the survivors with the colour blend's own rules and arithmetic, so the weights are the colour blend's bit for bit).
// Beside the record an entry's colour and depth value are staged as ONE float4 (r, g, b, d); u_i is formed per lane from the
// pixel's five upstream gradients, held in registers.  The running "everything behind" starts from the forward's own planes,
//     R_0 + T_f·u_bg = g_C·C + g_D·D + g_A·(1 − T_f)          (T_f: the final T the image buffer holds; bg is inside C already)
// as blend_feat_bwd takes its total from out_features: one sweep, no checkpoints, no n_contrib.  A pixel whose five gradients are
// all exactly zero adds exactly nothing: it takes no entry (blend_bwd.hip's zero-gradient skip).
//
// Per entry a lane has |gx|, |gy|, gx, gy (+ four zeros: the butterfly of blend_butterfly.h as blend_dist_bwd_kernel runs it, 8
// entries × 8 values); afterwards lane 8·entry + c owns sum c over the wave's 64 pixels and commits it, if non-zero, with one
// float atomic: c = 0, 1 into out_absgrad, c = 2, 3 into out_grad (if given).  The backward's scratch records are not touched.
#include "blend_butterfly.h"
#include "blend_common.h"
#include "blend_absgrad.h"

namespace ggr {

#define BATCH GGR_BATCH
#define ABSGRAD_GROUP 8   // entries per butterfly

// stage_feat_splat plus the entry's colour and depth value as one float4, the depth value from the one load of the record's
// second float4 (the same products as stage_feat_splat, so the weights stay the colour blend's)
__device__ __forceinline__ FeatSplat stage_absgrad_splat(const float4* __restrict__ splat, const float4* __restrict__ colour,
                                                         uint32_t g, float4& colour_depth) {
    float4 a = splat[2 * (size_t)g];
    const float4 ge = splat[2 * (size_t)g + 1];
    const float4 col = colour[g];
    float4 b = make_float4(ge.x, ge.y, 0.f, 0.f), c = make_float4(0.f, ge.z, ge.w, 0.f);
    stage_scale_conic(a, b, c);
    colour_depth = make_float4(col.x, col.y, col.z, ge.z);
    FeatSplat r;
    r.a = a;
    r.b = make_float4(b.x, b.y, c.z, __uint_as_float(g));
    return r;
}

// A lane's values of one entry: |gx|, |gy|, gx, gy and four zeros: VC = 8 values, RB = 8 entries per butterfly, after which lane
// 8·entry + c owns sum c of its entry.
__global__ void __launch_bounds__(256)
blend_absgrad_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                     const float4* __restrict__ splat, const float4* __restrict__ colour,
                     const float* __restrict__ final_T, const float* __restrict__ out_color, const float* __restrict__ out_depth,
                     const float* __restrict__ dL_dcolor, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha,
                     float* __restrict__ out_absgrad, float* __restrict__ out_grad, int views) {
    constexpr int RB = ABSGRAD_GROUP, VC = 8, N = RB * VC, LPE = 64 / RB /*lanes per entry*/;
    static_assert(RB == 8 && VC == LPE && N == 64, "one finished sum per lane");
    __shared__ FeatSplat stage[BATCH + 1];                               // + the null record that pads a survivor list
    __shared__ float4 cdval[BATCH + 1];                                  // the entries' (r, g, b, depth value)
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + RB];
    __shared__ int wave_done[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles1 = grid_x * ((H + GGR_TILE - 1) / GGR_TILE), ntiles = tiles1 * views;
    const int vtile = xcd_tile((int)blockIdx.x, ntiles, true);
    if (vtile < 0) return;  // padding workgroup (before any barrier)
    const int view = vtile / tiles1, tile = vtile - view * tiles1;
    const int tile_x = tile % grid_x, tile_y = tile / grid_x;
    const int qx0 = tile_x * GGR_TILE + (wave & 1) * 8, qy0 = tile_y * GGR_TILE + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pixx = (float)px, pixy = (float)py;
    const float rx0 = (float)qx0, ry0 = (float)qy0;
    const float rx1 = (float)min(qx0 + 7, W - 1), ry1 = (float)min(qy0 + 7, H - 1);

    const uint2 range = ranges[vtile];
    const int total = (int)(range.y - range.x);
    const size_t hw = (size_t)H * W;
    const size_t pid = inside ? (size_t)py * W + px : 0;

    // the pixel's upstream gradients and R = everything behind the current entry, the background included.  A pixel whose
    // gradients are all exactly zero adds exactly zero to every sum: it takes no entry (blend_bwd.hip's zero-gradient skip)
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, gD = 0.f, gA = 0.f, R = 0.f;
    if (inside) {
        const size_t vo = (size_t)view * hw;
        const float* dc = dL_dcolor + 3 * vo;
        const float* oc = out_color + 3 * vo;
        g0 = dc[pid]; g1 = dc[hw + pid]; g2 = dc[2 * hw + pid];
        R = g0 * oc[pid] + g1 * oc[hw + pid] + g2 * oc[2 * hw + pid];
        if (dL_ddepth) {
            gD = dL_ddepth[vo + pid];
            R = fmaf(gD, out_depth[vo + pid], R);
        }
        if (dL_dalpha) {
            gA = dL_dalpha[vo + pid];
            R = fmaf(gA, 1.f - final_T[vo + pid], R);
        }
    }
    bool live = inside && (g0 != 0.f || g1 != 0.f || g2 != 0.f || gD != 0.f || gA != 0.f);
    float T = 1.0f;
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    const float cX = 2.f * GGR_INV_KQ * 0.5f * (float)W, cY = 2.f * GGR_INV_KQ * 0.5f * (float)H;   // 1/k and the NDC scaling of the mean

    if (tid == 0) {   // the null record: opacity 0 → α = 0 → never contributes
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
        cdval[BATCH] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    bool wdone = !__any(live);
    if (lane == 0) wave_done[wave] = wdone ? 1 : 0;

    const int my_slot = lane / LPE, my_c = lane % LPE;
    // which array this lane's sum goes to: c = 0, 1 → out_absgrad, c = 2, 3 → out_grad (or nowhere), c ≥ 4: the zeros
    float* const my_out = my_c < 2 ? out_absgrad : (my_c < 4 ? out_grad : nullptr);
    uint32_t g_next = tid < total ? point_list[range.x + tid] : 0u;
    for (int b0 = 0; b0 < total; b0 += BATCH) {
        __syncthreads();  // previous batch fully consumed; wave_done visible
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;
        const int nb = min(BATCH, total - b0);
        const uint32_t g = g_next;
        if (b0 + BATCH + tid < total) g_next = point_list[range.x + b0 + BATCH + tid];
        if (tid < nb) {
            float4 cd;
            stage[tid] = stage_absgrad_splat(splat, colour, g, cd);
            cdval[tid] = cd;
        }
        __syncthreads();
        if (!wdone) {
            uint32_t* my_surv = surv[wave];
            float bx0 = rx0, by0 = ry0, bx1 = rx1, by1 = ry1;   // the pixels that can still take an entry
            {
                const uint64_t act = __ballot(live);
                if (act) active_box(act, rx0, ry0, bx0, by0, bx1, by1);
            }
            const int ns = cull_batch(stage, nb, my_surv, lane, bx0, by0, bx1, by1);
            if (lane < RB) my_surv[ns + lane] = (uint32_t)BATCH;   // pad the last butterfly with the null record
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k0 = 0; k0 < ns; k0 += RB) {
                uint32_t pkw[RB];
                __builtin_memcpy(pkw, my_surv + k0, sizeof pkw);
                const uint32_t my_e = my_surv[k0 + my_slot];   // the entry whose sum this lane commits
                float v[N];
#pragma unroll
                for (int sl = 0; sl < RB; sl++) {
                    const uint32_t e = pkw[sl];   // (VGPR, uniform)
                    const float4 a = stage[e].a;
                    const float2 rbx = *reinterpret_cast<const float2*>(&stage[e].b);   // (k·cyy, opacity)
                    const float4 rb = make_float4(rbx.x, rbx.y, 0.f, 0.f);
                    const float dx = a.x - pixx, dy = a.y - pixy;
                    const float q2 = staged_q2(a, rb, dx, dy);
                    const float G = __builtin_amdgcn_exp2f(-q2);
                    const float alpha = fminf(amax, rb.y * G);
                    // skip: power > 0, α < 1/255, or the pixel is saturated / carries no gradient
                    const bool cand = live & (q2 >= 0.0f) & (alpha >= GGR_ALPHA_MIN);
                    const float wr = alpha * T;
                    const float test_T = T - wr;               // T·(1−α)
                    const bool stop = cand & (test_T < GGR_T_MIN);
                    const bool take = cand & !stop;
                    live = live & !stop;
                    const float w = take ? wr : 0.f;
                    const float4 cd = cdval[e];
                    const float u = fmaf(g0, cd.x, fmaf(g1, cd.y, fmaf(g2, cd.z, fmaf(gD, cd.w, gA))));
                    R = fmaf(-w, u, R);   // now: everything BEHIND this entry (+ the background)
                    const float inv = __builtin_amdgcn_rcpf(1.f - (take ? alpha : 0.f));
                    const float dL_dalpha_e = T * u - R * inv;
                    const float mm = take ? G * dL_dalpha_e : 0.f;
                    // with h = −½·opacity·m:  dL/dmean = 2·conic·h·d (blend_dist_bwd_kernel's chain, the same operations)
                    const float h = -0.5f * rb.y * mm, u2 = h * dx, v2 = h * dy, hw2 = 0.5f * a.w;
                    const float gx = cX * fmaf(a.z, u2, hw2 * v2);
                    const float gy = cY * fmaf(rb.x, v2, hw2 * u2);
                    v[sl * VC + 0] = fabsf(gx);
                    v[sl * VC + 1] = fabsf(gy);
                    v[sl * VC + 2] = gx;
                    v[sl * VC + 3] = gy;
                    v[sl * VC + 4] = 0.f;
                    v[sl * VC + 5] = 0.f;
                    v[sl * VC + 6] = 0.f;
                    v[sl * VC + 7] = 0.f;
                    T -= w;
                }
                // ---- the butterfly: 64 lanes × 64 values → every lane ONE finished sum of entry `my_slot`
                fold_swap32<N / 2>(v);
                fold_swap16<N / 4>(v);
                fold_dpp<N / 8, 0x128>(v, (lane & 8) != 0);     // row_ror:8
                fold_dpp<N / 16, 0x141>(v, (lane & 4) != 0);    // row_half_mirror (pairs c with 7 − c: bit 2 differs)
                fold_dpp<N / 32, 0x4E>(v, (lane & 2) != 0);     // quad_perm [2,3,0,1]
                fold_dpp<N / 64, 0xB1>(v, (lane & 1) != 0);     // quad_perm [1,0,3,2]
                // ---- commit: one atomic per finished sum (zero sums — the null record's, the padding values — are not sent)
                const float val = v[0];
                if (my_e != (uint32_t)BATCH && val != 0.f && my_out != nullptr) {
                    const uint32_t gid = __float_as_uint(stage[my_e].b.w);
                    atomicAdd(my_out + 2 * (size_t)gid + (my_c & 1), val);
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
    }
}

void launch_blend_absgrad(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat, const float4* colour,
                          const float* final_T, const float* out_color, const float* out_depth,
                          const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, float* out_absgrad,
                          float* out_grad, int views, hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    hipLaunchKernelGGL(blend_absgrad_kernel, dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges, point_list, splat, colour,
                       final_T, out_color, out_depth, dL_dcolor, dL_ddepth, dL_dalpha, out_absgrad, out_grad, views);
}

}  // namespace ggr

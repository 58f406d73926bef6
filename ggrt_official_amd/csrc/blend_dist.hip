// blend_dist.hip — the distortion pass: the depth-distortion regulariser of Mip-NeRF 360 / 2DGS over the tile lists of a forward,
// for gfx950.
//
// No counterpart in the reference.  Per pixel, over the entries the colour blend composited there, in list order i = 1..n, with
// w_i = α_i·T_i and d_i the Gaussian's DEPTH VALUE (the .z of its record's second float4: what the depth plane blends):
//     A_i = Σ_{j<i} w_j      B_i = Σ_{j<i} w_j·d_j      distortion = 2·Σ_i w_i·(d_i·A_i − B_i)   ( = 2·Σ_{j<i} w_i·w_j·(d_i − d_j) )
// — Σ_{i,j} w_i·w_j·|d_i − d_j| whenever d does not decrease along the list (view z, the sort key; aux_affine with b ≥ 0), the
// signed list-ordered form for an arbitrary aux_precomp.  It needs the prefix sums along the list, so it is no function of any
// set of composited planes: it has its own forward and backward over the lists.
//
// Both kernels REPLAY the sorted tile lists and the 32-B splat records a forward left in the caller's buffers, as the feature
// pass does (blend_feat.hip: same mapping — one 256-thread workgroup per 16×16 tile, wave w owns the 8×8 quadrant (w&1, w>>1),
// batches of 256 entries staged through LDS, every wave culls the batch against the box of its live pixels and walks the
// survivors — and the colour blend's own rules and arithmetic, so the weights are the colour blend's bit for bit).  An entry's
// depth value is staged beside its record.
//
// Origin.  The sum is invariant under d → d + const, and d_i·A_i − B_i cancels catastrophically for distant, tightly spaced
// surfaces.  Every d therefore enters B and the products less d0, the depth value of the pixel's FIRST composited entry.
//
// Forward: A, B and the sum in registers, one pixel per lane, in list order — no cross-lane sum, no atomic: the plane is
// bit-identical from run to run and across the forms of the depth sort.  Beside the plane the pixel's totals A_tot and (origin-
// relative) B_tot are stored for the backward, where asked for.
//
// Backward: a FRONT-TO-BACK replay.  With g = dL/d(distortion) of the pixel and Q its distortion,
//     c_i     = ∂Q/∂w_i (the other weights fixed) = 2·[ d_i·(2A_i − A_tot) + B_tot − 2B_i ]           (Σ_i w_i·c_i = 2Q)
//     dL/dd_i = g·2·w_i·(2A_i + w_i − A_tot)
//     dL/dα_s = g·( T_s·c_s − R_s/(1−α_s) ),   R_s = Σ_{s' behind s} w_s'·c_s' = 2Q − Σ_{s' up to s} w_s'·c_s'
// — the feature backward's recurrence with the per-pixel "feature" c_s; no checkpoints, no n_contrib, no final T; d0 is met
// again as the first composited entry.  dL/dα is chained to the 2D mean, conic and opacity as blend_feat_bwd_kernel does it; per
// entry a wave has 6 geometric sums + dL/dd (+ one zero) over its 64 pixels, 8 entries at a time go through the transposing
// butterfly (blend_butterfly.h) and lane 8·entry + c commits sum c with one atomic into slot GGR_G2D_MEAN + c of the entry's
// per-(view, Gaussian) record: 3..8 are the geometric slots, 9 is GGR_G2D_Z, which preprocess_bwd chains to means3D, the camera
// and dL_daux.
#include "blend_butterfly.h"
#include "blend_common.h"
#include "blend_dist.h"

namespace ggr {

#define BATCH GGR_BATCH
#define DIST_GROUP 8   // survivors per unrolled trip of the forward; entries per butterfly of the backward

// stage_feat_splat plus the entry's depth value, from the one load of the record's second float4 (the same products as
// stage_feat_splat, so the weights stay the colour blend's)
__device__ __forceinline__ FeatSplat stage_dist_splat(const float4* __restrict__ splat, uint32_t g, float& depth_value) {
    float4 a = splat[2 * (size_t)g];
    const float4 ge = splat[2 * (size_t)g + 1];
    float4 b = make_float4(ge.x, ge.y, 0.f, 0.f), c = make_float4(0.f, ge.z, ge.w, 0.f);
    stage_scale_conic(a, b, c);
    depth_value = ge.z;
    FeatSplat r;
    r.a = a;
    r.b = make_float4(b.x, b.y, c.z, __uint_as_float(g));
    return r;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
blend_dist_fwd_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                      const float4* __restrict__ splat, float* __restrict__ out_distortion, float* __restrict__ totals, int views,
                      int interleaved) {
    __shared__ FeatSplat stage[BATCH + 1];                               // + the null record that pads a survivor list
    __shared__ float dval[BATCH + 1];                                    // the entries' depth values
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + DIST_GROUP];
    __shared__ int wave_done[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles1 = grid_x * ((H + GGR_TILE - 1) / GGR_TILE), ntiles = tiles1 * views;
    const int vtile = xcd_tile((int)blockIdx.x, ntiles, interleaved != 0);
    if (vtile < 0) return;  // padding workgroup (before any barrier)
    const int view = vtile / tiles1, tile = vtile - view * tiles1;
    const int tile_x = tile % grid_x, tile_y = tile / grid_x;
    const int qx0 = tile_x * GGR_TILE + (wave & 1) * 8, qy0 = tile_y * GGR_TILE + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pixx = (float)px, pixy = (float)py;
    const float rx0 = (float)qx0, ry0 = (float)qy0;
    const float rx1 = (float)min(qx0 + 7, W - 1), ry1 = (float)min(qy0 + 7, H - 1);
    const bool quad_live = qx0 < W && qy0 < H;

    const uint2 range = ranges[vtile];
    const int total = (int)(range.y - range.x);

    float T = 1.0f, A = 0.f, B = 0.f, D = 0.f, d0 = 0.f;
    bool live = inside, first = true;   // first: no entry composited yet (d0 open)
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    if (tid == 0) {   // the null record: opacity 0 → α = 0 → never contributes
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
        dval[BATCH] = 0.f;
    }
    if (lane == 0) wave_done[wave] = quad_live ? 0 : 1;
    bool wdone = !quad_live;

    uint32_t g_next = tid < total ? point_list[range.x + tid] : 0u;
    for (int b0 = 0; b0 < total; b0 += BATCH) {
        __syncthreads();  // previous batch fully consumed; wave_done visible
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;
        const int nb = min(BATCH, total - b0);
        const uint32_t g = g_next;
        if (b0 + BATCH + tid < total) g_next = point_list[range.x + b0 + BATCH + tid];
        if (tid < nb) {
            float dv;
            stage[tid] = stage_dist_splat(splat, g, dv);
            dval[tid] = dv;
        }
        __syncthreads();
        if (!wdone) {
            uint32_t* my_surv = surv[wave];
            float bx0 = rx0, by0 = ry0, bx1 = rx1, by1 = ry1;   // the pixels that are not saturated yet
            {
                const uint64_t act = __ballot(live);
                if (act) active_box(act, rx0, ry0, bx0, by0, bx1, by1);
            }
            const int ns = cull_batch(stage, nb, my_surv, lane, bx0, by0, bx1, by1);
            if (lane < DIST_GROUP) my_surv[ns + lane] = (uint32_t)BATCH;   // pad the last group with the null record
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k0 = 0; k0 < ns; k0 += DIST_GROUP) {
                uint32_t pkw[DIST_GROUP];
                __builtin_memcpy(pkw, my_surv + k0, sizeof pkw);
#pragma unroll
                for (int u = 0; u < DIST_GROUP; u++) {
                    const uint32_t e = pkw[u];   // (VGPR, uniform)
                    const float4 a = stage[e].a;
                    const float2 rbx = *reinterpret_cast<const float2*>(&stage[e].b);   // (k·cyy, opacity)
                    const float4 rb = make_float4(rbx.x, rbx.y, 0.f, 0.f);
                    const float q2 = staged_q2(a, rb, a.x - pixx, a.y - pixy);  // = −power·log2(e)
                    const float alpha = fminf(amax, rb.y * __builtin_amdgcn_exp2f(-q2));
                    // skip: power > 0, α < 1/255, or the pixel is saturated
                    const bool cand = live & (q2 >= 0.0f) & (alpha >= GGR_ALPHA_MIN);
                    const float wr = alpha * T;
                    const float test_T = T - wr;               // T·(1−α)
                    const bool stop = cand & (test_T < GGR_T_MIN);
                    const bool take = cand & !stop;
                    live = live & !stop;
                    const float w = take ? wr : 0.f;
                    const float d = dval[e];
                    d0 = (take & first) ? d : d0;
                    first = first & !take;
                    const float dr = take ? d - d0 : 0.f;      // (an entry that is not taken adds exactly nothing)
                    D = fmaf(w, fmaf(dr, A, -B), D);
                    A += w;
                    B = fmaf(w, dr, B);
                    T -= w;
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
    }
    if (inside) {
        const size_t hw = (size_t)H * W, pid = (size_t)py * W + px;
        out_distortion[(size_t)view * hw + pid] = 2.f * D;
        if (totals) {
            totals[((size_t)view * 2) * hw + pid] = A;
            totals[((size_t)view * 2 + 1) * hw + pid] = B;
        }
    }
}

void launch_blend_dist_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           float* out_distortion, float* totals, int views, int scissored, hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    hipLaunchKernelGGL(blend_dist_fwd_kernel, dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges, point_list, splat,
                       out_distortion, totals, views, xcd_forward_interleaved(nt, scissored != 0) ? 1 : 0);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// A lane's values of one entry: the six geometric terms in record order (mean x, y; conic xx, xy, yy; opacity), dL/dd and one
// zero: VC = 8 values, RB = 8 entries per butterfly, after which lane 8·entry + c owns sum c of its entry.
__global__ void __launch_bounds__(256)
blend_dist_bwd_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                      const float4* __restrict__ splat, const float* __restrict__ out_distortion,
                      const float* __restrict__ totals, const float* __restrict__ dL_dout, float* __restrict__ grad2d, int views) {
    constexpr int RB = DIST_GROUP, VC = 8, N = RB * VC, LPE = 64 / RB /*lanes per entry*/;
    static_assert(RB == 8 && VC == LPE && N == 64, "one finished sum per lane");
    static_assert(GGR_G2D_MEAN == 3 && GGR_G2D_CONIC == 5 && GGR_G2D_OPACITY == 8 && GGR_G2D_Z == 9,
                  "the six geometric sums and dL/dd are committed in record order");
    __shared__ FeatSplat stage[BATCH + 1];
    __shared__ float dval[BATCH + 1];
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

    // the pixel's upstream gradient, its totals and R = Σ_i w_i·c_i = 2Q.  A pixel whose gradient is exactly zero adds exactly
    // zero to every sum: it takes no entry (blend_bwd.hip's zero-gradient skip)
    float gq = 0.f, R = 0.f, Atot = 0.f, Btot = 0.f;
    if (inside) {
        gq = dL_dout[(size_t)view * hw + pid];
        R = 2.f * out_distortion[(size_t)view * hw + pid];
        Atot = totals[((size_t)view * 2) * hw + pid];
        Btot = totals[((size_t)view * 2 + 1) * hw + pid];
    }
    bool live = inside && gq != 0.f, first = true;
    float T = 1.0f, A = 0.f, B = 0.f, d0 = 0.f;
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    const float cX = 2.f * GGR_INV_KQ * 0.5f * (float)W, cY = 2.f * GGR_INV_KQ * 0.5f * (float)H;   // 1/k and the NDC scaling of the mean

    if (tid == 0) {
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
        dval[BATCH] = 0.f;
    }
    bool wdone = !__any(live);
    if (lane == 0) wave_done[wave] = wdone ? 1 : 0;

    const int my_slot = lane / LPE, my_c = lane % LPE;
    uint32_t g_next = tid < total ? point_list[range.x + tid] : 0u;
    for (int b0 = 0; b0 < total; b0 += BATCH) {
        __syncthreads();
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;
        const int nb = min(BATCH, total - b0);
        const uint32_t g = g_next;
        if (b0 + BATCH + tid < total) g_next = point_list[range.x + b0 + BATCH + tid];
        if (tid < nb) {
            float dv;
            stage[tid] = stage_dist_splat(splat, g, dv);
            dval[tid] = dv;
        }
        __syncthreads();
        if (!wdone) {
            uint32_t* my_surv = surv[wave];
            float bx0 = rx0, by0 = ry0, bx1 = rx1, by1 = ry1;
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
                    const bool cand = live & (q2 >= 0.0f) & (alpha >= GGR_ALPHA_MIN);
                    const float wr = alpha * T;
                    const float test_T = T - wr;
                    const bool stop = cand & (test_T < GGR_T_MIN);
                    const bool take = cand & !stop;
                    live = live & !stop;
                    const float w = take ? wr : 0.f;
                    const float d = dval[e];
                    d0 = (take & first) ? d : d0;
                    first = first & !take;
                    const float dr = take ? d - d0 : 0.f;
                    const float A2 = 2.f * A - Atot;
                    const float c = 2.f * (fmaf(dr, A2, Btot) - 2.f * B);   // ∂Q/∂w of this entry
                    R = fmaf(-w, c, R);   // now: everything BEHIND this entry
                    const float inv = __builtin_amdgcn_rcpf(1.f - (take ? alpha : 0.f));
                    const float dL_dalpha = gq * (T * c - R * inv);
                    const float mm = take ? G * dL_dalpha : 0.f;
                    // with h = −½·opacity·m:  dL/dconic = Σ h·d dᵀ (xy in the half convention), dL/dmean = 2·conic·Σ h·d
                    const float h = -0.5f * rb.y * mm, u2 = h * dx, v2 = h * dy, hw2 = 0.5f * a.w;
                    v[sl * VC + 0] = cX * fmaf(a.z, u2, hw2 * v2);
                    v[sl * VC + 1] = cY * fmaf(rb.x, v2, hw2 * u2);
                    v[sl * VC + 2] = u2 * dx;
                    v[sl * VC + 3] = u2 * dy;
                    v[sl * VC + 4] = v2 * dy;
                    v[sl * VC + 5] = mm;
                    v[sl * VC + 6] = gq * 2.f * w * (A2 + w);   // dL/dd
                    v[sl * VC + 7] = 0.f;
                    A += w;
                    B = fmaf(w, dr, B);
                    T -= w;
                }
                // ---- the butterfly: 64 lanes × 64 values → every lane ONE finished sum of entry `my_slot`
                fold_swap32<N / 2>(v);
                fold_swap16<N / 4>(v);
                fold_dpp<N / 8, 0x128>(v, (lane & 8) != 0);     // row_ror:8
                fold_dpp<N / 16, 0x141>(v, (lane & 4) != 0);    // row_half_mirror (pairs c with 7 − c: bit 2 differs)
                fold_dpp<N / 32, 0x4E>(v, (lane & 2) != 0);     // quad_perm [2,3,0,1]
                fold_dpp<N / 64, 0xB1>(v, (lane & 1) != 0);     // quad_perm [1,0,3,2]
                // ---- commit: one atomic per finished sum (zero sums — the null record's, the padding value — are not sent)
                const float val = v[0];
                if (my_e != (uint32_t)BATCH && val != 0.f && my_c < 7) {
                    const uint32_t gid = __float_as_uint(stage[my_e].b.w);
                    atomicAdd(grad2d + GGR_G2D_STRIDE * (size_t)gid + GGR_G2D_MEAN + my_c, val);
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
    }
}

void launch_blend_dist_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           const float* out_distortion, const float* totals, const float* dL_dout, float* grad2d, int views,
                           hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    hipLaunchKernelGGL(blend_dist_bwd_kernel, dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges, point_list, splat,
                       out_distortion, totals, dL_dout, grad2d, views);
}

}  // namespace ggr

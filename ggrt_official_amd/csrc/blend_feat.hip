// blend_feat.hip — the feature pass: K per-Gaussian channels composited over the tile lists of a forward, for gfx950.
//
// No counterpart in the reference (its rasterizer blends three colour channels and one scalar; a host that wants more calls
// it once per three channels).  Both kernels REPLAY the sorted tile lists and the 32-B splat records a forward left in the
// caller's buffers — no preprocess, no sort, no list build — with the colour blend's own rules and arithmetic
// (blend_fwd.hip: power > 0 skip, α < 1/255 skip, α capped at 0.99, stop at T·(1−α) < 1e-4; stage_scale_conic, staged_q2,
// exp2, the same operation order), so the weights w = α·T are the colour blend's bit for bit.
//
// Mapping, as blend_fwd: one 256-thread workgroup per 16×16 tile, wave w owns the 8×8 quadrant (w&1, w>>1); the list is staged
// through LDS in batches of 256 entries, a batch's K feature values beside its records (rows padded to KC floats, read back
// as wave-uniform 16-B broadcasts); every wave culls the batch against its quadrant and walks the survivors.
//
// Backward: a FRONT-TO-BACK replay.  With dF_k = dL/dF_k of the pixel and c_s = Σ_k f_sk·dF_k,
//     dL/df_gk   = Σ_pixels w_s·dF_k
//     dL/dα_s    = T_s·c_s − R_s/(1−α_s),   R_s = Σ_{s' behind s} w_s'·c_s' = Σ_k F_k·dF_k − Σ_{s' up to s} w_s'·c_s'
// — "everything behind" is the pixel's final F (the forward's output, handed back in) less the running prefix: no
// checkpoints, no n_contrib, no final T.  dL/dα is chained to the 2D mean, conic and opacity as blend_bwd.hip does it and the
// six sums are added into the same per-(view, Gaussian) record slots (GGR_G2D_MEAN … GGR_G2D_OPACITY), so preprocess_bwd
// carries the feature loss on unchanged.  Per entry a wave has KC + 6 sums over its 64 pixels; RB entries at a time go through
// ONE transposing butterfly (each level halves the values a lane holds: ≈ one exchange + one add per value instead of six),
// after which every lane owns (KC + 8)/8 — or /16 — finished sums of one entry and commits them with one atomic each.
#include "blend_butterfly.h"
#include "blend_common.h"
#include "blend_feat.h"

namespace ggr {

#define BATCH GGR_BATCH
#define FEAT_GROUP 4   // survivors per trip of the forward's blend loop (one broadcast read of their indices)

// row of `features` that list id g (pair index view·P1 + Gaussian) reads: Gaussian set view / vps, same Gaussian
__device__ __forceinline__ size_t feat_row(uint32_t g, int view, int P1, int vps) {
    return (size_t)(view / vps) * (size_t)P1 + (size_t)(g - (uint32_t)view * (uint32_t)P1);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int KC>
__global__ void __launch_bounds__(256)
blend_feat_fwd_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                      const float4* __restrict__ splat, const float* __restrict__ features, int K, int P1, int vps,
                      float* __restrict__ out_features, int views, int interleaved) {
    __shared__ FeatSplat stage[BATCH + 1];                               // + the null record that pads a survivor list
    __shared__ __attribute__((aligned(16))) float feat[BATCH + 1][KC];   // the entries' channels, zero beyond K
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + FEAT_GROUP];
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
    const size_t hw = (size_t)H * W;
    const size_t pid = inside ? (size_t)py * W + px : 0;
    out_features += (size_t)view * (size_t)K * hw;

    float T = 1.0f;
    float F[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) F[k] = 0.f;
    bool live = inside;
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    if (tid == 0) {   // the null record: opacity 0 → α = 0 → never contributes
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < KC) feat[BATCH][tid] = 0.f;
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
            stage[tid] = stage_feat_splat(splat, g);
            const float* row = features + feat_row(g, view, P1, vps) * (size_t)K;
#pragma unroll
            for (int k = 0; k < KC; k++) feat[tid][k] = k < K ? row[k] : 0.f;
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
            if (lane < FEAT_GROUP) my_surv[ns + lane] = (uint32_t)BATCH;   // pad with the null record
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k0 = 0; k0 < ns; k0 += FEAT_GROUP) {
                uint32_t pkw[FEAT_GROUP];
                __builtin_memcpy(pkw, my_surv + k0, sizeof pkw);
#pragma unroll
                for (int u = 0; u < FEAT_GROUP; u++) {
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
                    const float4* fr = reinterpret_cast<const float4*>(feat[e]);
#pragma unroll
                    for (int k4 = 0; k4 < KC / 4; k4++) {
                        const float4 f = fr[k4];
                        F[4 * k4] = fmaf(f.x, w, F[4 * k4]); F[4 * k4 + 1] = fmaf(f.y, w, F[4 * k4 + 1]);
                        F[4 * k4 + 2] = fmaf(f.z, w, F[4 * k4 + 2]); F[4 * k4 + 3] = fmaf(f.w, w, F[4 * k4 + 3]);
                    }
                    T -= w;
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
    }
    if (inside) {
#pragma unroll
        for (int k = 0; k < KC; k++)
            if (k < K) out_features[(size_t)k * hw + pid] = F[k];
    }
}

void launch_blend_feat_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           const float* features, int K, int P1, int vps, float* out_features, int views, int scissored,
                           hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
#define GGR_LAUNCH_FFWD(KC_)                                                                                                  \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_feat_fwd_kernel<KC_>), dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges,       \
                       point_list, splat, features, K, P1, vps, out_features, views,                                           \
                       xcd_forward_interleaved(nt, scissored != 0) ? 1 : 0)
    if (K <= 4) GGR_LAUNCH_FFWD(4);
    else if (K <= 8) GGR_LAUNCH_FFWD(8);
    else if (K <= 16) GGR_LAUNCH_FFWD(16);
    else GGR_LAUNCH_FFWD(32);
#undef GGR_LAUNCH_FFWD
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// (feat_dpp, fold_dpp, fold_swap32, fold_swap16 — the transposing butterfly's levels — live in blend_butterfly.h: the distortion
//  pass, blend_dist.hip, reduces its sums the same way)

// KC channels per walk of the list, RB entries per butterfly.  A lane's values of one entry: KC × w·dF_k, then the six
// geometric terms in record order (mean x, y; conic xx, xy, yy; opacity) and two zeros: VC = KC + 8 values, RB·VC in all.
// RB = 8 (VC a multiple of 8): lane = 8·entry + c ends with values [c·VC/8, (c+1)·VC/8) of its entry;
// RB = 4 (VC a multiple of 16): lane = 16·entry + c ends with values [c·VC/16, (c+1)·VC/16).
template <int KC, int RB>
__global__ void __launch_bounds__(256)
blend_feat_bwd_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                      const float4* __restrict__ splat, const float* __restrict__ features, int K, int kbase, int kn, int P1,
                      int vps, const float* __restrict__ out_features, const float* __restrict__ dL_dout,
                      float* __restrict__ dL_dfeatures, float* __restrict__ grad2d, int views) {
    constexpr int VC = KC + 8, N = RB * VC, LPE = 64 / RB /*lanes per entry*/, M = VC / LPE /*values a lane commits*/;
    static_assert(RB == 8 || RB == 4, "entries per butterfly");
    static_assert(VC % LPE == 0 && KC % 4 == 0, "values per entry must split evenly over the entry's lanes");
    static_assert(GGR_G2D_MEAN == 3 && GGR_G2D_CONIC == 5 && GGR_G2D_OPACITY == 8, "the six geometric sums are committed in record order");
    __shared__ FeatSplat stage[BATCH + 1];
    __shared__ __attribute__((aligned(16))) float feat[BATCH + 1][KC];
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
    const size_t plane0 = ((size_t)view * (size_t)K + (size_t)kbase) * hw;

    // the pixel's upstream gradient and R = Σ_k F_k·dF_k over this walk's channels.  A pixel whose gradient is exactly zero adds
    // exactly zero to every sum: it takes no entry (blend_bwd.hip's zero-gradient skip)
    float dF[KC];
    float R = 0.f;
    bool any_grad = false;
#pragma unroll
    for (int k = 0; k < KC; k++) {
        dF[k] = 0.f;
        if (inside && k < kn) {
            dF[k] = dL_dout[plane0 + (size_t)k * hw + pid];
            R = fmaf(out_features[plane0 + (size_t)k * hw + pid], dF[k], R);
            any_grad = any_grad || dF[k] != 0.f;
        }
    }
    bool live = inside && any_grad;
    float T = 1.0f;
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    const float cX = 2.f * GGR_INV_KQ * 0.5f * (float)W, cY = 2.f * GGR_INV_KQ * 0.5f * (float)H;   // 1/k and the NDC scaling of the mean

    if (tid == 0) {
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < KC) feat[BATCH][tid] = 0.f;
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
            stage[tid] = stage_feat_splat(splat, g);
            const float* row = features + feat_row(g, view, P1, vps) * (size_t)K + kbase;
#pragma unroll
            for (int k = 0; k < KC; k++) feat[tid][k] = k < kn ? row[k] : 0.f;
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
                const uint32_t my_e = my_surv[k0 + my_slot];   // the entry whose sums this lane commits
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
                    const float4* fr = reinterpret_cast<const float4*>(feat[e]);
                    float cdp = 0.f;
#pragma unroll
                    for (int k4 = 0; k4 < KC / 4; k4++) {
                        const float4 f = fr[k4];
                        cdp = fmaf(f.x, dF[4 * k4], cdp); cdp = fmaf(f.y, dF[4 * k4 + 1], cdp);
                        cdp = fmaf(f.z, dF[4 * k4 + 2], cdp); cdp = fmaf(f.w, dF[4 * k4 + 3], cdp);
                    }
#pragma unroll
                    for (int k = 0; k < KC; k++) v[sl * VC + k] = w * dF[k];
                    R = fmaf(-w, cdp, R);   // now: everything BEHIND this entry
                    const float inv = __builtin_amdgcn_rcpf(1.f - (take ? alpha : 0.f));
                    const float dL_dalpha = T * cdp - R * inv;
                    const float mm = take ? G * dL_dalpha : 0.f;
                    T -= w;
                    // with h = −½·opacity·m:  dL/dconic = Σ h·d dᵀ (xy in the half convention), dL/dmean = 2·conic·Σ h·d
                    const float h = -0.5f * rb.y * mm, u2 = h * dx, v2 = h * dy, hw2 = 0.5f * a.w;
                    v[sl * VC + KC + 0] = cX * fmaf(a.z, u2, hw2 * v2);
                    v[sl * VC + KC + 1] = cY * fmaf(rb.x, v2, hw2 * u2);
                    v[sl * VC + KC + 2] = u2 * dx;
                    v[sl * VC + KC + 3] = u2 * dy;
                    v[sl * VC + KC + 4] = v2 * dy;
                    v[sl * VC + KC + 5] = mm;
                    v[sl * VC + KC + 6] = 0.f;
                    v[sl * VC + KC + 7] = 0.f;
                }
                // ---- the butterfly: 64 lanes × N values → every lane M finished sums of entry `my_slot`
                fold_swap32<N / 2>(v);
                fold_swap16<N / 4>(v);
                fold_dpp<N / 8, 0x128>(v, (lane & 8) != 0);     // row_ror:8
                fold_dpp<N / 16, 0x141>(v, (lane & 4) != 0);    // row_half_mirror (pairs c with 7 − c: bit 2 differs)
                fold_dpp<N / 32, 0x4E>(v, (lane & 2) != 0);     // quad_perm [2,3,0,1]
                fold_dpp<N / 64, 0xB1>(v, (lane & 1) != 0);     // quad_perm [1,0,3,2]
                static_assert(N / 64 == M, "values left per lane");
                // ---- commit: one atomic per finished sum (zero sums — the null record's, padded channels — are not sent)
                const uint32_t gid = __float_as_uint(stage[my_e].b.w);
                float* const frow = dL_dfeatures + feat_row(gid, view, P1, vps) * (size_t)K + kbase;
                float* const rec = grad2d + GGR_G2D_STRIDE * (size_t)gid + GGR_G2D_MEAN;
#pragma unroll
                for (int i = 0; i < M; i++) {
                    const int j = my_c * M + i;
                    const float val = v[i];
                    if (my_e != (uint32_t)BATCH && val != 0.f) {
                        if (j < KC) { if (j < kn) atomicAdd(frow + j, val); }
                        else if (j < KC + 6) atomicAdd(rec + (j - KC), val);
                    }
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
    }
}

void launch_blend_feat_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                           const float* features, int K, int P1, int vps, const float* out_features, const float* dL_dout,
                           float* dL_dfeatures, float* grad2d, int views, hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
#define GGR_LAUNCH_FBWD(KC_, RB_, KB_, KN_)                                                                                   \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_feat_bwd_kernel<KC_, RB_>), dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges,  \
                       point_list, splat, features, K, KB_, KN_, P1, vps, out_features, dL_dout, dL_dfeatures, grad2d, views)
    // the list is walked once per group of channels: 24 at a time while more than 8 are left, then 8
    for (int kb = 0; kb < K;) {
        const int left = K - kb;
        if (left > 8) { const int kn = min(left, 24); GGR_LAUNCH_FBWD(24, 4, kb, kn); kb += kn; }
        else { GGR_LAUNCH_FBWD(8, 8, kb, left); kb += left; }
    }
#undef GGR_LAUNCH_FBWD
}

}  // namespace ggr

// blend_hits_grad.hip — the hit pass's backward: a loss over the per-pixel hit weights (blend_hits.hip's `weight` and `rest`)
// differentiated w.r.t. the 2D mean, conic and opacity of every Gaussian, for gfx950.
//
// No counterpart in the reference.  Per pixel, over its LIVE entries in list order i = 0 … n−1 (n = count), with α_i, T_i and
// w_i = α_i·T_i the colour blend's own values, the upstream gradient of entry i is
//     g_i = dL_dweight[i]  (i < K)          g_i = dL_drest  (i >= K)
// — the entry's weight sits in slot i, or in the rest-sum —, and
//     dL/dα_i = T_i·g_i − S_i/(1−α_i),    S_i = Σ_{j behind i} g_j·w_j
// — the feature backward's front-to-back recurrence (blend_feat.hip) with a "feature" that belongs to the (pixel, entry) pair
// instead of the Gaussian.  S_i is NOT formed as total − prefix over all n entries: where the g are (nearly) equal — a loss on
// alpha = Σ weight + rest is the extreme — T_i·g_i and S_i/(1−α_i) cancel down to g·T_final/(1−α_i), and a float32 total − prefix
// leaves an error of 1e-7·total in a value of 1e-4·total at a saturated pixel.  Every entry behind the K-th has the SAME gradient,
// so the kernel splits off a per-pixel constant c — dL_drest where n > K, else the gradient of the pixel's last filled slot — and
// uses Σ_{j behind i} w_j = T_{i+1} − T_final (T_final: the colour forward's final transmittance, read from its image buffer):
//     dL/dα_i = T_i·(g_i − c) + ( c·T_final − S'_i )/(1−α_i),    S'_i = Σ_{i<j<min(n,K)} (g_j − c)·w_j = total' − prefix',
//     total'  = Σ_{k<min(n,K)} (dL_dweight[k] − c)·weight[k]
// — the cancelling part is exact, behind the K-th entry nothing is left of the recurrence (g − c = 0 there), and total' − prefix'
// runs over the K slots only, with total' from the `weight` array the forward wrote (the same products in the same order, as
// the feature backward takes its total from out_features).  `rest` is not needed.
// dL/dα is chained to the 2D mean, conic and opacity as blend_feat_bwd_kernel / blend_dist_bwd_kernel do it (the 0.99 cap
// straight-through; skip, threshold and stop decisions constants; the stop entry and skipped entries get nothing), and the six
// sums are added into slots GGR_G2D_MEAN … GGR_G2D_OPACITY of the entry's per-(view, Gaussian) record, so preprocess_bwd carries
// the loss on unchanged.
//
// Mapping and staging, as blend_hits_kernel: one 256-thread workgroup per 16×16 tile, wave w owns the 8×8 quadrant (w&1, w>>1),
// the list staged through LDS in batches of 256 entries, every wave culls the batch against the box of its live pixels and
// walks the survivors with the colour blend's α / T / stop lines.
//
// The gradient at the slot a lane is about to fill.  A lane needs g at ITS slot counter, which differs from lane to lane — a
// register array indexed by it would spill to scratch (blend_hits.hip), a load from memory behind every taken entry would put a
// memory latency into the T recurrence.  The tile's gradients are therefore staged ONCE, in the prologue, into an LDS table of
// K + 1 rows × 256 floats: row k = dL_dweight[k] − c of the workgroup's 256 pixels, row K = 0 (behind the slots g − c = 0);
// thread t reads and writes column t only (no barrier, and word (row·256 + t) is in bank t mod 64 whatever the row: every read is conflict-free).  The
// prologue zeroes what the forward padded — rows k >= count — WITHOUT loading it, reads dL_drest only where count > K, and forms
// total' over the filled slots only: nothing the forward padded is read, whatever it holds.  The table is dynamic LDS, (K + 1) KB.
//
// A pixel whose gradients are all exactly zero takes no entry (blend_bwd.hip's zero-gradient skip), and a pixel whose rest has
// no gradient is finished once its last slot with one is filled: everything behind adds exactly nothing.
#include "blend_butterfly.h"
#include "blend_common.h"
#include "blend_hits_grad.h"

namespace ggr {

#define BATCH GGR_BATCH
#define HITG_GROUP 8   // entries per butterfly

// A lane's values of one entry: the six geometric terms in record order (mean x, y; conic xx, xy, yy; opacity) and two zeros:
// VC = 8 values, RB = 8 entries per butterfly, after which lane 8·entry + c owns sum c of its entry.
__global__ void __launch_bounds__(256)
blend_hits_bwd_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                      const float4* __restrict__ splat, const float* __restrict__ final_T, int K, const float* __restrict__ weight,
                      const int32_t* __restrict__ count, const float* __restrict__ dL_dweight, const float* __restrict__ dL_drest,
                      float* __restrict__ grad2d, int views) {
    constexpr int RB = HITG_GROUP, VC = 8, N = RB * VC, LPE = 64 / RB /*lanes per entry*/;
    static_assert(RB == 8 && VC == LPE && N == 64, "one finished sum per lane");
    static_assert(GGR_G2D_MEAN == 3 && GGR_G2D_CONIC == 5 && GGR_G2D_OPACITY == 8, "the six geometric sums are committed in record order");
    __shared__ FeatSplat stage[BATCH + 1];
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + RB];
    __shared__ int wave_done[4];
    extern __shared__ float gtab[];   // [K + 1][256]: g − c of slot k (row K: 0), per pixel of the tile

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
    const size_t hw = (size_t)H * (size_t)W;
    const size_t pix = inside ? (size_t)py * (size_t)W + (size_t)px : 0;
    const size_t slot0 = (size_t)view * (size_t)K * hw + pix;   // slot k of this pixel: slot0 + k·hw
    const size_t plane = (size_t)view * hw + pix;

    // the pixel's constant c, its gradients less c into its column of the table, and R = total'.  Only the places the forward
    // filled are read
    const int n = inside ? count[plane] : 0;
    const int nk = min(n, K);   // the slots that hold an entry
    float* const my_g = gtab + tid;
    float c = 0.f;
    if (n > K) { if (dL_drest) c = dL_drest[plane]; }
    else if (nk > 0 && dL_dweight) c = dL_dweight[slot0 + (size_t)(nk - 1) * hw];
    float R = 0.f;
    bool any_grad = c != 0.f;
    for (int k = 0; k < K; k++) {
        float gd = 0.f;
        if (k < nk) {
            const float g = dL_dweight ? dL_dweight[slot0 + (size_t)k * hw] : 0.f;
            gd = g - c;
            R = fmaf(gd, weight[slot0 + (size_t)k * hw], R);
            any_grad = any_grad || g != 0.f;
        }
        my_g[k * 256] = gd;
    }
    my_g[K * 256] = 0.f;
    const float cTf = any_grad ? c * final_T[plane] : 0.f;   // c·T_final: what is left of T_i·c − c·Σ_{j behind i} w_j/(1−α_i), times (1−α_i)
    const bool has_rest = n > K && c != 0.f;                // the entries behind the K-th carry a gradient

    bool live = inside && any_grad;
    float T = 1.0f;
    int cnt = 0;
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    const float cX = 2.f * GGR_INV_KQ * 0.5f * (float)W, cY = 2.f * GGR_INV_KQ * 0.5f * (float)H;   // 1/k and the NDC scaling of the mean

    if (tid == 0) {   // the null record: opacity 0 → α = 0 → never live
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    bool wdone = !__any(live);
    if (lane == 0) wave_done[wave] = wdone ? 1 : 0;

    const int my_slot = lane / LPE, my_c = lane % LPE;
    uint32_t g_next = tid < total ? point_list[range.x + tid] : 0u;
    for (int b0 = 0; b0 < total; b0 += BATCH) {
        __syncthreads();  // previous batch fully consumed; wave_done visible
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;
        const int nb = min(BATCH, total - b0);
        const uint32_t gl = g_next;
        if (b0 + BATCH + tid < total) g_next = point_list[range.x + b0 + BATCH + tid];
        if (tid < nb) stage[tid] = stage_feat_splat(splat, gl);
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
                    const float w = take ? wr : 0.f;
                    const float g = my_g[min(cnt, K) * 256];   // g − c of the slot this entry would fill (row K: behind the slots)
                    R = fmaf(-w, g, R);   // now: the slots BEHIND this entry
                    const float inv = __builtin_amdgcn_rcpf(1.f - (take ? alpha : 0.f));
                    const float dL_dalpha = fmaf(T, g, (cTf - R) * inv);
                    const float mm = take ? G * dL_dalpha : 0.f;
                    cnt += take ? 1 : 0;
                    T -= w;
                    // (behind the last slot that carries a gradient, with none on the rest, every entry adds exactly nothing)
                    live = live & !stop & ((cnt < nk) | has_rest);
                    // with h = −½·opacity·m:  dL/dconic = Σ h·d dᵀ (xy in the half convention), dL/dmean = 2·conic·Σ h·d
                    const float h = -0.5f * rb.y * mm, u2 = h * dx, v2 = h * dy, hw2 = 0.5f * a.w;
                    v[sl * VC + 0] = cX * fmaf(a.z, u2, hw2 * v2);
                    v[sl * VC + 1] = cY * fmaf(rb.x, v2, hw2 * u2);
                    v[sl * VC + 2] = u2 * dx;
                    v[sl * VC + 3] = u2 * dy;
                    v[sl * VC + 4] = v2 * dy;
                    v[sl * VC + 5] = mm;
                    v[sl * VC + 6] = 0.f;
                    v[sl * VC + 7] = 0.f;
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
                if (my_e != (uint32_t)BATCH && val != 0.f && my_c < 6) {
                    const uint32_t gid = __float_as_uint(stage[my_e].b.w);
                    atomicAdd(grad2d + GGR_G2D_STRIDE * (size_t)gid + GGR_G2D_MEAN + my_c, val);
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
    }
}

void launch_blend_hits_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat, const float* final_T,
                           int K, const float* weight, const int32_t* count, const float* dL_dweight, const float* dL_drest,
                           float* grad2d, int views, hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    const size_t table_bytes = (size_t)(K + 1) * 256 * sizeof(float);   // <= 33 KB at K = GGR_MAX_HITS
    hipLaunchKernelGGL(blend_hits_bwd_kernel, dim3(xcd_grid(nt)), dim3(256), table_bytes, s, W, H, gx, ranges, point_list, splat,
                       final_T, K, weight, count, dL_dweight, dL_drest, grad2d, views);
}

}  // namespace ggr

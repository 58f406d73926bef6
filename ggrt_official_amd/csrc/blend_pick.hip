// blend_pick.hip — the pick pass: per-PIXEL picks over the entries the colour blend composited, for gfx950.
//
// No counterpart in the reference.  Like the contribution pass (blend_contrib.hip) the kernel REPLAYS the sorted tile lists and
// the 32-B splat records a forward left in the caller's buffers, with the colour blend's own rules and arithmetic
// (blend_common.h: power > 0 skip, α < 1/255 skip, α capped at 0.99, stop at T·(1−α) < 1e-4; stage_scale_conic, staged_q2,
// exp2, the same operation order as blend_contrib_kernel line for line), so w = α·T_before — and with it the T_before > 0.5
// decision — is the colour blend's bit for bit.  It applies the stop rule itself: a no_backward forward's smaller buffers serve.
// Where the contribution pass reduces over the pixels of a Gaussian, this pass keeps, per pixel, over its LIVE entries
//     median_index = the id of the last one with T_before > 0.5 (2DGS / gsplat's median rule; the first live entry qualifies),
//     median_depth = that Gaussian's depth value (the .z of its record's second float4: what the depth plane blends),
//     max_index / max_weight = the id and w of the largest w (strict > while walking: among equal w the earliest),
//     count = their number;      −1 / 0 / −1 / 0 / 0 for a pixel without a live entry.
//
// Mapping and staging, as blend_contrib's: one 256-thread workgroup per 16×16 tile, wave w owns the 8×8 quadrant (w&1, w>>1);
// the list is staged through LDS in batches of 256 entries; every wave culls the batch against the box of its still-live pixels
// and walks the survivors, 8 at a time; the tile is left once all four waves are done.  What is different: every quantity
// belongs to ONE pixel, hence to one lane — no cross-lane reduction, no LDS result tables, no atomics.  A lane carries T, live,
// the two ids, the best w and the count in registers and stores its own pixel at the end with plain vector stores.  The depth
// value is not in the staged record: it is gathered once per pixel behind the walk (where asked for and the median exists).
//
// Every plane is order-independent (no sum, no atomic): bit-identical from run to run and across the forms of the depth sort.
#include "blend_common.h"
#include "blend_pick.h"

namespace ggr {

#define BATCH GGR_BATCH
#define PICK_GROUP 8   // survivors per unrolled trip

__global__ void __launch_bounds__(256)
blend_pick_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                  const float4* __restrict__ splat, int32_t* __restrict__ median_index, float* __restrict__ median_depth,
                  int32_t* __restrict__ max_index, float* __restrict__ max_weight, int32_t* __restrict__ count, int views,
                  int P1, int interleaved) {
    __shared__ FeatSplat stage[BATCH + 1];                               // + the null record that pads a survivor list
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + PICK_GROUP];
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

    float T = 1.0f;
    bool live = inside;
    uint32_t med_id = 0xFFFFFFFFu, best_id = 0xFFFFFFFFu;   // list ids; all ones = none
    float best_w = 0.f;
    int cnt = 0;
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    if (tid == 0) {   // the null record: opacity 0 → α = 0 → never live
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane == 0) wave_done[wave] = quad_live ? 0 : 1;
    bool wdone = !quad_live;

    uint32_t g_next = tid < total ? point_list[range.x + tid] : 0u;
    for (int b0 = 0; b0 < total; b0 += BATCH) {
        // (the barrier that ended the previous batch: its records are consumed)
        const int nb = min(BATCH, total - b0);
        const uint32_t g = g_next;
        if (b0 + BATCH + tid < total) g_next = point_list[range.x + b0 + BATCH + tid];
        if (tid < nb) stage[tid] = stage_feat_splat(splat, g);
        __syncthreads();
        if (!wdone) {
            uint32_t* my_surv = surv[wave];
            float bx0 = rx0, by0 = ry0, bx1 = rx1, by1 = ry1;   // the pixels that are not saturated yet
            {
                const uint64_t act = __ballot(live);
                if (act) active_box(act, rx0, ry0, bx0, by0, bx1, by1);
            }
            const int ns = cull_batch(stage, nb, my_surv, lane, bx0, by0, bx1, by1);
            if (lane < PICK_GROUP) my_surv[ns + lane] = (uint32_t)BATCH;   // pad the last group with the null record
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k0 = 0; k0 < ns; k0 += PICK_GROUP) {
                uint32_t pkw[PICK_GROUP];
                __builtin_memcpy(pkw, my_surv + k0, sizeof pkw);
#pragma unroll
                for (int u = 0; u < PICK_GROUP; u++) {
                    const uint32_t e = pkw[u];   // (VGPR, uniform)
                    const float4 a = stage[e].a;
                    const float4 rb = stage[e].b;   // (k·cyy, opacity, k·qmax, id)
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
                    const uint32_t id = __float_as_uint(rb.w);
                    med_id = (take & (T > 0.5f)) ? id : med_id;   // T is still T_before here
                    const bool better = w > best_w;               // (w = 0 where the entry is not taken: never better)
                    best_id = better ? id : best_id;
                    best_w = better ? w : best_w;
                    cnt += take ? 1 : 0;
                    T -= w;
                }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
        __syncthreads();   // the records are consumed, wave_done is visible
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;   // every pixel of the tile has stopped
    }

    if (!inside) return;   // a pixel (or a whole quadrant) outside the frame stores nothing
    const size_t pix = ((size_t)view * (size_t)H + (size_t)py) * (size_t)W + (size_t)px;
    const int32_t base = view * P1;   // list id → Gaussian index within the view's set
    const bool has_med = med_id != 0xFFFFFFFFu;
    if (median_index) median_index[pix] = has_med ? (int32_t)med_id - base : -1;
    if (median_depth) median_depth[pix] = has_med ? splat[2 * (size_t)med_id + 1].z : 0.f;
    if (max_index) max_index[pix] = best_id != 0xFFFFFFFFu ? (int32_t)best_id - base : -1;
    if (max_weight) max_weight[pix] = best_w;
    if (count) count[pix] = cnt;
}

void launch_blend_pick(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                       int32_t* median_index, float* median_depth, int32_t* max_index, float* max_weight, int32_t* count,
                       int views, int P1, int scissored, hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    hipLaunchKernelGGL(blend_pick_kernel, dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges, point_list, splat,
                       median_index, median_depth, max_index, max_weight, count, views, P1,
                       xcd_forward_interleaved(nt, scissored != 0) ? 1 : 0);
}

}  // namespace ggr

// blend_hits.hip — the hit pass: per-PIXEL hit lists over the entries the colour blend composited, for gfx950.
//
// No counterpart in the reference.  Like the pick pass (blend_pick.hip) the kernel REPLAYS the sorted tile lists and the 32-B
// splat records a forward left in the caller's buffers, with the colour blend's own rules and arithmetic (blend_common.h:
// power > 0 skip, α < 1/255 skip, α capped at 0.99, stop at T·(1−α) < 1e-4; stage_scale_conic, staged_q2, exp2, the same
// operation order as blend_pick_kernel line for line), so w = α·T_before is the colour blend's bit for bit.  It applies the
// stop rule itself: a no_backward forward's smaller buffers serve.  Where the pick pass keeps ONE entry per pixel, this pass
// keeps the list itself, cut at K: per pixel, over its LIVE entries in list order (front to back),
//     index[k] / weight[k] = the id and w of the k-th one, k < K                        (−1 / 0 for k >= count),
//     rest  = Σ w of those behind the K-th, summed in list order                        (what the K slots leave out of alpha),
//     count = their number (all of them, not min(count, K)).
//
// Mapping and staging, as blend_pick's: one 256-thread workgroup per 16×16 tile, wave w owns the 8×8 quadrant (w&1, w>>1);
// the list is staged through LDS in batches of 256 entries; every wave culls the batch against the box of its still-live pixels
// and walks the survivors, 8 at a time; the tile is left once all four waves are done.  Every quantity belongs to ONE pixel,
// hence to one lane — no cross-lane reduction, no LDS result tables, no atomics.  K is a runtime argument and the slots live in
// MEMORY, not in registers: a lane carries T, live, its slot counter and the rest-sum, and a taken entry with cnt < K goes
// straight to index / weight[(view·K + cnt)·H·W + pixel] with two plain vector stores (a register array indexed by cnt would
// spill to scratch).  Behind the walk a lane pads its slots cnt … K−1 and stores rest and count.
//
// Without rest and count (a C host that wants the slots only) a pixel is finished once it holds K entries: it leaves the box the
// batch is culled against and the wave's exit test — the α / T lines do not see that, so index / weight keep every byte.
//
// Every array is a per-pixel result of a walk in list order (no atomic, no cross-lane sum): bit-identical from run to run and
// across the forms of the depth sort.
#include "blend_common.h"
#include "blend_hits.h"

namespace ggr {

#define BATCH GGR_BATCH
#define HIT_GROUP 8   // survivors per unrolled trip

__global__ void __launch_bounds__(256)
blend_hits_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                  const float4* __restrict__ splat, int K, int32_t* __restrict__ index, float* __restrict__ weight,
                  float* __restrict__ rest_out, int32_t* __restrict__ count, int views, int P1, int interleaved) {
    __shared__ FeatSplat stage[BATCH + 1];                               // + the null record that pads a survivor list
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + HIT_GROUP];
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

    const bool has_slots = index != nullptr;           // (index and weight come as a pair)
    const bool full_walk = rest_out || count;          // false: a pixel with K entries is finished
    const size_t hw = (size_t)H * (size_t)W;
    const size_t pix = (size_t)py * (size_t)W + (size_t)px;
    const size_t slot0 = (size_t)view * (size_t)K * hw + pix;   // slot k of this pixel: slot0 + k·hw
    const int32_t base = view * P1;   // list id → Gaussian index within the view's set

    float T = 1.0f;
    bool live = inside;
    int cnt = 0;
    float rest = 0.f;
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
            float bx0 = rx0, by0 = ry0, bx1 = rx1, by1 = ry1;   // the pixels that can still take an entry
            {
                const uint64_t act = __ballot(live & (full_walk | (cnt < K)));
                if (act) active_box(act, rx0, ry0, bx0, by0, bx1, by1);
            }
            const int ns = cull_batch(stage, nb, my_surv, lane, bx0, by0, bx1, by1);
            if (lane < HIT_GROUP) my_surv[ns + lane] = (uint32_t)BATCH;   // pad the last group with the null record
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k0 = 0; k0 < ns; k0 += HIT_GROUP) {
                uint32_t pkw[HIT_GROUP];
                __builtin_memcpy(pkw, my_surv + k0, sizeof pkw);
#pragma unroll
                for (int u = 0; u < HIT_GROUP; u++) {
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
                    const bool slot = take & (cnt < K);
                    if (slot & has_slots) {   // (take ⇒ live ⇒ inside the frame; cnt < K: inside the pixel's K slots)
                        const size_t o = slot0 + (size_t)cnt * hw;
                        index[o] = (int32_t)id - base;
                        weight[o] = w;
                    }
                    rest += (take & !slot) ? w : 0.f;
                    cnt += take ? 1 : 0;
                    T -= w;
                }
                if (!__any(live & (full_walk | (cnt < K)))) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
        __syncthreads();   // the records are consumed, wave_done is visible
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;   // every pixel of the tile has finished
    }

    if (!inside) return;   // a pixel (or a whole quadrant) outside the frame stores nothing
    if (has_slots) {
        for (int k = cnt; k < K; k++) {   // the slots behind the last live entry
            const size_t o = slot0 + (size_t)k * hw;
            index[o] = -1;
            weight[o] = 0.f;
        }
    }
    const size_t plane = (size_t)view * hw + pix;
    if (rest_out) rest_out[plane] = rest;
    if (count) count[plane] = cnt;
}

void launch_blend_hits(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat, int K,
                       int32_t* index, float* weight, float* rest, int32_t* count, int views, int P1, int scissored,
                       hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    hipLaunchKernelGGL(blend_hits_kernel, dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges, point_list, splat, K, index,
                       weight, rest, count, views, P1, xcd_forward_interleaved(nt, scissored != 0) ? 1 : 0);
}

}  // namespace ggr

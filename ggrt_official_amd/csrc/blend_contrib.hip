// blend_contrib.hip — the contribution pass: per-(view, Gaussian) statistics of the blend weight, for gfx950.
//
// No counterpart in the reference (whose rasterizer reports `radii > 0` and nothing about whether a Gaussian was ever seen).
// The kernel REPLAYS the sorted tile lists and the 32-B splat records a forward left in the caller's buffers, like the feature
// pass (blend_feat.hip), with the colour blend's own rules and arithmetic (blend_common.h: power > 0 skip, α < 1/255 skip,
// α capped at 0.99, stop at T·(1−α) < 1e-4; stage_scale_conic, staged_q2, exp2, the same operation order), so w = α·T is the
// colour blend's weight bit for bit.  It applies the stop rule itself: nothing a training forward stores for its backward is
// read, and a no_backward forward's smaller buffers serve.  Per list id it reduces, over the pixels where the entry is live,
//     weight_sum = Σ w,   weight_max = max w,   pixel_count = the number of those pixels.
//
// Mapping, as blend_feat's forward: one 256-thread workgroup per 16×16 tile, wave w owns the 8×8 quadrant (w&1, w>>1); the
// list is staged through LDS in batches of 256 entries; every wave culls the batch against its quadrant and walks the
// survivors, 8 at a time.  A wave's 64 pixels × 8 entries × {sum, max, count} go through three TRANSPOSING butterflies
// (v_permlane32_swap, v_permlane16_swap, row_ror:8 halve the values a lane holds; three plain levels finish the 8 lanes of an
// entry): 10 exchanges per quantity and 8 entries instead of 48, after which lane 8·j holds entry j's three results and
// stores them in the wave's column of the batch's LDS table — plain stores, no LDS atomics: a wave meets an entry once.
// Behind the walk, thread e adds up the four waves' columns of entry e in fixed order and, if the tile's count for the
// entry is not zero, issues the global updates — at most three vector atomics per (tile, entry) instead of per (quadrant,
// entry): a float atomicAdd for the sum, an integer atomicMax on the float's bits for the max (w >= 0: the bit order is the
// value order) and an integer atomicAdd for the count.
//
// Reproducibility: weight_max and pixel_count are integer atomics of values that do not depend on any order: bit-identical
// from run to run.  weight_sum is a float sum whose per-tile terms are formed in a fixed order but arrive in any order: it is
// reproducible only up to the order of those additions.
#include "blend_common.h"
#include "blend_contrib.h"

namespace ggr {

#define BATCH GGR_BATCH
#define CONTRIB_GROUP 8   // survivors per butterfly

struct SumOp { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct MaxOp { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

template <int CTRL>
__device__ __forceinline__ float contrib_dpp(float v) {   // (every lane has a source under the controls used below)
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// 64 lanes × 8 values → lane 8·j + c holds op over the wave's 64 lanes of value j (every c)
template <class Op>
__device__ __forceinline__ float reduce8(float* v, int lane, Op op) {
#pragma unroll
    for (int i = 0; i < 4; i++) {   // lanes 0-31 keep values 0-3, lanes 32-63 values 4-7
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 4]), false, false);
        v[i] = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {   // even 16-lane rows keep the lower two, odd rows the upper two
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 2]), false, false);
        v[i] = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    const bool upper = (lane & 8) != 0;
    const float keep = upper ? v[1] : v[0], send = upper ? v[0] : v[1];
    float x = op(keep, contrib_dpp<0x128>(send));   // row_ror:8
    x = op(x, contrib_dpp<0x141>(x));               // row_half_mirror
    x = op(x, contrib_dpp<0x4E>(x));                // quad_perm [2,3,0,1]
    x = op(x, contrib_dpp<0xB1>(x));                // quad_perm [1,0,3,2]
    return x;
}

__global__ void __launch_bounds__(256)
blend_contrib_kernel(int W, int H, int grid_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                     const float4* __restrict__ splat, float* __restrict__ weight_sum, float* __restrict__ weight_max,
                     int32_t* __restrict__ pixel_count, int views, int interleaved) {
    __shared__ FeatSplat stage[BATCH + 1];                               // + the null record that pads a survivor list
    __shared__ __attribute__((aligned(16))) uint32_t surv[4][BATCH + CONTRIB_GROUP];
    // the batch's table: per entry one column per wave (.x … .w = waves 0 … 3); row BATCH takes the null record's zeros
    __shared__ float4 part_sum[BATCH + 1], part_max[BATCH + 1], part_cnt[BATCH + 1];
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
    float amax = GGR_ALPHA_MAX;
    __asm__ volatile("" : "+s"(amax));
    if (tid == 0) {   // the null record: opacity 0 → α = 0 → never live
        stage[BATCH].a = make_float4(0.f, 0.f, 0.f, 0.f);
        stage[BATCH].b = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane == 0) wave_done[wave] = quad_live ? 0 : 1;
    bool wdone = !quad_live;
    float* const my_sum = reinterpret_cast<float*>(part_sum) + wave;   // this wave's column: entry e at [4·e]
    float* const my_max = reinterpret_cast<float*>(part_max) + wave;
    float* const my_cnt = reinterpret_cast<float*>(part_cnt) + wave;
    const int my_slot = lane >> 3;   // the entry of a group whose results this lane ends up with

    uint32_t g_next = tid < total ? point_list[range.x + tid] : 0u;
    for (int b0 = 0; b0 < total; b0 += BATCH) {
        // (the barrier that ended the previous batch: its records and its table are consumed, by this very thread where it matters)
        const int nb = min(BATCH, total - b0);
        const uint32_t g = g_next;
        if (b0 + BATCH + tid < total) g_next = point_list[range.x + b0 + BATCH + tid];
        if (tid < nb) {
            stage[tid] = stage_feat_splat(splat, g);
            part_cnt[tid] = make_float4(0.f, 0.f, 0.f, 0.f);   // (sum and max are read only where the count is not zero)
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
            if (lane < CONTRIB_GROUP) my_surv[ns + lane] = (uint32_t)BATCH;   // pad the last group with the null record
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k0 = 0; k0 < ns; k0 += CONTRIB_GROUP) {
                uint32_t pkw[CONTRIB_GROUP];
                __builtin_memcpy(pkw, my_surv + k0, sizeof pkw);
                const uint32_t my_e = my_surv[k0 + my_slot];
                float vs[CONTRIB_GROUP], vm[CONTRIB_GROUP], vc[CONTRIB_GROUP];
#pragma unroll
                for (int u = 0; u < CONTRIB_GROUP; u++) {
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
                    vs[u] = w; vm[u] = w; vc[u] = take ? 1.f : 0.f;
                    T -= w;
                }
                const float s = reduce8(vs, lane, SumOp()), m = reduce8(vm, lane, MaxOp());
                const float c = reduce8(vc, lane, SumOp());   // (exact: at most 64)
                if ((lane & 7) == 0 && c != 0.f) { my_sum[4 * my_e] = s; my_max[4 * my_e] = m; my_cnt[4 * my_e] = c; }
                if (!__any(live)) { wdone = true; break; }
            }
            if (wdone && lane == 0) wave_done[wave] = 1;
        }
        __syncthreads();   // the table is complete, the records are consumed, wave_done is visible
        if (tid < nb) {
            const float4 c4 = part_cnt[tid];
            const float c = (c4.x + c4.y) + (c4.z + c4.w);
            if (c != 0.f) {
                const float4 s4 = part_sum[tid], m4 = part_max[tid];
                // a wave that did not take the entry left its column of sum / max unwritten: masked by its zero count
                const float s = ((c4.x != 0.f ? s4.x : 0.f) + (c4.y != 0.f ? s4.y : 0.f)) +
                                ((c4.z != 0.f ? s4.z : 0.f) + (c4.w != 0.f ? s4.w : 0.f));
                const float m = fmaxf(fmaxf(c4.x != 0.f ? m4.x : 0.f, c4.y != 0.f ? m4.y : 0.f),
                                      fmaxf(c4.z != 0.f ? m4.z : 0.f, c4.w != 0.f ? m4.w : 0.f));
                const uint32_t gid = __float_as_uint(stage[tid].b.w);
                if (weight_sum) atomicAdd(weight_sum + gid, s);
                if (weight_max) atomicMax(reinterpret_cast<unsigned int*>(weight_max) + gid, __float_as_uint(m));
                if (pixel_count) atomicAdd(pixel_count + gid, (int)c);
            }
        }
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;   // every pixel of the tile has stopped
    }
}

void launch_blend_contrib(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat,
                          float* weight_sum, float* weight_max, int32_t* pixel_count, int views, int scissored, hipStream_t s) {
    const int gx = (W + GGR_TILE - 1) / GGR_TILE, gy = (H + GGR_TILE - 1) / GGR_TILE;
    const int nt = gx * gy * views;
    if (nt == 0) return;
    hipLaunchKernelGGL(blend_contrib_kernel, dim3(xcd_grid(nt)), dim3(256), 0, s, W, H, gx, ranges, point_list, splat,
                       weight_sum, weight_max, pixel_count, views, xcd_forward_interleaved(nt, scissored != 0) ? 1 : 0);
}

}  // namespace ggr

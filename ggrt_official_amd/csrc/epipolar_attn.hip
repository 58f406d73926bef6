// epipolar_attn.hip — the core of GGRt's epipolar cross-attention for one query token per ray, on the raw samples.
//
// Per ray n the contract is GgrEpipolarAttnPass in include/ggr_raster.h:
//   forward:   logit[h,s] = Σ_c qk[h,c]·z[s,c];   attn[h,·] = softmax_s(logit[h,·]) (row maximum subtracted);
//              ctx[h,c] = Σ_s attn[h,s]·z[s,c]
//   backward:  da[h,s] = Σ_c g_ctx[h,c]·z[s,c];   dl[h,s] = attn[h,s]·(da[h,s] − Σ_s' attn[h,s']·da[h,s']);
//              g_qk[h,c] = Σ_s dl[h,s]·z[s,c];    g_z[s,c] = Σ_h (attn[h,s]·g_ctx[h,c] + dl[h,s]·qk[h,c])
// qk is the query with the key projection folded in (scale · Wk_hᵀ q_h) and ctx goes through the value projection afterwards:
// both are [N, ·]-sized GEMMs of the caller's.  What is left is memory-bound (about 4 flop per byte of z) and has no dense
// contraction: VALU work.
//
// Launch shape.  A WAVE owns a ray and a workgroup is one wave: the waves share nothing, and LDS, not the wave slots, sets the
// occupancy, so the smallest workgroup packs a CU best (at S = 32, C = 128 the tile is 16 896 B: ⌊160 KiB / 16 896⌋ = 9 waves per
// CU; four-wave workgroups would get 8).  The ray's [S, C] tile (contiguous in z) is loaded ONCE, with 16-byte loads where C and
// the pointer allow, into LDS at a pitch of an ODD number of 16-byte slots.  Two phases read it:
//   by rows      lane s walks sample s across the channels with ds_read_b128: with the odd slot pitch the 16 lanes that one LDS
//                cycle serves start in 16 different slots — no conflict; qk (or g_ctx) is the same address in every lane, so it
//                comes through the scalar cache; H ≤ 8 accumulators per lane
//   by columns   lane c walks channel c (and c + 64, …) down the samples with ds_read_b32: a row's channels are consecutive
//                banks — no conflict; attn[h,s] and dl[h,s] live in lane s and are broadcast with v_readlane
// The softmax's maximum and sums are xor-shuffles over the wave.  Every output element is written once by the wave that owns
// its ray, in a fixed order of summation: no atomics, and two runs give the same bits.  Element offsets are 64-bit.
#include "epipolar_attn.h"
#include <cmath>

namespace ggr {

namespace {

constexpr int WAVE = 64;
constexpr int HMAX = kEpiAttnMaxHeads;

__host__ __device__ __forceinline__ int tile_pitch(int C) { return 4 * (((C + 3) >> 2) | 1); }   // floats; an odd number of float4

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// lane `from`'s value in every lane (`from` is wave-uniform)
__device__ __forceinline__ float from_lane(float v, int from) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), from)); }

// z's [S, C] rows → tile rows of pitch P; the columns C .. 4·⌈C/4⌉ − 1 that the row phase's last float4 covers are zeroed
__device__ __forceinline__ void load_tile(float* tile, const float* zr, int S, int C, int P, int lane, bool vec) {
    if (vec) {
        const int c4 = C >> 2, total = S * c4;
        const float4* src = reinterpret_cast<const float4*>(zr);
#pragma unroll 4
        for (int k = lane; k < total; k += WAVE) {
            const int row = k / c4, col = k - row * c4;
            *reinterpret_cast<float4*>(tile + row * P + 4 * col) = src[k];
        }
    } else {
        const int cr = (C + 3) & ~3, total = S * cr;
#pragma unroll 4
        for (int k = lane; k < total; k += WAVE) {
            const int row = k / cr, col = k - row * cr;
            tile[row * P + col] = col < C ? zr[row * C + col] : 0.f;
        }
    }
}

// acc[h] = Σ_c w[h,c]·row[c] for h < H: the tile row of this lane against H wave-uniform vectors of length C (global memory)
__device__ __forceinline__ void row_dots(const float* row, const float* __restrict__ w, int C, int H, float (&acc)[HMAX]) {
    const float4* r4 = reinterpret_cast<const float4*>(row);
    const int full = C >> 2;
    for (int j = 0; j < full; ++j) {
        const float4 zv = r4[j];
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < H) {
                const float* q = w + h * C + 4 * j;
                acc[h] = fmaf(zv.x, q[0], acc[h]);
                acc[h] = fmaf(zv.y, q[1], acc[h]);
                acc[h] = fmaf(zv.z, q[2], acc[h]);
                acc[h] = fmaf(zv.w, q[3], acc[h]);
            }
    }
    if (C & 3) {   // the last, partial float4: the tile's pad columns are zero, w is not read past C
        const float4 zv = r4[full];
        const int rest = C & 3;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < H) {
                const float* q = w + h * C + 4 * full;
                acc[h] = fmaf(zv.x, q[0], acc[h]);
                if (rest > 1) acc[h] = fmaf(zv.y, q[1], acc[h]);
                if (rest > 2) acc[h] = fmaf(zv.z, q[2], acc[h]);
            }
    }
}

__global__ void __launch_bounds__(WAVE)
epipolar_attn_fwd_kernel(const EpiAttnArgs a, const int vec) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int lane = threadIdx.x, S = a.S, C = a.C, H = a.H, P = tile_pitch(C);
    const size_t n = blockIdx.x;
    load_tile(tile, a.z + n * S * C, S, C, P, lane, vec != 0);
    __syncthreads();

    // ---- by rows: lane s holds logit[·, s], then attn[·, s]
    const float* qk = a.qk + n * H * C;
    float att[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h) att[h] = 0.f;
    if (lane < S) row_dots(tile + lane * P, qk, C, H, att);
#pragma unroll
    for (int h = 0; h < HMAX; ++h)
        if (h < H) {
            const float logit = lane < S ? att[h] : -INFINITY;
            const float m = wave_max(logit);
            const float e = lane < S ? expf(logit - m) : 0.f;
            const float sum = wave_sum(e);
            att[h] = e / sum;
            if (lane < S) a.attn_out[(n * H + h) * S + lane] = att[h];
        }

    // ---- by columns: lane c holds ctx[·, c]
    for (int c = lane; c < C; c += WAVE) {
        float out[HMAX];
#pragma unroll
        for (int h = 0; h < HMAX; ++h) out[h] = 0.f;
        for (int s = 0; s < S; ++s) {
            const float zv = tile[s * P + c];
#pragma unroll
            for (int h = 0; h < HMAX; ++h)
                if (h < H) out[h] = fmaf(from_lane(att[h], s), zv, out[h]);
        }
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < H) a.ctx[(n * H + h) * C + c] = out[h];
    }
}

__global__ void __launch_bounds__(WAVE)
epipolar_attn_bwd_kernel(const EpiAttnArgs a, const int vec) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int lane = threadIdx.x, S = a.S, C = a.C, H = a.H, P = tile_pitch(C);
    const size_t n = blockIdx.x;
    load_tile(tile, a.z + n * S * C, S, C, P, lane, vec != 0);
    __syncthreads();

    // ---- by rows: lane s holds attn[·, s] and dl[·, s]
    const float* qk = a.qk + n * H * C;
    const float* g_ctx = a.g_ctx + n * H * C;
    float att[HMAX], dl[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h) att[h] = dl[h] = 0.f;
    if (lane < S) row_dots(tile + lane * P, g_ctx, C, H, dl);
#pragma unroll
    for (int h = 0; h < HMAX; ++h)
        if (h < H) {
            att[h] = lane < S ? a.attn[(n * H + h) * S + lane] : 0.f;
            const float dot = wave_sum(att[h] * dl[h]);
            dl[h] = att[h] * (dl[h] - dot);
        }

    // ---- by columns: lane c holds g_qk[·, c] and writes g_z[·, c] row by row
    for (int c = lane; c < C; c += WAVE) {
        float qv[HMAX], gv[HMAX], gq[HMAX];
#pragma unroll
        for (int h = 0; h < HMAX; ++h) {
            qv[h] = h < H ? qk[h * C + c] : 0.f;
            gv[h] = h < H ? g_ctx[h * C + c] : 0.f;
            gq[h] = 0.f;
        }
        float* gz = a.g_z + n * S * C + c;
        for (int s = 0; s < S; ++s) {
            const float zv = tile[s * P + c];
            float acc = 0.f;
#pragma unroll
            for (int h = 0; h < HMAX; ++h)
                if (h < H) {
                    const float d = from_lane(dl[h], s);
                    acc = fmaf(from_lane(att[h], s), gv[h], acc);
                    acc = fmaf(d, qv[h], acc);
                    gq[h] = fmaf(d, zv, gq[h]);
                }
            gz[(size_t)s * C] = acc;
        }
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < H) a.g_qk[(n * H + h) * C + c] = gq[h];
    }
}

// dynamic LDS above 64 KiB has to be asked for, once per kernel and device context
template <typename K>
hipError_t allow_lds(K kernel, int bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kEpiAttnLdsLimit);
}

bool vector_loads(const EpiAttnArgs& a) { return (a.C & 3) == 0 && (reinterpret_cast<uintptr_t>(a.z) & 15u) == 0; }

}  // namespace

int epipolar_attn_lds_bytes(int S, int C) { return S * tile_pitch(C) * (int)sizeof(float); }

hipError_t launch_epipolar_attn_forward(const EpiAttnArgs& a, hipStream_t s) {
    if (a.N <= 0) return hipSuccess;
    const int lds = epipolar_attn_lds_bytes(a.S, a.C);
    const hipError_t e = allow_lds(epipolar_attn_fwd_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(epipolar_attn_fwd_kernel, dim3((unsigned)a.N), dim3(WAVE), (size_t)lds, s, a, vector_loads(a) ? 1 : 0);
    return hipSuccess;
}

hipError_t launch_epipolar_attn_backward(const EpiAttnArgs& a, hipStream_t s) {
    if (a.N <= 0) return hipSuccess;
    const int lds = epipolar_attn_lds_bytes(a.S, a.C);
    const hipError_t e = allow_lds(epipolar_attn_bwd_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(epipolar_attn_bwd_kernel, dim3((unsigned)a.N), dim3(WAVE), (size_t)lds, s, a, vector_loads(a) ? 1 : 0);
    return hipSuccess;
}

}  // namespace ggr

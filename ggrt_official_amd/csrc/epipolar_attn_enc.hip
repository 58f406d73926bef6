// epipolar_attn_enc.hip — the core of GGRt's epipolar cross-attention on z_s = f_s + W·pe(d_s) + b, without z.
//
// Per ray n the contract is GgrEpipolarAttnEncPass in include/ggr_raster.h.  With E = 2·O and
//   pe[2k+p](d) = sin(F·2^k·d + p·P),   F = float32(2π), P = float32(π/2) taken as real numbers,
//   forward:   logit[h,s] = Σ_c qk[h,c]·f[s,c] + Σ_j qe[h,j]·pe_j(d_s);   attn[h,·] = softmax_s(logit[h,·]);
//              ctx_f[h,c] = Σ_s attn[h,s]·f[s,c];   ctx_e[h,j] = Σ_s attn[h,s]·pe_j(d_s)
//   backward:  da[h,s] = Σ_c g_f_ctx[h,c]·f[s,c] + Σ_j g_e_ctx[h,j]·pe_j(d_s);   dl[h,s] = attn[h,s]·(da[h,s] − Σ_s' attn[h,s']·da[h,s']);
//              g_qk[h,c] = Σ_s dl[h,s]·f[s,c];   g_qe[h,j] = Σ_s dl[h,s]·pe_j(d_s);
//              g_f[s,c] = Σ_h (attn[h,s]·g_f_ctx[h,c] + dl[h,s]·qk[h,c]);
//              g_d[s] = Σ_k Σ_p (Σ_h attn[h,s]·g_e_ctx[h,2k+p] + dl[h,s]·qe[h,2k+p])·F·2^k·cos(F·2^k·d_s + p·P)
// qe = qk·W and the value side's W·ctx_e + b are the caller's, over N·H rows instead of N·S samples.
//
// Layout: the encoding as EXTRA TILE COLUMNS.  The launch shape, the tile and both phases are those of epipolar_attn.hip (one wave
// per ray and per workgroup; the [S, C] tile loaded once into LDS at an odd pitch of 16-byte slots; lane s owns sample s by rows,
// lanes go across channels by columns; xor-shuffles for the softmax; every output element written once in a fixed order).  The
// ray's row s is [ f_s : 4·⌈C/4⌉ floats | pe(d_s) : 4·⌈E/4⌉ floats ], the pads zero, and both phases walk the C + E columns
// against [qk | qe] and [g_f_ctx | g_e_ctx].  The alternative — the sines in lane s's registers, ctx_e and g_qe as H·E wave
// reductions — keeps the LDS footprint (9 waves per CU at S = 32, C = 128 instead of 8 here) but pays 6 shuffle steps for each of
// 80 sums where the column phase pays one more trip of S steps.
//
// The sines.  m = 2^k·d is exact, r = rint(m) and u = m − r in [−½, ½] are exact, and F·m = F·u + 2π·r + (F − 2π)·r, so
//   θ = F·u + (F − 2π)·r    (one fused multiply-add; |θ| <= π + 1.75e-7·|r|: below 3.15 for d in [0, 1] — half an ulp is 1.2e-7)
// has the sine and cosine of F·2^k·d, and  sin(θ + P) = cos(θ + (P − π/2)) = cos θ − (P − π/2)·sin θ  to 1e-15.  One sincosf
// per (sample, octave); the S·O of them are spread over all 64 lanes (S <= 32 leaves half the wave idle otherwise).
// The helpers of epipolar_attn.hip are repeated here and not shared: that file's kernels keep their bits.
#include "epipolar_attn_enc.h"
#include <cmath>

namespace ggr {

namespace {

constexpr int WAVE = 64;
constexpr int HMAX = kEpiAttnMaxHeads;
constexpr float kF = 6.2831854820251465f;          // float32(2π), bits 0x40C90FDB
constexpr float kFminus2Pi = 1.7484556000744883e-7f;   // float32(2π) − 2π
constexpr float kPminusHalfPi = 4.371139000186241e-8f; // float32(π/2) − π/2   (float32(π/2): bits 0x3FC90FDB)

__host__ __device__ __forceinline__ int enc_offset(int C) { return (C + 3) & ~3; }                 // floats: where the encoding starts in a row
__host__ __device__ __forceinline__ int tile_pitch(int C, int E) { return 4 * (((enc_offset(C) + ((E + 3) & ~3)) >> 2) | 1); }   // floats; an odd number of float4

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

// f's [S, C] rows → tile rows of pitch P; the columns C .. 4·⌈C/4⌉ − 1 that the row phase's last float4 covers are zeroed
__device__ __forceinline__ void load_tile(float* tile, const float* fr, int S, int C, int P, int lane, bool vec) {
    if (vec) {
        const int c4 = C >> 2, total = S * c4;
        const float4* src = reinterpret_cast<const float4*>(fr);
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
            tile[row * P + col] = col < C ? fr[row * C + col] : 0.f;
        }
    }
}

// pe(d_s) → columns CP .. CP + E − 1 of tile row s, zeros up to the next multiple of 4.  With SC the power of two at or above S,
// lane = g·SC + s: the 64 / SC groups g share a sample's octaves among them.
__device__ __forceinline__ void encode_tile(float* tile, const float* dr, int S, int O, int P, int CP, int lane) {
    const int sh = S > 1 ? 32 - __clz(S - 1) : 0;
    const int s = lane & ((1 << sh) - 1), group = lane >> sh, groups = WAVE >> sh;
    if (s >= S) return;
    float* row = tile + s * P + CP;
    const float d = dr[s];
    for (int k = group; k < O; k += groups) {
        const float m = ldexpf(d, k);
        const float r = rintf(m);
        const float theta = fmaf(kF, m - r, kFminus2Pi * r);
        float sn, cs;
        sincosf(theta, &sn, &cs);
        *reinterpret_cast<float2*>(row + 2 * k) = make_float2(sn, fmaf(-kPminusHalfPi, sn, cs));
    }
    if ((O & 1) && group == 0) *reinterpret_cast<float2*>(row + 2 * O) = make_float2(0.f, 0.f);
}

// acc[h] += Σ_c w[h,c]·row[c] for h < H: the tile row of this lane against H wave-uniform vectors of length C (global memory)
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
epipolar_attn_enc_fwd_kernel(const EpiAttnEncArgs a, const int vec) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int lane = threadIdx.x, S = a.S, C = a.C, H = a.H, E = 2 * a.O, CP = enc_offset(C), P = tile_pitch(C, E);
    const size_t n = blockIdx.x;
    load_tile(tile, a.f + n * S * C, S, C, P, lane, vec != 0);
    encode_tile(tile, a.d + n * S, S, a.O, P, CP, lane);
    __syncthreads();

    // ---- by rows: lane s holds logit[·, s], then attn[·, s]
    const float* qk = a.qk + n * H * C;
    const float* qe = a.qe + n * H * E;
    float att[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h) att[h] = 0.f;
    if (lane < S) {
        row_dots(tile + lane * P, qk, C, H, att);
        row_dots(tile + lane * P + CP, qe, E, H, att);
    }
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

    // ---- by columns: lane v holds ctx_f[·, v], or ctx_e[·, v − C] past the channels
    for (int v = lane; v < C + E; v += WAVE) {
        const bool enc = v >= C;
        const int col = enc ? CP + (v - C) : v;
        float out[HMAX];
#pragma unroll
        for (int h = 0; h < HMAX; ++h) out[h] = 0.f;
        for (int s = 0; s < S; ++s) {
            const float zv = tile[s * P + col];
#pragma unroll
            for (int h = 0; h < HMAX; ++h)
                if (h < H) out[h] = fmaf(from_lane(att[h], s), zv, out[h]);
        }
        float* dst = enc ? a.ctx_e + n * H * E + (v - C) : a.ctx_f + n * H * C + v;
        const int stride = enc ? E : C;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < H) dst[h * stride] = out[h];
    }
}

__global__ void __launch_bounds__(WAVE)
epipolar_attn_enc_bwd_kernel(const EpiAttnEncArgs a, const int vec) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int lane = threadIdx.x, S = a.S, C = a.C, H = a.H, O = a.O, E = 2 * O, CP = enc_offset(C), P = tile_pitch(C, E);
    const size_t n = blockIdx.x;
    load_tile(tile, a.f + n * S * C, S, C, P, lane, vec != 0);
    encode_tile(tile, a.d + n * S, S, O, P, CP, lane);
    __syncthreads();

    // ---- by rows: lane s holds attn[·, s] and dl[·, s]
    const float* qk = a.qk + n * H * C;
    const float* qe = a.qe + n * H * E;
    const float* g_f_ctx = a.g_f_ctx + n * H * C;
    const float* g_e_ctx = a.g_e_ctx + n * H * E;
    float att[HMAX], dl[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h) att[h] = dl[h] = 0.f;
    if (lane < S) {
        row_dots(tile + lane * P, g_f_ctx, C, H, dl);
        row_dots(tile + lane * P + CP, g_e_ctx, E, H, dl);
    }
#pragma unroll
    for (int h = 0; h < HMAX; ++h)
        if (h < H) {
            att[h] = lane < S ? a.attn[(n * H + h) * S + lane] : 0.f;
            const float dot = wave_sum(att[h] * dl[h]);
            dl[h] = att[h] * (dl[h] - dot);
        }

    // ---- still by rows: g_d[s], from lane s's own sines.  cos θ = pe[2k+1] + (P − π/2)·pe[2k] and cos(θ + P) = −(pe[2k] + (P − π/2)·pe[2k+1])
    if (a.g_d != nullptr && lane < S) {
        const float* pe = tile + lane * P + CP;
        float gd = 0.f;
        for (int k = 0; k < O; ++k) {
            const float2 sc = *reinterpret_cast<const float2*>(pe + 2 * k);
            float w0 = 0.f, w1 = 0.f;
#pragma unroll
            for (int h = 0; h < HMAX; ++h)
                if (h < H) {
                    w0 = fmaf(att[h], g_e_ctx[h * E + 2 * k], w0);
                    w0 = fmaf(dl[h], qe[h * E + 2 * k], w0);
                    w1 = fmaf(att[h], g_e_ctx[h * E + 2 * k + 1], w1);
                    w1 = fmaf(dl[h], qe[h * E + 2 * k + 1], w1);
                }
            const float c0 = fmaf(kPminusHalfPi, sc.x, sc.y), c1 = -fmaf(kPminusHalfPi, sc.y, sc.x);
            gd = fmaf(ldexpf(kF, k), fmaf(w0, c0, w1 * c1), gd);
        }
        a.g_d[n * S + lane] = gd;
    }

    // ---- by columns: lane v holds g_qk[·, v] and writes g_f[·, v] row by row, or holds g_qe[·, v − C] past the channels
    for (int v = lane; v < C + E; v += WAVE) {
        const bool enc = v >= C;
        const int col = enc ? CP + (v - C) : v;
        float qv[HMAX], gv[HMAX], gq[HMAX];
#pragma unroll
        for (int h = 0; h < HMAX; ++h) {
            qv[h] = h < H && !enc ? qk[h * C + v] : 0.f;
            gv[h] = h < H && !enc ? g_f_ctx[h * C + v] : 0.f;
            gq[h] = 0.f;
        }
        float* gf = a.g_f + n * S * C + (enc ? 0 : v);
        for (int s = 0; s < S; ++s) {
            const float zv = tile[s * P + col];
            float acc = 0.f;
#pragma unroll
            for (int h = 0; h < HMAX; ++h)
                if (h < H) {
                    const float d = from_lane(dl[h], s);
                    acc = fmaf(from_lane(att[h], s), gv[h], acc);
                    acc = fmaf(d, qv[h], acc);
                    gq[h] = fmaf(d, zv, gq[h]);
                }
            if (!enc) gf[(size_t)s * C] = acc;
        }
        float* dst = enc ? a.g_qe + n * H * E + (v - C) : a.g_qk + n * H * C + v;
        const int stride = enc ? E : C;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < H) dst[h * stride] = gq[h];
    }
}

// dynamic LDS above 64 KiB has to be asked for, once per kernel and device context
template <typename K>
hipError_t allow_lds(K kernel, int bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kEpiAttnLdsLimit);
}

bool vector_loads(const EpiAttnEncArgs& a) { return (a.C & 3) == 0 && (reinterpret_cast<uintptr_t>(a.f) & 15u) == 0; }

}  // namespace

int epipolar_attn_enc_lds_bytes(int S, int C, int O) { return S * tile_pitch(C, 2 * O) * (int)sizeof(float); }

hipError_t launch_epipolar_attn_enc_forward(const EpiAttnEncArgs& a, hipStream_t s) {
    if (a.N <= 0) return hipSuccess;
    const int lds = epipolar_attn_enc_lds_bytes(a.S, a.C, a.O);
    const hipError_t e = allow_lds(epipolar_attn_enc_fwd_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(epipolar_attn_enc_fwd_kernel, dim3((unsigned)a.N), dim3(WAVE), (size_t)lds, s, a, vector_loads(a) ? 1 : 0);
    return hipSuccess;
}

hipError_t launch_epipolar_attn_enc_backward(const EpiAttnEncArgs& a, hipStream_t s) {
    if (a.N <= 0) return hipSuccess;
    const int lds = epipolar_attn_enc_lds_bytes(a.S, a.C, a.O);
    const hipError_t e = allow_lds(epipolar_attn_enc_bwd_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(epipolar_attn_enc_bwd_kernel, dim3((unsigned)a.N), dim3(WAVE), (size_t)lds, s, a, vector_loads(a) ? 1 : 0);
    return hipSuccess;
}

}  // namespace ggr

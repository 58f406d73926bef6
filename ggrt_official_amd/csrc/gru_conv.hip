// gru_conv.hip — the convolutions of one ConvGRU half-step (GGRt's SepConvGRU / ConvGRU, ggrt/optimizer.py:33-78) as an implicit
// GEMM on v_mfma_f32_32x32x2_f32, with the gate math of gru_gates.hip evaluated on the accumulators.  Inference only.
//
//     acc[n, co, y, x] = bias[co] + sum_{ci < Ch, t} w_h[co, ci, t] a[n, ci, (y, x) + t - pad]
//                                 + sum_{ci < Cx, t} w_x[co, ci, t] x[n, ci, (y, x) + t - pad]          (cross-correlation, zero padding)
//     GATE   co < Ch: z = sigmoid(acc)       co >= Ch: rh = sigmoid(acc) h            (a = h, 2 Ch columns)
//     BLEND  out_h = (1 - z) h + z tanh(acc)                                         (a = rh, Ch columns)
//     RAW    raw = acc
//
// The GEMM: rows are output channels (the MFMA's A operand: the weights, whose K index (ci, t) is contiguous per channel in torch's
// [Cout,Cin,kh,kw]), columns are pixels p = (n H + y) W + x over the whole batch (the B operand: activations gathered per tap), so
// that a lane of the result owns ONE pixel and 16 channels, and each store of a wave covers 32 consecutive pixels of a channel.
// A workgroup owns 64 channels x BP pixels (BP = 64: four waves as 2 x 2; BP = 32: two waves), a wave a 32 x 32 tile.  K is walked
// in stages of 32, first the a side (K = Ch taps), then the x side (K = Cx taps); the tail of either is zero-filled.  A stage:
//     global -> registers (the NEXT stage's 8 activations and 8 or 16 weights per thread, issued before this stage's MFMAs),
//     registers -> LDS as Ws[k][channel], Bs[k][pixel] (rows of 65 floats: both the writes and the reads are conflict-free),
//     16 MFMAs per wave, each fed by two 4-byte LDS reads (A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]).
// The gather is where an implicit GEMM goes wrong: a pixel is decoded ONCE into (n, y, x), and a tap is taken only if
// 0 <= y + ty - pad_y < H and 0 <= x + tx - pad_x < W, so it can reach neither the neighbouring row nor the neighbouring sample,
// wherever the tile's 64 pixels start.
// Four accumulators per wave — (a side, x side) x (even, odd k-pair of a stage) — each a k-ordered fmaf chain of a quarter of the
// terms; they are added as (a_even + a_odd) + (x_even + x_odd) + bias.  Nothing is split across workgroups, there are no atomics
// and no workspace: the same bits on every run.  One launch per call.
#include "gru_conv.h"
#include "gru_math.h"

namespace ggr {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BCO = kGruConvTileCo, BK = kGruConvTileK, LDW = 65;

struct Pixel {
    int valid, n, y, x;
};

// one side of the sum: `src` [N,C,H,W] against `w` [Cout,C,kh,kw], into acc0 (even k-pairs of every stage) and acc1 (odd)
template <int KH, int KW, int BP>
__device__ __forceinline__ void conv_side(const GruConvArgs& g, const float* __restrict__ src, const float* __restrict__ w, const int C, const Pixel px,
                                          const int co0, float* Ws, float* Bs, const int wco, const int wpx, f32x16& acc0, f32x16& acc1) {
    constexpr int NT = 4 * BP, KSTEP = NT / BP, WROWS = NT / 32, NW = BCO / WROWS, NA = BK / KSTEP;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int kh = KH ? KH : g.KH, kw = KW ? KW : g.KW, taps = kh * kw, ph = (kh - 1) / 2, pw = (kw - 1) / 2;
    const int H = g.H, W = g.W, HW = H * W, K = C * taps;
    const float* srcn = src + (size_t)px.n * C * HW;
    const int pl = tid % BP, kl0 = tid / BP;            // this thread's pixel of the tile and its first k of a stage
    const int wk = tid & 31, wr0 = tid >> 5;            // this thread's k of a stage and its first channel of the tile
    float ra[NA], rw[NW];

    auto load = [&](const int k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int k = k0 + kl0 + KSTEP * i, ci = k / taps, t = k - ci * taps, ty = t / kw, tx = t - ty * kw;
            const int yy = px.y + ty - ph, xx = px.x + tx - pw;
            const bool ok = px.valid && k < K && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            ra[i] = ok ? srcn[(size_t)ci * HW + yy * W + xx] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int co = co0 + wr0 + WROWS * i, k = k0 + wk;
            rw[i] = (co < g.Cout && k < K) ? w[(size_t)co * K + k] : 0.f;
        }
    };

    load(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        __syncthreads();                                // the previous stage's reads are done
#pragma unroll
        for (int i = 0; i < NA; ++i) Bs[(kl0 + KSTEP * i) * LDW + pl] = ra[i];
#pragma unroll
        for (int i = 0; i < NW; ++i) Ws[wk * LDW + wr0 + WROWS * i] = rw[i];
        __syncthreads();
        if (k0 + BK < K) load(k0 + BK);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            const int kk = 2 * ks + (lane >> 5);
            const float av = Ws[kk * LDW + wco + (lane & 31)], bv = Bs[kk * LDW + wpx + (lane & 31)];
            if (ks & 1) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc0, 0, 0, 0);
        }
    }
}

template <int KH, int KW, int EPI, int BP> __global__ __launch_bounds__(4 * BP) void gru_conv_kernel(const GruConvArgs g) {
    __shared__ float Ws[BK * LDW], Bs[BK * LDW];
    constexpr int NWP = BP / 32;                        // waves along the pixels
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = g.H * g.W, P = g.N * HW;
    const int co0 = (int)blockIdx.y * BCO, p0 = (int)blockIdx.x * BP;
    const int wco = (wave / NWP) * 32, wpx = (wave % NWP) * 32;

    Pixel px;                                           // the pixel this thread gathers
    const int gp = p0 + tid % BP;
    px.valid = gp < P;
    px.n = px.valid ? gp / HW : 0;
    const int sp = px.valid ? gp - px.n * HW : 0;
    px.y = sp / g.W;
    px.x = sp - px.y * g.W;

    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    conv_side<KH, KW, BP>(g, g.a, g.w_h, g.Ch, px, co0, Ws, Bs, wco, wpx, acc[0], acc[1]);
    conv_side<KH, KW, BP>(g, g.x, g.w_x, g.Cx, px, co0, Ws, Bs, wco, wpx, acc[2], acc[3]);

    // C/D of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int op = p0 + wpx + (lane & 31);
    if (op >= P) return;
    const int n = op / HW, s = op - n * HW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + wco + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (co >= g.Cout) continue;
        float v = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
        if (g.bias) v += g.bias[co];
        if constexpr (EPI == kGruConvRaw) {
            g.raw[((size_t)n * g.Cout + co) * HW + s] = v;
        } else if constexpr (EPI == kGruConvGate) {
            const float sg = gru_sigmoid(v);
            if (co < g.Ch) {
                g.z[((size_t)n * g.Ch + co) * HW + s] = sg;
            } else {
                const size_t e = ((size_t)n * g.Ch + (co - g.Ch)) * HW + s;
                g.rh[e] = sg * g.h[e];
            }
        } else {
            const size_t e = ((size_t)n * g.Ch + co) * HW + s;
            const float q = gru_tanh(v), z = g.z[e], h = g.h[e];
            g.out_h[e] = (1.f - z) * h + z * q;
        }
    }
}

template <int KH, int KW, int BP> void launch_shape(const GruConvArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(4 * BP);
    switch (a.epilogue) {
    case kGruConvGate: hipLaunchKernelGGL((gru_conv_kernel<KH, KW, kGruConvGate, BP>), grid, block, 0, s, a); break;
    case kGruConvBlend: hipLaunchKernelGGL((gru_conv_kernel<KH, KW, kGruConvBlend, BP>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((gru_conv_kernel<KH, KW, kGruConvRaw, BP>), grid, block, 0, s, a); break;
    }
}

template <int BP> void launch_tile(const GruConvArgs& a, hipStream_t s) {
    const int64_t P = (int64_t)a.N * a.H * a.W;
    const dim3 grid((unsigned)((P + BP - 1) / BP), (unsigned)((a.Cout + BCO - 1) / BCO));
    // the three kernel shapes of GGRt's GRUs have their tap arithmetic compiled in; any other odd sides take the general form
    if (a.KH == 1 && a.KW == 5) launch_shape<1, 5, BP>(a, grid, s);
    else if (a.KH == 5 && a.KW == 1) launch_shape<5, 1, BP>(a, grid, s);
    else if (a.KH == 3 && a.KW == 3) launch_shape<3, 3, BP>(a, grid, s);
    else launch_shape<0, 0, BP>(a, grid, s);
}

}  // namespace

int gru_conv_tile_pixels(const GruConvArgs& a) {
    // 256 compute units: with fewer workgroups than that at 64 pixels each, halve the tile (N = 1 of GGRt's 48 x 63 map: 48 x 2
    // workgroups for the blend's 128 channels)
    const int64_t P = (int64_t)a.N * a.H * a.W, blocks = ((P + 63) / 64) * ((a.Cout + BCO - 1) / BCO);
    return blocks < 256 ? 32 : 64;
}

void launch_gru_conv(const GruConvArgs& a, hipStream_t s) {
    if (gru_conv_tile_pixels(a) == 32) launch_tile<32>(a, s);
    else launch_tile<64>(a, s);
}

}  // namespace ggr

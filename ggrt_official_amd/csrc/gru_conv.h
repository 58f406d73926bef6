// gru_conv.h — launcher of the ConvGRU half-step's convolutions as an implicit GEMM on the f32-input MFMA (gru_conv.hip): the
// convolution of two separate inputs (the hidden state's side and the features' side) with the GRU's gate or blend evaluated in the
// accumulator registers.  Forward only; float32 dense NCHW activations and [Cout,Cin,kh,kw] weights, read in place.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kGruConvMaxSide = 5;      // kernel sides are odd and at most this
constexpr int kGruConvTileCo = 64;      // output channels per workgroup
constexpr int kGruConvTileK = 32;       // K = (input channel, tap) indices per LDS stage

enum { kGruConvGate = 0, kGruConvBlend = 1, kGruConvRaw = 2 };

// acc[n, co, y, x] = bias[co] + sum_{ci < Ch, t} w_h[co, ci, t] a[n, ci, (y, x) + t - pad] + sum_{ci < Cx, t} w_x[co, ci, t] x[...]
// with Cout = 2 Ch (GATE), Ch (BLEND) or `Cout` (RAW).  A pointer that an epilogue does not use is NULL.
struct GruConvArgs {
    int N, Ch, Cx, H, W, KH, KW, Cout, epilogue;
    const float *a, *x;                 // [N,Ch,H,W], [N,Cx,H,W]
    const float *w_h, *w_x;             // [Cout,Ch,KH,KW], [Cout,Cx,KH,KW]
    const float* bias;                  // [Cout] or NULL
    const float* h;                     // GATE, BLEND: [N,Ch,H,W]
    float* z;                           // [N,Ch,H,W]: written by GATE, read by BLEND
    float* rh;                          // GATE writes sigmoid(acc_r) h
    float* out_h;                       // BLEND writes (1 - z) h + z tanh(acc)
    float* raw;                         // RAW writes acc, [N,Cout,H,W]
};

// pixels per workgroup the launch takes for this problem: 64, or 32 where 64 would leave compute units without a workgroup
int gru_conv_tile_pixels(const GruConvArgs& a);
void launch_gru_conv(const GruConvArgs& a, hipStream_t s);

}  // namespace ggr

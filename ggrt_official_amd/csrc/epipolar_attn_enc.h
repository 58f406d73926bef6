// epipolar_attn_enc.h — launchers of the epipolar cross-attention core with GGRt's depth encoding folded in (epipolar_attn_enc.hip):
// the core of epipolar_attn.h on z_s = f_s + W·pe(d_s) + b without z — the sampler's raw features f and depth d go in, the
// 2·num_octaves sines of pe(d_s) are computed in the kernel, and the nn.Linear (W, b) becomes two [N·H, ·]-sized GEMMs of the caller's.
#pragma once
#include "epipolar_attn.h"

namespace ggr {

constexpr int kEpiAttnEncMaxOctaves = 16;   // E = 2·O <= 32 encoding columns beside the ray's channels

// N rays × S samples × C channels × H heads, O octaves (E = 2·O); all pointers are device pointers, float32, dense:
//   qk [N,H,C]  qe [N,H,E]  f [N,S,C]  d [N,S]  ctx_f [N,H,C]  ctx_e [N,H,E]  attn [N,H,S]
//   g_f_ctx [N,H,C]  g_e_ctx [N,H,E]  g_qk [N,H,C]  g_qe [N,H,E]  g_f [N,S,C]  g_d [N,S] (or NULL: not computed)
struct EpiAttnEncArgs {
    int N, S, C, H, O;
    const float *qk, *qe, *f, *d;
    float *ctx_f, *ctx_e, *attn_out;
    const float *attn, *g_f_ctx, *g_e_ctx;
    float *g_qk, *g_qe, *g_f, *g_d;
};

// bytes of LDS one workgroup (one wave, one ray) uses: S rows of 4·⌈C/4⌉ + 4·⌈E/4⌉ floats at a pitch of an odd number of 16-byte slots
int epipolar_attn_enc_lds_bytes(int S, int C, int O);

// hipSuccess, or the error of raising the kernel's dynamic-LDS limit (tiles above 64 KiB) — nothing is enqueued then
hipError_t launch_epipolar_attn_enc_forward(const EpiAttnEncArgs& a, hipStream_t s);
hipError_t launch_epipolar_attn_enc_backward(const EpiAttnEncArgs& a, hipStream_t s);

}  // namespace ggr

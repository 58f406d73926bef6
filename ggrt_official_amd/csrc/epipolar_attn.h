// epipolar_attn.h — launchers of the epipolar cross-attention core (epipolar_attn.hip): GGRt's Attention.forward(x, z) for ONE query
// token per ray, with the key and value projections folded out of the per-sample work — logits, softmax over the ray's samples and
// the attention-weighted sum, all on the raw samples z, and the backward of those three.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kEpiAttnMaxSamples = 64;      // one sample per lane of the wave that owns the ray
constexpr int kEpiAttnMaxChannels = 256;
constexpr int kEpiAttnMaxHeads = 8;         // per-lane accumulators of the logit phase
constexpr int kEpiAttnMaxRays = 1 << 25;    // one workgroup of 64 threads per ray: the launch stays below 2^32 threads
constexpr int kEpiAttnLdsLimit = 160 * 1024;   // LDS of a CU, and the most one workgroup may have

// N rays × S samples × C channels × H heads; all pointers are device pointers, float32, dense:
//   qk [N,H,C]  z [N,S,C]  ctx [N,H,C]  attn [N,H,S]  g_ctx [N,H,C]  g_qk [N,H,C]  g_z [N,S,C]
struct EpiAttnArgs {
    int N, S, C, H;
    const float *qk, *z;
    float *ctx, *attn_out;
    const float *attn, *g_ctx;
    float *g_qk, *g_z;
};

// bytes of LDS one workgroup (one wave, one ray) uses: the ray's [S, C] tile at a pitch of an odd number of 16-byte slots
int epipolar_attn_lds_bytes(int S, int C);

// hipSuccess, or the error of raising the kernel's dynamic-LDS limit (tiles above 64 KiB) — nothing is enqueued then
hipError_t launch_epipolar_attn_forward(const EpiAttnArgs& a, hipStream_t s);
hipError_t launch_epipolar_attn_backward(const EpiAttnArgs& a, hipStream_t s);

}  // namespace ggr

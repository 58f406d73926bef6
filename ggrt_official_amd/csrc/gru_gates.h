// gru_gates.h — launchers of the ConvGRU gate math (gru_gates.hip): what GGRt's SepConvGRU / ConvGRU (ggrt/optimizer.py) do between
// their convolutions — two sigmoids, r h, a tanh and the blend (1 - z) h + z q — as two launches forward and two backward per
// half-step, on float32 dense NCHW maps.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kGruThreads = 256;
constexpr int kGruMaxBlocks = 2048;     // 8 workgroups on each of 256 CUs; the rest of a larger map is walked by a grid-stride loop

// M = Ch H W.  Element (n, c, p) of a [N,Ch,H,W] map is at n M + c HW + p; in a [N,2Ch,H,W] map its z value is at n 2M + c HW + p
// and its r value M further on.  vec: every array is 16-byte aligned and M % 4 == 0, so that a lane's four consecutive elements
// are one 16-byte access and share their n.  A pointer that a call does not use is NULL.
struct GruArgs {
    int N, M, vec;
    const float *a_zr_h, *a_zr_x;       // gate forward: [N,2Ch,H,W]; a_zr_x may be NULL
    const float* h;                     // [N,Ch,H,W]
    float *z, *r, *rh;                  // written by the gate forward; z and r read by the backward calls
    const float *a_q_h, *a_q_x;         // blend forward: [N,Ch,H,W]; a_q_x may be NULL
    float *q, *out_h;                   // written by the blend forward; q read by the blend backward
    const float* g_out_h;               // blend backward: dL/dh'
    float *g_a_q, *g_a_zr, *g_h_part;   // blend backward writes g_a_q, the z half of g_a_zr and g_h_part (each may be NULL);
                                        // the gate backward writes the r half of g_a_zr (or NULL) and reads g_h_part (or NULL)
    const float* g_rh;                  // gate backward: dL/d(r h)
    float* g_h;                         // gate backward: dL/dh or NULL
};

void launch_gru_gate_forward(const GruArgs& a, hipStream_t s);
void launch_gru_blend_forward(const GruArgs& a, hipStream_t s);
void launch_gru_blend_backward(const GruArgs& a, hipStream_t s);
void launch_gru_gate_backward(const GruArgs& a, hipStream_t s);

}  // namespace ggr

// gru_gates.hip — the gate math of GGRt's SepConvGRU / ConvGRU (ggrt/optimizer.py:33-78) between its convolutions.  With the
// convolutions split by input (h-side and x-side, the x-side carrying the bias) one half-step is
//     a_zr_h = conv(h, w_zr_h)   a_zr_x = conv(x, w_zr_x, b_zr)   a_q_x = conv(x, w_q_x, b_q)
//     GATE   z = sigmoid(a_zr_h[z] + a_zr_x[z])   r = sigmoid(a_zr_h[r] + a_zr_x[r])   rh = r h
//     a_q_h  = conv(rh, w_q_h)
//     BLEND  q = tanh(a_q_h + a_q_x)   h' = (1 - z) h + z q
// and backward, with g = dL/dh' and dL/drh from the w_q_h convolution:
//     BLEND  dL/da_q = g z (1 - q q)   dL/da_z = g (q - h) z (1 - z)   dL/dh_part = g (1 - z)
//     GATE   dL/da_r = dL/drh h r (1 - r)   dL/dh = dL/dh_part + dL/drh r
// Everything is elementwise over N M elements (M = Ch H W): one launch each, no LDS, no atomics, nothing to zero, the same bits on
// every run.  A lane owns four consecutive elements — one 16-byte access per array — where M % 4 == 0 and the arrays are 16-byte
// aligned, and one element otherwise; consecutive lanes own consecutive accesses, so a wave reads and writes 1 KiB (or 256 B) runs.
// The grid is capped and strides over the rest.  No pointer is __restrict__: an output may be the very array of an input of the
// same call (a lane reads its elements before it writes them); only h' over h is refused, by the entry point.
#include "gru_gates.h"
#include "gru_math.h"

namespace ggr {
namespace {

constexpr int NT = kGruThreads;

// (the sigmoid and the tanh: gru_math.h, shared with the inference route's epilogues in gru_conv.hip)
__device__ __forceinline__ float sigmoid_f(float a) { return gru_sigmoid(a); }
__device__ __forceinline__ float tanh_f(float a) { return gru_tanh(a); }

template <int V> __device__ __forceinline__ void ld(const float* p, float* v) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int V> __device__ __forceinline__ void st(float* p, const float* v) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// item i of a launch is V consecutive elements from e = i V of a [N,Ch,H,W] map; its z value in a [N,2Ch,H,W] map is at
// e + n M.  Every index stays below N 2 M < 2^31.
#define GRU_ITEMS_LOOP(a)                                                                                         \
    const int items = (int)(((int64_t)(a).N * (a).M) / V), stride = (int)gridDim.x * NT;                          \
    for (int i = (int)blockIdx.x * NT + (int)threadIdx.x; i < items; i += stride)

template <int V> __global__ __launch_bounds__(NT) void gru_gate_fwd_kernel(const GruArgs a) {
    GRU_ITEMS_LOOP(a) {
        const int e = i * V, n = e / a.M, zi = e + n * a.M, ri = zi + a.M;
        float az[V], ar[V], h[V], z[V], r[V], rh[V];
        ld<V>(a.a_zr_h + zi, az);
        ld<V>(a.a_zr_h + ri, ar);
        ld<V>(a.h + e, h);
        if (a.a_zr_x) {
            float bz[V], br[V];
            ld<V>(a.a_zr_x + zi, bz);
            ld<V>(a.a_zr_x + ri, br);
#pragma unroll
            for (int k = 0; k < V; ++k) { az[k] += bz[k]; ar[k] += br[k]; }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            z[k] = sigmoid_f(az[k]);
            r[k] = sigmoid_f(ar[k]);
            rh[k] = r[k] * h[k];
        }
        st<V>(a.z + e, z);
        st<V>(a.r + e, r);
        st<V>(a.rh + e, rh);
    }
}

template <int V> __global__ __launch_bounds__(NT) void gru_blend_fwd_kernel(const GruArgs a) {
    GRU_ITEMS_LOOP(a) {
        const int e = i * V;
        float aq[V], z[V], h[V], q[V], o[V];
        ld<V>(a.a_q_h + e, aq);
        ld<V>(a.z + e, z);
        ld<V>(a.h + e, h);
        if (a.a_q_x) {
            float b[V];
            ld<V>(a.a_q_x + e, b);
#pragma unroll
            for (int k = 0; k < V; ++k) aq[k] += b[k];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            q[k] = tanh_f(aq[k]);
            o[k] = (1.f - z[k]) * h[k] + z[k] * q[k];
        }
        st<V>(a.q + e, q);
        st<V>(a.out_h + e, o);
    }
}

template <int V> __global__ __launch_bounds__(NT) void gru_blend_bwd_kernel(const GruArgs a) {
    GRU_ITEMS_LOOP(a) {
        const int e = i * V, n = e / a.M, zi = e + n * a.M;
        float g[V], z[V], q[V], h[V], o[V];
        ld<V>(a.g_out_h + e, g);
        ld<V>(a.z + e, z);
        ld<V>(a.q + e, q);
        ld<V>(a.h + e, h);
        if (a.g_a_q) {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = g[k] * (z[k] * (1.f - q[k] * q[k]));
            st<V>(a.g_a_q + e, o);
        }
        if (a.g_a_zr) {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = (g[k] * (q[k] - h[k])) * (z[k] * (1.f - z[k]));
            st<V>(a.g_a_zr + zi, o);
        }
        if (a.g_h_part) {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = g[k] * (1.f - z[k]);
            st<V>(a.g_h_part + e, o);
        }
    }
}

template <int V> __global__ __launch_bounds__(NT) void gru_gate_bwd_kernel(const GruArgs a) {
    GRU_ITEMS_LOOP(a) {
        const int e = i * V, n = e / a.M, ri = e + n * a.M + a.M;
        float d[V], r[V], h[V], o[V];
        ld<V>(a.g_rh + e, d);
        ld<V>(a.r + e, r);
        ld<V>(a.h + e, h);
        if (a.g_a_zr) {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = (d[k] * h[k]) * (r[k] * (1.f - r[k]));
            st<V>(a.g_a_zr + ri, o);
        }
        if (a.g_h) {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = d[k] * r[k];
            if (a.g_h_part) {
                float p[V];
                ld<V>(a.g_h_part + e, p);
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = p[k] + o[k];
            }
            st<V>(a.g_h + e, o);
        }
    }
}

unsigned gru_blocks(const GruArgs& a) {
    const int64_t items = (int64_t)a.N * a.M / (a.vec ? 4 : 1), blocks = (items + NT - 1) / NT;
    return (unsigned)(blocks < kGruMaxBlocks ? blocks : kGruMaxBlocks);
}

}  // namespace

#define GRU_LAUNCH(kernel, a, s)                                                                       \
    do {                                                                                               \
        if ((a).vec) hipLaunchKernelGGL(kernel<4>, dim3(gru_blocks(a)), dim3(NT), 0, s, a);            \
        else hipLaunchKernelGGL(kernel<1>, dim3(gru_blocks(a)), dim3(NT), 0, s, a);                    \
    } while (0)

void launch_gru_gate_forward(const GruArgs& a, hipStream_t s) { GRU_LAUNCH(gru_gate_fwd_kernel, a, s); }
void launch_gru_blend_forward(const GruArgs& a, hipStream_t s) { GRU_LAUNCH(gru_blend_fwd_kernel, a, s); }
void launch_gru_blend_backward(const GruArgs& a, hipStream_t s) { GRU_LAUNCH(gru_blend_bwd_kernel, a, s); }
void launch_gru_gate_backward(const GruArgs& a, hipStream_t s) { GRU_LAUNCH(gru_gate_bwd_kernel, a, s); }

}  // namespace ggr

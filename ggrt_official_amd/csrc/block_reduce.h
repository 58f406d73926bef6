// block_reduce.h — the double sums of the loss passes (image_loss.hip, photometric_loss.hip, warp_cost.hip) over a wave and over a
// workgroup, in a fixed order: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ggr {

// the sum over the wave's 64 lanes; valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the sums of N values per thread over the workgroup's WAVES waves, in a fixed order; valid in thread 0.  The caller synchronises
// before the next use of `sred`.
template <int N, int WAVES>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*sred)[WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = 0; q < N; ++q) {
        v[q] = wave_sum(v[q]);
        if (lane == 0) sred[q][wave] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 0; q < N; ++q) {
            double s = sred[q][0];
            for (int w = 1; w < WAVES; ++w) s += sred[q][w];
            v[q] = s;
        }
}

}  // namespace ggr

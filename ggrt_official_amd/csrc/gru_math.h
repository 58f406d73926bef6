// gru_math.h — the two squashing functions of the ConvGRU kernels (gru_gates.hip, gru_conv.hip): one definition, so that an
// inference step squashes exactly as a training step does.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

namespace ggr {

// exp(-|a|) with results below the smallest normal float taken as 0, whatever the denormal mode: from |a| = 87.4 on the sigmoid is
// exactly 0 or 1, and neither it nor the tanh can overflow or turn NaN for a finite a.
__device__ __forceinline__ float gru_sigmoid(float a) {
    float e = expf(-fabsf(a));
    e = e < FLT_MIN ? 0.f : e;
    const float p = 1.f / (1.f + e);
    return a >= 0.f ? p : e * p;
}

// tanh|a| = (1 - e) / (1 + e) with e = exp(-2|a|), formed as -m / (2 + m) from m = expm1(-2|a|) so that small |a| lose nothing;
// m is exactly -1 from |a| = 9.1 on, and the tanh exactly 1.
__device__ __forceinline__ float gru_tanh(float a) {
    const float m = expm1f(-2.f * fabsf(a));
    return copysignf(-m / (2.f + m), a);
}

}  // namespace ggr

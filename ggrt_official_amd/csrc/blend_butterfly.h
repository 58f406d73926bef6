// blend_butterfly.h — the transposing butterfly of the replay backwards (blend_feat.hip, blend_dist.hip): a wave holds N values
// per lane and ends with every lane owning N/64 sums over the 64 lanes.  Included by those two kernels only.
#pragma once
#include "blend_common.h"

namespace ggr {

template <int CTRL>
__device__ __forceinline__ float feat_dpp(float v) {   // (every lane has a source under the controls used below)
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// One level of the transposing butterfly over v[0 .. 2·HALF): the lanes whose bit is clear keep the lower half of the values,
// their partners the upper half, each adds what the partner sends.  Afterwards v[0 .. HALF) is live.
template <int HALF, int CTRL>
__device__ __forceinline__ void fold_dpp(float* v, bool upper) {
#pragma unroll
    for (int i = 0; i < HALF; i++) {
        const float keep = upper ? v[i + HALF] : v[i], send = upper ? v[i] : v[i + HALF];
        v[i] = keep + feat_dpp<CTRL>(send);
    }
}
template <int HALF>
__device__ __forceinline__ void fold_swap32(float* v) {   // lanes 0-31 keep the lower half, lanes 32-63 the upper
#pragma unroll
    for (int i = 0; i < HALF; i++) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + HALF]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}
template <int HALF>
__device__ __forceinline__ void fold_swap16(float* v) {   // even 16-lane rows keep the lower half, odd rows the upper
#pragma unroll
    for (int i = 0; i < HALF; i++) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + HALF]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}

}  // namespace ggr

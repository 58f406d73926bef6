// blend_hits.h — launcher of the hit pass (blend_hits.hip): per-PIXEL hit lists over the list entries the colour blend composited —
// the first K of them in list order (front to back) with their blend weights, what the K slots leave out, and their number.
#pragma once
#include "ggr_common.h"

#define GGR_MAX_HITS 32

namespace ggr {

// The list ids are (view, Gaussian) pair indices v·P1 + g; the index slots hold g (the id minus view·P1).  `index` / `weight`
// are [V,K,H,W] and come as a pair (both or neither); `rest` / `count` are [V,H,W]; each may be null (not computed).  The
// kernel writes every element of every array it is given — nothing has to be cleared — with plain stores and per-pixel sums
// in list order: all four are bit-reproducible from run to run.
//   index   int32  the id of the k-th live entry, −1 for k >= count       weight  float  its w = α·T_before, 0 for k >= count
//   rest    float  Σ w of the live entries behind the K-th                count   int32  the number of live entries (all)
// With rest == count == null a pixel is finished once it holds K entries (the walk then ends earlier; same index / weight).
void launch_blend_hits(int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* splat, int K,
                       int32_t* index, float* weight, float* rest, int32_t* count, int views, int P1, int scissored,
                       hipStream_t s);

}  // namespace ggr

// epipolar.h — launchers of the epipolar-sampler pass (epipolar.hip): GGRt's EpipolarSampler.forward and the depth lines of
// EpipolarTransformer.forward (ray setup, project_rays, the sample points, the bilinear gather from the other views' feature maps,
// get_depth → clip → relative disparity) in one launch behind a small layout launch, and the scatter of dL/dfeatures back into the
// feature maps.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kEpipolarMaxSamples = 64;     // one sample per lane of the wave that owns the ray
constexpr int kEpipolarMaxChannels = 512;
constexpr int kEpipolarMinViews = 2, kEpipolarMaxViews = 8;
constexpr int kEpipolarWaves = 4;           // waves (= rays in flight) per workgroup
constexpr int kEpipolarMaxGroups = 4096;    // workgroups; the rest of the rays is strided over

// b batches × v views × (v−1) other views × r rays (the window's (y1−y0)·(x1−x0)) × s samples × c channels.  Pair-ray
// p = ((bi·v + vi)·(v−1) + ov)·r + ri samples view o = ov + (ov >= vi).  All pointers are device pointers, float32 unless said:
//   c2w [b,v,4,4]  w2c [b,v,4,4]  K [b,v,3,3]  Kinv [b,v,3,3]  near [b,v]  far [b,v]
//   images: element (bi, vi, ch, y, x) at bi·img_sb + vi·img_sv + ch·img_sc + y·img_sh + x·img_sw
//   features [P,s,c]  valid [P] uint8  xy_ray [b,v,r,2]  xy_sample / xy_near / xy_far [P,s,2]  origins / directions [b,v,r,3]
//   depth [P,s]  seg [P,4] = (xy_min, xy_max) after nan_to_num and the mask       — each output may be null (not written)
//   backward: g_features [P,s,c], valid, seg (read) → g_images [b,v,c,h,w] dense, written whole
//   scratch [b·v,h·w,c]: the feature maps channel-last (forward), the gradient's accumulator (backward)
struct EpipolarArgs {
    int b, v, c, h, w, s;
    int y0, y1, x0, x1;
    long long img_sb, img_sv, img_sc, img_sh, img_sw;
    const float *c2w, *w2c, *K, *Kinv, *near, *far, *images;
    float* features;
    unsigned char* valid;
    float *xy_ray, *xy_sample, *xy_near, *xy_far, *origins, *directions, *depth, *seg;
    const float* g_features;
    float* g_images;
    float* scratch;
};

void launch_epipolar_forward(const EpipolarArgs& a, hipStream_t s);
void launch_epipolar_backward(const EpipolarArgs& a, hipStream_t s);

}  // namespace ggr

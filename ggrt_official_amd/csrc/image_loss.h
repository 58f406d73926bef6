// image_loss.h — launchers of the image-loss pass (image_loss.hip): GGRt's img2mse (masked MSE) and ssim (Gaussian window,
// zero padding) of a rendered image against its target in one launch plus a small finishing launch, and the gradient with
// respect to either image in one launch each.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kImageLossTileH = 16;        // a workgroup owns 16 x 32 pixels of one (b, c) plane
constexpr int kImageLossTileW = 32;        // (one row of the tile = one 32-lane group of an LDS access: conflict-free at any pitch)
constexpr int kImageLossThreads = 256;
constexpr int kImageLossMaxWindow = 11;
constexpr int kImageLossMaxSide = 1 << 20;          // H and W
constexpr int64_t kImageLossMaxTiles = 1 << 30;     // workgroups of one launch
constexpr int kImageLossPartials = 3;               // doubles per workgroup: sum of the SSIM map, of d^2*mask, of mask (plane c = 0)

// pred, target [B,C,H,W]; mask [B,H,W] or null; all device pointers, float32, dense.  nout = size_average ? 1 : B.
struct ImageLossArgs {
    int B, C, H, W, window, size_average;
    const float *pred, *target, *mask;
    float *mse, *ssim;          // [nout]
    float* mse_scale;           // [nout]: 1 / (sum(mask)*C + 1e-6), or 1 / count without a mask (forward writes, backward reads)
    double* partials;           // [tiles][3]
    const float *g_mse, *g_ssim;   // [nout] each, either may be null (taken as zero)
    float* g_image;             // [B,C,H,W], written whole: the gradient with respect to `pred` as the struct names it
    float w[kImageLossMaxWindow];   // the normalised 1-D window (image_loss_window)
};

// workgroups (tiles over all planes) of a launch: B*C*ceil(H/16)*ceil(W/32)
int64_t image_loss_tiles(int B, int C, int H, int W);

// the reference's gaussian(window_size, 1.5): float32(exp(-(k - window_size/2)^2 / 4.5)) over their float32 sum
void image_loss_window(int window_size, float* w);

void launch_image_loss_forward(const ImageLossArgs& a, hipStream_t s);
// one launch: the gradient with respect to a.pred.  The gradient with respect to the target is the same call with pred and target
// exchanged (SSIM is symmetric; the MSE term changes its sign with the difference).
void launch_image_loss_backward(const ImageLossArgs& a, hipStream_t s);

}  // namespace ggr

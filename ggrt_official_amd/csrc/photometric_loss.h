// photometric_loss.h — launchers of the multi-view photometric loss pass (photometric_loss.hip): GGRt's
// MultiViewPhotometricDecayLoss (ggrt/loss/photometric_loss.py) — warp, L1 + 3x3 SSIM, clip, per-pixel minimum over the candidates,
// edge-aware smoothness — in four launches forward and two backward, whatever the number of iterations and views.
#pragma once
#include "ggr_common.h"

namespace ggr {

constexpr int kPhotoTileH = 16;             // a workgroup owns 16 x 32 pixels of one plane (as image_loss.hip)
constexpr int kPhotoTileW = 32;
constexpr int kPhotoThreads = 256;
constexpr int kPhotoMaxCandidates = 16;     // C = 2V with the auto-mask (V <= 8), V without (V <= 16)
constexpr int kPhotoMaxSide = 1 << 14;      // H and W
constexpr int kPhotoMaxIters = 1024;        // n
constexpr int kPhotoFwdPartials = 3;        // doubles per (plane, tile): sum p, sum p^2, sum of the iteration's inverse depth (view 0)
constexpr int kPhotoSelPartials = 3;        // doubles per (iteration, tile): sum of the minimum, sum |smoothness_x|, sum |smoothness_y|
constexpr int kPhotoPosePartials = 12;      // doubles per (tile, iteration, view): dL/dR (9, row-major) and dL/dt (3)

// image [3,H,W]; ref_imgs [V,3,H,W]; inv_depths [n,H,W]; K [9]; ref_Ks [V,9]; poses [V,n,6] (t, then the Euler angles x, y, z);
// all device pointers, float32, dense.  C = automask ? 2V : V candidates per pixel, in the order warped j, unwarped j, warped j+1 ...
struct PhotoLossArgs {
    int V, n, H, W, automask, clip_on, C;
    float w_ssim, w_smooth, C1, C2, clip, gamma;
    const float *image, *ref_imgs, *inv_depths, *K, *ref_Ks, *poses;
    float* planes;              // [n*V + (automask ? V : 0)][H,W]: the candidates before the clip (forward writes, backward reads)
    double* workspace;          // forward: [planes][tiles][3] then [n][tiles][3]; backward: [tiles][n][V][12]
    float* thresholds;          // [n,C]: mean + clip * std of each candidate (forward writes, backward reads)
    float* state;               // [2n]: the mean of each inverse-depth map, then each iteration's smoothness term (forward writes, backward reads)
    unsigned char* choice;      // [n,H,W]: the candidate that won the minimum (forward writes, backward reads)
    float *loss, *photo, *smooth;   // [1] each
    const float* g_loss;        // backward: [1]
    float* g_inv;               // backward: [n,H,W], written whole
    float* g_poses;             // backward: [V,n,6], written whole
};

int64_t photo_loss_tiles(int H, int W);
int64_t photo_loss_planes(int V, int n, int automask);
// doubles of PhotoLossArgs.workspace: the larger of what the forward and the backward need
int64_t photo_loss_workspace_doubles(int V, int n, int H, int W, int automask);

void launch_photo_loss_forward(const PhotoLossArgs& a, hipStream_t s);
void launch_photo_loss_backward(const PhotoLossArgs& a, hipStream_t s);

}  // namespace ggr

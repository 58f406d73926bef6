// photometric_loss.hip — GGRt's multi-view photometric loss (ggrt/loss/photometric_loss.py: MultiViewPhotometricDecayLoss) with
// its geometry (ggrt/geometry/camera.py, depth.py; ggrt/pose_util.py: Pose.from_vec), for one target image, V reference views and n
// inverse-depth maps / poses per view.
//
// Forward, four launches whatever n and V:
//   1 planes  grid (tiles, n*V + V): a workgroup owns a 16 x 32 tile of one candidate plane.  For a warped candidate (iteration i,
//             view j) it lifts every pixel of the tile and of a 1-pixel halo with K^-1 and 1/inv_depth, moves it by the pose built
//             from the six numbers, projects with the view's K and gathers the reference image bilinearly (zeros outside) into
//             LDS — a halo pixel beyond the border is the reflected pixel's warped value; the warped image never reaches memory.
//             The unwarped candidates (the auto-mask) load the reference image itself, once per view.  Then L1 + the 3 x 3
//             reflection-padded SSIM give p, which is stored, and sum p, sum p^2 (double) go to the workgroup's slot.
//   2 stats   one workgroup per (iteration, candidate): threshold = mean + clip * std (unbiased) from the slots in a fixed order;
//             and one per iteration: the mean of its inverse-depth map.
//   3 select  grid (tiles, n): per pixel the minimum of the clamped candidates (ties: the lowest index) and its index, and the
//             smoothness terms of the pixel's right and lower edge; three sums per workgroup.
//   4 finish  one workgroup: the gamma-weighted sum, the smoothness sum, the loss.
// The candidate planes are STORED (not recomputed in launch 3): 4 bytes written and read per candidate pixel against a second
// projection, twelve gathers and three 3 x 3 SSIMs.
//
// Backward, two launches:
//   1 grid (tiles, n), a loop over the views inside: the upstream factor of a pixel is nonzero only where view j's warped
//     candidate won the minimum (the forward's `choice`) and was not clamped (the stored p against the stored threshold: the same
//     bits, the same decision).  The workgroup recomputes the warped values on a 2-pixel halo, the three SSIM derivative maps on a
//     1-pixel halo, gathers them over the up to nine windows that hold a pixel (reflection: a border window counts its inner
//     neighbour twice), adds the L1 term, and goes through the bilinear weights into (u, v), the projection, the pose (12 sums
//     per workgroup: dL/dR and dL/dt) and the pixel's inverse depth.  A view that has no such pixel in the tile is skipped.  The
//     smoothness gradient (its part through the per-map mean is the iteration's own smoothness value, see below) is added and
//     dL/dinv_depths is written once.
//   2 one workgroup per (iteration, view): adds the 12 sums over the tiles in a fixed order and chains them into the six numbers.
// No atomics, fixed summation orders: two runs give the same bits.
//
// The camera model — Kinv, the pose, project, the bilinear taps, the projection's backward and the pose chain — is warp_geometry.h's,
// shared with warp_cost.hip; the double sums are block_reduce.h's.  `project` and `taps_at` are compiled without contraction, so the
// backward's two call sites (the halo loop that fills sx, the per-pixel gradient loop) and the forward perform the same IEEE
// operations and land in the same bilinear cell.  This file keeps what is the loss's own: tiles, halos, reflection, SSIM, the
// statistics, the selection, the finish and the smoothness terms.
#include "photometric_loss.h"
#include "block_reduce.h"
#include "warp_geometry.h"
#include <math.h>

namespace ggr {

int64_t photo_loss_tiles(int H, int W) { return (int64_t)((H + kPhotoTileH - 1) / kPhotoTileH) * ((W + kPhotoTileW - 1) / kPhotoTileW); }
int64_t photo_loss_planes(int V, int n, int automask) { return (int64_t)n * V + (automask ? V : 0); }
int64_t photo_loss_workspace_doubles(int V, int n, int H, int W, int automask) {
    const int64_t tiles = photo_loss_tiles(H, W);
    const int64_t fwd = (photo_loss_planes(V, n, automask) * kPhotoFwdPartials + (int64_t)n * kPhotoSelPartials) * tiles;
    const int64_t bwd = tiles * n * V * kPhotoPosePartials;
    return fwd > bwd ? fwd : bwd;
}

namespace {

constexpr int TH = kPhotoTileH, TW = kPhotoTileW, NT = kPhotoThreads;
constexpr int H1 = TH + 2, W1 = TW + 2, N1 = H1 * W1;       // the tile with a halo of 1
constexpr int H2 = TH + 4, W2 = TW + 4, N2 = H2 * W2;       // the tile with a halo of 2
constexpr int PIX = TH * TW / NT;                            // pixels of the tile per thread

// ReflectionPad2d(1) as an index; clamped, so that a partial tile's overhang (whose values nobody uses) stays inside the plane
__device__ __forceinline__ int reflect(int y, int n) {
    y = y < 0 ? -y : y;
    y = y >= n ? 2 * (n - 1) - y : y;
    return min(max(y, 0), n - 1);
}

// the target camera's Kinv, the pose of (iteration i, view j) and the view's intrinsics
__device__ void setup_cam(const PhotoLossArgs& a, int i, int j, Cam* c) {
    kinv_closed_form(a.K, c->Kinv);
    pose_from_vec(a.poses + ((int64_t)j * a.n + i) * 6, c->R, c->t);
    for (int k = 0; k < 9; ++k) c->Kr[k] = a.ref_Ks[(int64_t)j * 9 + k];
}

// the 3 x 3 means of x and y, their variances and covariance, and what SSIM makes of them.  The reference forms the variances as
// E[xx] - mu^2, which in float32 loses four digits beside C2 = 9e-4; here they are the means of the CENTRED products — the same
// numbers, without the cancellation — so the planes are closer to the exact ones than a float32 run of the reference is.
struct Stats { float mu1, mu2, sig1, sig2, sig12; };
struct Ssim { float A1, A2, B1, B2, value; };

// the window is nine floats of x and of y, `pitch` apart per row
__device__ __forceinline__ Stats window_stats(const float* X, const float* Y, int r0, int r1, int r2, int c0, int c1, int c2) {
    const int ro[3] = {r0, r1, r2}, co[3] = {c0, c1, c2};
    Stats s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            s.mu1 += X[ro[dy] + co[dx]];
            s.mu2 += Y[ro[dy] + co[dx]];
        }
    s.mu1 /= 9.f;
    s.mu2 /= 9.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float x = X[ro[dy] + co[dx]] - s.mu1, y = Y[ro[dy] + co[dx]] - s.mu2;
            s.sig1 += x * x;
            s.sig2 += y * y;
            s.sig12 += x * y;
        }
    s.sig1 /= 9.f;
    s.sig2 /= 9.f;
    s.sig12 /= 9.f;
    return s;
}

__device__ __forceinline__ Ssim ssim_of(const Stats& s, float C1, float C2) {
#pragma clang fp contract(off)      // (the two numerator and the two denominator factors are formed the same way, product by product)
    Ssim r;
    r.A1 = 2.f * (s.mu1 * s.mu2) + C1;
    r.A2 = 2.f * s.sig12 + C2;
    r.B1 = s.mu1 * s.mu1 + s.mu2 * s.mu2 + C1;
    r.B2 = s.sig1 + s.sig2 + C2;
    r.value = (r.A1 * r.A2) / (r.B1 * r.B2);
    return r;
}

__device__ __forceinline__ void tile_origin(const PhotoLossArgs& a, int& y0, int& x0) {
    const unsigned nx = (unsigned)(a.W + TW - 1) / TW;
    x0 = (int)(blockIdx.x % nx) * TW;
    y0 = (int)(blockIdx.x / nx) * TH;
}

__device__ __forceinline__ int64_t planes_of(const PhotoLossArgs& a) { return (int64_t)a.n * a.V + (a.automask ? a.V : 0); }

// the plane of candidate c of iteration i
__device__ __forceinline__ const float* candidate_plane(const PhotoLossArgs& a, int i, int c, int64_t hw) {
    if (!a.automask) return a.planes + ((int64_t)i * a.V + c) * hw;
    return (c & 1) ? a.planes + ((int64_t)a.n * a.V + (c >> 1)) * hw : a.planes + ((int64_t)i * a.V + (c >> 1)) * hw;
}

// ---- forward 1: the candidate planes --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void photo_planes_kernel(const PhotoLossArgs a) {
    __shared__ float sx[3][N1], sy[3][N1];
    __shared__ Cam cam;
    __shared__ double sred[kPhotoFwdPartials][NT / 64];
    int y0, x0;
    tile_origin(a, y0, x0);
    const int64_t hw = (int64_t)a.H * a.W;
    const int plane = blockIdx.y, nv = a.n * a.V;
    const bool warped = plane < nv;
    const int i = warped ? plane / a.V : 0, j = warped ? plane - i * a.V : plane - nv;
    const float* ref = a.ref_imgs + (int64_t)j * 3 * hw;
    const float* inv = a.inv_depths + (int64_t)i * hw;
    if (warped && threadIdx.x == 0) setup_cam(a, i, j, &cam);
    __syncthreads();
    for (int idx = threadIdx.x; idx < N1; idx += NT) {
        const int ly = idx / W1, lx = idx - ly * W1;
        const int py = reflect(y0 - 1 + ly, a.H), px = reflect(x0 - 1 + lx, a.W);
        const int64_t off = (int64_t)py * a.W + px;
        for (int c = 0; c < 3; ++c) sy[c][idx] = a.image[c * hw + off];
        if (warped) {
            const Proj pr = project(cam, inv[off], px, py);
            const Taps t = taps_at(pr.u, pr.v, a.H, a.W);
            for (int c = 0; c < 3; ++c) sx[c][idx] = sample(ref + c * hw, t);
        } else {
            for (int c = 0; c < 3; ++c) sx[c][idx] = ref[c * hw + off];
        }
    }
    __syncthreads();
    double v[kPhotoFwdPartials] = {0.0, 0.0, 0.0};
    for (int k = 0; k < PIX; ++k) {
        const int q = threadIdx.x + k * NT, r = q / TW, c = q - r * TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy < a.H && gx < a.W) {
            float ssim_sum = 0.f, l1_sum = 0.f;
            for (int ch = 0; ch < 3; ++ch) {
                const float *X = sx[ch] + r * W1 + c, *Y = sy[ch] + r * W1 + c;
                const Stats s = window_stats(X, Y, 0, W1, 2 * W1, 0, 1, 2);
                const Ssim m = ssim_of(s, a.C1, a.C2);
                ssim_sum += fminf(fmaxf((1.f - m.value) / 2.f, 0.f), 1.f);
                l1_sum += fabsf(X[W1 + 1] - Y[W1 + 1]);
            }
            const float p = a.w_ssim * (ssim_sum / 3.f) + (1.f - a.w_ssim) * (l1_sum / 3.f);
            const int64_t off = (int64_t)gy * a.W + gx;
            a.planes[plane * hw + off] = p;
            v[0] += (double)p;
            v[1] += (double)p * (double)p;
            if (warped && j == 0) v[2] += (double)inv[off];
        }
    }
    block_sum(v, sred);
    if (threadIdx.x == 0) {
        double* o = a.workspace + ((int64_t)plane * gridDim.x + blockIdx.x) * kPhotoFwdPartials;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

// ---- forward 2: thresholds and inverse-depth means ------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void photo_stats_kernel(const PhotoLossArgs a, const int64_t tiles) {
    __shared__ double sred[kPhotoFwdPartials][NT / 64];
    const int i = blockIdx.x / (a.C + 1), c = blockIdx.x - i * (a.C + 1);
    int64_t plane;
    if (c == a.C) plane = (int64_t)i * a.V;
    else if (!a.automask) plane = (int64_t)i * a.V + c;
    else plane = (c & 1) ? (int64_t)a.n * a.V + (c >> 1) : (int64_t)i * a.V + (c >> 1);
    double v[kPhotoFwdPartials] = {0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < tiles; t += NT) {
        const double* p = a.workspace + (plane * tiles + t) * kPhotoFwdPartials;
        v[0] += p[0]; v[1] += p[1]; v[2] += p[2];
    }
    block_sum(v, sred);
    if (threadIdx.x == 0) {
        const double N = (double)a.H * (double)a.W;
        if (c == a.C) {
            a.state[i] = (float)(v[2] / N);
        } else {
            const double mean = v[0] / N;
            const double var = fmax((v[1] - v[0] * mean) / (N - 1.0), 0.0);
            a.thresholds[(int64_t)i * a.C + c] = (float)(mean + (double)a.clip * sqrt(var));
        }
    }
}

// exp(-mean_c |I(a) - I(b)|): the smoothness weight of the edge between two pixels
__device__ __forceinline__ float edge_weight(const float* __restrict__ img, int64_t hw, int64_t oa, int64_t ob) {
    const float s = fabsf(img[oa] - img[ob]) + fabsf(img[hw + oa] - img[hw + ob]) + fabsf(img[2 * hw + oa] - img[2 * hw + ob]);
    return expf(-(s / 3.f));
}

// ---- forward 3: the minimum over the candidates, its index, the smoothness sums -------------------------------------------------
__global__ __launch_bounds__(NT) void photo_select_kernel(const PhotoLossArgs a, const int64_t tiles) {
    __shared__ double sred[kPhotoSelPartials][NT / 64];
    int y0, x0;
    tile_origin(a, y0, x0);
    const int i = blockIdx.y;
    const int64_t hw = (int64_t)a.H * a.W;
    const float* inv = a.inv_depths + (int64_t)i * hw;
    const float mc = fmaxf(a.state[i], 1e-6f);
    double v[kPhotoSelPartials] = {0.0, 0.0, 0.0};
    for (int k = 0; k < PIX; ++k) {
        const int q = threadIdx.x + k * NT, r = q / TW, c = q - r * TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy < a.H && gx < a.W) {
            const int64_t off = (int64_t)gy * a.W + gx;
            float best = 0.f;
            int which = 0;
            for (int cand = 0; cand < a.C; ++cand) {
                float p = candidate_plane(a, i, cand, hw)[off];
                if (a.clip_on) p = fminf(p, a.thresholds[(int64_t)i * a.C + cand]);
                if (cand == 0 || p < best) { best = p; which = cand; }
            }
            a.choice[(int64_t)i * hw + off] = (unsigned char)which;
            v[0] += (double)best;
            if (a.w_smooth > 0.f) {
                const float dn = inv[off] / mc;
                if (gx + 1 < a.W) v[1] += (double)fabsf((dn - inv[off + 1] / mc) * edge_weight(a.image, hw, off, off + 1));
                if (gy + 1 < a.H) v[2] += (double)fabsf((dn - inv[off + a.W] / mc) * edge_weight(a.image, hw, off, off + a.W));
            }
        }
    }
    block_sum(v, sred);
    if (threadIdx.x == 0) {
        double* o = a.workspace + planes_of(a) * tiles * kPhotoFwdPartials + ((int64_t)i * tiles + blockIdx.x) * kPhotoSelPartials;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

// ---- forward 4: the loss ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void photo_finish_kernel(const PhotoLossArgs a, const int64_t tiles) {
    __shared__ double sred[kPhotoSelPartials][NT / 64];
    const double* base = a.workspace + planes_of(a) * tiles * kPhotoFwdPartials;
    const double N = (double)a.H * (double)a.W, Nx = (double)a.H * (double)(a.W - 1), Ny = (double)(a.H - 1) * (double)a.W;
    double photo = 0.0, smooth = 0.0;
    for (int i = 0; i < a.n; ++i) {
        double v[kPhotoSelPartials] = {0.0, 0.0, 0.0};
        for (int64_t t = threadIdx.x; t < tiles; t += NT) {
            const double* p = base + ((int64_t)i * tiles + t) * kPhotoSelPartials;
            v[0] += p[0]; v[1] += p[1]; v[2] += p[2];
        }
        block_sum(v, sred);
        if (threadIdx.x == 0) {
            photo += pow((double)a.gamma, (double)(a.n - i - 1)) * (v[0] / N);
            const double s = a.w_smooth > 0.f ? (double)a.w_smooth * (v[1] / Nx + v[2] / Ny) / ldexp(1.0, i) / (double)a.n : 0.0;
            a.state[a.n + i] = (float)s;
            smooth += s;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.photo[0] = (float)(photo + smooth);    // the reference's metric aliases the tensor that `loss += smoothness` changes in place
        a.smooth[0] = (float)smooth;
        a.loss[0] = (float)(photo + smooth);
    }
}

// ---- backward 1 -------------------------------------------------------------------------------------------------------------------
// how often the 3-wide reflection-padded window centred on p (inside 0..n-1) holds q, |p - q| <= 1
__device__ __forceinline__ float window_count(int p, int q, int n) { return 1.f + (float)(p == 0 && q == 1) + (float)(p == n - 1 && q == n - 2); }

__global__ __launch_bounds__(NT) void photo_bwd_kernel(const PhotoLossArgs a) {
    __shared__ float sx[3][N2], sy[3][N2], sD[9][N1], sG[N1];
    __shared__ Cam cam;
    __shared__ double sred[kPhotoPosePartials][NT / 64];
    int y0, x0;
    tile_origin(a, y0, x0);
    const int i = blockIdx.y;
    const int64_t hw = (int64_t)a.H * a.W;
    const float* inv = a.inv_depths + (int64_t)i * hw;
    const unsigned char* choice = a.choice + (int64_t)i * hw;
    const float gout = a.g_loss[0];
    const float gphoto = gout * (float)(pow((double)a.gamma, (double)(a.n - i - 1)) / ((double)a.H * (double)a.W));

    for (int idx = threadIdx.x; idx < N2; idx += NT) {
        const int ly = idx / W2, lx = idx - ly * W2;
        const int py = y0 - 2 + ly, px = x0 - 2 + lx;
        const bool in = py >= 0 && py < a.H && px >= 0 && px < a.W;
        const int64_t off = (int64_t)py * a.W + px;
        for (int c = 0; c < 3; ++c) sy[c][idx] = in ? a.image[c * hw + off] : 0.f;
    }
    float gd[PIX];
    for (int k = 0; k < PIX; ++k) gd[k] = 0.f;

    for (int j = 0; j < a.V; ++j) {
        const int cand = a.automask ? 2 * j : j;
        const float thr = a.thresholds[(int64_t)i * a.C + cand];
        const float* pl = a.planes + ((int64_t)i * a.V + j) * hw;
        const float* ref = a.ref_imgs + (int64_t)j * 3 * hw;
        double* out = a.workspace + (((int64_t)blockIdx.x * a.n + i) * a.V + j) * kPhotoPosePartials;
        if (threadIdx.x == 0) setup_cam(a, i, j, &cam);
        int any = 0;
        for (int idx = threadIdx.x; idx < N1; idx += NT) {
            const int ly = idx / W1, lx = idx - ly * W1;
            const int py = y0 - 1 + ly, px = x0 - 1 + lx;
            float g = 0.f;
            if (py >= 0 && py < a.H && px >= 0 && px < a.W) {
                const int64_t off = (int64_t)py * a.W + px;
                if ((int)choice[off] == cand && (!a.clip_on || pl[off] <= thr)) g = gphoto;
            }
            sG[idx] = g;
            any |= g != 0.f;
        }
        any = __syncthreads_or(any);
        if (!any) {     // nobody in this tile (or next to it) listens to view j
            if (threadIdx.x == 0)
                for (int k = 0; k < kPhotoPosePartials; ++k) out[k] = 0.0;
            __syncthreads();    // (the next view rewrites cam and sG)
            continue;
        }
        for (int idx = threadIdx.x; idx < N2; idx += NT) {
            const int ly = idx / W2, lx = idx - ly * W2;
            const int py = y0 - 2 + ly, px = x0 - 2 + lx;
            float x[3] = {0.f, 0.f, 0.f};
            if (py >= 0 && py < a.H && px >= 0 && px < a.W) {
                const Proj pr = project(cam, inv[(int64_t)py * a.W + px], px, py);
                const Taps t = taps_at(pr.u, pr.v, a.H, a.W);
                for (int c = 0; c < 3; ++c) x[c] = sample(ref + c * hw, t);
            }
            for (int c = 0; c < 3; ++c) sx[c][idx] = x[c];
        }
        __syncthreads();
        // with A1 = 2 mu1 mu2 + C1, A2 = 2 sig12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = sig1 + sig2 + C2 and m = A1 A2 / (B1 B2), as
        // functions of the five window means mu1, mu2, E[xx], E[yy], E[xy] (sig1 = E[xx] - mu1^2, sig12 = E[xy] - mu1 mu2):
        //   dm/dE[xx] = -m / B2     dm/dE[xy] = 2 A1 / (B1 B2)
        //   dm/dmu1   = 2 mu2 A2 / (B1 B2) - 2 mu1 m / B1 - 2 mu1 dm/dE[xx] - mu2 dm/dE[xy]
        // each scaled by the pixel's upstream factor, the SSIM weight / 3 channels, the -1/2 of (1 - m) / 2 and the 1/9 of the mean
        for (int idx = threadIdx.x; idx < N1; idx += NT) {
            const float g = sG[idx];
            const int ly = idx / W1, lx = idx - ly * W1;
            const int py = y0 - 1 + ly, px = x0 - 1 + lx;
            int ry[3], rx[3];
            for (int d = 0; d < 3; ++d) {
                ry[d] = (reflect(py - 1 + d, a.H) - (y0 - 2)) * W2;
                rx[d] = reflect(px - 1 + d, a.W) - (x0 - 2);
            }
            for (int ch = 0; ch < 3; ++ch) {
                float d_mu = 0.f, d_xx = 0.f, d_xy = 0.f;
                if (g != 0.f) {
                    const Stats s = window_stats(sx[ch], sy[ch], ry[0], ry[1], ry[2], rx[0], rx[1], rx[2]);
                    const Ssim m = ssim_of(s, a.C1, a.C2);
                    const float half = (1.f - m.value) / 2.f;
                    if (half >= 0.f && half <= 1.f) {
                        const float scale = g * (a.w_ssim / 3.f) * (-0.5f / 9.f);
                        const float inv12 = 1.f / (m.B1 * m.B2);
                        const float e_xx = -m.value / m.B2, e_xy = 2.f * m.A1 * inv12;
                        d_mu = scale * (2.f * s.mu2 * m.A2 * inv12 - 2.f * s.mu1 * m.value / m.B1 - 2.f * s.mu1 * e_xx - s.mu2 * e_xy);
                        d_xx = scale * e_xx;
                        d_xy = scale * e_xy;
                    }
                }
                sD[3 * ch + 0][idx] = d_mu;
                sD[3 * ch + 1][idx] = d_xx;
                sD[3 * ch + 2][idx] = d_xy;
            }
        }
        __syncthreads();
        double acc[kPhotoPosePartials];
        for (int k = 0; k < kPhotoPosePartials; ++k) acc[k] = 0.0;
        for (int k = 0; k < PIX; ++k) {
            const int q = threadIdx.x + k * NT, r = q / TW, c = q - r * TW;
            const int gy = y0 + r, gx = x0 + c;
            if (!(gy < a.H && gx < a.W)) continue;
            const int l1 = (r + 1) * W1 + c + 1, l2 = (r + 2) * W2 + c + 2;
            float gw[3];     // dL/d(warped value) of the three channels
            bool live = false;
            for (int ch = 0; ch < 3; ++ch) {
                const float x = sx[ch][l2], y = sy[ch][l2];
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
                for (int dy = -1; dy <= 1; ++dy) {
                    const int py = gy + dy;
                    if (py < 0 || py >= a.H) continue;
                    const float my = window_count(py, gy, a.H);
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int px = gx + dx;
                        if (px < 0 || px >= a.W) continue;
                        const float m = my * window_count(px, gx, a.W);
                        const int o = l1 + dy * W1 + dx;
                        s0 += m * sD[3 * ch + 0][o];
                        s1 += m * sD[3 * ch + 1][o];
                        s2 += m * sD[3 * ch + 2][o];
                    }
                }
                const float d = x - y, sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                gw[ch] = s0 + 2.f * x * s1 + y * s2 + sG[l1] * ((1.f - a.w_ssim) / 3.f) * sign;
                live |= gw[ch] != 0.f;
            }
            if (!live) continue;
            const float dv = inv[(int64_t)gy * a.W + gx];
            const Proj pr = project(cam, dv, gx, gy);
            const Taps t = taps_at(pr.u, pr.v, a.H, a.W);
            float gu = 0.f, gv = 0.f;
            for (int ch = 0; ch < 3; ++ch) {
                const float* p = ref + ch * hw;
                const float v00 = tap(p, t.o00), v01 = tap(p, t.o01), v10 = tap(p, t.o10), v11 = tap(p, t.o11);
                gu += gw[ch] * (t.wy0 * (v01 - v00) + t.wy1 * (v11 - v10));
                gv += gw[ch] * (t.wx0 * (v10 - v00) + t.wx1 * (v11 - v01));
            }
            // u = P0 / Z, v = P1 / Z, Z = max(P2, 1e-5); P = Kr (R X + t); X = ray / inv_depth.  Written out here and in
            // warp_cost.hip, not a function of warp_geometry.h: as one it cost this kernel 8 VGPRs (174: two workgroups a CU, not three)
            float gP[3], gY[3], gX[3];
            gP[0] = gu / pr.Z;
            gP[1] = gv / pr.Z;
            gP[2] = pr.P2 >= 1e-5f ? -(gu * pr.u + gv * pr.v) / pr.Z : 0.f;
            for (int m = 0; m < 3; ++m) gY[m] = cam.Kr[m] * gP[0] + cam.Kr[3 + m] * gP[1] + cam.Kr[6 + m] * gP[2];
            for (int m = 0; m < 3; ++m) gX[m] = cam.R[m] * gY[0] + cam.R[3 + m] * gY[1] + cam.R[6 + m] * gY[2];
            for (int m = 0; m < 3; ++m) {
                for (int l = 0; l < 3; ++l) acc[3 * m + l] += (double)(gY[m] * pr.X[l]);
                acc[9 + m] += (double)gY[m];
            }
            const float gdepth = gX[0] * pr.ray[0] + gX[1] * pr.ray[1] + gX[2] * pr.ray[2];
            if (dv >= 1e-6f) gd[k] += -gdepth * pr.depth * pr.depth;     // (below the clamp, and at or below zero, the depth is a constant)
        }
        block_sum(acc, sred);
        if (threadIdx.x == 0)
            for (int k = 0; k < kPhotoPosePartials; ++k) out[k] = acc[k];
        __syncthreads();
    }

    // the smoothness term S_i = coef * (mean |sx| + mean |sy|) of dn = d / max(mean d, 1e-6): with h = dS/d(dn) the gradient is
    // h / mc minus, through the mean, sum(h d) / (mc^2 HW) = S_i / (mc HW)  (sum(h dn) is S_i itself: |s| = sign(s) s)
    const float mean = a.state[i], mc = fmaxf(mean, 1e-6f);
    const float coef = a.w_smooth > 0.f ? gout * (float)((double)a.w_smooth / ldexp(1.0, i) / (double)a.n) : 0.f;
    const float through_mean = (a.w_smooth > 0.f && mean >= 1e-6f) ? gout * a.state[a.n + i] / (mc * (float)a.H * (float)a.W) : 0.f;
    const float inx = 1.f / ((float)a.H * (float)(a.W - 1)), iny = 1.f / ((float)(a.H - 1) * (float)a.W);
    for (int k = 0; k < PIX; ++k) {
        const int q = threadIdx.x + k * NT, r = q / TW, c = q - r * TW;
        const int gy = y0 + r, gx = x0 + c;
        if (!(gy < a.H && gx < a.W)) continue;
        const int64_t off = (int64_t)gy * a.W + gx;
        float g = gd[k];
        if (a.w_smooth > 0.f) {
            const float dn = inv[off] / mc;
            float h = 0.f;
            auto sgn = [](float s) { return s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f); };
            if (gx + 1 < a.W) h += sgn(dn - inv[off + 1] / mc) * edge_weight(a.image, hw, off, off + 1) * inx;
            if (gx > 0) h -= sgn(inv[off - 1] / mc - dn) * edge_weight(a.image, hw, off - 1, off) * inx;
            if (gy + 1 < a.H) h += sgn(dn - inv[off + a.W] / mc) * edge_weight(a.image, hw, off, off + a.W) * iny;
            if (gy > 0) h -= sgn(inv[off - a.W] / mc - dn) * edge_weight(a.image, hw, off - a.W, off) * iny;
            g += coef * h / mc - through_mean;
        }
        a.g_inv[(int64_t)i * hw + off] = g;
    }
}

// ---- backward 2: dL/dposes from the workgroups' sums ------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void photo_pose_kernel(const PhotoLossArgs a, const int64_t tiles) {
    __shared__ double sred[kPhotoPosePartials][NT / 64];
    const int i = blockIdx.x / a.V, j = blockIdx.x - i * a.V;
    double v[kPhotoPosePartials];
    for (int k = 0; k < kPhotoPosePartials; ++k) v[k] = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += NT) {
        const double* p = a.workspace + ((t * a.n + i) * a.V + j) * kPhotoPosePartials;
        for (int k = 0; k < kPhotoPosePartials; ++k) v[k] += p[k];
    }
    block_sum(v, sred);
    if (threadIdx.x == 0) {
        const int64_t o = ((int64_t)j * a.n + i) * 6;
        pose_chain(v, a.poses + o, a.g_poses + o);
    }
}

}  // namespace

void launch_photo_loss_forward(const PhotoLossArgs& a, hipStream_t s) {
    const int64_t tiles = photo_loss_tiles(a.H, a.W);
    hipLaunchKernelGGL(photo_planes_kernel, dim3((unsigned)tiles, (unsigned)photo_loss_planes(a.V, a.n, a.automask)), dim3(NT), 0, s, a);
    hipLaunchKernelGGL(photo_stats_kernel, dim3((unsigned)(a.n * (a.C + 1))), dim3(NT), 0, s, a, tiles);
    hipLaunchKernelGGL(photo_select_kernel, dim3((unsigned)tiles, (unsigned)a.n), dim3(NT), 0, s, a, tiles);
    hipLaunchKernelGGL(photo_finish_kernel, dim3(1), dim3(NT), 0, s, a, tiles);
}

void launch_photo_loss_backward(const PhotoLossArgs& a, hipStream_t s) {
    const int64_t tiles = photo_loss_tiles(a.H, a.W);
    hipLaunchKernelGGL(photo_bwd_kernel, dim3((unsigned)tiles, (unsigned)a.n), dim3(NT), 0, s, a);
    hipLaunchKernelGGL(photo_pose_kernel, dim3((unsigned)(a.n * a.V)), dim3(NT), 0, s, a, tiles);
}

}  // namespace ggr

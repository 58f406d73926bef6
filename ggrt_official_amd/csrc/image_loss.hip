// image_loss.hip — the image loss behind the blend: GGRt's img2mse (utils_loc.py: masked MSE) and ssim (ggrt/loss/ssim_torch.py:
// Gaussian window, sigma 1.5, zero padding) of pred against target, and the gradient with respect to either image.
//
// Forward, one launch: a workgroup of 256 threads owns a 16 x 32 tile of one (b, c) plane.  It loads the tile of both images with
// a halo of R = window/2 into LDS (zeros outside the image), runs the window separably — a row pass over the five quantities x, y,
// x^2, y^2, xy, then a column pass — forms the SSIM value and the masked squared difference of its pixels and leaves three sums
// (double) in its own slot of `partials`.  A finishing launch of one workgroup per result adds the slots in a fixed order.
//
// Backward, one launch per image: NOTHING is saved by the forward.  The workgroup loads its tile with a halo of 2R, recomputes the
// five window sums on the tile and a halo of R, forms there the three partial derivatives of the SSIM value that multiply 1, 2x and
// y (zero outside the image: the map has no pixels there), and convolves those with the same window — the window is symmetric and
// the padding is zeros, so the adjoint of the convolution is the convolution.  Every pixel of the gradient is written once.
//
// LDS: every access is a 4-byte access whose 32-lane groups walk consecutive columns of one row (the tile is 32 wide), so the banks
// (address/4 mod 32) never collide whatever the pitch; only the backward's 42-wide regions let a group straddle two rows of a
// 52-wide array (at most 10 lanes two-way).  Forward 25 472 bytes a workgroup at window 11 (6 per CU), backward 45 216 (3 per CU):
// the derivative maps live where the image tiles were, which are dead after the first row pass.
#include "image_loss.h"
#include "block_reduce.h"
#include <math.h>

namespace ggr {

int64_t image_loss_tiles(int B, int C, int H, int W) {
    return (int64_t)B * C * ((H + kImageLossTileH - 1) / kImageLossTileH) * ((W + kImageLossTileW - 1) / kImageLossTileW);
}

void image_loss_window(int window_size, float* w) {
    // gaussian(): torch.Tensor([exp(...) in double]) is a float32 rounding of each tap; its float32 .sum() of these (at most 11,
    // symmetric) taps equals the rounded exact sum, which is what the double accumulation gives
    double sum = 0.0;
    for (int k = 0; k < window_size; ++k) {
        const int d = k - window_size / 2;
        w[k] = (float)exp(-(double)(d * d) / (2.0 * 1.5 * 1.5));
        sum += (double)w[k];
    }
    const float s = (float)sum;
    for (int k = 0; k < window_size; ++k) w[k] = w[k] / s;
    for (int k = window_size; k < kImageLossMaxWindow; ++k) w[k] = 0.f;
}

namespace {

constexpr int TH = kImageLossTileH, TW = kImageLossTileW, NT = kImageLossThreads;
constexpr int cmax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ void tile_of(const ImageLossArgs& a, int& plane, int& y0, int& x0) {
    const unsigned nx = (unsigned)(a.W + TW - 1) / TW, ny = (unsigned)(a.H + TH - 1) / TH;
    unsigned wg = blockIdx.x;
    x0 = (int)(wg % nx) * TW;
    wg /= nx;
    y0 = (int)(wg % ny) * TH;
    plane = (int)(wg / ny);
}

// zero-padded load of an LH x LW window of both planes whose top-left corner is pixel (gy0, gx0)
template <int LH, int LW>
__device__ __forceinline__ void load_tiles(const ImageLossArgs& a, const float* __restrict__ px, const float* __restrict__ py, int gy0,
                                           int gx0, float* sx, float* sy) {
    for (int i = threadIdx.x; i < LH * LW; i += NT) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = gy0 + ly, gx = gx0 + lx;
        const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        const int64_t off = (int64_t)gy * a.W + gx;
        sx[i] = in ? px[off] : 0.f;
        sy[i] = in ? py[off] : 0.f;
    }
}

// row pass of the five quantities: rows x OW outputs, output (r, c) from sx / sy [r][c .. c + 2R] at pitch LW
template <int R, int ROWS, int OW, int LW>
__device__ __forceinline__ void row_pass5(const ImageLossArgs& a, const float* sx, const float* sy, float* rowbuf) {
    for (int i = threadIdx.x; i < ROWS * OW; i += NT) {
        const int r = i / OW, c = i - r * OW;
        const float *xr = sx + r * LW + c, *yr = sy + r * LW + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const float w = a.w[k], x = xr[k], y = yr[k];
            s0 += w * x;
            s1 += w * y;
            s2 += w * (x * x);
            s3 += w * (y * y);
            s4 += w * (x * y);
        }
        rowbuf[0 * ROWS * OW + i] = s0;
        rowbuf[1 * ROWS * OW + i] = s1;
        rowbuf[2 * ROWS * OW + i] = s2;
        rowbuf[3 * ROWS * OW + i] = s3;
        rowbuf[4 * ROWS * OW + i] = s4;
    }
}

// The variances are differences of nearly equal numbers, E[xx] - mu^2: the squares of the means are ROUNDED products
// (no contraction inside moments()), never fused into the subtraction as a multiply-add — as the reference computes them, and so
// that a window of one tap gives the exact zeros it gives there (a contracted fma(-mu, mu, E[xx]) leaves the rounding error of x*x,
// 6e-8 beside C2 = 9e-4: SSIM values off by 1e-4, measured).  (__fmul_rn is a plain product in HIP and contracts like one.)
struct Stats { float mu1, mu2, e11, e22, e12; };
struct Moments { float mu1_sq, mu2_sq, mu12, sig1, sig2, sig12; };

__device__ __forceinline__ Moments moments(const Stats& s) {
#pragma clang fp contract(off)
    Moments m;
    m.mu1_sq = s.mu1 * s.mu1;
    m.mu2_sq = s.mu2 * s.mu2;
    m.mu12 = s.mu1 * s.mu2;
    m.sig1 = s.e11 - m.mu1_sq;
    m.sig2 = s.e22 - m.mu2_sq;
    m.sig12 = s.e12 - m.mu12;
    return m;
}

// column pass: output (r, c) from rowbuf[q][r .. r + 2R][c] at pitch OW, planes PLANE apart
template <int R, int OW, int PLANE>
__device__ __forceinline__ Stats col_pass5(const ImageLossArgs& a, const float* rowbuf, int r, int c) {
    const float* p = rowbuf + r * OW + c;
    Stats s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {
        const float w = a.w[k];
        s.mu1 += w * p[0 * PLANE + k * OW];
        s.mu2 += w * p[1 * PLANE + k * OW];
        s.e11 += w * p[2 * PLANE + k * OW];
        s.e22 += w * p[3 * PLANE + k * OW];
        s.e12 += w * p[4 * PLANE + k * OW];
    }
    return s;
}

__device__ __forceinline__ float c1() { return (float)(0.01 * 0.01); }
__device__ __forceinline__ float c2() { return (float)(0.03 * 0.03); }

template <int R>
__global__ __launch_bounds__(NT) void image_loss_fwd_kernel(const ImageLossArgs a) {
    constexpr int LH = TH + 2 * R, LW = TW + 2 * R;
    __shared__ float sx[LH * LW], sy[LH * LW];
    __shared__ float rowbuf[5 * LH * TW];
    __shared__ double sred[kImageLossPartials][NT / 64];
    int plane, y0, x0;
    tile_of(a, plane, y0, x0);
    const int64_t hw = (int64_t)a.H * a.W;
    const float *px = a.pred + plane * hw, *py = a.target + plane * hw;
    const int b = plane / a.C, ch = plane - b * a.C;
    load_tiles<LH, LW>(a, px, py, y0 - R, x0 - R, sx, sy);
    __syncthreads();
    row_pass5<R, LH, TW, LW>(a, sx, sy, rowbuf);
    __syncthreads();
    float acc_s = 0.f, acc_m = 0.f, acc_k = 0.f;
    for (int i = threadIdx.x; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy < a.H && gx < a.W) {
            const Stats s = col_pass5<R, TW, LH * TW>(a, rowbuf, r, c);
            const Moments q = moments(s);
            const float mu1_sq = q.mu1_sq, mu2_sq = q.mu2_sq, mu12 = q.mu12, sig1 = q.sig1, sig2 = q.sig2, sig12 = q.sig12;
            acc_s += ((2.f * mu12 + c1()) * (2.f * sig12 + c2())) / ((mu1_sq + mu2_sq + c1()) * (sig1 + sig2 + c2()));
            const float d = sx[(r + R) * LW + c + R] - sy[(r + R) * LW + c + R];
            const float mk = a.mask ? a.mask[b * hw + (int64_t)gy * a.W + gx] : 1.f;
            acc_m += d * d * mk;
            if (ch == 0) acc_k += mk;
        }
    }
    double v[kImageLossPartials] = {(double)acc_s, (double)acc_m, (double)acc_k};
    block_sum(v, sred);
    if (threadIdx.x == 0) {
        double* p = a.partials + (int64_t)blockIdx.x * kImageLossPartials;
        p[0] = v[0];
        p[1] = v[1];
        p[2] = v[2];
    }
}

// one workgroup per result: the slots of its planes in ascending order
__global__ __launch_bounds__(NT) void image_loss_finish_kernel(const ImageLossArgs a, const int64_t tiles_per_image) {
    __shared__ double sred[kImageLossPartials][NT / 64];
    const int o = blockIdx.x;
    const int64_t first = a.size_average ? 0 : o * tiles_per_image, n = a.size_average ? a.B * tiles_per_image : tiles_per_image;
    double v[kImageLossPartials] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += NT) {
        const double* p = a.partials + (first + i) * kImageLossPartials;
        v[0] += p[0];
        v[1] += p[1];
        v[2] += p[2];
    }
    block_sum(v, sred);
    if (threadIdx.x == 0) {
        const double count = (double)a.C * (double)a.H * (double)a.W * (double)(a.size_average ? a.B : 1);
        const double den = a.mask ? v[2] * (double)a.C + 1e-6 : count;
        a.mse[o] = (float)(v[1] / den);
        a.ssim[o] = (float)(v[0] / count);
        a.mse_scale[o] = (float)(1.0 / den);
    }
}

template <int R>
__global__ __launch_bounds__(NT) void image_loss_bwd_kernel(const ImageLossArgs a) {
    constexpr int MH = TH + 2 * R, MW = TW + 2 * R, LH = TH + 4 * R, LW = TW + 4 * R;
    __shared__ float simg[cmax(2 * LH * LW, 3 * MH * MW)];      // the two image tiles, then the three derivative maps
    __shared__ float rowbuf[5 * LH * MW];                       // row pass of the five sums, then of the three maps
    int plane, y0, x0;
    tile_of(a, plane, y0, x0);
    const int64_t hw = (int64_t)a.H * a.W;
    const float *px = a.pred + plane * hw, *py = a.target + plane * hw;
    float* g = a.g_image + plane * hw;
    const int b = plane / a.C, o = a.size_average ? 0 : b;
    const bool use_mse = a.g_mse != nullptr, use_ssim = a.g_ssim != nullptr;
    const float gm = use_mse ? a.g_mse[o] * a.mse_scale[o] : 0.f;
    const float gs = use_ssim ? a.g_ssim[o] / ((float)a.C * (float)a.H * (float)a.W * (float)(a.size_average ? a.B : 1)) : 0.f;

    if (use_ssim) {
        float *sx = simg, *sy = simg + LH * LW;
        load_tiles<LH, LW>(a, px, py, y0 - 2 * R, x0 - 2 * R, sx, sy);
        __syncthreads();
        row_pass5<R, LH, MW, LW>(a, sx, sy, rowbuf);
        __syncthreads();
        // with A1 = 2 mu1 mu2 + C1, A2 = 2 sig12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = sig1 + sig2 + C2 and m = A1 A2 / (B1 B2):
        //   dm/dE[xx] = -m / B2     dm/dE[xy] = 2 A1 / (B1 B2)
        //   dm/dmu1   = 2 mu2 A2 / (B1 B2) - 2 mu1 m / B1 - 2 mu1 dm/dE[xx] - mu2 dm/dE[xy]
        for (int i = threadIdx.x; i < MH * MW; i += NT) {
            const int r = i / MW, c = i - r * MW;
            const int gy = y0 - R + r, gx = x0 - R + c;
            float d_mu = 0.f, d_xx = 0.f, d_xy = 0.f;
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
                const Stats s = col_pass5<R, MW, LH * MW>(a, rowbuf, r, c);
                const Moments q = moments(s);
                const float mu1_sq = q.mu1_sq, mu2_sq = q.mu2_sq, mu12 = q.mu12, sig1 = q.sig1, sig2 = q.sig2, sig12 = q.sig12;
                const float A1 = 2.f * mu12 + c1(), A2 = 2.f * sig12 + c2(), B1 = mu1_sq + mu2_sq + c1(), B2 = sig1 + sig2 + c2();
                const float inv = 1.f / (B1 * B2), m = A1 * A2 * inv;
                d_xx = -m / B2;
                d_xy = 2.f * A1 * inv;
                d_mu = 2.f * s.mu2 * A2 * inv - 2.f * s.mu1 * m / B1 - 2.f * s.mu1 * d_xx - s.mu2 * d_xy;
            }
            simg[0 * MH * MW + i] = d_mu;
            simg[1 * MH * MW + i] = d_xx;
            simg[2 * MH * MW + i] = d_xy;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < MH * TW; i += NT) {
            const int r = i / TW, c = i - r * TW;
            const float* p = simg + r * MW + c;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) {
                const float w = a.w[k];
                s0 += w * p[0 * MH * MW + k];
                s1 += w * p[1 * MH * MW + k];
                s2 += w * p[2 * MH * MW + k];
            }
            rowbuf[0 * MH * TW + i] = s0;
            rowbuf[1 * MH * TW + i] = s1;
            rowbuf[2 * MH * TW + i] = s2;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy < a.H && gx < a.W) {
            const int64_t off = (int64_t)gy * a.W + gx;
            const float x = px[off], y = py[off];
            float grad = 0.f;
            if (use_ssim) {
                const float* p = rowbuf + r * TW + c;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int k = 0; k <= 2 * R; ++k) {
                    const float w = a.w[k];
                    s0 += w * p[0 * MH * TW + k * TW];
                    s1 += w * p[1 * MH * TW + k * TW];
                    s2 += w * p[2 * MH * TW + k * TW];
                }
                grad = gs * (s0 + 2.f * x * s1 + y * s2);
            }
            if (use_mse) {
                const float mk = a.mask ? a.mask[b * hw + off] : 1.f;
                grad += gm * (2.f * (x - y) * mk);
            }
            g[off] = grad;
        }
    }
}

template <template <int> class L>
void by_radius(int window, const ImageLossArgs& a, unsigned grid, hipStream_t s) {
    switch (window / 2) {
        case 0: L<0>::go(a, grid, s); break;
        case 1: L<1>::go(a, grid, s); break;
        case 2: L<2>::go(a, grid, s); break;
        case 3: L<3>::go(a, grid, s); break;
        case 4: L<4>::go(a, grid, s); break;
        default: L<5>::go(a, grid, s); break;
    }
}

template <int R>
struct Fwd {
    static void go(const ImageLossArgs& a, unsigned grid, hipStream_t s) { hipLaunchKernelGGL(image_loss_fwd_kernel<R>, dim3(grid), dim3(NT), 0, s, a); }
};
template <int R>
struct Bwd {
    static void go(const ImageLossArgs& a, unsigned grid, hipStream_t s) { hipLaunchKernelGGL(image_loss_bwd_kernel<R>, dim3(grid), dim3(NT), 0, s, a); }
};

}  // namespace

void launch_image_loss_forward(const ImageLossArgs& a, hipStream_t s) {
    const int64_t tiles = image_loss_tiles(a.B, a.C, a.H, a.W);
    by_radius<Fwd>(a.window, a, (unsigned)tiles, s);
    hipLaunchKernelGGL(image_loss_finish_kernel, dim3(a.size_average ? 1 : a.B), dim3(NT), 0, s, a, tiles / a.B);
}

void launch_image_loss_backward(const ImageLossArgs& a, hipStream_t s) {
    by_radius<Bwd>(a.window, a, (unsigned)image_loss_tiles(a.B, a.C, a.H, a.W), s);
}

}  // namespace ggr

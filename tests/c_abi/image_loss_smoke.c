/* image_loss_smoke.c — the image-loss pass driven from plain C (no Python, no torch).
 *   image_loss_smoke --host-only   needs no GPU: the struct's layout, the refusal of invalid passes before anything is enqueued
 *                                  (the pointers are never followed), the scratch size and the window (11 taps, symmetric, sum 1).
 *   image_loss_smoke               the same, then ggr_image_loss_forward and _backward over hipMalloc'd buffers with closed-form
 *                                  answers, B = 2, C = 3, H = 21, W = 37 (two tiles each way), target[b,c,y,x] = ((x + 2y + 3c + b) % 16) / 16:
 *                                  1. pred == target: mse == 0 exactly and |ssim - 1| <= 1e-6.
 *                                  2. pred = target + 1/4 without a mask: mse == 1/16 exactly; with dL/dmse = 1 alone the gradient
 *                                     is 2 * (1/4) / (B C H W) at every pixel, and dL/dtarget its negative.
 *                                  3. the same with the mask m[b,y,x] = ((x + y + b) % 3) / 2: mse = (1/16) sum(m) C / (sum(m) C + 1e-6)
 *                                     and per image with size_average = 0; the gradient is 2 * (1/4) * m / (sum(m) C + 1e-6). */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

enum { B = 2, C = 3, H = 21, W = 37, N = B * C * H * W };

static void* upload(const void* h, size_t bytes) {
    void* d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    return d;
}

static void* device_bytes(size_t bytes, int byte) {
    void* d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    hipMemset(d, byte, bytes);
    return d;
}

static GgrImageLossPass base_pass(void) {
    GgrImageLossPass lp; memset(&lp, 0, sizeof lp);
    lp.struct_size = (int32_t)sizeof lp; lp.batch = B; lp.channels = C; lp.height = H; lp.width = W; lp.window_size = 11; lp.size_average = 1;
    return lp;
}

static int host_checks(void) {
    int bad = 0;
    if (sizeof(GgrImageLossPass) != 128 || offsetof(GgrImageLossPass, batch) != 8 || offsetof(GgrImageLossPass, size_average) != 28 ||
        offsetof(GgrImageLossPass, pred) != 32 || offsetof(GgrImageLossPass, partials_bytes) != 88 || offsetof(GgrImageLossPass, dL_dtarget) != 120)
        { fprintf(stderr, "GgrImageLossPass layout\n"); bad = 1; }
    GgrImageLossPass lp = base_pass();
    float* fake = (float*)(uintptr_t)256;   /* never followed: every pass below is refused */
    lp.pred = lp.target = lp.mask = lp.dL_dmse = lp.dL_dssim = fake; lp.out_mse = lp.out_ssim = lp.mse_scale = lp.dL_dpred = lp.dL_dtarget = fake;
    lp.partials = fake; lp.partials_bytes = 1 << 20;
#define REFUSED(fn, what, edit) do { GgrImageLossPass b = lp; edit; if (fn(&b, NULL) != GGR_E_INVALID || !strstr(ggr_last_error(), "GgrImageLossPass")) \
        { fprintf(stderr, what " was not refused (%s)\n", ggr_last_error()); bad = 1; } } while (0)
    REFUSED(ggr_image_loss_forward, "struct_size 8", b.struct_size = 8);
    REFUSED(ggr_image_loss_backward, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_image_loss_forward, "batch = 0", b.batch = 0);
    REFUSED(ggr_image_loss_backward, "channels = 0", b.channels = 0);
    REFUSED(ggr_image_loss_forward, "height = 0", b.height = 0);
    REFUSED(ggr_image_loss_backward, "width = -1", b.width = -1);
    REFUSED(ggr_image_loss_forward, "window_size = 10", b.window_size = 10);
    REFUSED(ggr_image_loss_backward, "window_size = 13", b.window_size = 13);
    REFUSED(ggr_image_loss_forward, "size_average = 2", b.size_average = 2);
    REFUSED(ggr_image_loss_forward, "a misaligned buffer", b.target = (const float*)((const char*)fake + 2));
    REFUSED(ggr_image_loss_forward, "NULL pred", b.pred = NULL);
    REFUSED(ggr_image_loss_forward, "NULL out_ssim", b.out_ssim = NULL);
    REFUSED(ggr_image_loss_forward, "a small scratch", b.partials_bytes = 24);
    REFUSED(ggr_image_loss_backward, "NULL mse_scale", b.mse_scale = NULL);
    REFUSED(ggr_image_loss_backward, "no upstream gradient", b.dL_dmse = b.dL_dssim = NULL);
    REFUSED(ggr_image_loss_backward, "no gradient to write", b.dL_dpred = b.dL_dtarget = NULL);
    if (ggr_image_loss_partials_bytes(B, C, H, W) != (int64_t)B * C * 2 * 2 * 24 || ggr_image_loss_partials_bytes(B, C, 0, W) != -1)
        { fprintf(stderr, "partials bytes\n"); bad = 1; }
    float w[11];
    double sum = 0;
    if (ggr_image_loss_window(11, w) != GGR_OK) { fprintf(stderr, "window: %s\n", ggr_last_error()); bad = 1; }
    for (int k = 0; k < 11; ++k) { sum += w[k]; if (w[k] != w[10 - k] || !(w[k] > 0)) { fprintf(stderr, "window tap %d\n", k); bad = 1; } }
    if (fabs(sum - 1.0) > 2e-7 || fabs(w[5] / w[4] - exp(1.0 / 4.5)) > 1e-6) { fprintf(stderr, "window sum %.9g\n", sum); bad = 1; }
    if (ggr_image_loss_window(4, w) != GGR_E_INVALID) { fprintf(stderr, "an even window was not refused\n"); bad = 1; }
    if (ggr_abi_version() != 11) { fprintf(stderr, "abi version\n"); bad = 1; }
    if (!bad) printf("IMAGE LOSS C ABI HOST CHECKS OK\n");
    return bad;
}

static int close_to(const char* what, int i, double got, double want, double tol) {
    if (fabs(got - want) <= tol * fmax(1.0, fabs(want))) return 0;
    fprintf(stderr, "%s[%d] = %.9g, expected %.9g\n", what, i, got, want);
    return 1;
}

static float target[N], shifted[N], mask[B * H * W], grad[N], grad_t[N];

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    if (argc > 1 && !strcmp(argv[1], "--host-only")) return 0;

    double msum[B] = {0, 0};
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                mask[(b * H + y) * W + x] = (float)((x + y + b) % 3) / 2.f;
                msum[b] += mask[(b * H + y) * W + x];
                for (int c = 0; c < C; ++c) {
                    const int i = ((b * C + c) * H + y) * W + x;
                    target[i] = (float)((x + 2 * y + 3 * c + b) % 16) / 16.f;
                    shifted[i] = target[i] + 0.25f;
                }
            }
    const float one[B] = {1.f, 1.f};
    GgrImageLossPass lp = base_pass();
    float* d_target = upload(target, sizeof target);
    float* d_shifted = upload(shifted, sizeof shifted);
    float* d_mask = upload(mask, sizeof mask);
    lp.dL_dmse = upload(one, sizeof one);
    lp.out_mse = device_bytes(B * 4, 0xff); lp.out_ssim = device_bytes(B * 4, 0xff); lp.mse_scale = device_bytes(B * 4, 0xff);
    lp.partials_bytes = ggr_image_loss_partials_bytes(B, C, H, W);
    lp.partials = device_bytes((size_t)lp.partials_bytes, 0xff);
    lp.dL_dpred = device_bytes(sizeof grad, 0xff); lp.dL_dtarget = device_bytes(sizeof grad_t, 0xff);
    if (!d_target || !d_shifted || !d_mask || !lp.dL_dmse || !lp.out_mse || !lp.out_ssim || !lp.mse_scale || !lp.partials || !lp.dL_dpred || !lp.dL_dtarget)
        { fprintf(stderr, "hipMalloc failed\n"); return 2; }
    float mse[B], ssim[B];
    int bad = 0;

    /* 1. pred == target */
    lp.pred = d_target; lp.target = d_target;
    if (ggr_image_loss_forward(&lp, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(mse, lp.out_mse, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ssim, lp.out_ssim, 4, hipMemcpyDeviceToHost));
    if (mse[0] != 0.f) { fprintf(stderr, "pred == target: mse %.9g\n", mse[0]); bad = 1; }
    if (!(fabs((double)ssim[0] - 1.0) <= 1e-6)) { fprintf(stderr, "pred == target: ssim %.9g\n", ssim[0]); bad = 1; }
    printf("pred == target: mse %.9g ssim %.9g\n", mse[0], ssim[0]);

    /* 2. a constant offset, no mask */
    lp.pred = d_shifted;
    if (ggr_image_loss_forward(&lp, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    if (ggr_image_loss_backward(&lp, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(mse, lp.out_mse, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ssim, lp.out_ssim, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(grad, lp.dL_dpred, sizeof grad, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(grad_t, lp.dL_dtarget, sizeof grad_t, hipMemcpyDeviceToHost));
    if (mse[0] != 0.0625f) { fprintf(stderr, "offset 1/4: mse %.9g\n", mse[0]); bad = 1; }
    if (!(ssim[0] > 0.f && ssim[0] < 1.f)) { fprintf(stderr, "offset 1/4: ssim %.9g\n", ssim[0]); bad = 1; }
    for (int i = 0; i < N && !bad; ++i) {
        if (fabs(grad[i] - 0.5 / N) > 2e-7 * (0.5 / N)) { fprintf(stderr, "dL_dpred[%d] = %.9g, expected %.9g\n", i, grad[i], 0.5 / N); bad = 1; }
        if (grad_t[i] != -grad[i]) { fprintf(stderr, "dL_dtarget[%d] = %.9g is not -dL_dpred = %.9g\n", i, grad_t[i], -grad[i]); bad = 1; }
    }
    printf("offset 1/4: mse %.9g ssim %.9g dL_dpred[0] %.9g\n", mse[0], ssim[0], grad[0]);

    /* 3. the same with a mask, over the batch and per image */
    lp.mask = d_mask;
    for (int per_image = 0; per_image < 2; ++per_image) {
        lp.size_average = !per_image;
        if (ggr_image_loss_forward(&lp, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
        if (ggr_image_loss_backward(&lp, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(mse, lp.out_mse, per_image ? 8 : 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(grad, lp.dL_dpred, sizeof grad, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            const double m = per_image ? msum[b] : msum[0] + msum[1], den = m * C + 1e-6;
            if (b == 0 || per_image) bad |= close_to("masked mse", b, mse[per_image ? b : 0], 0.0625 * m * C / den, 2e-7);
            for (int j = 0; j < C * H * W && !bad; ++j) {
                const int i = b * C * H * W + j, px = j % (H * W);
                const double want = 0.5 * mask[b * H * W + px] / den;
                if (fabs(grad[i] - want) > 2e-7 * fabs(want)) { fprintf(stderr, "masked dL_dpred[%d] = %.9g, expected %.9g\n", i, grad[i], want); bad = 1; }
            }
        }
    }
    if (bad) return 1;
    printf("IMAGE LOSS C ABI SMOKE OK\n");
    return 0;
}

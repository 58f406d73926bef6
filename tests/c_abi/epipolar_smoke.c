/* epipolar_smoke.c — the epipolar-sampler pass driven from plain C (no Python, no torch).
 *   epipolar_smoke --host-only   needs no GPU: the struct's layout, the refusal of invalid passes before anything is enqueued (the
 *                                pointers are never followed), the scratch size query and the empty call with every pointer NULL.
 *   epipolar_smoke               the same, then ggr_epipolar_forward and ggr_epipolar_backward over hipMalloc'd buffers with a
 *                                closed-form answer: two identical cameras, the second shifted along x, and a CONSTANT image.  The
 *                                epipolar lines are then the pixel rows (xy_sample.y = the ray's y), every sample of a valid ray that
 *                                lies at least half a pixel inside the frame has all four taps inside and its feature equals the
 *                                constant, the others lie between 0 and the constant, invalid rays are exact zeros, and with
 *                                dL/dfeatures = 1 the gradient sums to sum(features) / constant (the sum of all in-frame weights). */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

enum { V = 2, C = 5, H = 6, W = 9, S = 8, R = H * W, P = V * (V - 1) * R };
static const float VALUE = 0.75f;

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

static GgrEpipolarPass base_pass(void) {
    GgrEpipolarPass ep; memset(&ep, 0, sizeof ep);
    ep.struct_size = (int32_t)sizeof ep; ep.batch = 1; ep.num_views = V; ep.channels = C; ep.height = H; ep.width = W; ep.num_samples = S;
    ep.debug = 1;
    ep.image_strides[0] = (int64_t)V * C * H * W; ep.image_strides[1] = (int64_t)C * H * W; ep.image_strides[2] = H * W;
    ep.image_strides[3] = W; ep.image_strides[4] = 1;
    ep.scratch_bytes = (int64_t)V * C * H * W * 4;
    return ep;
}

static int host_checks(void) {
    int bad = 0;
    if (sizeof(GgrEpipolarPass) != 264 || offsetof(GgrEpipolarPass, image_strides) != 56 || offsetof(GgrEpipolarPass, c2w) != 96 ||
        offsetof(GgrEpipolarPass, features) != 152 || offsetof(GgrEpipolarPass, segment) != 224 || offsetof(GgrEpipolarPass, scratch_bytes) != 256)
        { fprintf(stderr, "GgrEpipolarPass layout\n"); bad = 1; }
    GgrEpipolarPass ep = base_pass();
    float* fake = (float*)(uintptr_t)256;   /* never followed: every pass below is refused, or empty */
    ep.c2w = ep.w2c = ep.K = ep.Kinv = ep.near = ep.far = ep.images = fake; ep.features = ep.xy_ray = ep.xy_sample = fake;
    ep.valid = (uint8_t*)fake; ep.segment = ep.scratch = ep.dL_dimages = fake; ep.dL_dfeatures = fake;
#define REFUSED(fn, what, edit) do { GgrEpipolarPass b = ep; edit; if (fn(&b, NULL) != GGR_E_INVALID || !strstr(ggr_last_error(), "GgrEpipolarPass")) \
        { fprintf(stderr, what " was not refused (%s)\n", ggr_last_error()); bad = 1; } } while (0)
    REFUSED(ggr_epipolar_forward, "struct_size 8", b.struct_size = 8);
    REFUSED(ggr_epipolar_backward, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_epipolar_forward, "num_samples = 0", b.num_samples = 0);
    REFUSED(ggr_epipolar_forward, "num_samples = 65", b.num_samples = 65);
    REFUSED(ggr_epipolar_backward, "channels = 513", b.channels = 513);
    REFUSED(ggr_epipolar_forward, "one view", b.num_views = 1);
    REFUSED(ggr_epipolar_forward, "nine views", b.num_views = 9);
    REFUSED(ggr_epipolar_forward, "an empty window", (b.use_window = 1, b.window_y1 = 0, b.window_x1 = 2));
    REFUSED(ggr_epipolar_forward, "a window beyond the grid", (b.use_window = 1, b.window_y1 = H + 1, b.window_x1 = 2));
    REFUSED(ggr_epipolar_forward, "2^31 pair-rays x samples", (b.batch = 8000, b.num_views = 8, b.height = 64, b.width = 64, b.scratch_bytes = INT64_MAX));
    REFUSED(ggr_epipolar_forward, "a small scratch", b.scratch_bytes -= 4);
    REFUSED(ggr_epipolar_forward, "a misaligned buffer", b.K = (const float*)((const char*)fake + 2));
    REFUSED(ggr_epipolar_forward, "NULL w2c", b.w2c = NULL);
    REFUSED(ggr_epipolar_forward, "NULL images", b.images = NULL);
    REFUSED(ggr_epipolar_backward, "NULL segment", b.segment = NULL);
    REFUSED(ggr_epipolar_backward, "NULL dL_dimages", b.dL_dimages = NULL);
    GgrEpipolarPass e = base_pass();   /* every pointer NULL */
    e.batch = 0;
    if (ggr_epipolar_forward(&e, NULL) != GGR_OK || ggr_epipolar_backward(&e, NULL) != GGR_OK) { fprintf(stderr, "b = 0: %s\n", ggr_last_error()); bad = 1; }
    if (ggr_epipolar_scratch_bytes(1, V, C, H, W) != (int64_t)V * C * H * W * 4 || ggr_epipolar_scratch_bytes(1, 1, C, H, W) != -1)
        { fprintf(stderr, "ggr_epipolar_scratch_bytes\n"); bad = 1; }
    if (ggr_abi_version() != 11) { fprintf(stderr, "abi version\n"); bad = 1; }
    if (!bad) printf("EPIPOLAR C ABI HOST CHECKS OK\n");
    return bad;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    if (argc > 1 && !strcmp(argv[1], "--host-only")) return 0;

    const float fx = 1.1f, fy = 1.3f, cx = 0.5f, cy = 0.5f, baseline = 0.5f;
    float c2w[V * 16] = {0}, w2c[V * 16] = {0}, K[V * 9], Kinv[V * 9], near[V] = {1.f, 1.f}, far[V] = {10.f, 10.f};
    for (int v = 0; v < V; ++v) {
        for (int i = 0; i < 4; ++i) c2w[16 * v + 5 * i] = w2c[16 * v + 5 * i] = 1.f;
        c2w[16 * v + 3] = baseline * v; w2c[16 * v + 3] = -baseline * v;
        const float k[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1}, ki[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
        memcpy(K + 9 * v, k, sizeof k); memcpy(Kinv + 9 * v, ki, sizeof ki);
    }
    static float images[V * C * H * W], features[P * S * C], xy[P * S * 2], depth[P * S], g_images[V * C * H * W], ones[P * S * C];
    static uint8_t valid[P];
    for (int i = 0; i < V * C * H * W; ++i) images[i] = VALUE;
    for (int i = 0; i < P * S * C; ++i) ones[i] = 1.f;

    GgrEpipolarPass ep = base_pass();
    ep.c2w = upload(c2w, sizeof c2w); ep.w2c = upload(w2c, sizeof w2c); ep.K = upload(K, sizeof K); ep.Kinv = upload(Kinv, sizeof Kinv);
    ep.near = upload(near, sizeof near); ep.far = upload(far, sizeof far); ep.images = upload(images, sizeof images);
    ep.features = device_bytes(sizeof features, 0xff); ep.valid = device_bytes(sizeof valid, 0xff); ep.xy_sample = device_bytes(sizeof xy, 0xff);
    ep.depth = device_bytes(sizeof depth, 0xff); ep.segment = device_bytes(P * 4 * sizeof(float), 0xff);
    ep.scratch = device_bytes((size_t)ep.scratch_bytes, 0xff); ep.dL_dfeatures = upload(ones, sizeof ones);
    ep.dL_dimages = device_bytes(sizeof g_images, 0xff);
    if (!ep.c2w || !ep.w2c || !ep.K || !ep.Kinv || !ep.near || !ep.far || !ep.images || !ep.features || !ep.valid || !ep.xy_sample ||
        !ep.depth || !ep.segment || !ep.scratch || !ep.dL_dfeatures || !ep.dL_dimages) { fprintf(stderr, "hipMalloc failed\n"); return 2; }
    if (ggr_epipolar_forward(&ep, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    if (ggr_epipolar_backward(&ep, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(features, ep.features, sizeof features, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(valid, ep.valid, sizeof valid, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(xy, ep.xy_sample, sizeof xy, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(depth, ep.depth, sizeof depth, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_images, ep.dL_dimages, sizeof g_images, hipMemcpyDeviceToHost));

    int bad = 0, n_valid = 0, n_full = 0;
    double sum_features = 0, sum_grad = 0;
    for (int p = 0; p < P; ++p) {
        const int ri = p % R, y = ri / W;
        if (valid[p] > 1) { fprintf(stderr, "valid[%d] = %d\n", p, valid[p]); bad = 1; }
        n_valid += valid[p];
        for (int i = 0; i < S; ++i) {
            const float sx = xy[(p * S + i) * 2], sy = xy[(p * S + i) * 2 + 1], d = depth[p * S + i];
            if (!(d >= -1e-5f && d <= 1.f + 1e-5f)) { fprintf(stderr, "depth[%d,%d] = %g\n", p, i, d); bad = 1; }
            if (!valid[p] && (sx != 0.f || sy != 0.f)) { fprintf(stderr, "xy_sample of an invalid ray\n"); bad = 1; }
            if (valid[p] && fabsf(sy - (y + 0.5f) / H) > 1e-5f) { fprintf(stderr, "xy_sample[%d,%d].y = %g, not the ray's row\n", p, i, sy); bad = 1; }
            const int inside = sx >= 0.5f / W + 1e-5f && sx <= 1.f - 0.5f / W - 1e-5f;
            for (int ch = 0; ch < C; ++ch) {
                const float f = features[(p * S + i) * C + ch];
                sum_features += f;
                if (!valid[p]) { if (f != 0.f) { fprintf(stderr, "a feature of an invalid ray is %g\n", f); bad = 1; } }
                else if (inside) { n_full += ch == 0; if (fabsf(f - VALUE) > 1e-5f) { fprintf(stderr, "features[%d,%d,%d] = %g\n", p, i, ch, f); bad = 1; } }
                else if (!(f >= -1e-6f && f <= VALUE + 1e-5f)) { fprintf(stderr, "features[%d,%d,%d] = %g at the frame's edge\n", p, i, ch, f); bad = 1; }
            }
        }
    }
    for (int i = 0; i < V * C * H * W; ++i) { if (!isfinite(g_images[i])) { fprintf(stderr, "dL_dimages[%d] was not written\n", i); bad = 1; break; } sum_grad += g_images[i]; }
    if (n_valid < P / 4 || n_full < n_valid) { fprintf(stderr, "%d of %d rays valid, %d samples wholly inside\n", n_valid, P, n_full); bad = 1; }
    if (fabs(sum_grad - sum_features / VALUE) > 1e-4 * sum_grad) { fprintf(stderr, "sum dL_dimages %.6f, sum features / value %.6f\n", sum_grad, sum_features / VALUE); bad = 1; }
    printf("%d of %d rays valid, %d samples wholly inside, sum of gradient %.4f\n", n_valid, P, n_full, sum_grad);
    if (bad) return 1;
    printf("EPIPOLAR C ABI SMOKE OK\n");
    return 0;
}

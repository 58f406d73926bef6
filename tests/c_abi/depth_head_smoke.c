/* depth_head_smoke.c — the depth-head pass driven from plain C (no Python, no torch).
 *   depth_head_smoke --host-only   needs no GPU: the struct's layout, the refusal of every invalid pass before anything is enqueued
 *                                  (the pointers are never followed), and the empty calls with every pointer NULL.
 *   depth_head_smoke               the same, then ggr_depth_head_forward and ggr_depth_head_backward over hipMalloc'd buffers:
 *                                  one camera, 5 rays, s = 4 buckets, one surface, 2 samples, sampled with given uniform numbers,
 *                                  opacity_exponent 1 — checked against the contract evaluated in double on the host:
 *                                  index = searchsorted(cdf, u, right), depth from the relative disparity, opacity =
 *                                  scale * npdf[index], coords = ray_xy + (sigmoid(xy_raw) - 0.5) * pixel, and the backward of
 *                                  the loss  sum(depth) + sum(opacity) + sum(coords). */
#include <hip/hip_runtime_api.h>
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

enum { R = 5, S = 4, SPP = 2, G = R * SPP, W = 2 * S, XS = 5 /* xy_raw rows are 5 floats apart */ };

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

static int close_to(float a, double b) { return fabs((double)a - b) <= 2e-5 * (1.0 + fabs(b)); }
static double sigm(double x) { return 1.0 / (1.0 + exp(-x)); }

static GgrDepthHeadPass base_pass(void) {
    GgrDepthHeadPass dp; memset(&dp, 0, sizeof dp);
    dp.struct_size = (int32_t)sizeof dp; dp.num_cameras = 1; dp.rays_per_camera = R; dp.num_buckets = S; dp.num_surfaces = 1;
    dp.samples_per_ray = SPP; dp.xy_raw_stride = XS; dp.opacity_exponent = 1.f; dp.opacity_scale = 0.5f; dp.inv_w = 1.f / 8.f;
    dp.inv_h = 1.f / 4.f; dp.debug = 1;
    return dp;
}

static int host_checks(void) {
    int bad = 0;
    if (sizeof(GgrDepthHeadPass) != 184 || offsetof(GgrDepthHeadPass, opacity_exponent) != 48 || offsetof(GgrDepthHeadPass, logits) != 64 ||
        offsetof(GgrDepthHeadPass, index) != 136 || offsetof(GgrDepthHeadPass, dL_dxy_raw) != 176) { fprintf(stderr, "GgrDepthHeadPass layout\n"); bad = 1; }
    GgrDepthHeadPass dp = base_pass();
    float* fake = (float*)(uintptr_t)256;   /* never followed: every pass below is refused, or empty */
    dp.logits = dp.xy_raw = dp.ray_xy = dp.near = dp.far = dp.u = fake; dp.out_depth = dp.out_opacity = dp.out_coords = fake;
    dp.index = (int32_t*)fake; dp.dL_dlogits = dp.dL_dxy_raw = fake;
#define REFUSED(fn, code, what, edit) do { GgrDepthHeadPass b = dp; edit; if (fn(&b, NULL) != (code) || !strstr(ggr_last_error(), "GgrDepthHeadPass")) \
        { fprintf(stderr, what " was not refused (%s)\n", ggr_last_error()); bad = 1; } } while (0)
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "struct_size 8", b.struct_size = 8);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_depth_head_backward, GGR_E_INVALID, "reserved2 = 1", b.reserved2 = 1);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "a negative size", b.rays_per_camera = -1);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "num_buckets = 0", b.num_buckets = 0);
    REFUSED(ggr_depth_head_forward, GGR_E_LIMIT, "num_buckets = 65", b.num_buckets = 65);
    REFUSED(ggr_depth_head_backward, GGR_E_LIMIT, "samples_per_ray = 17", b.samples_per_ray = 17);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "samples_per_ray > num_buckets, deterministic", (b.deterministic = 1, b.num_buckets = 1));
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "num_surfaces = 0", b.num_surfaces = 0);
    REFUSED(ggr_depth_head_forward, GGR_E_LIMIT, "65536 cameras", b.num_cameras = 65536);
    REFUSED(ggr_depth_head_forward, GGR_E_LIMIT, "2^31 Gaussians", (b.num_cameras = 40000, b.rays_per_camera = 40000));
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "xy_raw_stride = 1", b.xy_raw_stride = 1);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "a misaligned buffer", b.logits = (const float*)((const char*)fake + 2));
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "NULL logits", b.logits = NULL);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "NULL u in sampled mode", b.u = NULL);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "NULL index", b.index = NULL);
    REFUSED(ggr_depth_head_forward, GGR_E_INVALID, "NULL out_coords", b.out_coords = NULL);
    REFUSED(ggr_depth_head_backward, GGR_E_INVALID, "NULL dL_dlogits", b.dL_dlogits = NULL);
    REFUSED(ggr_depth_head_backward, GGR_E_INVALID, "NULL far", b.far = NULL);
    GgrDepthHeadPass e = base_pass();   /* every pointer NULL */
    e.num_cameras = 0;
    if (ggr_depth_head_forward(&e, NULL) != GGR_OK || ggr_depth_head_backward(&e, NULL) != GGR_OK) { fprintf(stderr, "C = 0: %s\n", ggr_last_error()); bad = 1; }
    e.num_cameras = 3; e.rays_per_camera = 0;
    if (ggr_depth_head_forward(&e, NULL) != GGR_OK || ggr_depth_head_backward(&e, NULL) != GGR_OK) { fprintf(stderr, "R = 0: %s\n", ggr_last_error()); bad = 1; }
    return bad;
}

int main(int argc, char** argv) {
    if (ggr_abi_version() != GGR_ABI_VERSION || GGR_ABI_VERSION != 11) { fprintf(stderr, "ABI version mismatch\n"); return 1; }
    int bad = host_checks();
    if (argc > 1 && strcmp(argv[1], "--host-only") == 0) {
        printf(bad ? "DEPTH HEAD C ABI HOST CHECKS FAILED\n" : "DEPTH HEAD C ABI HOST CHECKS OK\n");
        return bad;
    }

    float logits[R * W], xy[R * XS], ray_xy[R * 2], near_[1] = {0.8f}, far_[1] = {50.f}, u[G];
    for (int r = 0; r < R; r++) {
        for (int k = 0; k < W; k++) logits[r * W + k] = 0.5f * (float)((r * 5 + k * 3) % 7) - 1.5f;
        for (int k = 0; k < XS; k++) xy[r * XS + k] = 0.3f * (float)((r * 3 + k) % 5) - 0.6f;
        ray_xy[2 * r] = (0.5f + (float)r) / 8.f; ray_xy[2 * r + 1] = 0.375f;
        u[2 * r] = 0.13f + 0.17f * (float)r; u[2 * r + 1] = 0.9999999f;   /* the second sample: above every boundary, clipped to S - 1 */
    }
    float ones[2 * G];
    for (int i = 0; i < 2 * G; i++) ones[i] = 1.f;
    float *d_logits = upload(logits, sizeof logits), *d_xy = upload(xy, sizeof xy), *d_ray = upload(ray_xy, sizeof ray_xy);
    float *d_near = upload(near_, sizeof near_), *d_far = upload(far_, sizeof far_), *d_u = upload(u, sizeof u), *d_ones = upload(ones, sizeof ones);
    /* both calls write their outputs whole: nothing is cleared for them */
    float *o_depth = device_bytes(G * 4, 0x7F), *o_op = device_bytes(G * 4, 0x7F), *o_coords = device_bytes(2 * G * 4, 0x7F);
    int32_t* o_index = device_bytes(G * 4, 0x7F);
    float *g_logits = device_bytes(sizeof logits, 0x7F), *g_xy = device_bytes(R * 2 * 4, 0x7F);
    if (!d_logits || !d_xy || !d_ray || !d_near || !d_far || !d_u || !d_ones || !o_depth || !o_op || !o_coords || !o_index || !g_logits || !g_xy) {
        fprintf(stderr, "allocation failed\n"); return 2;
    }
    GgrDepthHeadPass dp = base_pass();
    dp.logits = d_logits; dp.xy_raw = d_xy; dp.ray_xy = d_ray; dp.near = d_near; dp.far = d_far; dp.u = d_u;
    dp.out_depth = o_depth; dp.out_opacity = o_op; dp.out_coords = o_coords; dp.index = o_index;
    dp.dL_ddepth = d_ones; dp.dL_dopacity = d_ones; dp.dL_dcoords = d_ones; dp.dL_dlogits = g_logits; dp.dL_dxy_raw = g_xy;
    if (ggr_depth_head_forward(&dp, NULL) != GGR_OK) { fprintf(stderr, "depth head forward: %s\n", ggr_last_error()); return 1; }
    if (ggr_depth_head_backward(&dp, NULL) != GGR_OK) { fprintf(stderr, "depth head backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());

    float depth[G], op[G], coords[2 * G], gl[R * W], gxy[R * 2];
    int32_t index[G];
    CHECK(hipMemcpy(depth, o_depth, sizeof depth, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(op, o_op, sizeof op, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(coords, o_coords, sizeof coords, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(index, o_index, sizeof index, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(gl, g_logits, sizeof gl, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(gxy, g_xy, sizeof gxy, hipMemcpyDeviceToHost));
    const double dn = 1.0 / (0.8f + 1e-10), df = 1.0 / (50.0 + 1e-10), scale = 0.5;
    for (int r = 0; r < R; r++) {
        double pdf[S], m = -1e30, z = 0, sum = 0, cdf = 0, gp[S] = {0}, goff[S] = {0}, dot = 0;
        for (int d = 0; d < S; d++) m = fmax(m, logits[r * W + 2 * d]);
        for (int d = 0; d < S; d++) { pdf[d] = exp(logits[r * W + 2 * d] - m); z += pdf[d]; }
        for (int d = 0; d < S; d++) { pdf[d] /= z; sum += pdf[d]; }
        const double denom = (double)FLT_EPSILON + sum;
        for (int k = 0; k < SPP; k++) {
            int want = 0;
            cdf = 0;
            for (int d = 0; d < S; d++) { cdf += pdf[d] / denom; want += cdf <= (double)u[2 * r + k]; }
            if (want > S - 1) want = S - 1;
            const int p = r * SPP + k;
            if (index[p] != want) { fprintf(stderr, "index[%d] = %d, not %d\n", p, (int)index[p], want); bad = 1; continue; }
            const double sg = sigm(logits[r * W + 2 * want + 1]), rel = (want + sg) / S;
            const double dep = 1.0 / ((1.0 - rel) * (dn - df) + df + 1e-10), q = pdf[want] / denom;
            if (!close_to(depth[p], dep)) { fprintf(stderr, "depth[%d] = %g, not %g\n", p, depth[p], dep); bad = 1; }
            if (!close_to(op[p], scale * q)) { fprintf(stderr, "opacity[%d] = %g, not %g\n", p, op[p], scale * q); bad = 1; }
            const double cx = ray_xy[2 * r] + (sigm(xy[r * XS]) - 0.5) / 8.0, cy = ray_xy[2 * r + 1] + (sigm(xy[r * XS + 1]) - 0.5) / 4.0;
            if (!close_to(coords[2 * p], cx) || !close_to(coords[2 * p + 1], cy)) { fprintf(stderr, "coords[%d] = %g %g\n", p, coords[2 * p], coords[2 * p + 1]); bad = 1; }
            /* the loss is the sum of all outputs: every upstream gradient is 1 */
            goff[want] += (dn - df) * dep * dep * sg * (1.0 - sg) / S;
            gp[want] += scale / denom;
            for (int d = 0; d < S; d++) gp[d] -= scale * pdf[want] / (denom * denom);
        }
        for (int d = 0; d < S; d++) dot += pdf[d] * gp[d];
        for (int d = 0; d < S; d++) {
            if (!close_to(gl[r * W + 2 * d], pdf[d] * (gp[d] - dot))) { fprintf(stderr, "dL_dlogits pdf [%d][%d] = %g, not %g\n", r, d, gl[r * W + 2 * d], pdf[d] * (gp[d] - dot)); bad = 1; }
            if (!close_to(gl[r * W + 2 * d + 1], goff[d])) { fprintf(stderr, "dL_dlogits offset [%d][%d] = %g, not %g\n", r, d, gl[r * W + 2 * d + 1], goff[d]); bad = 1; }
        }
        for (int i = 0; i < 2; i++) {
            const double sg = sigm(xy[r * XS + i]), want = SPP * sg * (1.0 - sg) * (i ? 0.25 : 0.125);
            if (!close_to(gxy[2 * r + i], want)) { fprintf(stderr, "dL_dxy_raw[%d][%d] = %g, not %g\n", r, i, gxy[2 * r + i], want); bad = 1; }
        }
    }
    printf(bad ? "DEPTH HEAD C ABI SMOKE FAILED\n" : "DEPTH HEAD C ABI SMOKE OK\n");
    return bad;
}

/* adapter_smoke.c — the Gaussian adapter pass driven from plain C (no Python, no torch): ggr_adapter_forward and
 * ggr_adapter_backward over hipMalloc'd buffers.  One camera at the identity pose with identity intrinsics inverse and an identity
 * sh_transform, 5 Gaussians on 5 raw rows, d_sh = 4: the outputs have closed forms — means = normalize(x, y, 1)·depth, harmonics =
 * mask ⊙ raw_sh, quats = the normalised quaternion as (w,x,y,z) — and so has the backward of the loss Σ harmonics + Σ means.z:
 * dL/draw_sh = mask, dL/ddepth = u.z, dL/dc2w's translation column = (0, 0, P), dL/dsh_transform[i][j] = Σ mask_j·raw_sh[j] over
 * the block.  Invalid passes are refused first. */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

static float* upload(const float* h, size_t n) {
    float* d = NULL;
    if (hipMalloc((void**)&d, n * sizeof(float)) != hipSuccess) return NULL;
    hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice);
    return d;
}

static float* device_floats(size_t n, int byte) {
    float* d = NULL;
    if (hipMalloc((void**)&d, n * sizeof(float)) != hipSuccess) return NULL;
    hipMemset(d, byte, n * sizeof(float));
    return d;
}

static int near(float a, float b) { return fabsf(a - b) <= 1e-5f * (1.f + fabsf(b)); }

int main(void) {
    if (ggr_abi_version() != GGR_ABI_VERSION) { fprintf(stderr, "ABI version mismatch\n"); return 1; }
    enum { P = 5, DSH = 4, W = 7 + 3 * DSH };
    float depth[P], coords[P * 2], raw[P * W], c2w[12] = {1,0,0,0, 0,1,0,0, 0,0,1,0}, kinv[9] = {1,0,0, 0,1,0, 0,0,1};
    float qcam[4] = {1, 0, 0, 0}, mult[1] = {0.01f}, sht[DSH * DSH], mask[DSH] = {1.f, 0.025f, 0.025f, 0.025f};
    for (int i = 0; i < DSH * DSH; i++) sht[i] = (i / DSH == i % DSH) ? 1.f : 0.f;
    for (int p = 0; p < P; p++) {
        depth[p] = 2.f + 0.5f * (float)p; coords[2 * p] = 0.125f * (float)p - 0.25f; coords[2 * p + 1] = 0.5f - 0.125f * (float)p;
        for (int k = 0; k < W; k++) raw[p * W + k] = 0.25f * (float)((p * 7 + k * 3) % 11) - 1.f;
        raw[p * W + 6] = 1.5f;   /* a quaternion that is never zero */
    }
    float *d_depth = upload(depth, P), *d_coords = upload(coords, 2 * P), *d_raw = upload(raw, P * W), *d_c2w = upload(c2w, 12);
    float *d_kinv = upload(kinv, 9), *d_q = upload(qcam, 4), *d_mult = upload(mult, 1), *d_sht = upload(sht, DSH * DSH), *d_mask = upload(mask, DSH);
    /* the forward writes every element: nothing is cleared for it; the per-camera gradients are added into: zeroed */
    float *o_means = device_floats(P * 3, 0x7F), *o_scales = device_floats(P * 3, 0x7F), *o_quats = device_floats(P * 4, 0x7F), *o_harm = device_floats(P * 3 * DSH, 0x7F);
    float *g_raw = device_floats(P * W, 0x7F), *g_depth = device_floats(P, 0x7F), *g_c2w = device_floats(12, 0), *g_sht = device_floats(DSH * DSH, 0);
    float ones_h[P * 3 * DSH], gm_h[P * 3], zeros_h[P * 4] = {0};
    for (int i = 0; i < P * 3 * DSH; i++) ones_h[i] = 1.f;
    for (int i = 0; i < P * 3; i++) gm_h[i] = (i % 3 == 2) ? 1.f : 0.f;
    float *g_harm = upload(ones_h, P * 3 * DSH), *g_means = upload(gm_h, P * 3), *g_scales = upload(zeros_h, P * 3), *g_quats = upload(zeros_h, P * 4);
    if (!d_depth || !d_mask || !o_harm || !g_sht || !g_quats) { fprintf(stderr, "allocation failed\n"); return 2; }

    GgrAdapterPass ap; memset(&ap, 0, sizeof ap);
    ap.struct_size = (int32_t)sizeof ap; ap.num_cameras = 1; ap.gaussians_per_camera = P; ap.samples_per_row = 1; ap.d_sh = DSH;
    ap.scale_min = 0.5f; ap.scale_max = 15.f; ap.eps = 1e-8f; ap.debug = 1;
    ap.depth = d_depth; ap.coords = d_coords; ap.raw = d_raw; ap.c2w = d_c2w; ap.Kinv = d_kinv; ap.q_cam = d_q; ap.scale_mult = d_mult;
    ap.sh_transform = d_sht; ap.sh_mask = d_mask;
    ap.out_means = o_means; ap.out_scales = o_scales; ap.out_quats = o_quats; ap.out_harmonics = o_harm;
    ap.dL_dmeans = g_means; ap.dL_dscales = g_scales; ap.dL_dquats = g_quats; ap.dL_dharmonics = g_harm;
    ap.dL_draw = g_raw; ap.dL_ddepth = g_depth; ap.dL_dc2w = g_c2w; ap.dL_dsh_transform = g_sht;   /* the other gradients: NULL, skipped */
    int bad = 0;
#define REFUSED(fn, what, edit) do { GgrAdapterPass b = ap; edit; if (fn(&b, NULL) != GGR_E_INVALID) { fprintf(stderr, what " was not refused\n"); bad = 1; } } while (0)
    REFUSED(ggr_adapter_forward, "struct_size 8", b.struct_size = 8);
    REFUSED(ggr_adapter_forward, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_adapter_forward, "d_sh = 5", b.d_sh = 5);
    REFUSED(ggr_adapter_forward, "samples_per_row = 2", b.samples_per_row = 2);
    REFUSED(ggr_adapter_forward, "NULL raw", b.raw = NULL);
    REFUSED(ggr_adapter_forward, "NULL out_harmonics", b.out_harmonics = NULL);
    REFUSED(ggr_adapter_forward, "a misaligned buffer", b.depth = (const float*)((const char*)d_depth + 2));
    REFUSED(ggr_adapter_backward, "NULL dL_draw", b.dL_draw = NULL);
    REFUSED(ggr_adapter_backward, "NULL dL_dquats", b.dL_dquats = NULL);

    if (ggr_adapter_forward(&ap, NULL) != GGR_OK) { fprintf(stderr, "adapter forward: %s\n", ggr_last_error()); return 1; }
    if (ggr_adapter_backward(&ap, NULL) != GGR_OK) { fprintf(stderr, "adapter backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());

    float means[P * 3], scales[P * 3], quats[P * 4], harm[P * 3 * DSH], draw[P * W], ddepth[P], dc2w[12], dsht[DSH * DSH];
    CHECK(hipMemcpy(means, o_means, sizeof means, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(scales, o_scales, sizeof scales, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(quats, o_quats, sizeof quats, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(harm, o_harm, sizeof harm, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(draw, g_raw, sizeof draw, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(ddepth, g_depth, sizeof ddepth, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(dc2w, g_c2w, sizeof dc2w, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(dsht, g_sht, sizeof dsht, hipMemcpyDeviceToHost));
    float want_dsht[DSH * DSH] = {0};
    for (int p = 0; p < P; p++) {
        const float x = coords[2 * p], y = coords[2 * p + 1], n = sqrtf(x * x + y * y + 1.f);
        const float u[3] = {x / n, y / n, 1.f / n};
        const float* r = raw + p * W;
        const float nq = sqrtf(r[3] * r[3] + r[4] * r[4] + r[5] * r[5] + r[6] * r[6]) + 1e-8f;
        const float wq[4] = {r[6] / nq, r[3] / nq, r[4] / nq, r[5] / nq};
        for (int i = 0; i < 3; i++) {
            if (!near(means[3 * p + i], u[i] * depth[p])) { fprintf(stderr, "means[%d][%d] = %g\n", p, i, means[3 * p + i]); bad = 1; }
            const float s = (0.5f + 14.5f / (1.f + expf(-r[i]))) * depth[p] * 0.01f;
            if (!near(scales[3 * p + i], s)) { fprintf(stderr, "scales[%d][%d] = %g, not %g\n", p, i, scales[3 * p + i], s); bad = 1; }
        }
        for (int i = 0; i < 4; i++)
            if (!near(quats[4 * p + i], wq[i])) { fprintf(stderr, "quats[%d][%d] = %g, not %g\n", p, i, quats[4 * p + i], wq[i]); bad = 1; }
        for (int ch = 0; ch < 3; ch++)
            for (int k = 0; k < DSH; k++) {
                const float xs = mask[k] * r[7 + ch * DSH + k];
                if (!near(harm[(p * 3 + ch) * DSH + k], xs)) { fprintf(stderr, "harmonics[%d][%d][%d] = %g\n", p, ch, k, harm[(p * 3 + ch) * DSH + k]); bad = 1; }
                if (!near(draw[p * W + 7 + ch * DSH + k], mask[k])) { fprintf(stderr, "dL_draw sh [%d][%d][%d] = %g\n", p, ch, k, draw[p * W + 7 + ch * DSH + k]); bad = 1; }
                /* dL/dD[i][j] = Σ g_i·x_j with g = 1, within the block of j */
                for (int i = 0; i < DSH; i++)
                    if ((i == 0) == (k == 0)) want_dsht[i * DSH + k] += xs;
            }
        if (!near(ddepth[p], u[2])) { fprintf(stderr, "dL_ddepth[%d] = %g, not %g\n", p, ddepth[p], u[2]); bad = 1; }
    }
    for (int i = 0; i < DSH * DSH; i++)
        if (!near(dsht[i], want_dsht[i])) { fprintf(stderr, "dL_dsh_transform[%d] = %g, not %g\n", i, dsht[i], want_dsht[i]); bad = 1; }
    if (!near(dc2w[3], 0.f) || !near(dc2w[7], 0.f) || !near(dc2w[11], (float)P)) { fprintf(stderr, "dL_dc2w translation = %g %g %g\n", dc2w[3], dc2w[7], dc2w[11]); bad = 1; }
    printf(bad ? "ADAPTER C ABI SMOKE FAILED\n" : "ADAPTER C ABI SMOKE OK\n");
    return bad;
}

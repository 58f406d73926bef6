/* epipolar_attn_smoke.c — the epipolar-attention pass driven from plain C (no Python, no torch).
 *   epipolar_attn_smoke --host-only   needs no GPU: the struct's layout, the refusal of invalid passes before anything is enqueued
 *                                     (the pointers are never followed) and the empty call with every pointer NULL.
 *   epipolar_attn_smoke               the same, then ggr_epipolar_attention_forward and _backward over hipMalloc'd buffers with
 *                                     closed-form answers.  Ray n's samples are z[n,s,c] = s + c/8 + n (exact in float32).
 *                                     Rays 0, 1: qk = 0, so every weight is 1/S and ctx is the mean of the samples,
 *                                     (S-1)/2 + c/8 + n; with dL/dctx = 1 the backward gives da[h,s] = sum_c z[s,c],
 *                                     dl = (da - mean_s da)/S = C*(s - (S-1)/2)/S, dL/dqk[h,c] = sum_s dl*z = C*(S*S-1)/12, and
 *                                     dL/dz[s,c] = H/S.
 *                                     Ray 2: qk[h,c] = L*(h+1) for c == 0 and 0 otherwise, so logit[h,s] = L*(h+1)*(s + 2) —
 *                                     known exactly — and the last sample dominates: attn[h,s] = r^(S-1-s)*(1-r)/(1-r^S) with
 *                                     r = exp(-L*(h+1)), ctx[h,c] = z[S-1,c] - sum_s attn[h,s]*(S-1-s). */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

enum { N = 3, S = 6, C = 8, H = 3 };
static const float L = 3.0f;

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

static GgrEpipolarAttnPass base_pass(void) {
    GgrEpipolarAttnPass ap; memset(&ap, 0, sizeof ap);
    ap.struct_size = (int32_t)sizeof ap; ap.N = N; ap.S = S; ap.C = C; ap.H = H;
    return ap;
}

static int host_checks(void) {
    int bad = 0;
    if (sizeof(GgrEpipolarAttnPass) != 88 || offsetof(GgrEpipolarAttnPass, N) != 8 || offsetof(GgrEpipolarAttnPass, H) != 20 ||
        offsetof(GgrEpipolarAttnPass, qk) != 24 || offsetof(GgrEpipolarAttnPass, attn) != 56 || offsetof(GgrEpipolarAttnPass, dL_dz) != 80)
        { fprintf(stderr, "GgrEpipolarAttnPass layout\n"); bad = 1; }
    GgrEpipolarAttnPass ap = base_pass();
    float* fake = (float*)(uintptr_t)256;   /* never followed: every pass below is refused, or empty */
    ap.qk = ap.z = ap.attn = ap.dL_dctx = fake; ap.out_ctx = ap.out_attn = ap.dL_dqk = ap.dL_dz = fake;
#define REFUSED(fn, what, edit) do { GgrEpipolarAttnPass b = ap; edit; if (fn(&b, NULL) != GGR_E_INVALID || !strstr(ggr_last_error(), "GgrEpipolarAttnPass")) \
        { fprintf(stderr, what " was not refused (%s)\n", ggr_last_error()); bad = 1; } } while (0)
    REFUSED(ggr_epipolar_attention_forward, "struct_size 8", b.struct_size = 8);
    REFUSED(ggr_epipolar_attention_backward, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_epipolar_attention_forward, "S = 0", b.S = 0);
    REFUSED(ggr_epipolar_attention_backward, "S = 65", b.S = 65);
    REFUSED(ggr_epipolar_attention_forward, "C = 0", b.C = 0);
    REFUSED(ggr_epipolar_attention_backward, "C = 257", b.C = 257);
    REFUSED(ggr_epipolar_attention_forward, "H = 0", b.H = 0);
    REFUSED(ggr_epipolar_attention_forward, "H = 9", b.H = 9);
    REFUSED(ggr_epipolar_attention_forward, "N = -1", b.N = -1);
    REFUSED(ggr_epipolar_attention_forward, "a misaligned buffer", b.z = (const float*)((const char*)fake + 2));
    REFUSED(ggr_epipolar_attention_forward, "NULL qk", b.qk = NULL);
    REFUSED(ggr_epipolar_attention_forward, "NULL out_attn", b.out_attn = NULL);
    REFUSED(ggr_epipolar_attention_backward, "NULL attn", b.attn = NULL);
    REFUSED(ggr_epipolar_attention_backward, "NULL dL_dz", b.dL_dz = NULL);
    GgrEpipolarAttnPass e = base_pass();   /* every pointer NULL */
    e.N = 0;
    if (ggr_epipolar_attention_forward(&e, NULL) != GGR_OK || ggr_epipolar_attention_backward(&e, NULL) != GGR_OK)
        { fprintf(stderr, "N = 0: %s\n", ggr_last_error()); bad = 1; }
    if (ggr_abi_version() != 11) { fprintf(stderr, "abi version\n"); bad = 1; }
    if (!bad) printf("EPIPOLAR ATTENTION C ABI HOST CHECKS OK\n");
    return bad;
}

static int close_to(const char* what, int i, double got, double want, double tol) {
    if (fabs(got - want) <= tol * fmax(1.0, fabs(want))) return 0;
    fprintf(stderr, "%s[%d] = %.9g, expected %.9g\n", what, i, got, want);
    return 1;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    if (argc > 1 && !strcmp(argv[1], "--host-only")) return 0;

    static float qk[N * H * C], z[N * S * C], ctx[N * H * C], attn[N * H * S], ones[N * H * C], g_qk[N * H * C], g_z[N * S * C];
    for (int n = 0; n < N; ++n)
        for (int s = 0; s < S; ++s)
            for (int c = 0; c < C; ++c) z[(n * S + s) * C + c] = (float)s + (float)c / 8.f + (float)n;
    for (int h = 0; h < H; ++h) qk[(2 * H + h) * C] = L * (float)(h + 1);
    for (int i = 0; i < N * H * C; ++i) ones[i] = 1.f;

    GgrEpipolarAttnPass ap = base_pass();
    ap.qk = upload(qk, sizeof qk); ap.z = upload(z, sizeof z); ap.dL_dctx = upload(ones, sizeof ones);
    ap.out_ctx = device_bytes(sizeof ctx, 0xff); ap.out_attn = device_bytes(sizeof attn, 0xff);
    ap.dL_dqk = device_bytes(sizeof g_qk, 0xff); ap.dL_dz = device_bytes(sizeof g_z, 0xff);
    if (!ap.qk || !ap.z || !ap.dL_dctx || !ap.out_ctx || !ap.out_attn || !ap.dL_dqk || !ap.dL_dz) { fprintf(stderr, "hipMalloc failed\n"); return 2; }
    ap.attn = ap.out_attn;
    if (ggr_epipolar_attention_forward(&ap, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    if (ggr_epipolar_attention_backward(&ap, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(ctx, ap.out_ctx, sizeof ctx, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(attn, ap.out_attn, sizeof attn, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_qk, ap.dL_dqk, sizeof g_qk, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_z, ap.dL_dz, sizeof g_z, hipMemcpyDeviceToHost));

    int bad = 0;
    const double tol = 2e-6;
    for (int n = 0; n < 2; ++n)          /* qk = 0: the mean of the samples */
        for (int h = 0; h < H; ++h) {
            for (int s = 0; s < S; ++s) bad |= close_to("attn", (n * H + h) * S + s, attn[(n * H + h) * S + s], 1.0 / S, 1e-7);
            for (int c = 0; c < C; ++c) {
                bad |= close_to("ctx", (n * H + h) * C + c, ctx[(n * H + h) * C + c], (S - 1) / 2.0 + c / 8.0 + n, tol);
                bad |= close_to("dL_dqk", (n * H + h) * C + c, g_qk[(n * H + h) * C + c], C * (S * S - 1) / 12.0, 1e-5);
            }
        }
    for (int i = 0; i < 2 * S * C; ++i) bad |= close_to("dL_dz", i, g_z[i], (double)H / S, tol);
    for (int h = 0; h < H; ++h) {        /* ray 2: the last sample dominates */
        const double r = exp(-(double)L * (h + 1));
        double lag = 0;
        for (int s = 0; s < S; ++s) {
            const double a = pow(r, S - 1 - s) * (1 - r) / (1 - pow(r, S));
            bad |= close_to("attn (one-hot)", (2 * H + h) * S + s, attn[(2 * H + h) * S + s], a, tol);
            lag += a * (S - 1 - s);
        }
        if (!(attn[(2 * H + h) * S + S - 1] > 0.94)) { fprintf(stderr, "head %d is not dominated by the last sample\n", h); bad = 1; }
        for (int c = 0; c < C; ++c) bad |= close_to("ctx (one-hot)", (2 * H + h) * C + c, ctx[(2 * H + h) * C + c], (S - 1) + c / 8.0 + 2 - lag, tol);
    }
    for (int i = 2 * S * C; i < N * S * C; ++i) if (!isfinite(g_z[i])) { fprintf(stderr, "dL_dz[%d] was not written\n", i); bad = 1; break; }
    for (int i = 2 * H * C; i < N * H * C; ++i) if (!isfinite(g_qk[i])) { fprintf(stderr, "dL_dqk[%d] was not written\n", i); bad = 1; break; }
    printf("ctx[0,0,0] = %.6f (mean), attn[2,0,S-1] = %.6f\n", ctx[0], attn[2 * H * S + S - 1]);
    if (bad) return 1;
    printf("EPIPOLAR ATTENTION C ABI SMOKE OK\n");
    return 0;
}

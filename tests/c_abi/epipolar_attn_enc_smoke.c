/* epipolar_attn_enc_smoke.c — the encoded epipolar-attention pass driven from plain C (no Python, no torch).
 *   epipolar_attn_enc_smoke --host-only   needs no GPU: the struct's layout, the refusal of invalid passes before anything is
 *                                         enqueued (the pointers are never followed) and the empty call with every pointer NULL.
 *   epipolar_attn_enc_smoke               the same, then ggr_epipolar_attention_encoded_forward and _backward over hipMalloc'd
 *                                         buffers with closed-form answers.  Two rays of S = 3 samples, C = 4 channels, H = 2 heads,
 *                                         two octaves (E = 4); f[n,s,c] = s + c/8 + n and d[n,s] = s/4 = 0, 1/4, 1/2, where the
 *                                         sines are 0 and +-1 (to 3e-7: F is float32(2 pi), not 2 pi):
 *                                             pe(0) = (0, 1, 0, 1)   pe(1/4) = (1, 0, 0, -1)   pe(1/2) = (0, -1, 0, 1)
 *                                         qk = qe = 0, so every weight is 1/3: ctx_f[h,c] = 1 + c/8 + n and ctx_e[h] = (1/3, 0, 0, 1/3).
 *                                         With dL/dctx_f = dL/dctx_e = 1: da[s] = sum_c f + sum_j pe_j = (2.75, 4.75, 8.75) + 4n,
 *                                         dl = (da - mean)/3 = (-8/9, -2/9, 10/9), dL/dqk[h,c] = sum_s dl*s = 2,
 *                                         dL/dqe[h] = sum_s dl*pe(d_s) = (-2/9, -2, 0, 4/9), dL/dfeatures = H/S, and
 *                                         dL/ddepth[s] = (H/S) F sum_k 2^k (cos - sin)(2 pi 2^k d_s) = (H/S) F (3, -3, 1). */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

enum { N = 2, S = 3, C = 4, H = 2, O = 2, E = 2 * O };
static const double F = 6.2831854820251465;

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

static GgrEpipolarAttnEncPass base_pass(void) {
    GgrEpipolarAttnEncPass ap; memset(&ap, 0, sizeof ap);
    ap.struct_size = (int32_t)sizeof ap; ap.N = N; ap.S = S; ap.C = C; ap.H = H; ap.num_octaves = O;
    return ap;
}

static int host_checks(void) {
    int bad = 0;
    if (sizeof(GgrEpipolarAttnEncPass) != 144 || offsetof(GgrEpipolarAttnEncPass, N) != 8 || offsetof(GgrEpipolarAttnEncPass, num_octaves) != 24 ||
        offsetof(GgrEpipolarAttnEncPass, qk) != 32 || offsetof(GgrEpipolarAttnEncPass, depth) != 56 || offsetof(GgrEpipolarAttnEncPass, attn) != 88 ||
        offsetof(GgrEpipolarAttnEncPass, dL_ddepth) != 136)
        { fprintf(stderr, "GgrEpipolarAttnEncPass layout\n"); bad = 1; }
    GgrEpipolarAttnEncPass ap = base_pass();
    float* fake = (float*)(uintptr_t)256;   /* never followed: every pass below is refused, or empty */
    ap.qk = ap.qe = ap.features = ap.depth = ap.attn = ap.dL_dctx_f = ap.dL_dctx_e = fake;
    ap.out_ctx_f = ap.out_ctx_e = ap.out_attn = ap.dL_dqk = ap.dL_dqe = ap.dL_dfeatures = ap.dL_ddepth = fake;
#define REFUSED(fn, what, edit) do { GgrEpipolarAttnEncPass b = ap; edit; if (fn(&b, NULL) != GGR_E_INVALID || !strstr(ggr_last_error(), "GgrEpipolarAttnEncPass")) \
        { fprintf(stderr, what " was not refused (%s)\n", ggr_last_error()); bad = 1; } } while (0)
    REFUSED(ggr_epipolar_attention_encoded_forward, "struct_size 88", b.struct_size = 88);
    REFUSED(ggr_epipolar_attention_encoded_backward, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_epipolar_attention_encoded_forward, "reserved2 = 1", b.reserved2 = 1);
    REFUSED(ggr_epipolar_attention_encoded_forward, "S = 0", b.S = 0);
    REFUSED(ggr_epipolar_attention_encoded_backward, "S = 65", b.S = 65);
    REFUSED(ggr_epipolar_attention_encoded_forward, "C = 0", b.C = 0);
    REFUSED(ggr_epipolar_attention_encoded_backward, "C = 257", b.C = 257);
    REFUSED(ggr_epipolar_attention_encoded_forward, "H = 0", b.H = 0);
    REFUSED(ggr_epipolar_attention_encoded_forward, "H = 9", b.H = 9);
    REFUSED(ggr_epipolar_attention_encoded_forward, "N = -1", b.N = -1);
    REFUSED(ggr_epipolar_attention_encoded_forward, "num_octaves = 0", b.num_octaves = 0);
    REFUSED(ggr_epipolar_attention_encoded_backward, "num_octaves = 17", b.num_octaves = 17);
    REFUSED(ggr_epipolar_attention_encoded_forward, "a misaligned buffer", b.depth = (const float*)((const char*)fake + 2));
    REFUSED(ggr_epipolar_attention_encoded_forward, "NULL qe", b.qe = NULL);
    REFUSED(ggr_epipolar_attention_encoded_forward, "NULL depth", b.depth = NULL);
    REFUSED(ggr_epipolar_attention_encoded_forward, "NULL out_ctx_e", b.out_ctx_e = NULL);
    REFUSED(ggr_epipolar_attention_encoded_backward, "NULL attn", b.attn = NULL);
    REFUSED(ggr_epipolar_attention_encoded_backward, "NULL dL_dqe", b.dL_dqe = NULL);
    REFUSED(ggr_epipolar_attention_encoded_backward, "NULL dL_dfeatures", b.dL_dfeatures = NULL);
    GgrEpipolarAttnEncPass e = base_pass();   /* every pointer NULL */
    e.N = 0;
    if (ggr_epipolar_attention_encoded_forward(&e, NULL) != GGR_OK || ggr_epipolar_attention_encoded_backward(&e, NULL) != GGR_OK)
        { fprintf(stderr, "N = 0: %s\n", ggr_last_error()); bad = 1; }
    if (ggr_abi_version() != 11) { fprintf(stderr, "abi version\n"); bad = 1; }
    if (!bad) printf("ENCODED EPIPOLAR ATTENTION C ABI HOST CHECKS OK\n");
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

    static float qk[N * H * C], qe[N * H * E], f[N * S * C], d[N * S], ctx_f[N * H * C], ctx_e[N * H * E], attn[N * H * S];
    static float ones_f[N * H * C], ones_e[N * H * E], g_qk[N * H * C], g_qe[N * H * E], g_f[N * S * C], g_d[N * S];
    for (int n = 0; n < N; ++n)
        for (int s = 0; s < S; ++s) {
            d[n * S + s] = (float)s / 4.f;
            for (int c = 0; c < C; ++c) f[(n * S + s) * C + c] = (float)s + (float)c / 8.f + (float)n;
        }
    for (int i = 0; i < N * H * C; ++i) ones_f[i] = 1.f;
    for (int i = 0; i < N * H * E; ++i) ones_e[i] = 1.f;

    GgrEpipolarAttnEncPass ap = base_pass();
    ap.qk = upload(qk, sizeof qk); ap.qe = upload(qe, sizeof qe); ap.features = upload(f, sizeof f); ap.depth = upload(d, sizeof d);
    ap.dL_dctx_f = upload(ones_f, sizeof ones_f); ap.dL_dctx_e = upload(ones_e, sizeof ones_e);
    ap.out_ctx_f = device_bytes(sizeof ctx_f, 0xff); ap.out_ctx_e = device_bytes(sizeof ctx_e, 0xff); ap.out_attn = device_bytes(sizeof attn, 0xff);
    ap.dL_dqk = device_bytes(sizeof g_qk, 0xff); ap.dL_dqe = device_bytes(sizeof g_qe, 0xff);
    ap.dL_dfeatures = device_bytes(sizeof g_f, 0xff); ap.dL_ddepth = device_bytes(sizeof g_d, 0xff);
    if (!ap.qk || !ap.qe || !ap.features || !ap.depth || !ap.dL_dctx_f || !ap.dL_dctx_e || !ap.out_ctx_f || !ap.out_ctx_e || !ap.out_attn ||
        !ap.dL_dqk || !ap.dL_dqe || !ap.dL_dfeatures || !ap.dL_ddepth) { fprintf(stderr, "hipMalloc failed\n"); return 2; }
    ap.attn = ap.out_attn;
    if (ggr_epipolar_attention_encoded_forward(&ap, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    if (ggr_epipolar_attention_encoded_backward(&ap, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(ctx_f, ap.out_ctx_f, sizeof ctx_f, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ctx_e, ap.out_ctx_e, sizeof ctx_e, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(attn, ap.out_attn, sizeof attn, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_qk, ap.dL_dqk, sizeof g_qk, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_qe, ap.dL_dqe, sizeof g_qe, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_f, ap.dL_dfeatures, sizeof g_f, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g_d, ap.dL_ddepth, sizeof g_d, hipMemcpyDeviceToHost));

    int bad = 0;
    const double tol = 2e-6;
    static const double want_ctx_e[E] = {1.0 / 3, 0, 0, 1.0 / 3}, want_g_qe[E] = {-2.0 / 9, -2, 0, 4.0 / 9}, want_g_d[S] = {3, -3, 1};
    for (int n = 0; n < N; ++n)
        for (int h = 0; h < H; ++h) {
            for (int s = 0; s < S; ++s) bad |= close_to("attn", (n * H + h) * S + s, attn[(n * H + h) * S + s], 1.0 / S, 1e-7);
            for (int c = 0; c < C; ++c) {
                bad |= close_to("ctx_f", (n * H + h) * C + c, ctx_f[(n * H + h) * C + c], 1 + c / 8.0 + n, tol);
                bad |= close_to("dL_dqk", (n * H + h) * C + c, g_qk[(n * H + h) * C + c], 2.0, 1e-5);
            }
            for (int j = 0; j < E; ++j) {
                bad |= close_to("ctx_e", (n * H + h) * E + j, ctx_e[(n * H + h) * E + j], want_ctx_e[j], tol);
                bad |= close_to("dL_dqe", (n * H + h) * E + j, g_qe[(n * H + h) * E + j], want_g_qe[j], 1e-5);
            }
        }
    for (int i = 0; i < N * S * C; ++i) bad |= close_to("dL_dfeatures", i, g_f[i], (double)H / S, tol);
    for (int i = 0; i < N * S; ++i) bad |= close_to("dL_ddepth", i, g_d[i], want_g_d[i % S] * F * H / S, 1e-5);
    printf("ctx_e[0,0,:] = %.6f %.6f %.6f %.6f, dL_ddepth[0,:] = %.5f %.5f %.5f\n", ctx_e[0], ctx_e[1], ctx_e[2], ctx_e[3], g_d[0], g_d[1], g_d[2]);
    if (bad) return 1;
    printf("ENCODED EPIPOLAR ATTENTION C ABI SMOKE OK\n");
    return 0;
}

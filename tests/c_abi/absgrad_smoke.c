/* absgrad_smoke.c — the absgrad pass driven from plain C (no Python, no torch): a training forward, then ggr_means2d_absgrad over
 * hipMalloc'd buffers.  Two isotropic Gaussians in the frame (one on the optical axis, one beside it) and one moved far off
 * screen, under a colour gradient whose sign alternates from pixel to pixel (a checkerboard), a depth and an alpha gradient: the
 * per-pixel terms of a footprint cancel in the signed sum and add up in the absolute one.  Checked: the return codes, absgrad >=
 * |grad| per element with absgrad > 2·|grad| for the Gaussians in the frame, exact zeros for the Gaussian off screen, that the
 * call writes every element, and that it gives the same absgrad without the optional outputs / gradients it can do without. */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

typedef struct { void* p[2]; int n; } Two;
static void* two_alloc(void* ctx, size_t bytes) {
    Two* t = (Two*)ctx;
    void* p = NULL;
    if (t->n >= 2 || hipMalloc(&p, bytes ? bytes : 256) != hipSuccess) return NULL;
    t->p[t->n++] = p;
    return p;
}

static float* upload(const float* h, size_t n) {
    float* d = NULL;
    if (hipMalloc((void**)&d, n * sizeof(float)) != hipSuccess) return NULL;
    hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice);
    return d;
}

int main(void) {
    if (ggr_abi_version() != GGR_ABI_VERSION) { fprintf(stderr, "ABI version mismatch\n"); return 1; }
    enum { W = 33, H = 17, P = 3, N = W * H };
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0.2f,0.5f,0.1f};
    float means[P*3] = {0,0,4,  0.8f,0.3f,3,  400,0,4};   /* Gaussian 2 is far off screen */
    float cov[P*6], colors[P*3] = {0.9f,0.1f,0.4f,  0.2f,0.8f,0.6f,  0.5f,0.5f,0.5f};
    for (int i = 0; i < P; i++) {
        const float c6[6] = {0.09f,0,0,0.09f,0,0.09f};
        memcpy(cov + 6*i, c6, sizeof c6);
    }
    float opac[P] = {0.6f, 0.7f, 0.9f};
    static float gC[3*N], gD[N], gA[N];
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const float s = ((x + y) & 1) ? -1.f : 1.f;
            gC[y*W + x] = s * 1e-3f; gC[N + y*W + x] = -s * 2e-3f; gC[2*N + y*W + x] = s * 0.5e-3f;
            gD[y*W + x] = s * 1e-4f; gA[y*W + x] = -s * 1e-3f;
        }
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_col = upload(colors,P*3), *d_op = upload(opac,P);
    float *d_gC = upload(gC,3*N), *d_gD = upload(gD,N), *d_gA = upload(gA,N);
    float *d_color, *d_depth, *d_abs, *d_grad, *d_abs2; int32_t* d_radii; void *d_geom, *d_img;
    CHECK(hipMalloc((void**)&d_color, 3*N*4)); CHECK(hipMalloc((void**)&d_depth, N*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc((void**)&d_abs, P*2*4)); CHECK(hipMalloc((void**)&d_grad, P*2*4)); CHECK(hipMalloc((void**)&d_abs2, P*2*4));
    /* the call writes every element: nothing is cleared here */
    CHECK(hipMemset(d_abs, 0x7F, P*2*4)); CHECK(hipMemset(d_grad, 0x7F, P*2*4)); CHECK(hipMemset(d_abs2, 0x7F, P*2*4));
    /* a training forward: the pass runs over buffers that kept the backward state */
    CHECK(hipMalloc(&d_geom, ggr_geom_bytes(P))); CHECK(hipMalloc(&d_img, ggr_image_bytes(W, H)));

    GgrSettings st; memset(&st, 0, sizeof st);
    st.image_height = H; st.image_width = W; st.num_points = P; st.tanfovx = tanx; st.tanfovy = tany; st.scale_modifier = 1.f;
    st.bg = d_bg; st.viewmatrix = d_view; st.projmatrix = d_proj; st.campos = d_cam;
    GgrForwardIn in; memset(&in, 0, sizeof in);
    in.means3D = d_means; in.colors_precomp = d_col; in.opacities = d_op; in.cov3D_precomp = d_cov;
    GgrForwardOut out; memset(&out, 0, sizeof out);
    out.out_color = d_color; out.radii = d_radii; out.out_depth = d_depth; out.geom_buffer = d_geom; out.image_buffer = d_img;
    Two mem; memset(&mem, 0, sizeof mem);
    if (ggr_forward(&st, &in, &out, two_alloc, &mem, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }

    GgrAbsgradPass ap; memset(&ap, 0, sizeof ap);
    ap.struct_size = (int32_t)sizeof ap;
    ap.geom_buffer = d_geom; ap.image_buffer = d_img; ap.binning_buffer = out.binning_buffer; ap.num_rendered = out.num_rendered;
    ap.out_color = d_color; ap.out_depth = d_depth; ap.dL_dout_color = d_gC; ap.dL_dout_depth = d_gD; ap.dL_dout_alpha = d_gA;
    ap.out_absgrad = d_abs; ap.out_grad = d_grad;
    int bad = 0;
    /* refused before anything runs */
    { GgrAbsgradPass b = ap; b.struct_size = 8; if (ggr_means2d_absgrad(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "struct_size 8 was not refused\n"); bad = 1; } }
    { GgrAbsgradPass b = ap; b.reserved = 1; if (ggr_means2d_absgrad(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "reserved = 1 was not refused\n"); bad = 1; } }
    { GgrAbsgradPass b = ap; b.out_absgrad = NULL; if (ggr_means2d_absgrad(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "a NULL out_absgrad was not refused\n"); bad = 1; } }
    { GgrAbsgradPass b = ap; b.out_depth = NULL; if (ggr_means2d_absgrad(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "a depth gradient without the depth plane was not refused\n"); bad = 1; } }
    { GgrAbsgradPass b = ap; b.dL_dout_color = NULL; if (ggr_means2d_absgrad(&st, NULL, &b, NULL) != GGR_E_INVALID || !strstr(ggr_last_error(), "dL_dout_color")) { fprintf(stderr, "a NULL dL_dout_color was not refused\n"); bad = 1; } }
    if (ggr_means2d_absgrad(&st, NULL, &ap, NULL) != GGR_OK) { fprintf(stderr, "absgrad: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    float h_abs[P*2], h_grad[P*2], h_abs2[P*2];
    CHECK(hipMemcpy(h_abs, d_abs, sizeof h_abs, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_grad, d_grad, sizeof h_grad, hipMemcpyDeviceToHost));
    for (int i = 0; i < P*2; i++) {
        if (!isfinite(h_abs[i]) || !isfinite(h_grad[i]) || h_abs[i] < 0.f) { fprintf(stderr, "element %d: absgrad %g grad %g\n", i, h_abs[i], h_grad[i]); bad = 1; }
        if (h_abs[i] < fabsf(h_grad[i]) * (1.f - 1e-5f)) { fprintf(stderr, "element %d: absgrad %g < |grad| %g\n", i, h_abs[i], fabsf(h_grad[i])); bad = 1; }
    }
    for (int i = 0; i < 4; i++)   /* the two Gaussians in the frame: the checkerboard cancels in the signed sum */
        if (!(h_abs[i] > 0.f) || !(h_abs[i] > 2.f * fabsf(h_grad[i]))) { fprintf(stderr, "element %d: absgrad %g, |grad| %g: no cancellation\n", i, h_abs[i], fabsf(h_grad[i])); bad = 1; }
    if (h_abs[4] != 0.f || h_abs[5] != 0.f || h_grad[4] != 0.f || h_grad[5] != 0.f) { fprintf(stderr, "the Gaussian off screen has a gradient\n"); bad = 1; }

    /* without the signed output: the same absgrad (up to the order of the atomics' additions) */
    ap.out_absgrad = d_abs2; ap.out_grad = NULL;
    if (ggr_means2d_absgrad(&st, NULL, &ap, NULL) != GGR_OK) { fprintf(stderr, "absgrad (no out_grad): %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h_abs2, d_abs2, sizeof h_abs2, hipMemcpyDeviceToHost));
    for (int i = 0; i < P*2; i++)
        if (fabsf(h_abs2[i] - h_abs[i]) > 1e-5f * h_abs[i]) { fprintf(stderr, "element %d: %g without out_grad, %g with\n", i, h_abs2[i], h_abs[i]); bad = 1; }
    /* a colour loss alone: the depth plane and the two optional gradients may be NULL */
    ap.out_depth = NULL; ap.dL_dout_depth = NULL; ap.dL_dout_alpha = NULL;
    if (ggr_means2d_absgrad(&st, NULL, &ap, NULL) != GGR_OK) { fprintf(stderr, "absgrad (colour only): %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h_abs2, d_abs2, sizeof h_abs2, hipMemcpyDeviceToHost));
    if (!(h_abs2[0] > 0.f) || h_abs2[0] == h_abs[0] || h_abs2[4] != 0.f) { fprintf(stderr, "colour only: %g (all three gradients: %g)\n", h_abs2[0], h_abs[0]); bad = 1; }
    /* no Gaussians: nothing to do */
    { GgrSettings s0 = st; s0.num_points = 0; if (ggr_means2d_absgrad(&s0, NULL, &ap, NULL) != GGR_OK) { fprintf(stderr, "P = 0: %s\n", ggr_last_error()); bad = 1; } }
    hipFree(mem.p[0]); hipFree(mem.p[1]);
    printf(bad ? "ABSGRAD C ABI SMOKE FAILED\n" : "ABSGRAD C ABI SMOKE OK (absgrad %g %g, grad %g %g)\n", h_abs[0], h_abs[1], h_grad[0], h_grad[1]);
    return bad;
}

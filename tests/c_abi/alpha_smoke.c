/* alpha_smoke.c — the accumulated-opacity plane through the C ABI from plain C (no Python, no torch): ggr_forward_ext writes
 * alpha = 1 − T beside the colour and ggr_backward_ext differentiates it, checked against the closed form of a single centred
 * Gaussian (as abi_smoke.c):
 *   alpha(centre pixel) = min(0.99, opacity)  (d = 0 there),  alpha = 0 where nothing is blended,
 *   d alpha(centre) / d opacity = G · T_final / (1 − α) = 1.
 * Build: gcc -std=c11 tests/c_abi/alpha_smoke.c -Iinclude -Lggrt_official_amd -lggr_raster -lamdhip64 -lm -o alpha_smoke */
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
    enum { W = 33, H = 17, P = 2 };
    /* the camera of abi_smoke.c: identity view down +z, tan(fovx/2) = 1, near 1, far 100 */
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0.25f, 0.5f, 0.75f};
    /* Gaussian 0: on the optical axis at z = 4, sigma 0.3, opacity 0.6; Gaussian 1: behind the camera (culled) */
    float means[P*3] = {0,0,4,  0,0,-3};
    float cov[P*6] = {0.09f,0,0,0.09f,0,0.09f,  0.09f,0,0,0.09f,0,0.09f};
    float colors[P*3] = {0.9f,0.1f,0.4f,  1,1,1};
    float opac[P] = {0.6f, 0.9f};
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_col = upload(colors,P*3), *d_op = upload(opac,P);
    float *d_color, *d_depth, *d_alpha; int32_t* d_radii; void *d_geom, *d_img;
    CHECK(hipMalloc((void**)&d_color, 3*W*H*4)); CHECK(hipMalloc((void**)&d_depth, W*H*4));
    CHECK(hipMalloc((void**)&d_alpha, W*H*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMemset(d_alpha, 0xFF, W*H*4));   /* NaN everywhere: every pixel must be written */
    CHECK(hipMalloc(&d_geom, ggr_geom_bytes(P))); CHECK(hipMalloc(&d_img, ggr_image_bytes(W, H)));

    GgrSettings st; memset(&st, 0, sizeof st);
    st.image_height = H; st.image_width = W; st.num_points = P;
    st.tanfovx = tanx; st.tanfovy = tany; st.scale_modifier = 1.f;
    st.bg = d_bg; st.viewmatrix = d_view; st.projmatrix = d_proj; st.campos = d_cam;
    GgrForwardIn in; memset(&in, 0, sizeof in);
    in.means3D = d_means; in.colors_precomp = d_col; in.opacities = d_op; in.cov3D_precomp = d_cov;
    GgrForwardOut out; memset(&out, 0, sizeof out);
    out.out_color = d_color; out.radii = d_radii; out.out_depth = d_depth; out.geom_buffer = d_geom; out.image_buffer = d_img;
    int bad = 0;

    /* a malformed extra struct is refused before anything is enqueued */
    GgrForwardExtra fx_bad; memset(&fx_bad, 0, sizeof fx_bad);
    fx_bad.struct_size = 4; fx_bad.out_alpha = d_alpha;
    Two none; memset(&none, 0, sizeof none);
    if (ggr_forward_ext(&st, NULL, &fx_bad, &in, &out, two_alloc, &none, NULL) != GGR_E_INVALID || none.n != 0) {
        fprintf(stderr, "a struct_size of 4 was not refused\n"); bad = 1;
    }

    GgrForwardExtra fx; memset(&fx, 0, sizeof fx);
    fx.struct_size = (int32_t)sizeof fx; fx.out_alpha = d_alpha;
    Two mem; memset(&mem, 0, sizeof mem);
    if (ggr_forward_ext(&st, NULL, &fx, &in, &out, two_alloc, &mem, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());

    static float h_color[3*W*H], h_alpha[W*H];
    CHECK(hipMemcpy(h_color, d_color, sizeof h_color, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_alpha, d_alpha, sizeof h_alpha, hipMemcpyDeviceToHost));
    const int cx = 16, cy = 8;   /* the pixel at the Gaussian's mean (abi_smoke.c) */
    const float alpha = 0.6f;
    if (fabsf(h_alpha[cy*W + cx] - alpha) > 1e-6f) { fprintf(stderr, "alpha(centre) = %f, want %f\n", h_alpha[cy*W + cx], alpha); bad = 1; }
    if (h_alpha[0] != 0.f) { fprintf(stderr, "alpha(corner) = %f, want 0\n", h_alpha[0]); bad = 1; }
    for (int i = 0; i < W*H; i++) {
        /* everywhere: colour = Σ c·α·T + (1 − alpha)·bg, and alpha is a number in [0, 1) */
        if (!(h_alpha[i] >= 0.f && h_alpha[i] < 1.f)) { fprintf(stderr, "alpha[%d] = %f\n", i, h_alpha[i]); bad = 1; break; }
    }
    for (int c = 0; c < 3; c++) {
        const float want = colors[c] * alpha + (1.f - alpha) * bg[c];
        const float got = h_color[c*W*H + cy*W + cx];
        if (fabsf(got - want) > 1e-5f) { fprintf(stderr, "channel %d: got %f want %f\n", c, got, want); bad = 1; }
    }

    /* backward of L = alpha(centre): dL/dcolour = 0 everywhere, dL/dalpha = 1 at the centre pixel only */
    static float h_zero[3*W*H], h_da[W*H];
    memset(h_zero, 0, sizeof h_zero); memset(h_da, 0, sizeof h_da);
    h_da[cy*W + cx] = 1.f;
    float *d_dL = upload(h_zero, 3*W*H), *d_da = upload(h_da, W*H);
    void* d_scratch; CHECK(hipMalloc(&d_scratch, ggr_backward_scratch_bytes(P)));
    float *g_means, *g_m2d, *g_col, *g_op, *g_cov;
    CHECK(hipMalloc((void**)&g_means, P*3*4)); CHECK(hipMalloc((void**)&g_m2d, P*3*4)); CHECK(hipMalloc((void**)&g_col, P*3*4));
    CHECK(hipMalloc((void**)&g_op, P*4)); CHECK(hipMalloc((void**)&g_cov, P*6*4));
    GgrBackwardIn bi; memset(&bi, 0, sizeof bi);
    bi.fwd = in; bi.radii = d_radii; bi.geom_buffer = d_geom; bi.image_buffer = d_img; bi.binning_buffer = out.binning_buffer;
    bi.num_rendered = out.num_rendered; bi.dL_dout_color = d_dL; bi.scratch = d_scratch;
    GgrBackwardOut bo; memset(&bo, 0, sizeof bo);
    bo.dL_dmeans3D = g_means; bo.dL_dmeans2D = g_m2d; bo.dL_dcolors_precomp = g_col; bo.dL_dopacities = g_op; bo.dL_dcov3D = g_cov;
    GgrBackwardExtra bx_bad; memset(&bx_bad, 0, sizeof bx_bad);
    bx_bad.struct_size = (int32_t)sizeof bx_bad; bx_bad.reserved = 1; bx_bad.dL_dout_alpha = d_da;
    if (ggr_backward_ext(&st, &bx_bad, &bi, &bo, NULL) != GGR_E_INVALID) { fprintf(stderr, "reserved = 1 was not refused\n"); bad = 1; }
    GgrBackwardExtra bx; memset(&bx, 0, sizeof bx);
    bx.struct_size = (int32_t)sizeof bx; bx.dL_dout_alpha = d_da;
    if (ggr_backward_ext(&st, &bx, &bi, &bo, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    float h_gcol[P*3], h_gop[P];
    CHECK(hipMemcpy(h_gcol, g_col, sizeof h_gcol, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_gop, g_op, sizeof h_gop, hipMemcpyDeviceToHost));
    if (fabsf(h_gop[0] - 1.f) > 1e-5f || h_gop[1] != 0.f) { fprintf(stderr, "dL/dopacity = %f %f, want 1 0\n", h_gop[0], h_gop[1]); bad = 1; }
    for (int c = 0; c < 6; c++) if (h_gcol[c] != 0.f) { fprintf(stderr, "dL/dcolour[%d] = %f, want 0\n", c, h_gcol[c]); bad = 1; }

    hipFree(mem.p[0]); hipFree(mem.p[1]);
    if (bad) return 1;
    printf("C ABI ALPHA OK: alpha(centre) %.6f, dL/dopacity %.6f\n", h_alpha[cy*W + cx], h_gop[0]);
    return 0;
}

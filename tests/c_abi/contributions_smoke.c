/* contributions_smoke.c — the contribution pass driven from plain C (no Python, no torch): forward, then ggr_contributions
 * over hipMalloc'd buffers, checked against the closed form of a single centred isotropic Gaussian of opacity 0.8 over
 * nothing (the scene of abi_smoke.c): T = 1 at every pixel, so with α(d) = 0.8·exp(−d²/(2σ²)) and σ² the 2D variance
 *   weight_max  = α(0) = 0.8 (the centre pixel),  pixel_count = #{pixel centres with α >= 1/255},  weight_sum = Σ of those α.
 * d² is an integer here and the threshold d² = 2σ²·ln(0.8·255) = 19.48 lies between 18 and 20: no pixel is near it.
 * The second Gaussian stands behind the camera: zeros. */
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
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0,0,0};
    float means[P*3] = {0,0,4,  0,0,-3};   /* Gaussian 1 is behind the camera (culled) */
    float cov[P*6] = {0.09f,0,0,0.09f,0,0.09f,  0.09f,0,0,0.09f,0,0.09f};
    float colors[P*3] = {0.9f,0.1f,0.4f,  1,1,1};
    float opac[P] = {0.8f, 0.9f};
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_col = upload(colors,P*3), *d_op = upload(opac,P);
    float *d_color, *d_depth, *d_sum, *d_max; int32_t *d_radii, *d_count; void *d_geom, *d_img;
    CHECK(hipMalloc((void**)&d_color, 3*W*H*4)); CHECK(hipMalloc((void**)&d_depth, W*H*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc((void**)&d_sum, P*4)); CHECK(hipMalloc((void**)&d_max, P*4)); CHECK(hipMalloc((void**)&d_count, P*4));
    CHECK(hipMemset(d_sum, 0xFF, P*4)); CHECK(hipMemset(d_max, 0xFF, P*4)); CHECK(hipMemset(d_count, 0xFF, P*4));   /* the call clears them */
    /* an inference forward: the smaller buffers serve */
    CHECK(hipMalloc(&d_geom, ggr_geom_bytes_inference(P, 1))); CHECK(hipMalloc(&d_img, ggr_image_bytes_inference(W, H, 1)));

    GgrSettings st; memset(&st, 0, sizeof st);
    st.image_height = H; st.image_width = W; st.num_points = P; st.tanfovx = tanx; st.tanfovy = tany; st.scale_modifier = 1.f;
    st.bg = d_bg; st.viewmatrix = d_view; st.projmatrix = d_proj; st.campos = d_cam;
    GgrForwardIn in; memset(&in, 0, sizeof in);
    in.means3D = d_means; in.colors_precomp = d_col; in.opacities = d_op; in.cov3D_precomp = d_cov;
    GgrForwardOut out; memset(&out, 0, sizeof out);
    out.out_color = d_color; out.radii = d_radii; out.out_depth = d_depth; out.geom_buffer = d_geom; out.image_buffer = d_img;
    out.no_backward = 1;
    Two mem; memset(&mem, 0, sizeof mem);
    if (ggr_forward(&st, &in, &out, two_alloc, &mem, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }

    GgrContributionPass cp; memset(&cp, 0, sizeof cp);
    cp.struct_size = (int32_t)sizeof cp;
    cp.geom_buffer = d_geom; cp.image_buffer = d_img; cp.binning_buffer = out.binning_buffer; cp.num_rendered = out.num_rendered;
    cp.out_weight_sum = d_sum; cp.out_weight_max = d_max; cp.out_pixel_count = d_count;
    int bad = 0;
    /* refused before anything runs */
    { GgrContributionPass b = cp; b.struct_size = 8; if (ggr_contributions(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "struct_size 8 was not refused\n"); bad = 1; } }
    { GgrContributionPass b = cp; b.reserved = 1; if (ggr_contributions(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "reserved = 1 was not refused\n"); bad = 1; } }
    { GgrContributionPass b = cp; b.out_weight_sum = NULL; b.out_weight_max = NULL; b.out_pixel_count = NULL;
      if (ggr_contributions(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "three NULL outputs were not refused\n"); bad = 1; } }
    { GgrContributionPass b = cp; b.geom_buffer = NULL; if (ggr_contributions(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "a NULL geom buffer was not refused\n"); bad = 1; } }
    if (ggr_contributions(&st, NULL, &cp, NULL) != GGR_OK) { fprintf(stderr, "contributions: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    float h_sum[P], h_max[P]; int32_t h_count[P];
    CHECK(hipMemcpy(h_sum, d_sum, sizeof h_sum, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));

    /* the closed form, in double: σ² = (focal/z)²·0.09 + 0.3 (the screen-space dilation), the mean at pixel (16, 8) */
    const double focal = 0.5 * W / tanx, var2d = (focal / 4.0) * (focal / 4.0) * 0.09 + 0.3;
    double want_sum = 0.0; int want_count = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double d2 = (double)((x - 16) * (x - 16) + (y - 8) * (y - 8)), a = 0.8 * exp(-0.5 * d2 / var2d);
            if (a >= 1.0 / 255.0) { want_count++; want_sum += a; }
        }
    if (fabsf(h_max[0] - 0.8f) > 1e-4f) { fprintf(stderr, "weight_max = %f, want 0.8\n", h_max[0]); bad = 1; }
    if (h_count[0] != want_count) { fprintf(stderr, "pixel_count = %d, want %d\n", (int)h_count[0], want_count); bad = 1; }
    if (fabs(h_sum[0] - want_sum) > 1e-4 * want_sum) { fprintf(stderr, "weight_sum = %f, want %f\n", h_sum[0], want_sum); bad = 1; }
    if (h_sum[1] != 0.f || h_max[1] != 0.f || h_count[1] != 0) { fprintf(stderr, "the culled Gaussian has contributions\n"); bad = 1; }

    /* one output alone: the others are not touched */
    CHECK(hipMemset(d_sum, 0xFF, P*4)); CHECK(hipMemset(d_max, 0xFF, P*4));
    cp.out_weight_sum = NULL; cp.out_weight_max = NULL;
    if (ggr_contributions(&st, NULL, &cp, NULL) != GGR_OK) { fprintf(stderr, "contributions (count only): %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    int32_t h_raw[P];
    CHECK(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_raw, d_sum, sizeof h_raw, hipMemcpyDeviceToHost));
    if (h_count[0] != want_count || h_count[1] != 0 || h_raw[0] != -1) { fprintf(stderr, "count-only call: %d %d %d\n", (int)h_count[0], (int)h_count[1], (int)h_raw[0]); bad = 1; }
    hipFree(mem.p[0]); hipFree(mem.p[1]);
    printf(bad ? "CONTRIBUTIONS C ABI SMOKE FAILED\n" : "CONTRIBUTIONS C ABI SMOKE OK (count %d, sum %f)\n", want_count, want_sum);
    return bad;
}

/* picks_smoke.c — the pick pass driven from plain C (no Python, no torch): forward, then ggr_pixel_picks and ggr_contributions
 * over hipMalloc'd buffers.  Four isotropic Gaussians on the optical axis (z = 4, 2, 5, 3 with opacities 0.3, 0.3, 0.9, 0.3)
 * and one behind the camera: the centre pixel (16, 8) sees α = opacity exactly, so in depth order T_before = 1, 0.7, 0.49,
 * 0.343 and w = 0.3, 0.21, 0.147, 0.3087 — the median is the z = 3 Gaussian (index 3), the dominant one the z = 5 Gaussian
 * (index 2), four entries are live; the corners see nothing.  Over the frame Σ count equals Σ out_pixel_count of the contribution
 * pass: the same integer from two kernels. */
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
    enum { W = 33, H = 17, P = 5, N = W * H };
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0,0,0};
    float means[P*3] = {0,0,4,  0,0,2,  0,0,5,  0,0,3,  0,0,-3};   /* Gaussian 4 is behind the camera (culled) */
    float cov[P*6], colors[P*3];
    for (int i = 0; i < P; i++) {
        const float c6[6] = {0.09f,0,0,0.09f,0,0.09f};
        memcpy(cov + 6*i, c6, sizeof c6);
        colors[3*i] = 0.9f; colors[3*i+1] = 0.1f; colors[3*i+2] = 0.4f;
    }
    float opac[P] = {0.3f, 0.3f, 0.9f, 0.3f, 0.9f};
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_col = upload(colors,P*3), *d_op = upload(opac,P);
    float *d_color, *d_depth, *d_mdepth, *d_mweight; int32_t *d_radii, *d_mindex, *d_xindex, *d_count, *d_pcount; void *d_geom, *d_img;
    CHECK(hipMalloc((void**)&d_color, 3*N*4)); CHECK(hipMalloc((void**)&d_depth, N*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc((void**)&d_mdepth, N*4)); CHECK(hipMalloc((void**)&d_mweight, N*4)); CHECK(hipMalloc((void**)&d_mindex, N*4));
    CHECK(hipMalloc((void**)&d_xindex, N*4)); CHECK(hipMalloc((void**)&d_count, N*4)); CHECK(hipMalloc((void**)&d_pcount, P*4));
    /* the call writes every element: nothing is cleared here */
    CHECK(hipMemset(d_mdepth, 0x7F, N*4)); CHECK(hipMemset(d_mweight, 0x7F, N*4)); CHECK(hipMemset(d_mindex, 0x7F, N*4));
    CHECK(hipMemset(d_xindex, 0x7F, N*4)); CHECK(hipMemset(d_count, 0x7F, N*4));
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

    GgrPickPass pp; memset(&pp, 0, sizeof pp);
    pp.struct_size = (int32_t)sizeof pp;
    pp.geom_buffer = d_geom; pp.image_buffer = d_img; pp.binning_buffer = out.binning_buffer; pp.num_rendered = out.num_rendered;
    pp.out_median_index = d_mindex; pp.out_median_depth = d_mdepth; pp.out_max_index = d_xindex; pp.out_max_weight = d_mweight;
    pp.out_count = d_count;
    int bad = 0;
    /* refused before anything runs */
    { GgrPickPass b = pp; b.struct_size = 8; if (ggr_pixel_picks(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "struct_size 8 was not refused\n"); bad = 1; } }
    { GgrPickPass b = pp; b.reserved = 1; if (ggr_pixel_picks(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "reserved = 1 was not refused\n"); bad = 1; } }
    { GgrPickPass b = pp; b.out_median_index = NULL; b.out_median_depth = NULL; b.out_max_index = NULL; b.out_max_weight = NULL; b.out_count = NULL;
      if (ggr_pixel_picks(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "five NULL outputs were not refused\n"); bad = 1; } }
    { GgrPickPass b = pp; b.geom_buffer = NULL; if (ggr_pixel_picks(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "a NULL geom buffer was not refused\n"); bad = 1; } }
    if (ggr_pixel_picks(&st, NULL, &pp, NULL) != GGR_OK) { fprintf(stderr, "pixel picks: %s\n", ggr_last_error()); return 1; }

    GgrContributionPass cp; memset(&cp, 0, sizeof cp);
    cp.struct_size = (int32_t)sizeof cp;
    cp.geom_buffer = d_geom; cp.image_buffer = d_img; cp.binning_buffer = out.binning_buffer; cp.num_rendered = out.num_rendered;
    cp.out_pixel_count = d_pcount;
    if (ggr_contributions(&st, NULL, &cp, NULL) != GGR_OK) { fprintf(stderr, "contributions: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    static float h_mdepth[N], h_mweight[N]; static int32_t h_mindex[N], h_xindex[N], h_count[N]; int32_t h_pcount[P];
    CHECK(hipMemcpy(h_mdepth, d_mdepth, sizeof h_mdepth, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_mweight, d_mweight, sizeof h_mweight, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_mindex, d_mindex, sizeof h_mindex, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_xindex, d_xindex, sizeof h_xindex, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_pcount, d_pcount, sizeof h_pcount, hipMemcpyDeviceToHost));

    const int c = 8 * W + 16;   /* the centre pixel */
    if (h_mindex[c] != 3 || h_mdepth[c] != 3.0f) { fprintf(stderr, "median: index %d depth %f, want 3 and 3.0\n", (int)h_mindex[c], h_mdepth[c]); bad = 1; }
    if (h_xindex[c] != 2 || fabsf(h_mweight[c] - 0.3087f) > 1e-4f) { fprintf(stderr, "dominant: index %d weight %f, want 2 and 0.3087\n", (int)h_xindex[c], h_mweight[c]); bad = 1; }
    if (h_count[c] != 4) { fprintf(stderr, "count = %d, want 4\n", (int)h_count[c]); bad = 1; }
    const int corners[4] = {0, W - 1, (H - 1) * W, H * W - 1};
    for (int k = 0; k < 4; k++) {
        const int i = corners[k];
        if (h_mindex[i] != -1 || h_xindex[i] != -1 || h_count[i] != 0 || h_mdepth[i] != 0.f || h_mweight[i] != 0.f) { fprintf(stderr, "corner %d is not empty\n", k); bad = 1; }
    }
    long sum_count = 0, sum_pcount = 0;
    for (int i = 0; i < N; i++) {
        sum_count += h_count[i];
        if (h_mindex[i] < -1 || h_mindex[i] > 3 || h_xindex[i] < -1 || h_xindex[i] > 3 || (h_count[i] == 0) != (h_mindex[i] == -1)) { fprintf(stderr, "pixel %d: index %d / %d, count %d\n", i, (int)h_mindex[i], (int)h_xindex[i], (int)h_count[i]); bad = 1; break; }
    }
    for (int i = 0; i < P; i++) sum_pcount += h_pcount[i];
    if (sum_count != sum_pcount || sum_count < 100) { fprintf(stderr, "sum of count %ld, sum of pixel_count %ld\n", sum_count, sum_pcount); bad = 1; }
    if (h_pcount[4] != 0) { fprintf(stderr, "the culled Gaussian has pixels\n"); bad = 1; }

    /* one output alone: the others are not touched */
    CHECK(hipMemset(d_mdepth, 0x7F, N*4));
    pp.out_median_index = NULL; pp.out_median_depth = NULL; pp.out_max_index = NULL; pp.out_max_weight = NULL;
    CHECK(hipMemset(d_count, 0x7F, N*4));
    if (ggr_pixel_picks(&st, NULL, &pp, NULL) != GGR_OK) { fprintf(stderr, "pixel picks (count only): %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    int32_t h_raw[2];
    CHECK(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_raw, d_mdepth, sizeof h_raw, hipMemcpyDeviceToHost));
    long again = 0;
    for (int i = 0; i < N; i++) again += h_count[i];
    if (again != sum_count || h_raw[0] != 0x7F7F7F7F) { fprintf(stderr, "count-only call: %ld %x\n", again, (unsigned)h_raw[0]); bad = 1; }
    hipFree(mem.p[0]); hipFree(mem.p[1]);
    printf(bad ? "PICKS C ABI SMOKE FAILED\n" : "PICKS C ABI SMOKE OK (sum of count %ld)\n", sum_count);
    return bad;
}

/* features_smoke.c — the feature pass driven from plain C (no Python, no torch): forward, ggr_features_forward,
 * ggr_features_backward, backward, over hipMalloc'd buffers, checked against the closed form of a single centred Gaussian
 * (the scene of abi_smoke.c): at the centre pixel α = opacity, T = 1, so
 *   feature_k = f_k·α (no background),  dL/df_k = α,  dL/dopacity = Σ_c (colour_c − bg_c) + Σ_k f_k
 * for an upstream gradient of 1 on every colour and feature channel of that pixel — the colour's and the features' terms
 * meet in the backward scratch. */
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
    enum { W = 33, H = 17, P = 2, K = 5 };
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0.25f, 0.5f, 0.75f};
    float means[P*3] = {0,0,4,  0,0,-3};   /* Gaussian 1 is behind the camera (culled) */
    float cov[P*6] = {0.09f,0,0,0.09f,0,0.09f,  0.09f,0,0,0.09f,0,0.09f};
    float colors[P*3] = {0.9f,0.1f,0.4f,  1,1,1};
    float opac[P] = {0.6f, 0.9f};
    float feats[P*K] = {0.5f,-1.25f,2.0f,0.125f,3.0f,  7,7,7,7,7};
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_col = upload(colors,P*3), *d_op = upload(opac,P);
    float *d_feats = upload(feats, P*K);
    float *d_color, *d_depth, *d_planes; int32_t* d_radii; void *d_geom, *d_img, *d_scratch;
    CHECK(hipMalloc((void**)&d_color, 3*W*H*4)); CHECK(hipMalloc((void**)&d_depth, W*H*4)); CHECK(hipMalloc((void**)&d_planes, K*W*H*4));
    CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc(&d_geom, ggr_geom_bytes(P))); CHECK(hipMalloc(&d_img, ggr_image_bytes(W, H)));
    CHECK(hipMalloc(&d_scratch, ggr_backward_scratch_bytes(P)));

    GgrSettings st; memset(&st, 0, sizeof st);
    st.image_height = H; st.image_width = W; st.num_points = P; st.tanfovx = tanx; st.tanfovy = tany; st.scale_modifier = 1.f;
    st.bg = d_bg; st.viewmatrix = d_view; st.projmatrix = d_proj; st.campos = d_cam;
    GgrForwardIn in; memset(&in, 0, sizeof in);
    in.means3D = d_means; in.colors_precomp = d_col; in.opacities = d_op; in.cov3D_precomp = d_cov;
    GgrForwardOut out; memset(&out, 0, sizeof out);
    out.out_color = d_color; out.radii = d_radii; out.out_depth = d_depth; out.geom_buffer = d_geom; out.image_buffer = d_img;
    out.backward_scratch = d_scratch;   /* cleared by the forward: both backward calls below are told so */
    Two mem; memset(&mem, 0, sizeof mem);
    if (ggr_forward(&st, &in, &out, two_alloc, &mem, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }

    GgrFeaturePass fp; memset(&fp, 0, sizeof fp);
    fp.struct_size = (int32_t)sizeof fp; fp.num_features = K; fp.features = d_feats;
    fp.geom_buffer = d_geom; fp.image_buffer = d_img; fp.binning_buffer = out.binning_buffer; fp.num_rendered = out.num_rendered;
    fp.out_features = d_planes;
    int bad = 0;
    /* refused before anything runs */
    { GgrFeaturePass b = fp; b.num_features = 33; if (ggr_features_forward(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "K = 33 was not refused\n"); bad = 1; } }
    { GgrFeaturePass b = fp; b.struct_size = 8; if (ggr_features_forward(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, "struct_size 8 was not refused\n"); bad = 1; } }
    if (ggr_features_forward(&st, NULL, &fp, NULL) != GGR_OK) { fprintf(stderr, "features_forward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    static float h_planes[K*W*H];
    CHECK(hipMemcpy(h_planes, d_planes, sizeof h_planes, hipMemcpyDeviceToHost));
    const int cx = 16, cy = 8;
    const float alpha = 0.6f;
    for (int k = 0; k < K; k++) {
        const float got = h_planes[k*W*H + cy*W + cx], want = feats[k] * alpha;
        if (fabsf(got - want) > 1e-5f) { fprintf(stderr, "feature %d: got %f want %f\n", k, got, want); bad = 1; }
        if (h_planes[k*W*H] != 0.f) { fprintf(stderr, "feature %d: the corner pixel is not zero\n", k); bad = 1; }
    }

    /* backward: 1 on every colour and feature channel of the centre pixel; features first, then ggr_backward */
    static float h_dL[3*W*H], h_dF[K*W*H];
    memset(h_dL, 0, sizeof h_dL); memset(h_dF, 0, sizeof h_dF);
    for (int c = 0; c < 3; c++) h_dL[c*W*H + cy*W + cx] = 1.f;
    for (int k = 0; k < K; k++) h_dF[k*W*H + cy*W + cx] = 1.f;
    float *d_dL = upload(h_dL, 3*W*H), *d_dF = upload(h_dF, K*W*H), *g_feats;
    CHECK(hipMalloc((void**)&g_feats, P*K*4));
    fp.dL_dout_features = d_dF; fp.dL_dfeatures = g_feats; fp.scratch = d_scratch; fp.scratch_zeroed = 1;
    if (ggr_features_backward(&st, NULL, &fp, NULL) != GGR_OK) { fprintf(stderr, "features_backward: %s\n", ggr_last_error()); return 1; }
    float *g_means, *g_m2d, *g_col, *g_op, *g_cov;
    CHECK(hipMalloc((void**)&g_means, P*3*4)); CHECK(hipMalloc((void**)&g_m2d, P*3*4)); CHECK(hipMalloc((void**)&g_col, P*3*4));
    CHECK(hipMalloc((void**)&g_op, P*4)); CHECK(hipMalloc((void**)&g_cov, P*6*4));
    GgrBackwardIn bi; memset(&bi, 0, sizeof bi);
    bi.fwd = in; bi.radii = d_radii; bi.geom_buffer = d_geom; bi.image_buffer = d_img; bi.binning_buffer = out.binning_buffer;
    bi.num_rendered = out.num_rendered; bi.dL_dout_color = d_dL; bi.scratch = d_scratch;
    bi.scratch_zeroed = 1;   /* the feature terms are in it: it must not be cleared again */
    GgrBackwardOut bo; memset(&bo, 0, sizeof bo);
    bo.dL_dmeans3D = g_means; bo.dL_dmeans2D = g_m2d; bo.dL_dcolors_precomp = g_col; bo.dL_dopacities = g_op; bo.dL_dcov3D = g_cov;
    if (ggr_backward(&st, &bi, &bo, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    float h_gf[P*K], h_gop[P], h_gcol[P*3];
    CHECK(hipMemcpy(h_gf, g_feats, sizeof h_gf, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_gop, g_op, sizeof h_gop, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_gcol, g_col, sizeof h_gcol, hipMemcpyDeviceToHost));
    float want_gop = 0.f;
    for (int c = 0; c < 3; c++) want_gop += colors[c] - bg[c];
    for (int k = 0; k < K; k++) want_gop += feats[k];
    for (int k = 0; k < K; k++) {
        if (fabsf(h_gf[k] - alpha) > 1e-6f) { fprintf(stderr, "dL/dfeature[%d] = %f, want %f\n", k, h_gf[k], alpha); bad = 1; }
        if (h_gf[K + k] != 0.f) { fprintf(stderr, "the culled Gaussian has a feature gradient\n"); bad = 1; }
    }
    for (int c = 0; c < 3; c++) if (fabsf(h_gcol[c] - alpha) > 1e-6f) { fprintf(stderr, "dL/dcolour[%d] = %f\n", c, h_gcol[c]); bad = 1; }
    if (fabsf(h_gop[0] - want_gop) > 2e-5f || h_gop[1] != 0.f) { fprintf(stderr, "dL/dopacity = %f %f, want %f 0\n", h_gop[0], h_gop[1], want_gop); bad = 1; }
    hipFree(mem.p[0]); hipFree(mem.p[1]);
    printf(bad ? "FEATURES C ABI SMOKE FAILED\n" : "FEATURES C ABI SMOKE OK\n");
    return bad;
}

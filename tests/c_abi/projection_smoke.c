/* projection_smoke.c — the projection pass driven from plain C (no Python, no torch): a training forward, ggr_projection,
 * ggr_projection_backward and ggr_backward over hipMalloc'd buffers.  Four Gaussians in front of the camera and one behind it
 * (culled: its row is invalid).  The loss is Σ g·field over the five float arrays with the fixed gradients g below — NaN on the
 * culled row, which must reach nothing.  The scratch is NOT cleared by anybody beforehand (filled with 0x7F here): the seeding
 * call gets scratch_zeroed = 0 and clears it, ggr_backward gets scratch_zeroed = 1, zero colour and depth gradients.
 * The six arrays and the gradients are printed as "name v v v …" lines (%.9g: float32 round trips); tests/test_projection_c_host.py
 * compares them with what the Python binding computes for the same inputs. */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ggr_raster.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)

typedef struct { void* p[2]; int n; int calls; } Two;
static void* two_alloc(void* ctx, size_t bytes) {
    Two* t = (Two*)ctx;
    void* p = NULL;
    t->calls++;
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

static int show(const char* name, const float* d, int n) {
    float h[64];
    if (n > 64 || hipMemcpy(h, d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    printf("%s", name);
    for (int i = 0; i < n; i++) printf(" %.9g", h[i]);
    printf("\n");
    return 0;
}

int main(void) {
    if (ggr_abi_version() != GGR_ABI_VERSION) { fprintf(stderr, "ABI version mismatch\n"); return 1; }
    enum { W = 33, H = 17, P = 5, N = W * H };
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0,0,0};
    float means[P*3] = {0.5f,0.25f,4,  -0.25f,0.125f,2,  1.0f,-0.5f,5,  0,0,3,  0,0,-3};   /* Gaussian 4 is behind the camera */
    float cov[P*6], colors[P*3], opac[P] = {0.3f, 0.5f, 0.9f, 0.7f, 0.9f};
    float g_m2d[P*2], g_depth[P], g_conic[P*3], g_op[P], g_col[P*3];
    for (int i = 0; i < P; i++) {
        const float c6[6] = {0.09f + 0.01f*i, 0.01f*i, 0, 0.06f, -0.005f*i, 0.09f};
        memcpy(cov + 6*i, c6, sizeof c6);
        for (int k = 0; k < 3; k++) { colors[3*i+k] = 0.125f * (float)(i + k + 1); g_conic[3*i+k] = 0.25f * (float)(k - 1) + 0.125f * (float)i; g_col[3*i+k] = 0.5f * (float)(i - k); }
        g_m2d[2*i] = 0.5f - 0.25f * (float)i; g_m2d[2*i+1] = 0.125f * (float)(i + 1);
        g_depth[i] = 1.0f - 0.5f * (float)i; g_op[i] = 0.75f * (float)(i + 1);
    }
    /* the culled row: NaN in every gradient */
    g_m2d[8] = g_m2d[9] = g_depth[4] = g_op[4] = NAN;
    for (int k = 0; k < 3; k++) g_conic[12+k] = g_col[12+k] = NAN;
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_colors = upload(colors,P*3), *d_opac = upload(opac,P);
    float *d_gm = upload(g_m2d,P*2), *d_gd = upload(g_depth,P), *d_gc = upload(g_conic,P*3), *d_go = upload(g_op,P), *d_gcol = upload(g_col,P*3);
    float *d_color, *d_depth, *d_zc, *d_zd; int32_t* d_radii; void *d_geom, *d_img, *d_scratch;
    float *o_m2d, *o_depth, *o_conic, *o_op, *o_col; uint8_t* o_valid;
    float *d_dmeans, *d_dm2d, *d_dcol, *d_dop, *d_dcov;
    CHECK(hipMalloc((void**)&d_color, 3*N*4)); CHECK(hipMalloc((void**)&d_depth, N*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc((void**)&d_zc, 3*N*4)); CHECK(hipMalloc((void**)&d_zd, N*4));
    CHECK(hipMemset(d_zc, 0, 3*N*4)); CHECK(hipMemset(d_zd, 0, N*4));
    CHECK(hipMalloc(&d_geom, ggr_geom_bytes(P))); CHECK(hipMalloc(&d_img, ggr_image_bytes(W, H)));
    CHECK(hipMalloc(&d_scratch, ggr_backward_scratch_bytes(P))); CHECK(hipMemset(d_scratch, 0x7F, ggr_backward_scratch_bytes(P)));
    CHECK(hipMalloc((void**)&o_m2d, P*2*4)); CHECK(hipMalloc((void**)&o_depth, P*4)); CHECK(hipMalloc((void**)&o_conic, P*3*4));
    CHECK(hipMalloc((void**)&o_op, P*4)); CHECK(hipMalloc((void**)&o_col, P*3*4)); CHECK(hipMalloc((void**)&o_valid, P));
    /* the call writes every element: nothing is cleared here */
    CHECK(hipMemset(o_m2d, 0x7F, P*2*4)); CHECK(hipMemset(o_depth, 0x7F, P*4)); CHECK(hipMemset(o_conic, 0x7F, P*3*4));
    CHECK(hipMemset(o_op, 0x7F, P*4)); CHECK(hipMemset(o_col, 0x7F, P*3*4)); CHECK(hipMemset(o_valid, 0x7F, P));
    CHECK(hipMalloc((void**)&d_dmeans, P*3*4)); CHECK(hipMalloc((void**)&d_dm2d, P*3*4)); CHECK(hipMalloc((void**)&d_dcol, P*3*4));
    CHECK(hipMalloc((void**)&d_dop, P*4)); CHECK(hipMalloc((void**)&d_dcov, P*6*4));

    GgrSettings st; memset(&st, 0, sizeof st);
    st.image_height = H; st.image_width = W; st.num_points = P; st.tanfovx = tanx; st.tanfovy = tany; st.scale_modifier = 1.f;
    st.bg = d_bg; st.viewmatrix = d_view; st.projmatrix = d_proj; st.campos = d_cam;
    GgrForwardIn in; memset(&in, 0, sizeof in);
    in.means3D = d_means; in.colors_precomp = d_colors; in.opacities = d_opac; in.cov3D_precomp = d_cov;
    GgrForwardOut out; memset(&out, 0, sizeof out);
    out.out_color = d_color; out.radii = d_radii; out.out_depth = d_depth; out.geom_buffer = d_geom; out.image_buffer = d_img;
    Two mem; memset(&mem, 0, sizeof mem);
    if (ggr_forward(&st, &in, &out, two_alloc, &mem, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }

    GgrProjectionPass pp; memset(&pp, 0, sizeof pp);
    pp.struct_size = (int32_t)sizeof pp; pp.geom_buffer = d_geom; pp.radii = d_radii;
    pp.out_means2d = o_m2d; pp.out_depth = o_depth; pp.out_conic = o_conic; pp.out_opacity = o_op; pp.out_color = o_col; pp.out_valid = o_valid;
    pp.dL_dmeans2d = d_gm; pp.dL_ddepth = d_gd; pp.dL_dconic = d_gc; pp.dL_dopacity = d_go; pp.dL_dcolor = d_gcol;
    pp.scratch = d_scratch; pp.scratch_zeroed = 0;
    int bad = 0;
#define REFUSED(fn, what, edit) do { GgrProjectionPass b = pp; edit; if (fn(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, what " was not refused\n"); bad = 1; } } while (0)
    REFUSED(ggr_projection, "struct_size 8", b.struct_size = 8);
    REFUSED(ggr_projection, "reserved = 1", b.reserved = 1);
    REFUSED(ggr_projection, "six NULL outputs", (b.out_means2d = NULL, b.out_depth = NULL, b.out_conic = NULL, b.out_opacity = NULL, b.out_color = NULL, b.out_valid = NULL));
    REFUSED(ggr_projection, "a NULL geom buffer", b.geom_buffer = NULL);
    REFUSED(ggr_projection, "NULL radii", b.radii = NULL);
    REFUSED(ggr_projection_backward, "five NULL gradients", (b.dL_dmeans2d = NULL, b.dL_ddepth = NULL, b.dL_dconic = NULL, b.dL_dopacity = NULL, b.dL_dcolor = NULL));
    REFUSED(ggr_projection_backward, "a NULL scratch", b.scratch = NULL);
    REFUSED(ggr_projection_backward, "reserved2 = 1", b.reserved2 = 1);

    const int allocs = mem.calls;
    if (ggr_projection(&st, NULL, &pp, NULL) != GGR_OK) { fprintf(stderr, "projection: %s\n", ggr_last_error()); return 1; }
    if (ggr_projection_backward(&st, NULL, &pp, NULL) != GGR_OK) { fprintf(stderr, "projection backward: %s\n", ggr_last_error()); return 1; }
    if (mem.calls != allocs) { fprintf(stderr, "the projection pass allocated\n"); bad = 1; }

    GgrBackwardIn bin; memset(&bin, 0, sizeof bin);
    bin.fwd = in; bin.radii = d_radii; bin.geom_buffer = d_geom; bin.image_buffer = d_img; bin.binning_buffer = out.binning_buffer;
    bin.num_rendered = out.num_rendered; bin.dL_dout_color = d_zc; bin.dL_dout_depth = d_zd; bin.scratch = d_scratch; bin.scratch_zeroed = 1;
    GgrBackwardOut bout; memset(&bout, 0, sizeof bout);
    bout.dL_dmeans3D = d_dmeans; bout.dL_dmeans2D = d_dm2d; bout.dL_dcolors_precomp = d_dcol; bout.dL_dopacities = d_dop; bout.dL_dcov3D = d_dcov;
    if (ggr_backward(&st, &bin, &bout, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());

    int32_t radii[P]; uint8_t valid[P]; float h_op[P], h_dop[P], h_dmeans[P*3];
    CHECK(hipMemcpy(radii, d_radii, sizeof radii, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(valid, o_valid, sizeof valid, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_op, o_op, sizeof h_op, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h_dop, d_dop, sizeof h_dop, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_dmeans, d_dmeans, sizeof h_dmeans, hipMemcpyDeviceToHost));
    printf("valid");
    for (int i = 0; i < P; i++) {
        printf(" %d", (int)valid[i]);
        if (valid[i] != (radii[i] > 0 ? 1 : 0)) { fprintf(stderr, "valid[%d] = %d with radius %d\n", i, (int)valid[i], (int)radii[i]); bad = 1; }
        /* the opacity the pixels see is the input's (no anti-aliasing), and d(Σ g·opacity)/d opacity = g on valid rows, 0 elsewhere */
        if (h_op[i] != (valid[i] ? opac[i] : 0.f)) { fprintf(stderr, "opacity[%d] = %g\n", i, h_op[i]); bad = 1; }
        if (h_dop[i] != (valid[i] ? g_op[i] : 0.f)) { fprintf(stderr, "dL_dopacities[%d] = %g\n", i, h_dop[i]); bad = 1; }
    }
    printf("\n");
    if (valid[4] != 0 || valid[0] != 1 || valid[3] != 1) { fprintf(stderr, "unexpected valid flags\n"); bad = 1; }
    for (int i = 0; i < P*3; i++) if (!isfinite(h_dmeans[i])) { fprintf(stderr, "dL_dmeans3D[%d] is not finite\n", i); bad = 1; }
    if (h_dmeans[12] != 0.f || h_dmeans[13] != 0.f || h_dmeans[14] != 0.f) { fprintf(stderr, "the culled row has a gradient\n"); bad = 1; }
    bad |= show("means2d", o_m2d, P*2) | show("depth", o_depth, P) | show("conic", o_conic, P*3) | show("opacity", o_op, P) | show("color", o_col, P*3);
    bad |= show("dL_dmeans3D", d_dmeans, P*3) | show("dL_dmeans2D", d_dm2d, P*3) | show("dL_dcolors_precomp", d_dcol, P*3);
    bad |= show("dL_dopacities", d_dop, P) | show("dL_dcov3D", d_dcov, P*6);
    hipFree(mem.p[0]); hipFree(mem.p[1]);
    printf(bad ? "PROJECTION C ABI SMOKE FAILED\n" : "PROJECTION C ABI SMOKE OK\n");
    return bad;
}

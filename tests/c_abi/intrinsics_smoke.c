/* intrinsics_smoke.c — the intrinsics gradient driven from plain C (no Python, no torch): ggr_backward_ext with a
 * GgrBackwardExtra2 (dL_dtanfov) on the scene of abi_smoke.c, checked against central finite differences of the forward in
 * tan(fov/2) (projmatrix held fixed: the pixel means do not depend on tanfov), and ggr_camera_setup /
 * ggr_camera_setup_backward on a camera whose answers are known in closed form:
 *   identity pose, near = 0.5 (scale 2), K = [[f,0,.5],[0,f,.5],[0,0,1]]:  tan(fov_x/2) = 0.5/f, so an upstream gradient of 1
 *   on it gives dL/dK[0][0] = -0.5/f^2 and, by symmetry, nothing for the principal point or f_y; an upstream gradient g on
 *   campos alone gives dL/dextrinsics[r][3] = scale * g[r] and nothing else. */
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

enum { W = 33, H = 17, P = 2 };
static const int PX = 19, PY = 10;   /* the loss: the three colour channels of this pixel, off the Gaussian's centre (16, 8) */

/* one forward with (tanx, tany); returns the loss, leaves the buffers for a backward */
static int forward(GgrSettings* st, const GgrForwardIn* in, GgrForwardOut* out, float tanx, float tany, double* loss) {
    st->tanfovx = tanx; st->tanfovy = tany;
    Two mem; memset(&mem, 0, sizeof mem);
    out->binning_buffer = NULL; out->num_rendered = 0;
    if (ggr_forward(st, in, out, two_alloc, &mem, NULL) != GGR_OK) { fprintf(stderr, "forward: %s\n", ggr_last_error()); return 1; }
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    static float h[3 * W * H];
    if (hipMemcpy(h, out->out_color, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    *loss = 0.0;
    for (int c = 0; c < 3; c++) *loss += h[c * W * H + PY * W + PX];
    hipFree(mem.p[0]);   /* the work area; the lists (mem.p[1]) stay for the backward (a few hundred bytes per call) */
    return 0;
}

int main(void) {
    if (ggr_abi_version() != GGR_ABI_VERSION) { fprintf(stderr, "ABI version mismatch\n"); return 1; }
    int bad = 0;
    const float tanx = 1.0f, tany = (float)H / (float)W;
    const float fxn = 0.5f / tanx, fyn = 0.5f / tany, zn = 1.f, zf = 100.f;
    float view[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    float proj[16] = {2*zn*fxn,0,0,0,  0,2*zn*fyn,0,0,  0,0,zf/(zf-zn),1,  0,0,-(zf*zn)/(zf-zn),0};
    float campos[3] = {0,0,0}, bg[3] = {0.25f, 0.5f, 0.75f};
    float means[P*3] = {0,0,4,  0,0,-3};   /* Gaussian 1 is behind the camera (culled) */
    float cov[P*6] = {0.09f,0.01f,0,0.16f,0,0.09f,  0.09f,0,0,0.09f,0,0.09f};
    float colors[P*3] = {0.9f,0.1f,0.4f,  1,1,1};
    float opac[P] = {0.6f, 0.9f};
    float *d_view = upload(view,16), *d_proj = upload(proj,16), *d_cam = upload(campos,3), *d_bg = upload(bg,3);
    float *d_means = upload(means,P*3), *d_cov = upload(cov,P*6), *d_col = upload(colors,P*3), *d_op = upload(opac,P);
    float *d_color, *d_depth; int32_t* d_radii; void *d_geom, *d_img, *d_scratch;
    CHECK(hipMalloc((void**)&d_color, 3*W*H*4)); CHECK(hipMalloc((void**)&d_depth, W*H*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc(&d_geom, ggr_geom_bytes(P))); CHECK(hipMalloc(&d_img, ggr_image_bytes(W, H)));
    CHECK(hipMalloc(&d_scratch, ggr_backward_scratch_bytes(P)));
    GgrSettings st; memset(&st, 0, sizeof st);
    st.image_height = H; st.image_width = W; st.num_points = P; st.scale_modifier = 1.f;
    st.bg = d_bg; st.viewmatrix = d_view; st.projmatrix = d_proj; st.campos = d_cam;
    GgrForwardIn in; memset(&in, 0, sizeof in);
    in.means3D = d_means; in.colors_precomp = d_col; in.opacities = d_op; in.cov3D_precomp = d_cov;
    GgrForwardOut out; memset(&out, 0, sizeof out);
    out.out_color = d_color; out.radii = d_radii; out.out_depth = d_depth; out.geom_buffer = d_geom; out.image_buffer = d_img;

    /* ---- finite differences of the forward in tan(fov/2) ---- */
    double lp, lm, fd[2];
    const float eps = 1e-2f;
    if (forward(&st, &in, &out, tanx + eps, tany, &lp) || forward(&st, &in, &out, tanx - eps, tany, &lm)) return 1;
    fd[0] = (lp - lm) / (2.0 * eps);
    if (forward(&st, &in, &out, tanx, tany + eps, &lp) || forward(&st, &in, &out, tanx, tany - eps, &lm)) return 1;
    fd[1] = (lp - lm) / (2.0 * eps);
    if (forward(&st, &in, &out, tanx, tany, &lp)) return 1;

    /* ---- the backward with dL_dtanfov ---- */
    static float h_dL[3*W*H];
    memset(h_dL, 0, sizeof h_dL);
    for (int c = 0; c < 3; c++) h_dL[c*W*H + PY*W + PX] = 1.f;
    float *d_dL = upload(h_dL, 3*W*H);
    float *g_means, *g_m2d, *g_col, *g_op, *g_cov, *g_view, *g_proj, *g_cam, *g_tf;
    CHECK(hipMalloc((void**)&g_means, P*3*4)); CHECK(hipMalloc((void**)&g_m2d, P*3*4)); CHECK(hipMalloc((void**)&g_col, P*3*4));
    CHECK(hipMalloc((void**)&g_op, P*4)); CHECK(hipMalloc((void**)&g_cov, P*6*4));
    CHECK(hipMalloc((void**)&g_view, 64)); CHECK(hipMalloc((void**)&g_proj, 64)); CHECK(hipMalloc((void**)&g_cam, 12));
    CHECK(hipMalloc((void**)&g_tf, 8));
    GgrBackwardIn bi; memset(&bi, 0, sizeof bi);
    bi.fwd = in; bi.radii = d_radii; bi.geom_buffer = d_geom; bi.image_buffer = d_img; bi.binning_buffer = out.binning_buffer;
    bi.num_rendered = out.num_rendered; bi.dL_dout_color = d_dL; bi.scratch = d_scratch;
    GgrBackwardOut bo; memset(&bo, 0, sizeof bo);
    bo.dL_dmeans3D = g_means; bo.dL_dmeans2D = g_m2d; bo.dL_dcolors_precomp = g_col; bo.dL_dopacities = g_op; bo.dL_dcov3D = g_cov;
    GgrBackwardExtra2 ex; memset(&ex, 0, sizeof ex);
    ex.struct_size = (int32_t)sizeof ex; ex.dL_dtanfov = g_tf;
    /* without the three camera gradient outputs: refused before anything runs */
    if (ggr_backward_ext(&st, (const GgrBackwardExtra*)&ex, &bi, &bo, NULL) != GGR_E_INVALID) { fprintf(stderr, "dL_dtanfov without the pose outputs was not refused\n"); bad = 1; }
    bo.dL_dviewmatrix = g_view; bo.dL_dprojmatrix = g_proj; bo.dL_dcampos = g_cam;
    /* the ABI-11 size: the field is absent, the call is ggr_backward's */
    { GgrBackwardExtra2 old = ex; old.struct_size = (int32_t)sizeof(GgrBackwardExtra);
      CHECK(hipMemset(g_tf, 0xff, 8));
      if (ggr_backward_ext(&st, (const GgrBackwardExtra*)&old, &bi, &bo, NULL) != GGR_OK) { fprintf(stderr, "backward (old size): %s\n", ggr_last_error()); return 1; }
      uint32_t w[2]; CHECK(hipMemcpy(w, g_tf, 8, hipMemcpyDeviceToHost));
      if (w[0] != 0xffffffffu || w[1] != 0xffffffffu) { fprintf(stderr, "a struct of the old size wrote dL_dtanfov\n"); bad = 1; } }
    if (ggr_backward_ext(&st, (const GgrBackwardExtra*)&ex, &bi, &bo, NULL) != GGR_OK) { fprintf(stderr, "backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    float h_tf[2];
    CHECK(hipMemcpy(h_tf, g_tf, 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; k++)
        if (!(fabs(fd[k]) > 1e-3) || fabs(h_tf[k] - fd[k]) > 1e-2 * fabs(fd[k])) { fprintf(stderr, "dL/dtanfov[%d] = %g, finite differences %g\n", k, h_tf[k], fd[k]); bad = 1; }

    /* ---- camera setup and its backward ---- */
    const float f = 0.8f, near = 0.5f, far = 50.f;
    float E[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1}, K[9] = {f,0,0.5f, 0,f,0.5f, 0,0,1};
    float *d_E = upload(E,16), *d_K = upload(K,9), *d_near = upload(&near,1), *d_far = upload(&far,1);
    float *o_view, *o_full, *o_cam, *o_tf, *o_scale, *g_E, *g_K;
    CHECK(hipMalloc((void**)&o_view, 64)); CHECK(hipMalloc((void**)&o_full, 64)); CHECK(hipMalloc((void**)&o_cam, 12));
    CHECK(hipMalloc((void**)&o_tf, 8)); CHECK(hipMalloc((void**)&o_scale, 4)); CHECK(hipMalloc((void**)&g_E, 64)); CHECK(hipMalloc((void**)&g_K, 36));
    if (ggr_camera_setup(1, d_E, d_K, d_near, d_far, 1, o_view, o_full, o_cam, o_tf, o_scale, NULL) != GGR_OK) { fprintf(stderr, "camera_setup: %s\n", ggr_last_error()); return 1; }
    float zeros16[16] = {0}, up_cam[3] = {1.f, 2.f, 3.f}, up_tf[2] = {1.f, 0.f}, zeros2[2] = {0.f, 0.f}, zeros3[3] = {0.f, 0.f, 0.f};
    float *u_zero16 = upload(zeros16,16), *u_cam = upload(up_cam,3), *u_tf = upload(up_tf,2), *u_zero2 = upload(zeros2,2), *u_zero3 = upload(zeros3,3);
    float h_E[16], h_K[9], h_otf[2];
    if (ggr_camera_setup_backward(1, d_E, d_K, d_near, d_far, 1, u_zero16, u_zero16, u_cam, u_zero2, g_E, g_K, NULL) != GGR_OK) { fprintf(stderr, "camera_setup_backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h_E, g_E, 64, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h_K, g_K, 36, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_otf, o_tf, 8, hipMemcpyDeviceToHost));
    if (fabsf(h_otf[0] - 0.5f / f) > 1e-6f) { fprintf(stderr, "tan(fov_x/2) = %f, want %f\n", h_otf[0], 0.5f / f); bad = 1; }
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const float want = (c == 3 && r < 3) ? 2.f * up_cam[r] : 0.f;
            if (fabsf(h_E[4*r + c] - want) > 1e-6f) { fprintf(stderr, "dL/dextrinsics[%d][%d] = %f, want %f\n", r, c, h_E[4*r + c], want); bad = 1; }
        }
    for (int k = 0; k < 9; k++) if (h_K[k] != 0.f) { fprintf(stderr, "dL/dintrinsics[%d] = %f without a gradient that reaches it\n", k, h_K[k]); bad = 1; }
    if (ggr_camera_setup_backward(1, d_E, d_K, d_near, d_far, 1, u_zero16, u_zero16, u_zero3, u_tf, g_E, g_K, NULL) != GGR_OK) { fprintf(stderr, "camera_setup_backward: %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h_K, g_K, 36, hipMemcpyDeviceToHost));
    if (fabsf(h_K[0] + 0.5f / (f * f)) > 1e-5f || fabsf(h_K[2]) > 1e-6f || fabsf(h_K[4]) > 1e-6f) { fprintf(stderr, "dL/dK = %f %f %f, want %f 0 0\n", h_K[0], h_K[2], h_K[4], -0.5f / (f * f)); bad = 1; }
    printf(bad ? "INTRINSICS C ABI SMOKE FAILED\n" : "INTRINSICS C ABI SMOKE OK\n");
    return bad;
}

/* hits_smoke.c — the hit pass driven from plain C (no Python, no torch): forward, then ggr_pixel_hits and ggr_pixel_picks over
 * hipMalloc'd buffers.  Four isotropic Gaussians on the optical axis (z = 4, 2, 5, 3 with opacities 0.3, 0.3, 0.9, 0.3) and one
 * behind the camera: the centre pixel (16, 8) sees α = opacity exactly, so in depth order — ids 1, 3, 0, 2 — T_before = 1, 0.7,
 * 0.49, 0.343 and w = 0.3, 0.21, 0.147, 0.3087.  With K = 2 the slots hold ids 1, 3 with w = 0.3, 0.21, the rest is 0.147 +
 * 0.3087 and the count 4; the corners see nothing.  Over the frame the count plane equals the pick pass's.  A call WITHOUT rest
 * and count finishes a pixel once it holds K entries: its index / weight equal the full call's byte for byte. */
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

int main(void) {
    if (ggr_abi_version() != GGR_ABI_VERSION) { fprintf(stderr, "ABI version mismatch\n"); return 1; }
    enum { W = 33, H = 17, P = 5, N = W * H, K = 2 };
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
    float *d_color, *d_depth, *d_weight, *d_weight2, *d_rest; int32_t *d_radii, *d_index, *d_index2, *d_count, *d_pcount; void *d_geom, *d_img;
    CHECK(hipMalloc((void**)&d_color, 3*N*4)); CHECK(hipMalloc((void**)&d_depth, N*4)); CHECK(hipMalloc((void**)&d_radii, P*4));
    CHECK(hipMalloc((void**)&d_index, K*N*4)); CHECK(hipMalloc((void**)&d_weight, K*N*4)); CHECK(hipMalloc((void**)&d_index2, K*N*4));
    CHECK(hipMalloc((void**)&d_weight2, K*N*4)); CHECK(hipMalloc((void**)&d_rest, N*4)); CHECK(hipMalloc((void**)&d_count, N*4));
    CHECK(hipMalloc((void**)&d_pcount, N*4));
    /* the call writes every element: nothing is cleared here */
    CHECK(hipMemset(d_index, 0x7F, K*N*4)); CHECK(hipMemset(d_weight, 0x7F, K*N*4)); CHECK(hipMemset(d_index2, 0x7F, K*N*4));
    CHECK(hipMemset(d_weight2, 0x7F, K*N*4)); CHECK(hipMemset(d_rest, 0x7F, N*4)); CHECK(hipMemset(d_count, 0x7F, N*4));
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

    GgrHitPass hp; memset(&hp, 0, sizeof hp);
    hp.struct_size = (int32_t)sizeof hp; hp.num_hits = K;
    hp.geom_buffer = d_geom; hp.image_buffer = d_img; hp.binning_buffer = out.binning_buffer; hp.num_rendered = out.num_rendered;
    hp.out_index = d_index; hp.out_weight = d_weight; hp.out_rest = d_rest; hp.out_count = d_count;
    int bad = 0;
    /* refused before anything is enqueued: the outputs keep their 0x7F fill (checked below, before the first good call) */
#define REFUSED(what, edit) do { GgrHitPass b = hp; edit; if (ggr_pixel_hits(&st, NULL, &b, NULL) != GGR_E_INVALID) { fprintf(stderr, what " was not refused\n"); bad = 1; } } while (0)
    REFUSED("struct_size 8", b.struct_size = 8);
    REFUSED("num_hits = 0", b.num_hits = 0);
    REFUSED("num_hits = GGR_MAX_HITS + 1", b.num_hits = GGR_MAX_HITS + 1);
    REFUSED("out_index alone NULL", b.out_index = NULL);
    REFUSED("out_weight alone NULL", b.out_weight = NULL);
    REFUSED("four NULL outputs", (b.out_index = NULL, b.out_weight = NULL, b.out_rest = NULL, b.out_count = NULL));
    REFUSED("a NULL geom buffer", b.geom_buffer = NULL);
    REFUSED("a NULL image buffer", b.image_buffer = NULL);
    REFUSED("a NULL binning buffer", b.binning_buffer = NULL);
    CHECK(hipDeviceSynchronize());
    {
        static int32_t raw[K*N]; int32_t raw1[2];
        CHECK(hipMemcpy(raw, d_index, sizeof raw, hipMemcpyDeviceToHost));
        for (int i = 0; i < K*N; i++) if (raw[i] != 0x7F7F7F7F) { fprintf(stderr, "a refused call wrote out_index[%d]\n", i); bad = 1; break; }
        CHECK(hipMemcpy(raw, d_weight, sizeof raw, hipMemcpyDeviceToHost));
        for (int i = 0; i < K*N; i++) if (raw[i] != 0x7F7F7F7F) { fprintf(stderr, "a refused call wrote out_weight[%d]\n", i); bad = 1; break; }
        CHECK(hipMemcpy(raw1, d_rest, sizeof raw1, hipMemcpyDeviceToHost));
        if (raw1[0] != 0x7F7F7F7F) { fprintf(stderr, "a refused call wrote out_rest\n"); bad = 1; }
        CHECK(hipMemcpy(raw1, d_count, sizeof raw1, hipMemcpyDeviceToHost));
        if (raw1[0] != 0x7F7F7F7F) { fprintf(stderr, "a refused call wrote out_count\n"); bad = 1; }
    }
    const int allocs = mem.calls;
    if (ggr_pixel_hits(&st, NULL, &hp, NULL) != GGR_OK) { fprintf(stderr, "pixel hits: %s\n", ggr_last_error()); return 1; }
    if (mem.calls != allocs) { fprintf(stderr, "the hit pass allocated\n"); bad = 1; }

    GgrPickPass pp; memset(&pp, 0, sizeof pp);
    pp.struct_size = (int32_t)sizeof pp;
    pp.geom_buffer = d_geom; pp.image_buffer = d_img; pp.binning_buffer = out.binning_buffer; pp.num_rendered = out.num_rendered;
    pp.out_count = d_pcount;
    if (ggr_pixel_picks(&st, NULL, &pp, NULL) != GGR_OK) { fprintf(stderr, "pixel picks: %s\n", ggr_last_error()); return 1; }
    /* the slots alone: a pixel is finished once it holds K entries */
    GgrHitPass h2 = hp; h2.out_index = d_index2; h2.out_weight = d_weight2; h2.out_rest = NULL; h2.out_count = NULL;
    if (ggr_pixel_hits(&st, NULL, &h2, NULL) != GGR_OK) { fprintf(stderr, "pixel hits (slots only): %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    static float h_weight[K*N], h_weight2[K*N], h_rest[N]; static int32_t h_index[K*N], h_index2[K*N], h_count[N], h_pcount[N];
    CHECK(hipMemcpy(h_index, d_index, sizeof h_index, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_weight, d_weight, sizeof h_weight, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_index2, d_index2, sizeof h_index2, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_weight2, d_weight2, sizeof h_weight2, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_rest, d_rest, sizeof h_rest, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_pcount, d_pcount, sizeof h_pcount, hipMemcpyDeviceToHost));

    const int c = 8 * W + 16;   /* the centre pixel */
    if (h_index[c] != 1 || h_index[N + c] != 3) { fprintf(stderr, "slots: ids %d %d, want 1 3\n", (int)h_index[c], (int)h_index[N + c]); bad = 1; }
    if (fabsf(h_weight[c] - 0.3f) > 1e-4f || fabsf(h_weight[N + c] - 0.21f) > 1e-4f) { fprintf(stderr, "slots: w %f %f, want 0.3 0.21\n", h_weight[c], h_weight[N + c]); bad = 1; }
    if (fabsf(h_rest[c] - (0.147f + 0.3087f)) > 1e-4f) { fprintf(stderr, "rest = %f, want 0.4557\n", h_rest[c]); bad = 1; }
    if (h_count[c] != 4) { fprintf(stderr, "count = %d, want 4\n", (int)h_count[c]); bad = 1; }
    const int corners[4] = {0, W - 1, (H - 1) * W, H * W - 1};
    for (int k = 0; k < 4; k++) {
        const int i = corners[k];
        if (h_index[i] != -1 || h_index[N + i] != -1 || h_weight[i] != 0.f || h_weight[N + i] != 0.f || h_rest[i] != 0.f || h_count[i] != 0) { fprintf(stderr, "corner %d is not padding\n", k); bad = 1; }
    }
    long sum_count = 0;
    for (int i = 0; i < N; i++) {
        sum_count += h_count[i];
        const int filled = (h_index[i] >= 0) + (h_index[N + i] >= 0);
        if (h_count[i] != h_pcount[i] || filled != (h_count[i] < K ? h_count[i] : K) || h_index[i] > 3 || h_index[N + i] > 3 ||
            (h_count[i] <= K && h_rest[i] != 0.f)) { fprintf(stderr, "pixel %d: ids %d %d, count %d (picks: %d), rest %f\n", i, (int)h_index[i], (int)h_index[N + i], (int)h_count[i], (int)h_pcount[i], h_rest[i]); bad = 1; break; }
    }
    if (sum_count < 100) { fprintf(stderr, "sum of count %ld\n", sum_count); bad = 1; }
    if (memcmp(h_index, h_index2, sizeof h_index) || memcmp(h_weight, h_weight2, sizeof h_weight)) { fprintf(stderr, "the slots-only call differs from the full call\n"); bad = 1; }

    /* rest and count alone: the slots are not touched */
    CHECK(hipMemset(d_index, 0x7F, K*N*4)); CHECK(hipMemset(d_count, 0x7F, N*4));
    hp.out_index = NULL; hp.out_weight = NULL;
    if (ggr_pixel_hits(&st, NULL, &hp, NULL) != GGR_OK) { fprintf(stderr, "pixel hits (rest and count only): %s\n", ggr_last_error()); return 1; }
    CHECK(hipDeviceSynchronize());
    int32_t h_raw[2];
    CHECK(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_raw, d_index, sizeof h_raw, hipMemcpyDeviceToHost));
    long again = 0;
    for (int i = 0; i < N; i++) again += h_count[i];
    if (again != sum_count || h_raw[0] != 0x7F7F7F7F) { fprintf(stderr, "rest-and-count-only call: %ld %x\n", again, (unsigned)h_raw[0]); bad = 1; }
    hipFree(mem.p[0]); hipFree(mem.p[1]);
    printf(bad ? "HITS C ABI SMOKE FAILED\n" : "HITS C ABI SMOKE OK (sum of count %ld)\n", sum_count);
    return bad;
}

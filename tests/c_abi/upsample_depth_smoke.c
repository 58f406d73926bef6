/* The convex depth upsampling pass from plain C (C11, gcc): the header's additions are valid C and the library links.
 *   --host-only: no GPU work — the struct layout, the size query and the refusal of invalid passes before anything is enqueued.
 *   default: one forward and one backward on the GPU where the answer is known in closed form.  The logit of the CENTRE tap is 200
 *   and every other 0, so the other exponentials underflow to exactly zero and p = (0, 0, 0, 0, 1, 0, 0, 0, 0): at the identity size
 *   out[y r + i, x r + j] = depth[y, x] to the bit; with dL/dout = 1, dL/ddepth = r r (each cell's own r r sub-pixels) and
 *   dL/dmask = 0 (p_k (d_k - up) vanishes for the centre tap and p_k for the others). */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "ggr_raster.h"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("FAILED line %d: %s  [%s]\n", __LINE__, #cond, ggr_last_error()); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

enum { N = 2, H = 5, W = 15, R = 4, C = 9 * R * R, HO = H * R, WO = W * R };

static GgrUpsampleDepthPass base_pass(void) {
    GgrUpsampleDepthPass p;
    memset(&p, 0, sizeof p);
    p.struct_size = (int32_t)sizeof p;
    p.batch = N; p.height = H; p.width = W; p.ratio = R; p.out_height = HO; p.out_width = WO;
    return p;
}

static int host_checks(void) {
    CHECK(ggr_abi_version() == GGR_ABI_VERSION && GGR_ABI_VERSION == 11);
    CHECK(sizeof(GgrUpsampleDepthPass) == 112 && offsetof(GgrUpsampleDepthPass, depth) == 48 && offsetof(GgrUpsampleDepthPass, workspace_bytes) == 80);
    CHECK(ggr_upsample_depth_workspace_bytes(N, H, W, R) == (int64_t)N * H * W * R * R * 4);
    CHECK(ggr_upsample_depth_workspace_bytes(N, H, W, 2) == (int64_t)N * H * W * 9 * 4);
    CHECK(ggr_upsample_depth_workspace_bytes(N, H, W, 9) == -1 && ggr_upsample_depth_workspace_bytes(0, H, W, R) == -1);
    GgrUpsampleDepthPass p = base_pass();
    float* fake = (float*)(uintptr_t)256;
    p.depth = p.mask = p.dL_dout = fake;
    p.out = p.dL_dmask = p.dL_ddepth = fake;
    p.workspace = fake; p.workspace_bytes = 1 << 20;
    GgrUpsampleDepthPass q = p;
    q.ratio = 0;
    CHECK(ggr_upsample_depth_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "ratio"));
    q = p; q.batch = 0;
    CHECK(ggr_upsample_depth_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "batch"));
    q = p; q.out_width = 0;
    CHECK(ggr_upsample_depth_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out_width"));
    q = p; q.fold_disp = 1; q.min_depth = 3.f; q.max_depth = 2.f;
    CHECK(ggr_upsample_depth_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "min_depth"));
    q = p; q.out = NULL;
    CHECK(ggr_upsample_depth_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out is NULL"));
    q = p; q.workspace_bytes = 8;
    CHECK(ggr_upsample_depth_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "workspace_bytes"));
    q = p; q.dL_dmask = q.dL_ddepth = NULL;
    CHECK(ggr_upsample_depth_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "no output"));
    q = p; q.reserved = 7;
    CHECK(ggr_upsample_depth_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "reserved"));
    q = p; q.struct_size -= 4;
    CHECK(ggr_upsample_depth_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "struct_size"));
    CHECK(ggr_upsample_depth_forward(NULL, NULL) == GGR_E_INVALID);
    return 0;
}

#define HIP_OK(e) CHECK((e) == hipSuccess)

static int gpu_checks(void) {
    const size_t hw = (size_t)H * W, nd = N * hw, nm = (size_t)N * C * hw, no = (size_t)N * HO * WO;
    float* d = malloc(nd * 4);
    float* m = malloc(nm * 4);
    float* out = malloc(no * 4);
    float* ones = malloc(no * 4);
    float* gd = malloc(nd * 4);
    float* gm = malloc(nm * 4);
    for (size_t i = 0; i < nd; ++i) d[i] = 0.05f + (float)((i * 37u) % 101u) / 111.f;
    for (size_t i = 0; i < no; ++i) ones[i] = 1.f;
    for (size_t n = 0; n < N; ++n)
        for (size_t c = 0; c < C; ++c)
            for (size_t q = 0; q < hw; ++q) m[(n * C + c) * hw + q] = (c / (R * R) == 4) ? 200.f : 0.f;
    GgrUpsampleDepthPass p = base_pass();
    p.workspace_bytes = ggr_upsample_depth_workspace_bytes(N, H, W, R);
    float *d_d, *d_m, *d_out, *d_ones, *d_gd, *d_gm;
    void* d_ws;
    HIP_OK(hipMalloc((void**)&d_d, nd * 4)); HIP_OK(hipMalloc((void**)&d_m, nm * 4)); HIP_OK(hipMalloc((void**)&d_out, no * 4));
    HIP_OK(hipMalloc((void**)&d_ones, no * 4)); HIP_OK(hipMalloc((void**)&d_gd, nd * 4)); HIP_OK(hipMalloc((void**)&d_gm, nm * 4));
    HIP_OK(hipMalloc(&d_ws, (size_t)p.workspace_bytes));
    HIP_OK(hipMemcpy(d_d, d, nd * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_m, m, nm * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_ones, ones, no * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xff, no * 4)); HIP_OK(hipMemset(d_gd, 0xff, nd * 4)); HIP_OK(hipMemset(d_gm, 0xff, nm * 4));
    HIP_OK(hipMemset(d_ws, 0xff, (size_t)p.workspace_bytes));
    p.depth = d_d; p.mask = d_m; p.out = d_out; p.workspace = d_ws; p.dL_dout = d_ones; p.dL_dmask = d_gm; p.dL_ddepth = d_gd;
    CHECK(ggr_upsample_depth_forward(&p, NULL) == GGR_OK);
    CHECK(ggr_upsample_depth_backward(&p, NULL) == GGR_OK);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, d_out, no * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(gd, d_gd, nd * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gm, d_gm, nm * 4, hipMemcpyDeviceToHost));
    for (int n = 0; n < N; ++n)
        for (int y = 0; y < HO; ++y)
            for (int x = 0; x < WO; ++x) CHECK(out[((size_t)n * HO + y) * WO + x] == d[(size_t)n * hw + (size_t)(y / R) * W + x / R]);
    for (size_t i = 0; i < nd; ++i) CHECK(gd[i] == (float)(R * R));
    for (size_t i = 0; i < nm; ++i) CHECK(gm[i] == 0.f);
    printf("out[0] %g  dL/ddepth[0] %g\n", out[0], gd[0]);
    hipFree(d_d); hipFree(d_m); hipFree(d_out); hipFree(d_ones); hipFree(d_gd); hipFree(d_gm); hipFree(d_ws);
    free(d); free(m); free(out); free(ones); free(gd); free(gm);
    return 0;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    printf("UPSAMPLE DEPTH C ABI HOST CHECKS OK\n");
    if (argc > 1 && strcmp(argv[1], "--host-only") == 0) return 0;
    if (gpu_checks()) return 1;
    printf("UPSAMPLE DEPTH C ABI SMOKE OK\n");
    return 0;
}

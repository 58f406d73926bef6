/* The cost-map pass from plain C (C11, gcc): the header's additions are valid C and the library links.
 *   --host-only: no GPU work — the struct layout, the size query and the refusal of invalid passes before anything is enqueued.
 *   default: one forward and one backward on the GPU where the answer is known in closed form.  The poses are zero, both cameras
 *   have the same power-of-two intrinsics (128, principal point (27.5, 19.5) at full resolution: 16 and (3, 2) at 1/8) and the
 *   inverse depth is 0.5 everywhere, so every pixel is sampled at its own integer coordinate with weights (1, 0): the warped map IS
 *   the reference map and cost = (f - f_ref)^2 to the bit; with dL/dcost = 1, dL/dfmap = 2 (f - f_ref) summed over the views and
 *   dL/dfmaps_ref = -2 (f - f_ref). */
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

enum { V = 2, C = 9, H = 7, W = 11 };

static GgrWarpCostPass base_pass(void) {
    GgrWarpCostPass p;
    memset(&p, 0, sizeof p);
    p.struct_size = (int32_t)sizeof p;
    p.num_views = V; p.channels = C; p.height = H; p.width = W; p.reduce_mean = 0; p.scale_factor = 0.125f;
    return p;
}

static int host_checks(void) {
    CHECK(ggr_abi_version() == GGR_ABI_VERSION && GGR_ABI_VERSION == 11);
    CHECK(sizeof(GgrWarpCostPass) == 168 && offsetof(GgrWarpCostPass, fmap) == 48 && offsetof(GgrWarpCostPass, workspace_bytes) == 120);
    CHECK(ggr_warp_cost_workspace_bytes(V, H, W) == 2 * (int64_t)V * 12 * 8);      /* 77 pixels: two tiles of 64 */
    CHECK(ggr_warp_cost_workspace_bytes(17, H, W) == -1 && ggr_warp_cost_workspace_bytes(V, 1, W) == -1);
    GgrWarpCostPass p = base_pass();
    float* fake = (float*)(uintptr_t)256;
    p.fmap = p.fmaps_ref = p.inv_depth = p.K = p.ref_Ks = p.poses = p.dL_dcost = fake;
    p.out_cost = p.dL_dfmap = p.dL_dfmaps_ref = p.dL_dinv_depth = p.dL_dposes = fake;
    p.workspace = fake; p.workspace_bytes = 1 << 20;
    GgrWarpCostPass q = p;
    q.num_views = 0;
    CHECK(ggr_warp_cost_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "num_views"));
    q = p; q.height = 1;
    CHECK(ggr_warp_cost_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "height"));
    q = p; q.scale_factor = 0.f;
    CHECK(ggr_warp_cost_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "scale_factor"));
    q = p; q.fold_disp = 1; q.min_depth = 3.f; q.max_depth = 2.f;
    CHECK(ggr_warp_cost_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "min_depth"));
    q = p; q.out_cost = NULL;
    CHECK(ggr_warp_cost_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out_cost"));
    q = p; q.workspace_bytes = 8;
    CHECK(ggr_warp_cost_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "workspace_bytes"));
    q = p; q.dL_dfmap = q.dL_dfmaps_ref = q.dL_dinv_depth = q.dL_dposes = NULL;
    CHECK(ggr_warp_cost_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "no output"));
    q = p; q.struct_size -= 4;
    CHECK(ggr_warp_cost_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "struct_size"));
    CHECK(ggr_warp_cost_forward(NULL, NULL) == GGR_E_INVALID);
    return 0;
}

#define HIP_OK(e) CHECK((e) == hipSuccess)

static int gpu_checks(void) {
    const size_t hw = (size_t)H * W, n1 = C * hw, nv = V * n1;
    float* f = malloc(n1 * 4);
    float* r = malloc(nv * 4);
    float* inv = malloc(hw * 4);
    float* cost = malloc(nv * 4);
    float* gf = malloc(n1 * 4);
    float* gr = malloc(nv * 4);
    float* ones = malloc(nv * 4);
    int32_t* cells = malloc(V * hw * 3 * 4);
    float Kh[9] = {128.f, 0.f, 27.5f, 0.f, 128.f, 19.5f, 0.f, 0.f, 1.f}, Ks[V * 9], poses[V * 6];
    for (size_t i = 0; i < n1; ++i) f[i] = (float)((i * 37u) % 101u) / 101.f;
    for (size_t i = 0; i < nv; ++i) { r[i] = (float)((i * 53u) % 97u) / 97.f; ones[i] = 1.f; }
    for (size_t i = 0; i < hw; ++i) inv[i] = 0.5f;
    for (int j = 0; j < V; ++j) memcpy(Ks + 9 * j, Kh, sizeof Kh);
    memset(poses, 0, sizeof poses);
    GgrWarpCostPass p = base_pass();
    p.workspace_bytes = ggr_warp_cost_workspace_bytes(V, H, W);
    float *d_f, *d_r, *d_inv, *d_K, *d_Ks, *d_poses, *d_cost, *d_ones, *d_gf, *d_gr, *d_ginv, *d_gposes;
    void* d_ws; int32_t* d_cells;
    HIP_OK(hipMalloc((void**)&d_f, n1 * 4)); HIP_OK(hipMalloc((void**)&d_r, nv * 4)); HIP_OK(hipMalloc((void**)&d_inv, hw * 4));
    HIP_OK(hipMalloc((void**)&d_K, 36)); HIP_OK(hipMalloc((void**)&d_Ks, V * 36)); HIP_OK(hipMalloc((void**)&d_poses, sizeof poses));
    HIP_OK(hipMalloc((void**)&d_cost, nv * 4)); HIP_OK(hipMalloc((void**)&d_ones, nv * 4)); HIP_OK(hipMalloc((void**)&d_gf, n1 * 4));
    HIP_OK(hipMalloc((void**)&d_gr, nv * 4)); HIP_OK(hipMalloc((void**)&d_ginv, hw * 4)); HIP_OK(hipMalloc((void**)&d_gposes, V * 24));
    HIP_OK(hipMalloc(&d_ws, (size_t)p.workspace_bytes)); HIP_OK(hipMalloc((void**)&d_cells, V * hw * 12));
    HIP_OK(hipMemcpy(d_f, f, n1 * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_r, r, nv * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_inv, inv, hw * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_K, Kh, 36, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_Ks, Ks, V * 36, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_poses, poses, sizeof poses, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_ones, ones, nv * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_cost, 0xff, nv * 4)); HIP_OK(hipMemset(d_gf, 0xff, n1 * 4)); HIP_OK(hipMemset(d_gr, 0, nv * 4));
    HIP_OK(hipMemset(d_ginv, 0xff, hw * 4)); HIP_OK(hipMemset(d_gposes, 0xff, V * 24)); HIP_OK(hipMemset(d_cells, 0xff, V * hw * 12));
    p.fmap = d_f; p.fmaps_ref = d_r; p.inv_depth = d_inv; p.K = d_K; p.ref_Ks = d_Ks; p.poses = d_poses;
    p.out_cost = d_cost; p.out_cells = d_cells; p.workspace = d_ws;
    p.dL_dcost = d_ones; p.dL_dfmap = d_gf; p.dL_dfmaps_ref = d_gr; p.dL_dinv_depth = d_ginv; p.dL_dposes = d_gposes;
    CHECK(ggr_warp_cost_forward(&p, NULL) == GGR_OK);
    CHECK(ggr_warp_cost_backward(&p, NULL) == GGR_OK);
    HIP_OK(hipDeviceSynchronize());
    float ginv[H * W], gposes[V * 6];
    HIP_OK(hipMemcpy(cost, d_cost, nv * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(cells, d_cells, V * hw * 12, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gf, d_gf, n1 * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(gr, d_gr, nv * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ginv, d_ginv, hw * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(gposes, d_gposes, V * 24, hipMemcpyDeviceToHost));
    for (int j = 0; j < V; ++j)
        for (int c = 0; c < C; ++c)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const size_t q = (size_t)y * W + x, i = ((size_t)j * C + c) * hw + q;
                    const float d = f[c * hw + q] - r[i];
                    CHECK(cost[i] == d * d);
                    CHECK(gr[i] == -(2.f * d * 1.f));
                    if (c == 0) {
                        const int32_t* cell = cells + ((size_t)j * hw + q) * 3;
                        CHECK(cell[0] == x && cell[1] == y && cell[2] == 0);
                    }
                }
    for (size_t i = 0; i < n1; ++i) {
        const float d0 = 2.f * (f[i] - r[i]), d1 = 2.f * (f[i] - r[n1 + i]);
        CHECK(gf[i] == d0 + d1);
    }
    for (size_t i = 0; i < hw; ++i) CHECK(isfinite(ginv[i]));
    for (int i = 0; i < V * 6; ++i) CHECK(isfinite(gposes[i]));
    printf("cost[0] %g  dL/dposes[0] %g\n", cost[0], gposes[0]);
    hipFree(d_f); hipFree(d_r); hipFree(d_inv); hipFree(d_K); hipFree(d_Ks); hipFree(d_poses); hipFree(d_cost); hipFree(d_ones); hipFree(d_gf);
    hipFree(d_gr); hipFree(d_ginv); hipFree(d_gposes); hipFree(d_ws); hipFree(d_cells);
    free(f); free(r); free(inv); free(cost); free(gf); free(gr); free(ones); free(cells);
    return 0;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    printf("WARP COST C ABI HOST CHECKS OK\n");
    if (argc > 1 && strcmp(argv[1], "--host-only") == 0) return 0;
    if (gpu_checks()) return 1;
    printf("WARP COST C ABI SMOKE OK\n");
    return 0;
}

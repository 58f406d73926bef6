/* The photometric-loss pass from plain C (C11, gcc): the header's additions are valid C and the library links.
 *   --host-only: no GPU work — the struct layout, the size queries and the refusal of invalid passes before anything is enqueued.
 *   default: one forward on the GPU where the answer is known in closed form.  The reference views ARE the target image, the poses
 *   are zero, the inverse depth is 0.5 everywhere and the intrinsics are powers of two, so every pixel is sampled at its own integer
 *   coordinate and every candidate compares the image with itself: L1 is 0 and SSIM is 1 to within the few roundings of its two
 *   products (|SSIM - 1| <= 2.4e-7, so p <= 0.85 * 1.2e-7 and the loss, the sum of three such means weighted 1 + 0.85 + 0.7225, stays
 *   below 3e-7, as do the thresholds); warped and unwarped planes are the same bits, so every minimum is a tie that goes to
 *   candidate 0. */
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

enum { V = 2, N = 3, H = 17, W = 33, C = 2 * V };

static GgrPhotometricLossPass base_pass(void) {
    GgrPhotometricLossPass p;
    memset(&p, 0, sizeof p);
    p.struct_size = (int32_t)sizeof p;
    p.num_views = V; p.num_iters = N; p.height = H; p.width = W; p.automask = 1;
    p.ssim_loss_weight = 0.85f; p.smooth_loss_weight = 0.01f; p.C1 = 1e-4f; p.C2 = 9e-4f; p.clip_loss = 0.5f; p.gamma = 0.85f;
    return p;
}

static int host_checks(void) {
    CHECK(ggr_abi_version() == GGR_ABI_VERSION && GGR_ABI_VERSION == 11);
    CHECK(sizeof(GgrPhotometricLossPass) == 208 && offsetof(GgrPhotometricLossPass, image) == 56);
    CHECK(ggr_photometric_loss_planes_bytes(V, N, H, W, 1) == (int64_t)(N * V + V) * H * W * 4);
    CHECK(ggr_photometric_loss_planes_bytes(V, N, H, W, 0) == (int64_t)(N * V) * H * W * 4);
    CHECK(ggr_photometric_loss_workspace_bytes(V, N, H, W, 1) == 4 * (int64_t)N * V * 12 * 8);   /* four tiles; the backward's share is the larger */
    CHECK(ggr_photometric_loss_planes_bytes(9, N, H, W, 1) == -1 && ggr_photometric_loss_planes_bytes(9, N, H, W, 0) > 0);
    CHECK(ggr_photometric_loss_planes_bytes(V, N, 1, W, 1) == -1 && ggr_photometric_loss_workspace_bytes(V, 0, H, W, 1) == -1);
    GgrPhotometricLossPass p = base_pass();
    float* fake = (float*)(uintptr_t)256;
    p.image = p.ref_imgs = p.inv_depths = p.K = p.ref_Ks = p.poses = fake;
    p.planes = p.out_thresholds = p.state = p.out_loss = p.out_photometric = p.out_smoothness = fake;
    p.choice = (uint8_t*)fake; p.workspace = fake; p.planes_bytes = p.workspace_bytes = 1 << 24;
    p.dL_dloss = fake; p.dL_dinv_depths = p.dL_dposes = fake;
    GgrPhotometricLossPass q = p;
    q.num_views = 9;
    CHECK(ggr_photometric_loss_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "candidates"));
    q = p; q.height = 1;
    CHECK(ggr_photometric_loss_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "height"));
    q = p; q.ssim_loss_weight = 0.f;
    CHECK(ggr_photometric_loss_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "ssim_loss_weight"));
    q = p; q.planes_bytes = 16;
    CHECK(ggr_photometric_loss_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "planes_bytes"));
    q = p; q.out_loss = NULL;
    CHECK(ggr_photometric_loss_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out_loss"));
    q = p; q.dL_dposes = NULL;
    CHECK(ggr_photometric_loss_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "dL_dposes"));
    q = p; q.struct_size -= 4;
    CHECK(ggr_photometric_loss_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "struct_size"));
    CHECK(ggr_photometric_loss_forward(NULL, NULL) == GGR_E_INVALID);
    return 0;
}

#define HIP_OK(e) CHECK((e) == hipSuccess)

static int gpu_checks(void) {
    const size_t hw = (size_t)H * W;
    float* image = malloc(3 * hw * 4);
    float* refs = malloc(V * 3 * hw * 4);
    float* inv = malloc(N * hw * 4);
    float Kh[9] = {16.f, 0.f, 16.f, 0.f, 16.f, 8.f, 0.f, 0.f, 1.f}, Ks[V * 9], poses[V * N * 6];
    for (size_t i = 0; i < 3 * hw; ++i) image[i] = (float)((i * 37u) % 101u) / 101.f;
    for (int j = 0; j < V; ++j) { memcpy(refs + j * 3 * hw, image, 3 * hw * 4); memcpy(Ks + 9 * j, Kh, sizeof Kh); }
    for (size_t i = 0; i < N * hw; ++i) inv[i] = 0.5f;
    memset(poses, 0, sizeof poses);
    GgrPhotometricLossPass p = base_pass();
    p.planes_bytes = ggr_photometric_loss_planes_bytes(V, N, H, W, 1);
    p.workspace_bytes = ggr_photometric_loss_workspace_bytes(V, N, H, W, 1);
    float *d_image, *d_refs, *d_inv, *d_K, *d_Ks, *d_poses, *d_planes, *d_thr, *d_state, *d_out;
    void* d_ws; uint8_t* d_choice;
    HIP_OK(hipMalloc((void**)&d_image, 3 * hw * 4)); HIP_OK(hipMalloc((void**)&d_refs, V * 3 * hw * 4)); HIP_OK(hipMalloc((void**)&d_inv, N * hw * 4));
    HIP_OK(hipMalloc((void**)&d_K, 36)); HIP_OK(hipMalloc((void**)&d_Ks, V * 36)); HIP_OK(hipMalloc((void**)&d_poses, sizeof poses));
    HIP_OK(hipMalloc((void**)&d_planes, (size_t)p.planes_bytes)); HIP_OK(hipMalloc(&d_ws, (size_t)p.workspace_bytes));
    HIP_OK(hipMalloc((void**)&d_thr, N * C * 4)); HIP_OK(hipMalloc((void**)&d_state, 2 * N * 4)); HIP_OK(hipMalloc((void**)&d_out, 12));
    HIP_OK(hipMalloc((void**)&d_choice, N * hw));
    HIP_OK(hipMemcpy(d_image, image, 3 * hw * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_refs, refs, V * 3 * hw * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_inv, inv, N * hw * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_K, Kh, 36, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_Ks, Ks, V * 36, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_poses, poses, sizeof poses, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_choice, 0xff, N * hw)); HIP_OK(hipMemset(d_out, 0xff, 12)); HIP_OK(hipMemset(d_thr, 0xff, N * C * 4));
    p.image = d_image; p.ref_imgs = d_refs; p.inv_depths = d_inv; p.K = d_K; p.ref_Ks = d_Ks; p.poses = d_poses; p.planes = d_planes;
    p.workspace = d_ws; p.out_thresholds = d_thr; p.state = d_state; p.choice = d_choice;
    p.out_loss = d_out; p.out_photometric = d_out + 1; p.out_smoothness = d_out + 2;
    CHECK(ggr_photometric_loss_forward(&p, NULL) == GGR_OK);
    HIP_OK(hipDeviceSynchronize());
    float out[3], thr[N * C];
    uint8_t* choice = malloc(N * hw);
    HIP_OK(hipMemcpy(out, d_out, 12, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(thr, d_thr, sizeof thr, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(choice, d_choice, N * hw, hipMemcpyDeviceToHost));
    printf("loss %g photometric %g smoothness %g\n", out[0], out[1], out[2]);
    CHECK(out[0] >= 0.f && out[0] <= 3e-7f && out[1] == out[0] && out[2] == 0.f);
    for (int i = 0; i < N * C; ++i) CHECK(thr[i] >= 0.f && thr[i] <= 3e-7f);
    for (size_t i = 0; i < N * hw; ++i) CHECK(choice[i] == 0);
    hipFree(d_image); hipFree(d_refs); hipFree(d_inv); hipFree(d_K); hipFree(d_Ks); hipFree(d_poses); hipFree(d_planes); hipFree(d_ws);
    hipFree(d_thr); hipFree(d_state); hipFree(d_out); hipFree(d_choice);
    free(image); free(refs); free(inv); free(choice);
    return 0;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    printf("PHOTOMETRIC LOSS C ABI HOST CHECKS OK\n");
    if (argc > 1 && strcmp(argv[1], "--host-only") == 0) return 0;
    if (gpu_checks()) return 1;
    printf("PHOTOMETRIC LOSS C ABI SMOKE OK\n");
    return 0;
}

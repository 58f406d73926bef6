/* The ConvGRU gate math from plain C (C11, gcc): the header's additions are valid C and the library links.
 *   --host-only: no GPU work — the struct layout and the refusal of invalid passes before anything is enqueued.
 *   default: the four calls on a 2 x 3 x 3 x 5 case (M = 45: the 4-byte path, and the n 2M block offsets) against values this
 *   host computes in double, to 2e-6 of the largest value of each array; outputs are filled with NaN bytes first.  Then the same
 *   forward without the second addends against the sum passed as the first. */
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

enum { N = 2, CH = 3, H = 3, W = 5, M = CH * H * W, NM = N * M };

static GgrGruPass base_pass(void) {
    GgrGruPass p;
    memset(&p, 0, sizeof p);
    p.struct_size = (int32_t)sizeof p;
    p.batch = N; p.channels = CH; p.height = H; p.width = W;
    return p;
}

static int host_checks(void) {
    CHECK(ggr_abi_version() == GGR_ABI_VERSION && GGR_ABI_VERSION == 11);
    CHECK(sizeof(GgrGruPass) == 152 && offsetof(GgrGruPass, a_zr_h) == 24 && offsetof(GgrGruPass, dL_dh) == 144);
    GgrGruPass p = base_pass();
    float* fake = (float*)(uintptr_t)256;
    p.a_zr_h = p.a_zr_x = p.h = p.a_q_h = p.a_q_x = p.dL_dout_h = p.dL_drh = fake;
    p.z = p.r = p.rh = p.q = p.dL_da_q = p.dL_da_zr = p.dL_dh_part = p.dL_dh = fake;
    p.out_h = fake + 4;
    GgrGruPass q = p;
    q.batch = 0;
    CHECK(ggr_gru_gate_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "batch"));
    q = p; q.channels = 0;
    CHECK(ggr_gru_blend_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "channels"));
    q = p; q.width = -1;
    CHECK(ggr_gru_blend_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "width"));
    q = p; q.batch = 4; q.channels = 128; q.height = 2048; q.width = 1024;
    CHECK(ggr_gru_gate_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "32-bit"));
    q = p; q.rh = NULL;
    CHECK(ggr_gru_gate_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "rh is NULL"));
    q = p; q.out_h = (float*)q.h;
    CHECK(ggr_gru_blend_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out_h is h itself"));
    q = p; q.dL_da_q = q.dL_da_zr = q.dL_dh_part = NULL;
    CHECK(ggr_gru_blend_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "no output"));
    q = p; q.dL_da_zr = q.dL_dh = NULL;
    CHECK(ggr_gru_gate_backward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "no output"));
    q = p; q.reserved = 7;
    CHECK(ggr_gru_gate_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "reserved"));
    q = p; q.struct_size -= 4;
    CHECK(ggr_gru_gate_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "struct_size"));
    CHECK(ggr_gru_gate_backward(NULL, NULL) == GGR_E_INVALID);
    return 0;
}

#define HIP_OK(e) CHECK((e) == hipSuccess)

static float noise(unsigned i, unsigned salt, float scale) { return scale * ((float)((i * 2654435761u + salt * 40503u) % 2001u) / 1000.f - 1.f); }

static double sigmoid_d(double a) { return 1.0 / (1.0 + exp(-a)); }

/* max |got - want| over an array against 2e-6 of max |want| */
static int close_to(const float* got, const double* want, int n, const char* what) {
    double err = 0, top = 0;
    for (int i = 0; i < n; ++i) {
        if (got[i] != got[i]) { printf("%s[%d] is NaN\n", what, i); return 0; }
        if (fabs(got[i] - want[i]) > err) err = fabs(got[i] - want[i]);
        if (fabs(want[i]) > top) top = fabs(want[i]);
    }
    printf("%s: max error %.3g of max %.3g\n", what, err, top);
    return err <= 2e-6 * top;
}

static float* to_device(const float* src, size_t n) {
    float* d = NULL;
    if (hipMalloc((void**)&d, n * 4) != hipSuccess) return NULL;
    if (src ? hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice) != hipSuccess : hipMemset(d, 0xff, n * 4) != hipSuccess) return NULL;
    return d;
}

static int gpu_checks(void) {
    static float a_zr_h[2 * NM], a_zr_x[2 * NM], a_zr_sum[2 * NM], h[NM], a_q_x[NM], g[NM], a_q_h[NM], g_rh[NM];
    static float z[NM], r[NM], rh[NM], q[NM], out[NM], g_a_q[NM], g_a_zr[2 * NM], g_part[NM], g_h[NM], z2[NM], rh2[NM];
    static double wz[NM], wr[NM], wrh[NM], wq[NM], wout[NM], w_a_q[NM], w_a_zr[2 * NM], w_part[NM], w_h[NM];
    for (unsigned i = 0; i < 2 * NM; ++i) { a_zr_h[i] = noise(i, 1, 2.f); a_zr_x[i] = noise(i, 2, 2.f); a_zr_sum[i] = a_zr_h[i] + a_zr_x[i]; }
    for (unsigned i = 0; i < NM; ++i) { h[i] = noise(i, 3, 1.f); a_q_x[i] = noise(i, 4, 1.5f); g[i] = noise(i, 5, 1.f); a_q_h[i] = noise(i, 6, 1.5f); g_rh[i] = noise(i, 7, 1.f); }
    for (int n = 0; n < N; ++n)
        for (int m = 0; m < M; ++m) {
            const int e = n * M + m, zi = n * 2 * M + m, ri = zi + M;
            wz[e] = sigmoid_d((double)a_zr_h[zi] + a_zr_x[zi]);
            wr[e] = sigmoid_d((double)a_zr_h[ri] + a_zr_x[ri]);
            wrh[e] = wr[e] * h[e];
        }
    GgrGruPass p = base_pass();
    float *d_a_zr_h = to_device(a_zr_h, 2 * NM), *d_a_zr_x = to_device(a_zr_x, 2 * NM), *d_a_zr_sum = to_device(a_zr_sum, 2 * NM), *d_h = to_device(h, NM);
    float *d_a_q_x = to_device(a_q_x, NM), *d_g = to_device(g, NM), *d_a_q_h = to_device(a_q_h, NM), *d_g_rh = to_device(g_rh, NM);
    float *d_z = to_device(NULL, NM), *d_r = to_device(NULL, NM), *d_rh = to_device(NULL, NM), *d_q = to_device(NULL, NM), *d_out = to_device(NULL, NM);
    float *d_g_a_q = to_device(NULL, NM), *d_g_a_zr = to_device(NULL, 2 * NM), *d_g_part = to_device(NULL, NM), *d_g_h = to_device(NULL, NM);
    float *d_z2 = to_device(NULL, NM), *d_r2 = to_device(NULL, NM), *d_rh2 = to_device(NULL, NM);
    CHECK(d_a_zr_h && d_a_zr_x && d_a_zr_sum && d_h && d_a_q_x && d_g && d_a_q_h && d_g_rh && d_z && d_r && d_rh && d_q && d_out && d_g_a_q && d_g_a_zr &&
          d_g_part && d_g_h && d_z2 && d_r2 && d_rh2);
    p.a_zr_h = d_a_zr_h; p.a_zr_x = d_a_zr_x; p.h = d_h; p.z = d_z; p.r = d_r; p.rh = d_rh; p.a_q_h = d_a_q_h; p.a_q_x = d_a_q_x; p.q = d_q; p.out_h = d_out;
    p.dL_dout_h = d_g; p.dL_da_q = d_g_a_q; p.dL_da_zr = d_g_a_zr; p.dL_dh_part = d_g_part; p.dL_drh = d_g_rh; p.dL_dh = d_g_h;
    CHECK(ggr_gru_gate_forward(&p, NULL) == GGR_OK);
    CHECK(ggr_gru_blend_forward(&p, NULL) == GGR_OK);
    CHECK(ggr_gru_blend_backward(&p, NULL) == GGR_OK);
    CHECK(ggr_gru_gate_backward(&p, NULL) == GGR_OK);
    GgrGruPass one = p;         /* the sum as the only addend */
    one.a_zr_h = d_a_zr_sum; one.a_zr_x = NULL; one.z = d_z2; one.r = d_r2; one.rh = d_rh2;
    CHECK(ggr_gru_gate_forward(&one, NULL) == GGR_OK);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(z, d_z, NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(r, d_r, NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rh, d_rh, NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(q, d_q, NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out, d_out, NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(g_a_q, d_g_a_q, NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(g_a_zr, d_g_a_zr, 2 * NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(g_part, d_g_part, NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(g_h, d_g_h, NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(z2, d_z2, NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rh2, d_rh2, NM * 4, hipMemcpyDeviceToHost));
    /* the later calls read what the earlier ones wrote: the expected values follow the device's own z, r, q */
    for (int n = 0; n < N; ++n)
        for (int m = 0; m < M; ++m) {
            const int e = n * M + m, zi = n * 2 * M + m, ri = zi + M;
            wq[e] = tanh((double)a_q_h[e] + a_q_x[e]);
            wout[e] = (1.0 - z[e]) * h[e] + (double)z[e] * q[e];
            w_a_q[e] = (double)g[e] * z[e] * (1.0 - (double)q[e] * q[e]);
            w_a_zr[zi] = (double)g[e] * ((double)q[e] - h[e]) * z[e] * (1.0 - z[e]);
            w_part[e] = (double)g[e] * (1.0 - z[e]);
            w_a_zr[ri] = (double)g_rh[e] * h[e] * r[e] * (1.0 - r[e]);
            w_h[e] = w_part[e] + (double)g_rh[e] * r[e];
        }
    CHECK(close_to(z, wz, NM, "z") && close_to(r, wr, NM, "r") && close_to(rh, wrh, NM, "rh") && close_to(q, wq, NM, "q") && close_to(out, wout, NM, "out_h"));
    CHECK(close_to(g_a_q, w_a_q, NM, "dL_da_q") && close_to(g_a_zr, w_a_zr, 2 * NM, "dL_da_zr") && close_to(g_part, w_part, NM, "dL_dh_part") &&
          close_to(g_h, w_h, NM, "dL_dh"));
    CHECK(close_to(z2, wz, NM, "z (one addend)") && close_to(rh2, wrh, NM, "rh (one addend)"));
    float* all[] = {d_a_zr_h, d_a_zr_x, d_a_zr_sum, d_h, d_a_q_x, d_g, d_a_q_h, d_g_rh, d_z, d_r, d_rh, d_q, d_out, d_g_a_q, d_g_a_zr, d_g_part, d_g_h, d_z2, d_r2, d_rh2};
    for (size_t i = 0; i < sizeof all / sizeof all[0]; ++i) hipFree(all[i]);
    return 0;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    printf("GRU GATES C ABI HOST CHECKS OK\n");
    if (argc > 1 && strcmp(argv[1], "--host-only") == 0) return 0;
    if (gpu_checks()) return 1;
    printf("GRU GATES C ABI SMOKE OK\n");
    return 0;
}

/* The ConvGRU inference route from plain C (C11, gcc): the header's additions are valid C and the library links.
 *   --host-only: no GPU work — the struct layout and the refusal of invalid passes before anything is enqueued.
 *   default: one GATE and one BLEND (and the RAW sums of both) on a 2 x 3 x 3 x 5 hidden state with 2 feature channels, 1 x 5 and
 *   3 x 3 kernels, against values this host computes in double, to 2e-6 of the largest value of each array; outputs are filled
 *   with NaN bytes first. */
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

enum { N = 2, CH = 3, CX = 2, H = 3, W = 5, HW = H * W, NM = N * CH * HW, NX = N * CX * HW, MAXT = 9 };

static GgrGruConvPass base_pass(int kh, int kw) {
    GgrGruConvPass p;
    memset(&p, 0, sizeof p);
    p.struct_size = (int32_t)sizeof p;
    p.batch = N; p.channels = CH; p.in_channels = CX; p.height = H; p.width = W; p.kernel_h = kh; p.kernel_w = kw;
    return p;
}

static int host_checks(void) {
    CHECK(ggr_abi_version() == GGR_ABI_VERSION && GGR_ABI_VERSION == 11);
    CHECK(sizeof(GgrGruConvPass) == 144 && offsetof(GgrGruConvPass, a) == 48 && offsetof(GgrGruConvPass, workspace_bytes) == 136);
    CHECK(GGR_GRU_CONV_GATE == 0 && GGR_GRU_CONV_BLEND == 1 && GGR_GRU_CONV_RAW == 2);
    CHECK(ggr_gru_conv_workspace_bytes(NULL) == 0);
    GgrGruConvPass p = base_pass(1, 5);
    float* fake = (float*)(uintptr_t)256;
    p.a = p.x = p.w_h = p.w_x = p.bias = p.h = fake;
    p.z = p.rh = p.raw = fake;
    p.out_h = fake + 4;
    CHECK(ggr_gru_conv_workspace_bytes(&p) == 0);
    GgrGruConvPass q = p;
    q.batch = 0;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "batch"));
    q = p; q.in_channels = 0;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "in_channels"));
    q = p; q.kernel_w = 4;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "kernel_w"));
    q = p; q.kernel_h = 7;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "kernel_h"));
    q = p; q.epilogue = 3;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "epilogue"));
    q = p; q.epilogue = GGR_GRU_CONV_RAW; q.out_channels = 0;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out_channels"));
    q = p; q.batch = 4; q.channels = 128; q.height = 2048; q.width = 1024;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "32-bit"));
    q = p; q.rh = NULL;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "rh is NULL"));
    q = p; q.epilogue = GGR_GRU_CONV_BLEND; q.out_h = (float*)q.h;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "out_h is h itself"));
    q = p; q.workspace_bytes = -8;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "workspace_bytes"));
    q = p; q.x = (const float*)(uintptr_t)258;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "misaligned"));
    q = p; q.reserved = 7;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "reserved"));
    q = p; q.struct_size -= 4;
    CHECK(ggr_gru_conv_forward(&q, NULL) == GGR_E_INVALID && strstr(ggr_last_error(), "struct_size"));
    CHECK(ggr_gru_conv_forward(NULL, NULL) == GGR_E_INVALID);
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

/* acc[n, co, y, x] = bias[co] + sum w_h[co, ci, t] a[n, ci, (y, x) + t - pad] + sum w_x[co, ci, t] x[...], zero padding */
static void conv_d(const float* a, const float* x, const float* w_h, const float* w_x, const float* bias, int cout, int kh, int kw, double* acc) {
    const int ph = (kh - 1) / 2, pw = (kw - 1) / 2, taps = kh * kw;
    for (int n = 0; n < N; ++n)
        for (int co = 0; co < cout; ++co)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    double s = bias[co];
                    for (int ty = 0; ty < kh; ++ty)
                        for (int tx = 0; tx < kw; ++tx) {
                            const int yy = y + ty - ph, xc = xx + tx - pw, t = ty * kw + tx;
                            if (yy < 0 || yy >= H || xc < 0 || xc >= W) continue;
                            for (int ci = 0; ci < CH; ++ci) s += (double)w_h[(co * CH + ci) * taps + t] * a[(n * CH + ci) * HW + yy * W + xc];
                            for (int ci = 0; ci < CX; ++ci) s += (double)w_x[(co * CX + ci) * taps + t] * x[(n * CX + ci) * HW + yy * W + xc];
                        }
                    acc[(n * cout + co) * HW + y * W + xx] = s;
                }
}

static int gpu_case(int kh, int kw) {
    const int taps = kh * kw;
    static float h[NM], x[NX], w_zr_h[2 * CH * CH * MAXT], w_zr_x[2 * CH * CX * MAXT], b_zr[2 * CH], w_q_h[CH * CH * MAXT], w_q_x[CH * CX * MAXT], b_q[CH];
    static float z[NM], rh[NM], out[NM], raw_zr[2 * NM], raw_q[NM];
    static double a_zr[2 * NM], a_q[NM], wz[NM], wrh[NM], wout[NM];
    for (unsigned i = 0; i < NM; ++i) h[i] = noise(i, 1, 1.f);
    for (unsigned i = 0; i < NX; ++i) x[i] = noise(i, 2, 1.5f);
    for (unsigned i = 0; i < (unsigned)(2 * CH * CH * taps); ++i) w_zr_h[i] = noise(i, 3, 0.6f);
    for (unsigned i = 0; i < (unsigned)(2 * CH * CX * taps); ++i) w_zr_x[i] = noise(i, 4, 0.6f);
    for (unsigned i = 0; i < (unsigned)(CH * CH * taps); ++i) w_q_h[i] = noise(i, 5, 0.6f);
    for (unsigned i = 0; i < (unsigned)(CH * CX * taps); ++i) w_q_x[i] = noise(i, 6, 0.6f);
    for (unsigned i = 0; i < 2 * CH; ++i) b_zr[i] = noise(i, 7, 0.5f);
    for (unsigned i = 0; i < CH; ++i) b_q[i] = noise(i, 8, 0.5f);
    float *d_h = to_device(h, NM), *d_x = to_device(x, NX), *d_w_zr_h = to_device(w_zr_h, 2 * CH * CH * taps), *d_w_zr_x = to_device(w_zr_x, 2 * CH * CX * taps);
    float *d_b_zr = to_device(b_zr, 2 * CH), *d_w_q_h = to_device(w_q_h, CH * CH * taps), *d_w_q_x = to_device(w_q_x, CH * CX * taps), *d_b_q = to_device(b_q, CH);
    float *d_z = to_device(NULL, NM), *d_rh = to_device(NULL, NM), *d_out = to_device(NULL, NM), *d_raw_zr = to_device(NULL, 2 * NM), *d_raw_q = to_device(NULL, NM);
    CHECK(d_h && d_x && d_w_zr_h && d_w_zr_x && d_b_zr && d_w_q_h && d_w_q_x && d_b_q && d_z && d_rh && d_out && d_raw_zr && d_raw_q);
    GgrGruConvPass gate = base_pass(kh, kw);
    CHECK(ggr_gru_conv_workspace_bytes(&gate) == 0);
    gate.epilogue = GGR_GRU_CONV_GATE;
    gate.a = d_h; gate.x = d_x; gate.w_h = d_w_zr_h; gate.w_x = d_w_zr_x; gate.bias = d_b_zr; gate.h = d_h; gate.z = d_z; gate.rh = d_rh;
    GgrGruConvPass blend = base_pass(kh, kw);
    blend.epilogue = GGR_GRU_CONV_BLEND;
    blend.a = d_rh; blend.x = d_x; blend.w_h = d_w_q_h; blend.w_x = d_w_q_x; blend.bias = d_b_q; blend.h = d_h; blend.z = d_z; blend.out_h = d_out;
    GgrGruConvPass raw = gate;          /* the pre-activations of the gate, then of the blend */
    raw.epilogue = GGR_GRU_CONV_RAW; raw.out_channels = 2 * CH; raw.raw = d_raw_zr;
    CHECK(ggr_gru_conv_forward(&gate, NULL) == GGR_OK);
    CHECK(ggr_gru_conv_forward(&blend, NULL) == GGR_OK);
    CHECK(ggr_gru_conv_forward(&raw, NULL) == GGR_OK);
    raw = blend;
    raw.epilogue = GGR_GRU_CONV_RAW; raw.out_channels = CH; raw.raw = d_raw_q;
    CHECK(ggr_gru_conv_forward(&raw, NULL) == GGR_OK);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(z, d_z, NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(rh, d_rh, NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out, d_out, NM * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(raw_zr, d_raw_zr, 2 * NM * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(raw_q, d_raw_q, NM * 4, hipMemcpyDeviceToHost));
    conv_d(h, x, w_zr_h, w_zr_x, b_zr, 2 * CH, kh, kw, a_zr);
    conv_d(rh, x, w_q_h, w_q_x, b_q, CH, kh, kw, a_q);          /* the blend reads what the gate wrote: the device's own rh and z */
    for (int n = 0; n < N; ++n)
        for (int m = 0; m < CH * HW; ++m) {
            const int e = n * CH * HW + m, zi = n * 2 * CH * HW + m, ri = zi + CH * HW;
            wz[e] = sigmoid_d(a_zr[zi]);
            wrh[e] = sigmoid_d(a_zr[ri]) * h[e];
            wout[e] = (1.0 - z[e]) * h[e] + (double)z[e] * tanh(a_q[e]);
        }
    CHECK(close_to(raw_zr, a_zr, 2 * NM, "raw (gate)") && close_to(raw_q, a_q, NM, "raw (blend)"));
    CHECK(close_to(z, wz, NM, "z") && close_to(rh, wrh, NM, "rh") && close_to(out, wout, NM, "out_h"));
    float* all[] = {d_h, d_x, d_w_zr_h, d_w_zr_x, d_b_zr, d_w_q_h, d_w_q_x, d_b_q, d_z, d_rh, d_out, d_raw_zr, d_raw_q};
    for (size_t i = 0; i < sizeof all / sizeof all[0]; ++i) hipFree(all[i]);
    return 0;
}

int main(int argc, char** argv) {
    if (host_checks()) return 1;
    printf("GRU CONV C ABI HOST CHECKS OK\n");
    if (argc > 1 && strcmp(argv[1], "--host-only") == 0) return 0;
    if (gpu_case(1, 5) || gpu_case(3, 3)) return 1;
    printf("GRU CONV C ABI SMOKE OK\n");
    return 0;
}

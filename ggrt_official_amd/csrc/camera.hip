// camera.hip — per-view camera quantities of the call site in ONE small launch (gfx950).
//
// Reference cuda_splatting.py:66-73 (1/near renormalisation), :82-84 + ggrt/geometry/projection.py:233-247
// (fov from the normalised intrinsics), :18-46 (GGRt's projection matrix — built from intrinsics[0] for EVERY
// view), :86-89 (view = inverse(extrinsics)ᵀ, full = view @ projectionᵀ) run ≈ 40 tiny torch kernels plus two
// blocking copies (four host→device constants, tan(fov/2) back to the host) before the first rasterizer call.
// Here: one thread per view, fp64 inside, results rounded to fp32 once; tan(fov/2) and 1/near stay on the
// device (GgrSettings.tanfov_dev, GgrForwardIn.input_scale), so the whole call site can run without a host sync.
#include "ggr_common.h"

namespace ggr {

__device__ __forceinline__ bool invert4(const double* m, double* inv) {
    // Gauss-Jordan with partial pivoting on [m | I]
    double a[4][8];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) { a[i][j] = m[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 4; c++) {
        int piv = c;
        for (int r = c + 1; r < 4; r++) if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (a[piv][c] == 0.0) return false;
        if (piv != c) for (int j = 0; j < 8; j++) { const double t = a[c][j]; a[c][j] = a[piv][j]; a[piv][j] = t; }
        const double d = 1.0 / a[c][c];
        for (int j = 0; j < 8; j++) a[c][j] *= d;
        for (int r = 0; r < 4; r++) {
            if (r == c) continue;
            const double f = a[r][c];
            if (f != 0.0) for (int j = 0; j < 8; j++) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) inv[4 * i + j] = a[i][4 + j];
    return true;
}

__device__ __forceinline__ void k_inv_ray(const double* K, double u, double v, double* d) {
    // d = normalise(K⁻¹ · (u, v, 1)), K 3×3 (adjugate form; any non-singular K)
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[2] * K[7] - K[1] * K[8], c02 = K[1] * K[5] - K[2] * K[4];
    const double c10 = K[5] * K[6] - K[3] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[2] * K[3] - K[0] * K[5];
    const double c20 = K[3] * K[7] - K[4] * K[6], c21 = K[1] * K[6] - K[0] * K[7], c22 = K[0] * K[4] - K[1] * K[3];
    const double det = K[0] * c00 + K[1] * c10 + K[2] * c20;
    double x = (c00 * u + c01 * v + c02) / det, y = (c10 * u + c11 * v + c12) / det, z = (c20 * u + c21 * v + c22) / det;
    const double n = sqrt(x * x + y * y + z * z);
    d[0] = x / n; d[1] = y / n; d[2] = z / n;
}

__global__ void camera_setup_kernel(int n, const float* __restrict__ extrinsics /*[n,4,4] camera-to-world*/,
                                    const float* __restrict__ intrinsics /*[n,3,3] normalised*/,
                                    const float* __restrict__ near, const float* __restrict__ far,
                                    int scale_invariant, float* __restrict__ view /*[n,16]*/,
                                    float* __restrict__ full /*[n,16]*/, float* __restrict__ campos /*[n,3]*/,
                                    float* __restrict__ tanfov /*[n,2]*/, float* __restrict__ scale /*[n]*/) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // the reference multiplies in fp32 (scale = 1/near; t·scale; near·scale; far·scale): keep those roundings
    const float s = scale_invariant ? 1.0f / near[i] : 1.0f;
    scale[i] = s;
    const float nr = scale_invariant ? near[i] * s : near[i], fr = scale_invariant ? far[i] * s : far[i];
    double E[16], Ei[16];
    for (int k = 0; k < 16; k++) E[k] = (double)extrinsics[16 * (size_t)i + k];
    for (int r = 0; r < 3; r++) {
        const float t = scale_invariant ? extrinsics[16 * (size_t)i + 4 * r + 3] * s : extrinsics[16 * (size_t)i + 4 * r + 3];
        E[4 * r + 3] = (double)t;
        campos[3 * i + r] = t;
    }
    if (!invert4(E, Ei)) for (int k = 0; k < 16; k++) Ei[k] = nan("");
    // view = inverse(extrinsics)ᵀ  (row-vector convention of the rasterizer)
    double V[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) V[4 * r + c] = Ei[4 * c + r];
    for (int k = 0; k < 16; k++) view[16 * (size_t)i + k] = (float)V[k];
    // fov: angle between the rays through the mid-points of opposite image edges
    double K[9], l[3], r_[3], t_[3], b_[3];
    for (int k = 0; k < 9; k++) K[k] = (double)intrinsics[9 * (size_t)i + k];
    k_inv_ray(K, 0.0, 0.5, l); k_inv_ray(K, 1.0, 0.5, r_); k_inv_ray(K, 0.5, 0.0, t_); k_inv_ray(K, 0.5, 1.0, b_);
    const double fovx = acos(fmin(1.0, fmax(-1.0, l[0] * r_[0] + l[1] * r_[1] + l[2] * r_[2])));
    const double fovy = acos(fmin(1.0, fmax(-1.0, t_[0] * b_[0] + t_[1] * b_[1] + t_[2] * b_[2])));
    tanfov[2 * i] = (float)tan(0.5 * fovx);
    tanfov[2 * i + 1] = (float)tan(0.5 * fovy);
    // GGRt's projection (cuda_splatting.py:18-46): X/Y rows from intrinsics[0] for every view, fp32 products
    const float k00 = intrinsics[0], k11 = intrinsics[4], k02 = intrinsics[2], k12 = intrinsics[5];
    double Pm[16] = {0};
    Pm[0] = (double)(2.0f * nr * k00);
    Pm[5] = (double)(2.0f * nr * k11);
    Pm[2] = (double)(2.0f * k02 - 1.0f);
    Pm[6] = (double)(2.0f * k12 - 1.0f);
    Pm[14] = 1.0;
    Pm[10] = (double)(fr / (fr - nr));
    Pm[11] = (double)(-(fr * nr) / (fr - nr));
    // full = view @ Pmᵀ
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double a = 0.0;
            for (int k = 0; k < 4; k++) a += V[4 * r + k] * Pm[4 * c + k];
            full[16 * (size_t)i + 4 * r + c] = (float)a;
        }
}

void launch_camera_setup(int n, const float* extrinsics, const float* intrinsics, const float* near, const float* far,
                         int scale_invariant, float* view, float* full, float* campos, float* tanfov, float* scale,
                         hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(camera_setup_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, extrinsics, intrinsics, near, far,
                       scale_invariant, view, full, campos, tanfov, scale);
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// dL/d(K) through one ray d = normalise(K⁻¹·(u, v, 1)): with q = K⁻¹·p, dL/dq = (g − d·(d·g))/|q| and dL/dK = −K⁻ᵀ·dL/dq·qᵀ
__device__ __forceinline__ void k_inv_ray_bwd(const double* Kinv, double u, double v, const double* g, double* dK) {
    const double q[3] = {Kinv[0] * u + Kinv[1] * v + Kinv[2], Kinv[3] * u + Kinv[4] * v + Kinv[5],
                         Kinv[6] * u + Kinv[7] * v + Kinv[8]};
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double d[3] = {q[0] / n, q[1] / n, q[2] / n};
    const double dg = d[0] * g[0] + d[1] * g[1] + d[2] * g[2];
    const double gq[3] = {(g[0] - d[0] * dg) / n, (g[1] - d[1] * dg) / n, (g[2] - d[2] * dg) / n};
    for (int a = 0; a < 3; a++) {
        const double w = Kinv[a] * gq[0] + Kinv[3 + a] * gq[1] + Kinv[6 + a] * gq[2];   // (K⁻ᵀ·gq)[a]
        for (int b = 0; b < 3; b++) dK[3 * a + b] -= w * q[b];
    }
}

// dL/dK of tan(fov/2), fov = acos(clamp(d(u0,v0)·d(u1,v1))), times the upstream gradient g (0 where the clamp acted)
__device__ __forceinline__ void tanfov_bwd(const double* K, const double* Kinv, double u0, double v0, double u1, double v1,
                                           double g, double* dK) {
    double d0[3], d1[3];
    k_inv_ray(K, u0, v0, d0); k_inv_ray(K, u1, v1, d1);
    const double c = d0[0] * d1[0] + d0[1] * d1[1] + d0[2] * d1[2];
    if (!(c > -1.0 && c < 1.0)) return;   // (also a NaN: the forward's clamp gave ±1 there)
    const double th = tan(0.5 * acos(c));
    const double gc = g * 0.5 * (1.0 + th * th) * (-1.0 / sqrt(1.0 - c * c));
    const double g0[3] = {gc * d1[0], gc * d1[1], gc * d1[2]}, g1[3] = {gc * d0[0], gc * d0[1], gc * d0[2]};
    k_inv_ray_bwd(Kinv, u0, v0, g0, dK);
    k_inv_ray_bwd(Kinv, u1, v1, g1, dK);
}

// One launch, ONE block: thread t takes views t, t + 256, … (one thread per view up to 256 views), fp64 inside like the
// forward, which it re-runs for the view matrix.  The projection's four intrinsics-dependent entries are built from
// intrinsics[0] for EVERY view, so their gradients from all n views meet in row 0 of dL/dintrinsics: each thread sums its
// own views in ascending order, thread 0 then the 256 partials in ascending order — no atomics, bit-reproducible.
// A singular extrinsic (the forward wrote NaN) gives NaN gradients.  near / far get none.
#define GGR_CAMB_THREADS 256
__global__ void __launch_bounds__(GGR_CAMB_THREADS)
camera_setup_bwd_kernel(int n, const float* __restrict__ extrinsics, const float* __restrict__ intrinsics,
                        const float* __restrict__ near, const float* __restrict__ far, int scale_invariant,
                        const float* __restrict__ g_view /*[n,16]*/, const float* __restrict__ g_full /*[n,16]*/,
                        const float* __restrict__ g_campos /*[n,3]*/, const float* __restrict__ g_tanfov /*[n,2]*/,
                        float* __restrict__ dE_out /*[n,16]*/, float* __restrict__ dK_out /*[n,9]*/) {
    __shared__ double part[GGR_CAMB_THREADS][4];
    const int tid = threadIdx.x;
    double pk[4] = {0.0, 0.0, 0.0, 0.0};   // Σ over this thread's views of dL/d(k00, k11, k02, k12) of intrinsics[0]
    double row0[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // (thread 0) view 0's own fov terms
    for (int i = tid; i < n; i += GGR_CAMB_THREADS) {
        // ---- the forward's quantities, with its fp32 roundings ----
        const float s = scale_invariant ? 1.0f / near[i] : 1.0f;
        const float nr = scale_invariant ? near[i] * s : near[i], fr = scale_invariant ? far[i] * s : far[i];
        double E[16], Ei[16];
        for (int k = 0; k < 16; k++) E[k] = (double)extrinsics[16 * (size_t)i + k];
        for (int r = 0; r < 3; r++) {
            const float t = scale_invariant ? extrinsics[16 * (size_t)i + 4 * r + 3] * s : extrinsics[16 * (size_t)i + 4 * r + 3];
            E[4 * r + 3] = (double)t;
        }
        if (!invert4(E, Ei)) for (int k = 0; k < 16; k++) Ei[k] = nan("");
        double Pm[16] = {0};
        Pm[0] = (double)(2.0f * nr * intrinsics[0]);
        Pm[5] = (double)(2.0f * nr * intrinsics[4]);
        Pm[2] = (double)(2.0f * intrinsics[2] - 1.0f);
        Pm[6] = (double)(2.0f * intrinsics[5] - 1.0f);
        Pm[14] = 1.0;
        Pm[10] = (double)(fr / (fr - nr));
        Pm[11] = (double)(-(fr * nr) / (fr - nr));
        // ---- full = V·Pmᵀ:  dV = dview + dfull·Pm,  dPm = dfullᵀ·V  (V[r][k] = Ei[k][r]) ----
        double gF[16], dV[16];
        for (int k = 0; k < 16; k++) { gF[k] = (double)g_full[16 * (size_t)i + k]; dV[k] = (double)g_view[16 * (size_t)i + k]; }
        for (int r = 0; r < 4; r++)
            for (int k = 0; k < 4; k++) {
                double a = 0.0;
                for (int c = 0; c < 4; c++) a += gF[4 * r + c] * Pm[4 * c + k];
                dV[4 * r + k] += a;
            }
        double dP0 = 0.0, dP5 = 0.0, dP2 = 0.0, dP6 = 0.0;   // dPm[c][k] = Σ_r dfull[r][c]·V[r][k]
        for (int r = 0; r < 4; r++) {
            dP0 += gF[4 * r + 0] * Ei[4 * 0 + r];
            dP2 += gF[4 * r + 0] * Ei[4 * 2 + r];
            dP5 += gF[4 * r + 1] * Ei[4 * 1 + r];
            dP6 += gF[4 * r + 1] * Ei[4 * 2 + r];
        }
        pk[0] += 2.0 * (double)nr * dP0; pk[1] += 2.0 * (double)nr * dP5; pk[2] += 2.0 * dP2; pk[3] += 2.0 * dP6;
        // ---- V = inverse(E′)ᵀ:  dEi = dVᵀ,  dE′ = −Eiᵀ·dEi·Eiᵀ ----
        double T[16];   // T = dEi·Eiᵀ:  T[a][b] = Σ_k dV[k][a]·Ei[b][k]
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                double x = 0.0;
                for (int k = 0; k < 4; k++) x += dV[4 * k + a] * Ei[4 * b + k];
                T[4 * a + b] = x;
            }
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                double x = 0.0;
                for (int k = 0; k < 4; k++) x += Ei[4 * k + a] * T[4 * k + b];
                x = -x;
                // the translation column is extrinsics·scale, and campos is that column
                if (b == 3 && a < 3) x = (x + (double)g_campos[3 * (size_t)i + a]) * (double)s;
                dE_out[16 * (size_t)i + 4 * a + b] = (float)x;
            }
        // ---- tan(fov/2) into the view's own intrinsics ----
        double K[9], Kinv[9], dK[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 9; k++) K[k] = (double)intrinsics[9 * (size_t)i + k];
        {
            const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[2] * K[7] - K[1] * K[8], c02 = K[1] * K[5] - K[2] * K[4];
            const double c10 = K[5] * K[6] - K[3] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[2] * K[3] - K[0] * K[5];
            const double c20 = K[3] * K[7] - K[4] * K[6], c21 = K[1] * K[6] - K[0] * K[7], c22 = K[0] * K[4] - K[1] * K[3];
            const double det = K[0] * c00 + K[1] * c10 + K[2] * c20;
            Kinv[0] = c00 / det; Kinv[1] = c01 / det; Kinv[2] = c02 / det;
            Kinv[3] = c10 / det; Kinv[4] = c11 / det; Kinv[5] = c12 / det;
            Kinv[6] = c20 / det; Kinv[7] = c21 / det; Kinv[8] = c22 / det;
        }
        tanfov_bwd(K, Kinv, 0.0, 0.5, 1.0, 0.5, (double)g_tanfov[2 * (size_t)i], dK);
        tanfov_bwd(K, Kinv, 0.5, 0.0, 0.5, 1.0, (double)g_tanfov[2 * (size_t)i + 1], dK);
        if (i == 0) {
            for (int k = 0; k < 9; k++) row0[k] = dK[k];
        } else {
            for (int k = 0; k < 9; k++) dK_out[9 * (size_t)i + k] = (float)dK[k];
        }
    }
    for (int k = 0; k < 4; k++) part[tid][k] = pk[k];
    __syncthreads();
    if (tid == 0) {
        double tot[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = 0; t < GGR_CAMB_THREADS; t++)
            for (int k = 0; k < 4; k++) tot[k] += part[t][k];
        row0[0] += tot[0]; row0[4] += tot[1]; row0[2] += tot[2]; row0[5] += tot[3];
        for (int k = 0; k < 9; k++) dK_out[k] = (float)row0[k];
    }
}

void launch_camera_setup_bwd(int n, const float* extrinsics, const float* intrinsics, const float* near, const float* far,
                             int scale_invariant, const float* dL_dview, const float* dL_dfull, const float* dL_dcampos,
                             const float* dL_dtanfov, float* dL_dextrinsics, float* dL_dintrinsics, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(camera_setup_bwd_kernel, dim3(1), dim3(GGR_CAMB_THREADS), 0, s, n, extrinsics, intrinsics, near, far,
                       scale_invariant, dL_dview, dL_dfull, dL_dcampos, dL_dtanfov, dL_dextrinsics, dL_dintrinsics);
}

}  // namespace ggr

// adapter.hip — the Gaussian adapter pass: GGRt's encoder tail in one forward and one backward launch.
//
// Per Gaussian p = c·G + g of camera c (raw row r = g / spp, shared by `spp` consecutive Gaussians):
//   v = Kinv·(x, y, 1), u = v/|v|, means = t + (R·u)·depth                                   (c2w = [R | t])
//   scales = (scale_min + (scale_max − scale_min)·σ(raw[0:3]))·depth·scale_mult
//   quats  = q_cam ⊗ (q/(|q| + eps)), q = raw[3:7] as xyzw, result wxyz                      (adapter_scale_rotation's convention)
//   harmonics[ch, band] = D_band·(mask_band ⊙ raw_sh[ch, band]),  D_band = the band's diagonal block of sh_transform[c]
//
// Layout.  A raw row is 7 + 3·d_sh floats (82 at d_sh = 25: 328 B) and a harmonics row 3·d_sh (75: 300 B): neither is a multiple
// of 16 B, and a lane that walked its own row in global memory would touch 64 cache lines per wave-instruction.  So the rows go
// through LDS: a workgroup is ONE wave and owns tiles of 64 consecutive raw rows of one camera — 64·328 B of contiguous memory —
// which it copies into LDS one dword per lane (256 contiguous bytes per wave-instruction, whatever the tile's alignment: only a
// float's alignment is asked of any buffer), at an odd row pitch, so that lane i then reads row i without bank conflicts.  Rows
// leave the same way (harmonics forward, dL/draw backward): each lane puts its row into LDS, the wave streams the tile out.  With
// spp > 1 a tile's 64·spp harmonics rows pass through the same LDS region in pieces of 64.  21 KiB of LDS per wave: 7 waves per
// CU, each with a whole tile in flight.  The small per-Gaussian arrays (1–4 floats) are read and written directly, 4 B per lane at a
// 4–16 B stride: a wave's accesses cover whole lines between them.
//
// One lane owns one raw row and walks its spp Gaussians itself: dL/draw is summed in registers, no atomics.  The grid is
// (chunks, C): a workgroup never sees two cameras, strides over its camera's tiles and keeps the per-camera gradient sums
// (c2w 12, Kinv 9, q_cam 4, scale_mult 1, and — only in the kernel instantiated for it — the 165 entries of the sh_transform
// blocks) in registers across ALL its tiles; at the end one butterfly reduction per sum and one float atomic per workgroup and
// entry into the zero-initialised [C, …] buffers.
#include "adapter.h"
#include <algorithm>

namespace ggr {

namespace {

constexpr int TILE = kAdapterTile;

__host__ __device__ constexpr int isqrt_c(int n) { int l = 0; while ((l + 1) * (l + 1) <= n) ++l; return l; }
// offset of band l's (2l+1)² block in the packed block list: Σ_{k<l} (2k+1)²
__host__ __device__ constexpr int block_off(int l) { return l * (2 * l - 1) * (2 * l + 1) / 3; }

template <int DSH> struct Dim {
    static constexpr int L = isqrt_c(DSH);        // bands
    static constexpr int W = 7 + 3 * DSH;         // floats of a raw row
    static constexpr int WP = W | 1;              // its pitch in LDS (odd)
    static constexpr int H = 3 * DSH;             // floats of a harmonics row
    static constexpr int HP = H | 1;
    static constexpr int NB = block_off(L);       // floats of the packed blocks (165 at d_sh = 25)
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the blocks of sh_transform[c], each column times its mask entry, and the mask, into LDS (read wave-uniformly afterwards)
template <int DSH>
__device__ __forceinline__ void load_blocks(const float* __restrict__ sh_transform, const float* __restrict__ sh_mask, int c,
                                            int lane, float* dm, float* msk) {
    using S = Dim<DSH>;
    const float* T = sh_transform + (size_t)c * DSH * DSH;
    for (int l = 0; l < S::L; ++l) {
        const int n = 2 * l + 1, o = block_off(l), b = l * l;
        for (int e = lane; e < n * n; e += TILE) {
            const int i = e / n, j = e - i * n;
            dm[o + e] = T[(b + i) * DSH + b + j] * sh_mask[b + j];
        }
    }
    for (int e = lane; e < DSH; e += TILE) msk[e] = sh_mask[e];
}

struct Camera {
    float R[9], t[3], K[9], q[4], mult;
};

__device__ __forceinline__ Camera load_camera(const AdapterArgs& a, int c) {
    Camera cam;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { cam.R[3 * i + j] = a.c2w[c * 12 + 4 * i + j]; cam.K[3 * i + j] = a.Kinv[c * 9 + 3 * i + j]; }
        cam.t[i] = a.c2w[c * 12 + 4 * i + 3];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cam.q[i] = a.q_cam[c * 4 + i];
    cam.mult = a.scale_mult[c];
    return cam;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

template <int DSH>
__global__ void __launch_bounds__(TILE)
adapter_fwd_kernel(const AdapterArgs a, const int tiles_per_cam) {
    using S = Dim<DSH>;
    __shared__ float tile[TILE * S::WP];
    __shared__ float dm[S::NB];
    __shared__ float msk[DSH];
    const int c = blockIdx.y, lane = threadIdx.x, spp = a.spp, R = a.G / spp;
    const Camera cam = load_camera(a, c);
    load_blocks<DSH>(a.sh_transform, a.sh_mask, c, lane, dm, msk);
    const float cw = cam.q[0], cx = cam.q[1], cy = cam.q[2], cz = cam.q[3];

    for (int t = blockIdx.x; t < tiles_per_cam; t += gridDim.x) {
        const int r0 = t * TILE, nrows = min(TILE, R - r0);
        const bool live = lane < nrows;
        const float* __restrict__ src = a.raw + ((size_t)c * R + r0) * S::W;
        __syncthreads();   // (the previous tile's last piece has left; dm / msk are written)
        for (int i = lane; i < nrows * S::W; i += TILE) tile[(i / S::W) * S::WP + i % S::W] = src[i];
        __syncthreads();
        float row[S::W];
#pragma unroll
        for (int k = 0; k < S::W; ++k) row[k] = live ? tile[lane * S::WP + k] : 0.f;
        __syncthreads();

        // the row's quaternion and scale factors: the same for its spp Gaussians
        const float nq = sqrtf(row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
        const float inv = 1.f / (nq + a.eps);
        const float x = row[3] * inv, y = row[4] * inv, z = row[5] * inv, w = row[6] * inv;
        const float q0 = cw * w - cx * x - cy * y - cz * z, q1 = cw * x + cx * w + cy * z - cz * y;
        const float q2 = cw * y - cx * z + cy * w + cz * x, q3 = cw * z + cx * y - cy * x + cz * w;
        float base[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) base[k] = a.scale_min + (a.scale_max - a.scale_min) * sigmoidf(row[k]);

        if (live) {
            for (int s = 0; s < spp; ++s) {
                const size_t p = (size_t)c * a.G + (size_t)(r0 + lane) * spp + s;
                const float d = a.depth[p], px = a.coords[2 * p], py = a.coords[2 * p + 1];
                float v[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) v[i] = cam.K[3 * i] * px + cam.K[3 * i + 1] * py + cam.K[3 * i + 2];
                const float rn = 1.f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                const float u0 = v[0] * rn, u1 = v[1] * rn, u2 = v[2] * rn;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    a.means[3 * p + i] = cam.t[i] + (cam.R[3 * i] * u0 + cam.R[3 * i + 1] * u1 + cam.R[3 * i + 2] * u2) * d;
                    a.scales[3 * p + i] = base[i] * d * cam.mult;
                }
                a.quats[4 * p] = q0; a.quats[4 * p + 1] = q1; a.quats[4 * p + 2] = q2; a.quats[4 * p + 3] = q3;
            }
        }

        // harmonics: per band and channel  h = (D·diag(mask))·raw_sh
        float h[S::H];
#pragma unroll
        for (int l = 0; l < S::L; ++l) {
            const int n = 2 * l + 1, o = block_off(l), b = l * l;
#pragma unroll
            for (int i = 0; i < n; ++i) {
                float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < n; ++j) {
                    const float dij = dm[o + i * n + j];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] += dij * row[7 + ch * DSH + b + j];
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) h[ch * DSH + b + i] = acc[ch];
            }
        }
        // out through LDS, 64 Gaussians a piece: Gaussian r·spp + s of the tile holds row r's harmonics
        const int ng = nrows * spp;
        for (int g0 = 0; g0 < ng; g0 += TILE) {
            if (g0) __syncthreads();
            if (live) {
                for (int s = 0; s < spp; ++s) {
                    const int j = lane * spp + s - g0;
                    if (j >= 0 && j < TILE) {
#pragma unroll
                        for (int k = 0; k < S::H; ++k) tile[j * S::HP + k] = h[k];
                    }
                }
            }
            __syncthreads();
            const int cnt = min(TILE, ng - g0);
            float* __restrict__ dst = a.harmonics + ((size_t)c * a.G + (size_t)r0 * spp + g0) * S::H;
            for (int i = lane; i < cnt * S::H; i += TILE) dst[i] = tile[(i / S::H) * S::HP + i % S::H];
        }
    }
}

template <int DSH, bool DD>
__global__ void __launch_bounds__(TILE)
adapter_bwd_kernel(const AdapterArgs a, const int tiles_per_cam) {
    using S = Dim<DSH>;
    __shared__ float tile[TILE * S::WP];
    __shared__ float dm[S::NB];
    __shared__ float msk[DSH];
    const int c = blockIdx.y, lane = threadIdx.x, spp = a.spp, R = a.G / spp;
    const Camera cam = load_camera(a, c);
    load_blocks<DSH>(a.sh_transform, a.sh_mask, c, lane, dm, msk);
    const float cw = cam.q[0], cx = cam.q[1], cy = cam.q[2], cz = cam.q[3];
    const float span = a.scale_max - a.scale_min;

    // this lane's share of the per-camera sums, over all tiles of the workgroup
    float aR[9] = {}, at[3] = {}, aK[9] = {}, aq[4] = {}, am = 0.f;
    float aD[DD ? S::NB : 1] = {};

    for (int t = blockIdx.x; t < tiles_per_cam; t += gridDim.x) {
        const int r0 = t * TILE, nrows = min(TILE, R - r0);
        const bool live = lane < nrows;
        const float* __restrict__ src = a.raw + ((size_t)c * R + r0) * S::W;
        __syncthreads();   // (the previous tile has left; dm / msk are written)
        for (int i = lane; i < nrows * S::W; i += TILE) tile[(i / S::W) * S::WP + i % S::W] = src[i];
        __syncthreads();
        float row[S::W];
#pragma unroll
        for (int k = 0; k < S::W; ++k) row[k] = live ? tile[lane * S::WP + k] : 0.f;

        // Σ over the row's spp Gaussians of dL/dharmonics, the tile's 64·spp rows passing through LDS 64 at a time
        float gh[S::H];
#pragma unroll
        for (int k = 0; k < S::H; ++k) gh[k] = 0.f;
        const int ng = nrows * spp;
        for (int g0 = 0; g0 < ng; g0 += TILE) {
            __syncthreads();
            const int cnt = min(TILE, ng - g0);
            const float* __restrict__ gsrc = a.g_harmonics + ((size_t)c * a.G + (size_t)r0 * spp + g0) * S::H;
            for (int i = lane; i < cnt * S::H; i += TILE) tile[(i / S::H) * S::HP + i % S::H] = gsrc[i];
            __syncthreads();
            if (live) {
                for (int s = 0; s < spp; ++s) {
                    const int j = lane * spp + s - g0;
                    if (j >= 0 && j < TILE) {
#pragma unroll
                        for (int k = 0; k < S::H; ++k) gh[k] += tile[j * S::HP + k];
                    }
                }
            }
        }
        __syncthreads();   // (the last piece is read: the region takes dL/draw next)

        const float nq = sqrtf(row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
        const float inv = 1.f / (nq + a.eps);
        const float x = row[3] * inv, y = row[4] * inv, z = row[5] * inv, w = row[6] * inv;
        float sg[3], base[3], dlogit[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 3; ++k) { sg[k] = sigmoidf(row[k]); base[k] = a.scale_min + span * sg[k]; }

        if (live) {
            for (int s = 0; s < spp; ++s) {
                const size_t p = (size_t)c * a.G + (size_t)(r0 + lane) * spp + s;
                const float d = a.depth[p], px = a.coords[2 * p], py = a.coords[2 * p + 1];
                const float gm[3] = {a.g_means[3 * p], a.g_means[3 * p + 1], a.g_means[3 * p + 2]};
                const float gs[3] = {a.g_scales[3 * p], a.g_scales[3 * p + 1], a.g_scales[3 * p + 2]};
#pragma unroll
                for (int k = 0; k < 4; ++k) gq[k] += a.g_quats[4 * p + k];
                float v[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) v[i] = cam.K[3 * i] * px + cam.K[3 * i + 1] * py + cam.K[3 * i + 2];
                const float rn = 1.f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                const float u[3] = {v[0] * rn, v[1] * rn, v[2] * rn};
                float gd = 0.f, du[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float wi = cam.R[3 * i] * u[0] + cam.R[3 * i + 1] * u[1] + cam.R[3 * i + 2] * u[2];
                    const float dwi = gm[i] * d;
                    gd += gm[i] * wi + gs[i] * base[i] * cam.mult;
                    at[i] += gm[i];
                    am += gs[i] * base[i] * d;
                    dlogit[i] += gs[i] * d * cam.mult * span * sg[i] * (1.f - sg[i]);
#pragma unroll
                    for (int j = 0; j < 3; ++j) { aR[3 * i + j] += dwi * u[j]; du[j] += cam.R[3 * i + j] * dwi; }
                }
                const float udu = u[0] * du[0] + u[1] * du[1] + u[2] * du[2];
                float gx = 0.f, gy = 0.f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float dv = (du[i] - u[i] * udu) * rn;
                    aK[3 * i] += dv * px; aK[3 * i + 1] += dv * py; aK[3 * i + 2] += dv;
                    gx += dv * cam.K[3 * i]; gy += dv * cam.K[3 * i + 1];
                }
                if (a.g_depth) a.g_depth[p] = gd;
                if (a.g_coords) { a.g_coords[2 * p] = gx; a.g_coords[2 * p + 1] = gy; }
            }
        }
        // quats = q_cam ⊗ qn, qn = q·inv: the product's two sides, then the normalisation (|q| = 0: its subgradient 0, as torch)
        if (live) {
            aq[0] += gq[0] * w + gq[1] * x + gq[2] * y + gq[3] * z;
            aq[1] += -gq[0] * x + gq[1] * w - gq[2] * z + gq[3] * y;
            aq[2] += -gq[0] * y + gq[1] * z + gq[2] * w - gq[3] * x;
            aq[3] += -gq[0] * z - gq[1] * y + gq[2] * x + gq[3] * w;
        }
        const float dn[4] = {-gq[0] * cx + gq[1] * cw + gq[2] * cz - gq[3] * cy, -gq[0] * cy - gq[1] * cz + gq[2] * cw + gq[3] * cx,
                             -gq[0] * cz + gq[1] * cy - gq[2] * cx + gq[3] * cw, gq[0] * cw + gq[1] * cx + gq[2] * cy + gq[3] * cz};
        const float qdn = dn[0] * row[3] + dn[1] * row[4] + dn[2] * row[5] + dn[3] * row[6];
        const float fall = nq > 0.f ? qdn * inv * inv / nq : 0.f;

        if (live) {
            float* out = tile + lane * S::WP;
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = dlogit[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) out[3 + k] = dn[k] * inv - row[3 + k] * fall;
            // dL/draw_sh = diag(mask)·Dᵀ·gh per band and channel; dL/dD_band += gh ⊗ (mask ⊙ raw_sh)
#pragma unroll
            for (int l = 0; l < S::L; ++l) {
                const int n = 2 * l + 1, o = block_off(l), b = l * l;
#pragma unroll
                for (int j = 0; j < n; ++j) {
                    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < n; ++i) {
                        const float dij = dm[o + i * n + j];
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) acc[ch] += dij * gh[ch * DSH + b + i];
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) out[7 + ch * DSH + b + j] = acc[ch];
                }
                if (DD) {
#pragma unroll
                    for (int j = 0; j < n; ++j) {
                        const float mj = msk[b + j];
                        const float xs[3] = {mj * row[7 + b + j], mj * row[7 + DSH + b + j], mj * row[7 + 2 * DSH + b + j]};
#pragma unroll
                        for (int i = 0; i < n; ++i)
                            aD[DD ? o + i * n + j : 0] += gh[b + i] * xs[0] + gh[DSH + b + i] * xs[1] + gh[2 * DSH + b + i] * xs[2];
                    }
                }
            }
        }
        __syncthreads();
        float* __restrict__ dst = a.g_raw + ((size_t)c * R + r0) * S::W;
        for (int i = lane; i < nrows * S::W; i += TILE) dst[i] = tile[(i / S::W) * S::WP + i % S::W];
    }

    // the per-camera sums: across the wave, then one atomic per workgroup and entry
    if (a.g_c2w) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { const float v = wave_sum(aR[3 * i + j]); if (lane == 0) atomicAdd(a.g_c2w + c * 12 + 4 * i + j, v); }
            const float v = wave_sum(at[i]);
            if (lane == 0) atomicAdd(a.g_c2w + c * 12 + 4 * i + 3, v);
        }
    }
    if (a.g_Kinv) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { const float v = wave_sum(aK[k]); if (lane == 0) atomicAdd(a.g_Kinv + c * 9 + k, v); }
    }
    if (a.g_q_cam) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float v = wave_sum(aq[k]); if (lane == 0) atomicAdd(a.g_q_cam + c * 4 + k, v); }
    }
    if (a.g_scale_mult) { const float v = wave_sum(am); if (lane == 0) atomicAdd(a.g_scale_mult + c, v); }
    if (DD) {
        float* T = a.g_sh_transform + (size_t)c * DSH * DSH;
#pragma unroll
        for (int l = 0; l < S::L; ++l) {
            const int n = 2 * l + 1, o = block_off(l), b = l * l;
#pragma unroll
            for (int i = 0; i < n; ++i) {
#pragma unroll
                for (int j = 0; j < n; ++j) {
                    const float v = wave_sum(aD[DD ? o + i * n + j : 0]);
                    if (lane == 0) atomicAdd(T + (b + i) * DSH + b + j, v);
                }
            }
        }
    }
}

dim3 adapter_grid(const AdapterArgs& a, int* tiles_per_cam) {
    const int R = a.G / a.spp;
    *tiles_per_cam = (R + TILE - 1) / TILE;
    const int chunks = std::max(1, std::min(*tiles_per_cam, kAdapterMaxChunks / a.C));
    return dim3((unsigned)chunks, (unsigned)a.C);
}

template <int DSH>
void launch_bwd(const AdapterArgs& a, dim3 grid, int tiles, hipStream_t s) {
    if (a.g_sh_transform)
        hipLaunchKernelGGL((adapter_bwd_kernel<DSH, true>), grid, dim3(TILE), 0, s, a, tiles);
    else
        hipLaunchKernelGGL((adapter_bwd_kernel<DSH, false>), grid, dim3(TILE), 0, s, a, tiles);
}

}  // namespace

void launch_adapter_forward(const AdapterArgs& a, hipStream_t s) {
    if (a.C <= 0 || a.G <= 0) return;
    int tiles = 0;
    const dim3 grid = adapter_grid(a, &tiles);
    switch (a.d_sh) {
        case 1: hipLaunchKernelGGL(adapter_fwd_kernel<1>, grid, dim3(TILE), 0, s, a, tiles); break;
        case 4: hipLaunchKernelGGL(adapter_fwd_kernel<4>, grid, dim3(TILE), 0, s, a, tiles); break;
        case 9: hipLaunchKernelGGL(adapter_fwd_kernel<9>, grid, dim3(TILE), 0, s, a, tiles); break;
        case 16: hipLaunchKernelGGL(adapter_fwd_kernel<16>, grid, dim3(TILE), 0, s, a, tiles); break;
        default: hipLaunchKernelGGL(adapter_fwd_kernel<25>, grid, dim3(TILE), 0, s, a, tiles); break;
    }
}

void launch_adapter_backward(const AdapterArgs& a, hipStream_t s) {
    if (a.C <= 0 || a.G <= 0) return;
    int tiles = 0;
    const dim3 grid = adapter_grid(a, &tiles);
    switch (a.d_sh) {
        case 1: launch_bwd<1>(a, grid, tiles, s); break;
        case 4: launch_bwd<4>(a, grid, tiles, s); break;
        case 9: launch_bwd<9>(a, grid, tiles, s); break;
        case 16: launch_bwd<16>(a, grid, tiles, s); break;
        default: launch_bwd<25>(a, grid, tiles, s); break;
    }
}

}  // namespace ggr

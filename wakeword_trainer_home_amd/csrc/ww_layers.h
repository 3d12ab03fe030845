// Internal declarations shared by the generic channels-last layer library (ww_nhwc.hip), the squeeze-excitation block (ww_se.hip)
// and the matrix-core GEMMs (ww_linear.hip, ww_gemm16.hip) -- the MobileNetV3 body of SURVEY.md §8f rank 2.
#pragma once
#include "ww_internal.h"
#include <algorithm>

// The activations a layer can fuse (WW_LIN_*) and their derivatives with torch's conventions at the kinks: relu'(0) = 0,
// hardswish'(-3) = 0 and hardswish'(3) = 1, hardsigmoid'(+-3) = 0.  A constant `act` folds at compile time.
__device__ __forceinline__ float lin_act(int act, float z) {
    if (act == WW_LIN_HARDSWISH) return z * fminf(fmaxf(z + 3.f, 0.f), 6.f) * (1.f / 6.f);
    if (act == WW_LIN_RELU) return z < 0.f ? 0.f : z;
    if (act == WW_LIN_HARDSIGMOID) return fminf(fmaxf(z + 3.f, 0.f), 6.f) * (1.f / 6.f);
    return z;
}
__device__ __forceinline__ float lin_act_grad(int act, float z) {      // torch's hardswish / hardsigmoid / relu backward
    if (act == WW_LIN_HARDSWISH) return z <= -3.f ? 0.f : (z < 3.f ? z * (1.f / 3.f) + 0.5f : 1.f);   // 0 at -3, 1 at 3
    if (act == WW_LIN_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == WW_LIN_HARDSIGMOID) return (z > -3.f && z < 3.f) ? (1.f / 6.f) : 0.f;
    return 1.f;
}

// one element of the BatchNorm(+activation) backward apply pass: dx = gamma*rstd*(dz - mean(dz) - xhat*mean(dz*xhat)), dz = da act'(z)
// (training; s1, s2 = the column sums of dz and dz*xhat);  eval: dx = scale*dz
__device__ __forceinline__ float bnact_bwd_one(float xv, float dav, float sc, float sf, float mu, float rs, float s1, float s2,
                                               float invM, int act, int training) {
    const float dz = dav * lin_act_grad(act, fmaf(xv, sc, sf));
    if (!training) return sc * dz;
    const float xh = (xv - mu) * rs;
    return sc * (dz - s1 * invM - xh * s2 * invM);
}

// ---- the tiling of the BatchNorm apply passes that FINISH the statistics themselves (ww_nhwc.hip: k_bn_act_apply_fin,
// k_bnact_bwd_apply_fin; ww_conv2d16.hip: k_bn_bwd_apply_fin16): a workgroup owns (row chunk, group of CG4 <= 16 channel float4s)
struct BnTile { int CG4, G_c, R; long rows_per_block; };
// totals of the group's 2*CG partial columns -> tot[2*CG] (LDS, double).  part rows are [2C] floats.  256 threads.
__device__ __forceinline__ void bn_group_totals(const float *__restrict__ part, int chunks, int C, int c0, int CG4, double *tot,
                                                double *redd /* [256][4] */) {
    const int nq = 2 * CG4;                         // float4 columns of the group (both statistics)
    const int LA = 256 / nq;                        // chunk lanes (>= 8)
    const int k4 = threadIdx.x % nq, la = threadIdx.x / nq;
    // (the clamp is a bounds guard only: where the last group is short, the lanes past C re-read the last quad, and their totals
    //  land in tot entries of channels >= C that no caller reads -- no output depends on it, so no test can see it)
    const int comp = k4 / CG4, cq = k4 - comp * CG4, col = comp * C + min(c0 + 4 * cq, C - 4);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (la < LA)
        for (int q0 = la; q0 < chunks; q0 += 8 * LA) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4 *>(part + (size_t)min(q0 + u * LA, chunks - 1) * 2 * C + col);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (q0 + u * LA < chunks) { a0 += v[u].x; a1 += v[u].y; a2 += v[u].z; a3 += v[u].w; }
        }
    double *r = redd + (size_t)threadIdx.x * 4;
    r[0] = a0; r[1] = a1; r[2] = a2; r[3] = a3;
    __syncthreads();
    if (threadIdx.x < nq) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (int q = 0; q < LA; ++q) {
            const double *u = redd + (size_t)(q * nq + k4) * 4;
            t0 += u[0]; t1 += u[1]; t2 += u[2]; t3 += u[3];
        }
        double *o = tot + comp * 4 * CG4 + 4 * cq;
        o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
    }
    __syncthreads();
}
// (row chunk, channel group) tiling of k_bn_act_apply_fin: the widest group (16, 8 or 4 channel float4s) whose re-read of the
// partials stays <= 32 KB per workgroup; CG4 == 0: too many partial rows, take the finish launch instead
static inline BnTile bn_tile(long M, int C, int chunks) {
    BnTile t = {0, 0, 0, 0};
    const int C4 = C / 4;
    for (int cg4 = 16; cg4 >= 4; cg4 >>= 1) {
        const int G_c = (C4 + cg4 - 1) / cg4, CG4 = (C4 + G_c - 1) / G_c;
        if ((size_t)chunks * 2 * 4 * CG4 * sizeof(float) > 32 * 1024) continue;
        t.G_c = G_c; t.CG4 = CG4; t.R = 256 / CG4;
        const long G_r = std::max<long>(1, std::min<long>(std::max(1, 1024 / G_c), M / (4L * t.R)));
        t.rows_per_block = (M + G_r - 1) / G_r;
        break;
    }
    return t;
}
// ww_nhwc.hip: training-mode BatchNorm(+activation) of x (M, C) whose producer already wrote `chunks` rows of statistics partials
// ([sum (C) | sum of squares (C)] each) to `part`: the apply pass finishes them itself when that is cheap, else finish + apply.
// res (nullable): a residual tensor of x's shape added to the activated output (the inverted-residual skip connection).
int ww_bn_act_from_partials(ww_ctx *ctx, const float *x, long M, int C, const ww_bn_t *bn, int act, float *y, float *ss, float *mr,
                            const float *part, int chunks, const float *res, hipStream_t st);

// ww_nhwc.hip: k_bn_finish (`chunks` rows of [sum | sum of squares] partials -> ss, mr, running statistics; eval: from the running
// statistics) and k_bnact_bwd_finish (partials of [sum dz | sum dz*xhat] -> sums (2C), dbeta, dgamma) as launches of their own
int ww_bn_finish_launch(const float *part, int chunks, long M, int C, const ww_bn_t *bn, float *ss, float *mr, hipStream_t st);
int ww_bnact_bwd_finish_launch(const float *part, int chunks, int C, float *sums, float *dgamma, float *dbeta, hipStream_t st);

// ww_gemm16.hip: ww_gemm16_nt with an optional per-column fp32 bias added in the epilogue
int ww_gemm16_nt_bias(ww_ctx *ctx, int dtype, const void *A, const void *B, void *C, int c_f32, long M, long N, long K,
                      const float *bias, hipStream_t st);

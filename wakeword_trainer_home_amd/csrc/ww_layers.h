// Internal declarations shared by the generic channels-last layer library (ww_nhwc.hip), the squeeze-excitation block (ww_se.hip)
// and the matrix-core GEMMs (ww_linear.hip, ww_gemm16.hip) -- the MobileNetV3 body of SURVEY.md §8f rank 2.
#pragma once
#include "ww_internal.h"

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

// ww_nhwc.hip: training-mode BatchNorm(+activation) of x (M, C) whose producer already wrote `chunks` rows of statistics partials
// ([sum (C) | sum of squares (C)] each) to `part`: the apply pass finishes them itself when that is cheap, else finish + apply.
// res (nullable): a residual tensor of x's shape added to the activated output (the inverted-residual skip connection).
int ww_bn_act_from_partials(ww_ctx *ctx, const float *x, long M, int C, const ww_bn_t *bn, int act, float *y, float *ss, float *mr,
                            const float *part, int chunks, const float *res, hipStream_t st);

// ww_gemm16.hip: ww_gemm16_nt with an optional per-column fp32 bias added in the epilogue
int ww_gemm16_nt_bias(ww_ctx *ctx, int dtype, const void *A, const void *B, void *C, int c_f32, long M, long N, long K,
                      const float *bias, hipStream_t st);

// Integer-only inference of an exported int8 cnn_small bundle (DESIGN.md "Export", the int8 law).
//   k_q8_quantize : fp32 features -> int8, q = clamp(rne(x / s_x) + z_x)
//   k_q8_stem     : 3x3 s2 p1, 1 -> 64 channels, VALU int32
//   k_q8_dw       : depthwise 3x3 p1, VALU int32
//   k_q8_pw       : pointwise 1x1 on v_mfma_i32_16x16x64_i8, its 64x64 weights resident in registers
//   k_q8_dwpw     : the depthwise -> pointwise pair as one kernel (the depthwise output never leaves the registers)
//   k_q8_gap_fc   : sum over HxW, requantise, Linear(64,2), one fp32 multiply per logit
// Activations are int8 NHWC (N,64), N = B*H*W: a pixel is 64 contiguous bytes, the K of one MFMA.  Every conv kernel walks
// tiles of 16 pixels, one tile per wave and trip, with ONE lane map: lane l holds pixel p = l & 15 of the tile and the 16
// channels [16g, 16g + 16), g = l >> 4 -- one 16-byte vector of the pixel's row, on the way in and on the way out.
//
// The pointwise product.  D = A x B with A = weights (row = output channel), B = pixels (column = pixel).  Lane l supplies
// B[k][column p] for the 16 k of its channel group -- exactly the vector it loaded (or, fused, the depthwise output it
// just computed) -- and row l & 15 of A for the same 16 k, so the two operands walk k alike whatever order the instruction
// gives the 16 bytes of a lane.  The accumulator puts rows 4g .. 4g+3 of column p in lane l (C/D map of every 16x16 MFMA).
// Product m (m = 0..3) takes as its row i the output channel 16 (i >> 2) + 4 m + (i & 3), so lane l ends up with channels
// 16 g + 4 m + r (r = 0..3) in register r of product m: sixteen consecutive channels of pixel p, one 16-byte store.
//
// bias arguments are the EFFECTIVE bias q_b - z_in * sum(q_w) (host, once per bundle): the kernels then sum q_w * q_in with the
// border filled with z_in, which is sum q_w (q_in - z_in) + q_b in two's complement.  All adds that may wrap are unsigned.
#include "ww_q8_common.h"

namespace {

constexpr int Q8_BLOCK = 256;
constexpr int Q8_WAVES = Q8_BLOCK / 64;

// the requantisation of every tensor here is the shared law and the unsigned clamp, nothing of its own:
// clamp(-128 + R(acc, m, sh), -128, 127)
__device__ __forceinline__ int q8_requant(int acc, int m, int sh) { return q8_clamp(q8_round(acc, m, sh)); }

struct q8_chan {                      // per-output-channel tables of one conv: (64) int32 each, 16-byte aligned
    const int *bias, *mult, *shift;
};

// requantise the 16 accumulators of channels [c0, c0 + 16) into the 16 bytes of the lane's output vector
__device__ __forceinline__ v4i q8_requant16(const int (&acc)[16], const q8_chan &pc, int c0) {
    v4i out;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const v4i b = *(const v4i *)(pc.bias + c0 + 4 * d);
        const v4i m = *(const v4i *)(pc.mult + c0 + 4 * d);
        const v4i s = *(const v4i *)(pc.shift + c0 + 4 * d);
        int q[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = q8_requant((int)((unsigned)acc[4 * d + r] + (unsigned)b[r]), m[r], s[r]);
        out[d] = q8_pack4(q[0], q[1], q[2], q[3]);
    }
    return out;
}

// acc[c] += w[c] * q[c] over the 16 bytes of two vectors
__device__ __forceinline__ void q8_mac16(int (&acc)[16], const v4i &w, const v4i &q) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        acc[4 * d + 0] += q8_byte<0>(w[d]) * q8_byte<0>(q[d]);
        acc[4 * d + 1] += q8_byte<1>(w[d]) * q8_byte<1>(q[d]);
        acc[4 * d + 2] += q8_byte<2>(w[d]) * q8_byte<2>(q[d]);
        acc[4 * d + 3] += q8_byte<3>(w[d]) * q8_byte<3>(q[d]);
    }
}

// the nine tap vectors of a 3x3 kernel stored (9,64) int8: those of channel group g
__device__ __forceinline__ void q8_load_taps(const int8_t *__restrict__ w, int g, v4i (&wt)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = *(const v4i *)(w + t * 64 + 16 * g);
}

// depthwise 3x3 p1 at pixel n = (b, h, x) of a (B,H,W,64) tensor, channel group g; the border holds the zero point
__device__ __forceinline__ void q8_dw_acc(const int8_t *__restrict__ in, const v4i (&wt)[9], long n, int H, int W, int g, int zfill,
                                          int (&acc)[16]) {
    const int x = (int)(n % W);
    const long bh = n / W;
    const int h = (int)(bh % H);
    const long row0 = bh - h;             // b * H
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ih = h + kh - 1, iw = x + kw - 1;
            v4i q = {zfill, zfill, zfill, zfill};
            if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                q = *(const v4i *)(in + ((row0 + ih) * W + iw) * 64 + 16 * g);
            q8_mac16(acc, wt[kh * 3 + kw], q);
        }
    }
}

struct q8_pw_regs { v4i a[4]; };

__device__ __forceinline__ void q8_pw_load(const int8_t *__restrict__ w, int lane, q8_pw_regs &r) {
    const int i = lane & 15, gk = lane >> 4;
#pragma unroll
    for (int m = 0; m < 4; ++m) r.a[m] = *(const v4i *)(w + (16 * (i >> 2) + 4 * m + (i & 3)) * 64 + 16 * gk);
}

__device__ __forceinline__ void q8_pw_acc(const q8_pw_regs &r, const v4i &bq, int (&acc)[16]) {
    const v4i zero = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const v4i c = __builtin_amdgcn_mfma_i32_16x16x64_i8(r.a[m], bq, zero, 0, 0, 0);
        acc[4 * m + 0] = c[0];
        acc[4 * m + 1] = c[1];
        acc[4 * m + 2] = c[2];
        acc[4 * m + 3] = c[3];
    }
}

__global__ __launch_bounds__(Q8_BLOCK) void k_q8_quantize(const float *__restrict__ x, long n, float s, int z,
                                                          int8_t *__restrict__ out) {
    const long quads = (n + 3) / 4;
    for (long i = (long)blockIdx.x * Q8_BLOCK + threadIdx.x; i < quads; i += (long)gridDim.x * Q8_BLOCK) {
        int q[4] = {0, 0, 0, 0};
        const long e0 = 4 * i;
        const int cnt = n - e0 < 4 ? (int)(n - e0) : 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (cnt == 4) {
            const float4 f = *(const float4 *)(x + e0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
            for (int j = 0; j < cnt; ++j) v[j] = x[e0 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = rintf(__fdiv_rn(v[j], s));                        // NaN stays NaN, +-inf stays
            r = r != r ? 0.f : fminf(fmaxf(r, -512.f), 512.f);          // NaN -> z_x; anything past +-512 saturates below
            const int t = (int)r + z;
            q[j] = t < -128 ? -128 : (t > 127 ? 127 : t);
        }
        if (cnt == 4) {
            *(int *)(out + e0) = q8_pack4(q[0], q[1], q[2], q[3]);
        } else {
            for (int j = 0; j < cnt; ++j) out[e0 + j] = (int8_t)q[j];
        }
    }
}

__global__ __launch_bounds__(Q8_BLOCK) void k_q8_stem(const int8_t *__restrict__ xq, const int8_t *__restrict__ w, q8_chan pc,
                                                      int F, int T, int Ho, int Wo, long N, int z, int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, g = lane >> 4;
    v4i wt[9];
    q8_load_taps(w, g, wt);
    const long tiles = (N + 15) / 16;
    for (long tile = (long)blockIdx.x * Q8_WAVES + (threadIdx.x >> 6); tile < tiles; tile += (long)gridDim.x * Q8_WAVES) {
        const long n = tile * 16 + p;
        if (n >= N) continue;
        const int ow = (int)(n % Wo);
        const long bo = n / Wo;
        const int oh = (int)(bo % Ho);
        const long b = bo / Ho;
        int acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = 0;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
                int q = z;
                if ((unsigned)ih < (unsigned)F && (unsigned)iw < (unsigned)T) q = xq[(b * F + ih) * T + iw];
                const v4i wv = wt[kh * 3 + kw];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    acc[4 * d + 0] += q8_byte<0>(wv[d]) * q;
                    acc[4 * d + 1] += q8_byte<1>(wv[d]) * q;
                    acc[4 * d + 2] += q8_byte<2>(wv[d]) * q;
                    acc[4 * d + 3] += q8_byte<3>(wv[d]) * q;
                }
            }
        }
        *(v4i *)(out + n * 64 + 16 * g) = q8_requant16(acc, pc, 16 * g);
    }
}

__global__ __launch_bounds__(Q8_BLOCK) void k_q8_dw(const int8_t *__restrict__ in, const int8_t *__restrict__ w, q8_chan pc, int H,
                                                    int W, long N, int zfill, int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, g = lane >> 4;
    v4i wt[9];
    q8_load_taps(w, g, wt);
    const long tiles = (N + 15) / 16;
    for (long tile = (long)blockIdx.x * Q8_WAVES + (threadIdx.x >> 6); tile < tiles; tile += (long)gridDim.x * Q8_WAVES) {
        const long n = tile * 16 + p;
        if (n >= N) continue;
        int acc[16];
        q8_dw_acc(in, wt, n, H, W, g, zfill, acc);
        *(v4i *)(out + n * 64 + 16 * g) = q8_requant16(acc, pc, 16 * g);
    }
}

// the matrix instruction runs with every lane of the wave: a lane whose pixel lies past the end supplies zeros and stores nothing
__global__ __launch_bounds__(Q8_BLOCK) void k_q8_pw(const int8_t *__restrict__ in, const int8_t *__restrict__ w, q8_chan pc, long N,
                                                    int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, g = lane >> 4;
    q8_pw_regs wr;
    q8_pw_load(w, lane, wr);
    const long tiles = (N + 15) / 16;
    for (long tile = (long)blockIdx.x * Q8_WAVES + (threadIdx.x >> 6); tile < tiles; tile += (long)gridDim.x * Q8_WAVES) {
        const long n = tile * 16 + p;
        v4i bq = {0, 0, 0, 0};
        if (n < N) bq = *(const v4i *)(in + n * 64 + 16 * g);
        int acc[16];
        q8_pw_acc(wr, bq, acc);
        if (n < N) *(v4i *)(out + n * 64 + 16 * g) = q8_requant16(acc, pc, 16 * g);
    }
}

__global__ __launch_bounds__(Q8_BLOCK) void k_q8_dwpw(const int8_t *__restrict__ in, const int8_t *__restrict__ w_dw, q8_chan pc_dw,
                                                      const int8_t *__restrict__ w_pw, q8_chan pc_pw, int H, int W, long N,
                                                      int zfill, int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, g = lane >> 4;
    v4i wt[9];
    q8_load_taps(w_dw, g, wt);
    q8_pw_regs wr;
    q8_pw_load(w_pw, lane, wr);
    const long tiles = (N + 15) / 16;
    for (long tile = (long)blockIdx.x * Q8_WAVES + (threadIdx.x >> 6); tile < tiles; tile += (long)gridDim.x * Q8_WAVES) {
        const long n = tile * 16 + p;
        v4i bq = {0, 0, 0, 0};
        int acc[16];
        if (n < N) {
            q8_dw_acc(in, wt, n, H, W, g, zfill, acc);
            bq = q8_requant16(acc, pc_dw, 16 * g);
        }
        q8_pw_acc(wr, bq, acc);
        if (n < N) *(v4i *)(out + n * 64 + 16 * g) = q8_requant16(acc, pc_pw, 16 * g);
    }
}

// one workgroup per image: S[c] = sum_hw (q + 128), p = requant(S), logits[k] = float(sum_c w[k][c] (p[c] + 128) + b[k]) * scale[k]
__global__ __launch_bounds__(Q8_BLOCK) void k_q8_gap_fc(const int8_t *__restrict__ in, int HW, int pool_m, int pool_sh,
                                                        const int8_t *__restrict__ fc_w, const int *__restrict__ fc_b,
                                                        const float *__restrict__ fc_scale, int8_t *__restrict__ pool_out,
                                                        float *__restrict__ logits) {
    __shared__ int s_part[64][64 + 1];
    __shared__ int s_pool[64];
    const int tid = threadIdx.x, g = tid & 3, slot = tid >> 2;
    const int8_t *img = in + (long)blockIdx.x * HW * 64;
    int sum[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) sum[c] = 0;
    for (int pix = slot; pix < HW; pix += 64) {
        const v4i q = *(const v4i *)(img + (long)pix * 64 + 16 * g);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            sum[4 * d + 0] += q8_byte<0>(q[d]) + 128;
            sum[4 * d + 1] += q8_byte<1>(q[d]) + 128;
            sum[4 * d + 2] += q8_byte<2>(q[d]) + 128;
            sum[4 * d + 3] += q8_byte<3>(q[d]) + 128;
        }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) s_part[slot][16 * g + c] = sum[c];
    __syncthreads();
    if (tid < 64) {
        int S = 0;
        for (int s = 0; s < 64; ++s) S += s_part[s][tid];
        const int pq = q8_requant(S, pool_m, pool_sh);
        pool_out[(long)blockIdx.x * 64 + tid] = (int8_t)pq;
        s_pool[tid] = pq + 128;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned acc = (unsigned)fc_b[tid];
        for (int c = 0; c < 64; ++c) acc += (unsigned)((int)fc_w[tid * 64 + c] * s_pool[c]);
        logits[(long)blockIdx.x * 2 + tid] = (float)(int)acc * fc_scale[tid];
    }
}

template <typename K> int q8_tile_grid(ww_ctx *ctx, K fn, long N) {
    const long want = ((N + 15) / 16 + Q8_WAVES - 1) / Q8_WAVES;
    return ww_conv_grid(ctx, (const void *)fn, Q8_BLOCK, 0, want, 1 << 20);
}

int q8_check_conv(const char *what, ww_ctx *ctx, const void *in, const void *w, const int32_t *b, const int32_t *m,
                  const int32_t *sh, const void *out, long N) {
    WW_REQUIRE(ctx && in && w && b && m && sh && out, WW_E_INVALID, "%s: null argument", what);
    WW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(b) && aligned16(m) && aligned16(sh) && aligned16(out), WW_E_INVALID,
               "%s: tensors must be 16-byte aligned", what);
    WW_REQUIRE(N >= 1 && N <= (1l << 40), WW_E_INVALID, "%s: %ld pixels", what, N);
    return WW_OK;
}

}  // namespace

extern "C" int ww_q8_quantize(ww_ctx *ctx, const float *x, long n, float scale, int zero, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && out, WW_E_INVALID, "ww_q8_quantize: null argument");
    WW_REQUIRE(n >= 1, WW_E_INVALID, "ww_q8_quantize: n=%ld", n);
    WW_REQUIRE(scale > 0.f && scale < INFINITY, WW_E_INVALID, "ww_q8_quantize: scale must be positive and finite");
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_q8_quantize: zero point %d outside int8", zero);
    WW_REQUIRE(aligned16(x) && aligned16(out), WW_E_INVALID, "ww_q8_quantize: tensors must be 16-byte aligned");
    const int grid = ww_capped_grid(ctx, ww_pass_ew((n + 3) / 4).grid);
    hipLaunchKernelGGL(k_q8_quantize, dim3(grid), dim3(Q8_BLOCK), 0, (hipStream_t)stream, x, n, scale, zero, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_q8_stem_fwd(ww_ctx *ctx, const int8_t *xq, const int8_t *w, const int32_t *bias, const int32_t *mult,
                              const int32_t *shift, int B, int F, int T, int zero, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(B >= 1 && F >= 1 && T >= 1, WW_E_INVALID, "ww_q8_stem_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_q8_stem_fwd: zero point %d outside int8", zero);
    const int Ho = (F + 1) / 2, Wo = (T + 1) / 2;
    const long N = (long)B * Ho * Wo;
    const int rc = q8_check_conv("ww_q8_stem_fwd", ctx, xq, w, bias, mult, shift, out, N);
    if (rc != WW_OK) return rc;
    ww_prof_scope prof(ctx, WW_K_STEM_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_q8_stem, dim3(q8_tile_grid(ctx, k_q8_stem, N)), dim3(Q8_BLOCK), 0, (hipStream_t)stream, xq, w,
                       q8_chan{bias, mult, shift}, F, T, Ho, Wo, N, zero, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_q8_dwconv3x3_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                                   const int32_t *shift, int B, int H, int W, int zero, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1, WW_E_INVALID, "ww_q8_dwconv3x3_fwd: B=%d H=%d W=%d", B, H, W);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_q8_dwconv3x3_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(in != out, WW_E_INVALID, "ww_q8_dwconv3x3_fwd: in place");
    const long N = (long)B * H * W;
    const int rc = q8_check_conv("ww_q8_dwconv3x3_fwd", ctx, in, w, bias, mult, shift, out, N);
    if (rc != WW_OK) return rc;
    ww_prof_scope prof(ctx, WW_K_DW_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_q8_dw, dim3(q8_tile_grid(ctx, k_q8_dw, N)), dim3(Q8_BLOCK), 0, (hipStream_t)stream, in, w,
                       q8_chan{bias, mult, shift}, H, W, N, (zero & 255) * 0x01010101, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_q8_pwconv1x1_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                                   const int32_t *shift, long N, int8_t *out, ww_stream_t stream) {
    const int rc = q8_check_conv("ww_q8_pwconv1x1_fwd", ctx, in, w, bias, mult, shift, out, N);
    if (rc != WW_OK) return rc;
    ww_prof_scope prof(ctx, WW_K_PW_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_q8_pw, dim3(q8_tile_grid(ctx, k_q8_pw, N)), dim3(Q8_BLOCK), 0, (hipStream_t)stream, in, w,
                       q8_chan{bias, mult, shift}, N, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_q8_dwpw_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w_dw, const int32_t *bias_dw, const int32_t *mult_dw,
                              const int32_t *shift_dw, const int8_t *w_pw, const int32_t *bias_pw, const int32_t *mult_pw,
                              const int32_t *shift_pw, int B, int H, int W, int zero, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1, WW_E_INVALID, "ww_q8_dwpw_fwd: B=%d H=%d W=%d", B, H, W);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_q8_dwpw_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(in != out, WW_E_INVALID, "ww_q8_dwpw_fwd: in place");
    const long N = (long)B * H * W;
    int rc = q8_check_conv("ww_q8_dwpw_fwd", ctx, in, w_dw, bias_dw, mult_dw, shift_dw, out, N);
    if (rc != WW_OK) return rc;
    rc = q8_check_conv("ww_q8_dwpw_fwd", ctx, in, w_pw, bias_pw, mult_pw, shift_pw, out, N);
    if (rc != WW_OK) return rc;
    ww_prof_scope prof(ctx, WW_K_PW_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_q8_dwpw, dim3(q8_tile_grid(ctx, k_q8_dwpw, N)), dim3(Q8_BLOCK), 0, (hipStream_t)stream, in, w_dw,
                       q8_chan{bias_dw, mult_dw, shift_dw}, w_pw, q8_chan{bias_pw, mult_pw, shift_pw}, H, W, N,
                       (zero & 255) * 0x01010101, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_q8_gap_fc_fwd(ww_ctx *ctx, const int8_t *in, int B, int HW, int pool_mult, int pool_shift, const int8_t *fc_w,
                                const int32_t *fc_bias, const float *fc_scale, int8_t *pool_out, float *logits,
                                ww_stream_t stream) {
    WW_REQUIRE(ctx && in && fc_w && fc_bias && fc_scale && pool_out && logits, WW_E_INVALID, "ww_q8_gap_fc_fwd: null argument");
    WW_REQUIRE(B >= 1 && HW >= 1 && HW <= (1 << 23), WW_E_INVALID, "ww_q8_gap_fc_fwd: B=%d HW=%d", B, HW);
    WW_REQUIRE(q8_mult_ok(pool_mult, pool_shift), WW_E_INVALID,
               "ww_q8_gap_fc_fwd: multiplier %d / shift %d out of range", pool_mult, pool_shift);
    WW_REQUIRE(aligned16(in), WW_E_INVALID, "ww_q8_gap_fc_fwd: the activations must be 16-byte aligned");
    ww_prof_scope prof(ctx, WW_K_GAP_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_q8_gap_fc, dim3(B), dim3(Q8_BLOCK), 0, (hipStream_t)stream, in, HW, pool_mult, pool_shift, fc_w, fc_bias,
                       fc_scale, pool_out, logits);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" size_t ww_q8_cnn_small_workspace_bytes(int B, int F, int T) {
    if (B < 1 || F < 1 || T < 1) return 0;
    const long act = q8_round256((long)B * ((F + 1) / 2) * ((T + 1) / 2) * 64);
    return (size_t)(q8_round256((long)B * F * T) + WW_Q8_NACT * act + q8_round256((long)B * 64));
}

extern "C" int ww_q8_cnn_small_fwd(ww_ctx *ctx, const void *const *tab, const ww_q8_io *io, const float *x, int B, int F, int T,
                                   int form, void *ws, size_t ws_bytes, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && tab && io && x && ws && logits, WW_E_INVALID, "ww_q8_cnn_small_fwd: null argument");
    WW_REQUIRE(B >= 1 && F >= 1 && T >= 1, WW_E_INVALID, "ww_q8_cnn_small_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(form == WW_Q8_PAIR || form == WW_Q8_FUSED, WW_E_INVALID, "ww_q8_cnn_small_fwd: unknown form %d", form);
    WW_REQUIRE(ws_bytes >= ww_q8_cnn_small_workspace_bytes(B, F, T), WW_E_INVALID,
               "ww_q8_cnn_small_fwd: workspace of %zu bytes, need %zu", ws_bytes, ww_q8_cnn_small_workspace_bytes(B, F, T));
    WW_REQUIRE(aligned16(ws), WW_E_INVALID, "ww_q8_cnn_small_fwd: the workspace must be 16-byte aligned");
    for (int i = 0; i < WW_Q8_NPTR; ++i) WW_REQUIRE(tab[i], WW_E_INVALID, "ww_q8_cnn_small_fwd: table entry %d is null", i);
    const int H = (F + 1) / 2, W = (T + 1) / 2;
    const long N = (long)B * H * W, act = q8_round256(N * 64);
    int8_t *xq = (int8_t *)ws;
    int8_t *a0 = xq + q8_round256((long)B * F * T);
    int8_t *pool = a0 + WW_Q8_NACT * act;
    auto i8 = [&](int i) { return (const int8_t *)tab[i]; };
    auto i32 = [&](int i) { return (const int32_t *)tab[i]; };
    int rc = ww_q8_quantize(ctx, x, (long)B * F * T, io->in_scale, io->in_zero, xq, stream);
    if (rc != WW_OK) return rc;
    rc = ww_q8_stem_fwd(ctx, xq, i8(0), i32(1), i32(2), i32(3), B, F, T, io->in_zero, a0, stream);
    if (rc != WW_OK) return rc;
    for (int k = 0; k < 4; ++k) {
        const int t = 4 + 8 * k;
        const int8_t *in = a0 + (2 * k) * act;
        int8_t *mid = a0 + (2 * k + 1) * act, *out = a0 + (2 * k + 2) * act;
        if (form == WW_Q8_FUSED) {
            rc = ww_q8_dwpw_fwd(ctx, in, i8(t), i32(t + 1), i32(t + 2), i32(t + 3), i8(t + 4), i32(t + 5), i32(t + 6), i32(t + 7), B,
                                H, W, -128, out, stream);
        } else {
            rc = ww_q8_dwconv3x3_fwd(ctx, in, i8(t), i32(t + 1), i32(t + 2), i32(t + 3), B, H, W, -128, mid, stream);
            if (rc != WW_OK) return rc;
            rc = ww_q8_pwconv1x1_fwd(ctx, mid, i8(t + 4), i32(t + 5), i32(t + 6), i32(t + 7), N, out, stream);
        }
        if (rc != WW_OK) return rc;
    }
    return ww_q8_gap_fc_fwd(ctx, a0 + 8 * act, B, H * W, io->pool_mult, io->pool_shift, i8(36), i32(37), (const float *)tab[38], pool,
                            logits, stream);
}

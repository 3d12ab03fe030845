// Integer-only inference of an exported int8 TCNWakeword bundle (DESIGN.md "Export", the int8 law, subsection "TCN").
//   k_tq8_quantize_bt : fp32 features (B,F,T) -> int8 rows (B*T, Fp), q = clamp(rne(x / s_x) + z_x), transposed in the same pass
//   the conv          : causal dilated Conv1d as a shifted-row GEMM, the TqTime geometry of the int8 tap-GEMM core (ww_q8_tap_gemm.h:
//                       the lane map, the row tiles, the LDS weight slab); epilogue (a) requantise + clamp, (b) R(acc) + R(h2 + 128)
//                       + clamp: the downsample conv carrying the block's add and last ReLU
//   k_tq8_skip_add    : the identity-skip form of the add
//   k_tq8_pool_fc     : sum over T, requantise, Linear(C, num_classes), one fp32 multiply per logit
// Activations are int8 rows (B*T, Cp), Cp = the channel count rounded up to 64: every (row, tap) is a whole number of the
// instruction's 64-deep K chunks.  Pad channels hold the tensor's zero point and meet zero weights; pad OUTPUT channels have zero
// weights, a zero bias and m = 2^30, sh = 31, so they come out as -128, the zero point of every tensor a conv writes.
//
// A wave holds TQ_RT tiles of 16 rows at once.  The weights of a channel tile (64 k Cpi bytes) are held in LDS (the default up to
// 64 KB: measured 1.11 x faster over the default model's forward) or streamed through L2 (larger tiles, and
// WW_TQ8_WEIGHTS=stream in the environment, the A/B switch).
//
// bias arguments are the EFFECTIVE bias q_b - z_in * sum(q_w) (host, once per bundle), so "a source time below 0", "a pad
// channel" and "a row past the end" are all a vector of z_in bytes.  All adds that may wrap are unsigned.
#include "ww_q8_tap_gemm.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int TQ_BLOCK = 256;
constexpr int TQ_RT = 4;                       // 16-row tiles a wave holds at once
constexpr int TQ_MAX_CP = 1024;                // widest tensor k_tq8_pool_fc sums (its LDS image)
constexpr size_t TQ_SLAB_MAX = 64 * 1024;      // largest weight image of one channel tile the conv keeps in LDS

// row n = (b, t) of (B*T, Cpi); tap j reads time t - (k-1-j) d of the same sample, or the zero point where that time is negative
struct TqTime {
    const int8_t *in;
    long N;
    int T, Cpi, k, dil, zfill;
    struct Row { long n; int t; };
    struct Src { const int8_t *p; bool live; };
    __device__ int nseg() const { return k; }
    __device__ int K() const { return Cpi; }
    __device__ void row(long n, Row &r) const {
        r.n = n;
        r.t = n < N ? (int)(n % T) : -1;       // a row past the end has no valid source time
    }
    __device__ void seg(const Row &r, int j, int g, Src &s) const {
        const long off = (long)(k - 1 - j) * dil;
        s.live = (long)r.t - off >= 0;
        s.p = in + (r.n - off) * Cpi + 16 * g;  // dereferenced only where live
    }
    __device__ v4i load(const Src &s, int kc) const {
        v4i bq = {zfill, zfill, zfill, zfill};
        if (s.live) bq = *(const v4i *)(s.p + 64 * kc);
        return bq;
    }
};

// out = clamp(-128 + R(acc) [+ R(h2 + 128, m_a, sh_a)]); ADD: res is the residual tensor h2 (N, Cpo)
template <bool ADD> struct TqEpi : Q8Chan {
    const int8_t *res;
    int8_t *out;
    int res_m, res_sh;
    __device__ void store(const v4i (&acc)[4], long n, int c0) const {
        v4i hv = {0, 0, 0, 0};
        if (ADD) hv = *(const v4i *)(res + n * Cout + c0);
        q8_tap_store(*this, acc, hv, out, n, c0, [&](long long v, int h) {
            if (ADD) v += q8_round(h + 128, res_m, res_sh);
            return q8_clamp(v);
        });
    }
};

// out = clamp(-128 + R(q_in - z_in, m_i, sh_i) + R(q_h2 + 128, m_a, sh_a)) over nvec 16-byte vectors
__global__ __launch_bounds__(TQ_BLOCK) void k_tq8_skip_add(const int8_t *__restrict__ in, const int8_t *__restrict__ h2, long nvec,
                                                           int z_in, int m_i, int sh_i, int m_a, int sh_a, int8_t *__restrict__ out) {
    for (long i = (long)blockIdx.x * TQ_BLOCK + threadIdx.x; i < nvec; i += (long)gridDim.x * TQ_BLOCK) {
        const v4i x = *(const v4i *)(in + 16 * i), h = *(const v4i *)(h2 + 16 * i);
        v4i o;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int xs[4], hs[4], q[4];
            q8_unpack4(x[d], xs);
            q8_unpack4(h[d], hs);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = q8_clamp(q8_round(xs[e] - z_in, m_i, sh_i) + q8_round(hs[e] + 128, m_a, sh_a));
            o[d] = q8_pack4(q[0], q[1], q[2], q[3]);
        }
        *(v4i *)(out + 16 * i) = o;
    }
}

// one thread per (sample, channel quad, time), time fastest: the reads of x (B,F,T) run along T
__global__ __launch_bounds__(TQ_BLOCK) void k_tq8_quantize_bt(const float *__restrict__ x, int F, int T, int Fp, long quads, float s,
                                                              int z, int8_t *__restrict__ out) {
    const int nq = Fp / 4;
    for (long i = (long)blockIdx.x * TQ_BLOCK + threadIdx.x; i < quads; i += (long)gridDim.x * TQ_BLOCK) {
        const int t = (int)(i % T);
        const long bq = i / T;
        const int fq = (int)(bq % nq);
        const long b = bq / nq;
        int q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int f = 4 * fq + e;
            q[e] = z;                                                   // a pad channel holds the zero point
            if (f < F) {
                float r = rintf(__fdiv_rn(x[(b * F + f) * T + t], s));  // NaN stays NaN, +-inf stays
                r = r != r ? 0.f : fminf(fmaxf(r, -512.f), 512.f);      // NaN -> z_x; anything past +-512 saturates below
                const int v = (int)r + z;
                q[e] = v < -128 ? -128 : (v > 127 ? 127 : v);
            }
        }
        *(int *)(out + (b * T + t) * Fp + 4 * fq) = q8_pack4(q[0], q[1], q[2], q[3]);
    }
}

// one workgroup per sample: S[c] = sum_t (q + 128), p = requant(S), logits[k] = float(sum_c w[k][c] (p[c] + 128) + b[k]) * scale[k]
__global__ __launch_bounds__(TQ_BLOCK) void k_tq8_pool_fc(const int8_t *__restrict__ in, int T, int C, int Cp, int pool_m, int pool_sh,
                                                          const int8_t *__restrict__ fc_w, const int *__restrict__ fc_b,
                                                          const float *__restrict__ fc_scale, int nc, int8_t *__restrict__ pool_out,
                                                          float *__restrict__ logits) {
    __shared__ int s_part[TQ_MAX_CP];          // [slot][Cp], slots * Cp <= 1024
    __shared__ int s_pool[TQ_MAX_CP];
    const int tid = threadIdx.x, ncol = Cp / 4, slots = TQ_BLOCK / ncol;
    const int8_t *img = in + (long)blockIdx.x * T * Cp;
    if (tid < slots * ncol) {
        const int col = tid % ncol, slot = tid / ncol;
        int sum[4] = {0, 0, 0, 0};
        for (int t = slot; t < T; t += slots) {
            int q[4];
            q8_unpack4(*(const int *)(img + (long)t * Cp + 4 * col), q);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] += q[e] + 128;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s_part[slot * Cp + 4 * col + e] = sum[e];
    }
    __syncthreads();
    for (int c = tid; c < C; c += TQ_BLOCK) {
        int S = 0;
        for (int s = 0; s < slots; ++s) S += s_part[s * Cp + c];
        const int pq = q8_clamp(q8_round(S, pool_m, pool_sh));
        pool_out[(long)blockIdx.x * C + c] = (int8_t)pq;
        s_pool[c] = pq + 128;
    }
    __syncthreads();
    if (tid < nc) {
        unsigned acc = (unsigned)fc_b[tid];
        for (int c = 0; c < C; ++c) acc += (unsigned)((int)fc_w[(long)tid * C + c] * s_pool[c]);
        logits[(long)blockIdx.x * nc + tid] = (float)(int)acc * fc_scale[tid];
    }
}

}  // namespace

extern "C" int ww_tq8_quantize_bt(ww_ctx *ctx, const float *x, int B, int F, int T, int Fp, float scale, int zero, int8_t *out,
                                  ww_stream_t stream) {
    WW_REQUIRE(ctx && x && out, WW_E_INVALID, "ww_tq8_quantize_bt: null argument");
    WW_REQUIRE(B >= 1 && F >= 1 && T >= 1, WW_E_INVALID, "ww_tq8_quantize_bt: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(Fp >= F && Fp % 64 == 0, WW_E_INVALID, "ww_tq8_quantize_bt: Fp=%d is not F=%d rounded up to 64s", Fp, F);
    WW_REQUIRE(scale > 0.f && scale < INFINITY, WW_E_INVALID, "ww_tq8_quantize_bt: scale must be positive and finite");
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_tq8_quantize_bt: zero point %d outside int8", zero);
    WW_REQUIRE(aligned16(out), WW_E_INVALID, "ww_tq8_quantize_bt: the output must be 16-byte aligned");
    const long quads = (long)B * T * (Fp / 4);
    const int grid = ww_capped_grid(ctx, ww_pass_ew(quads).grid);
    hipLaunchKernelGGL(k_tq8_quantize_bt, dim3(grid), dim3(TQ_BLOCK), 0, (hipStream_t)stream, x, F, T, Fp, quads, scale, zero, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_tq8_conv1d_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                                 const int32_t *shift, int B, int T, int Cpi, int Cpo, int k, int dilation, int zero,
                                 const int8_t *residual, int res_mult, int res_shift, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w && bias && mult && shift && out, WW_E_INVALID, "ww_tq8_conv1d_fwd: null argument");
    WW_REQUIRE(B >= 1 && T >= 1, WW_E_INVALID, "ww_tq8_conv1d_fwd: B=%d T=%d", B, T);
    WW_REQUIRE(Cpi >= 64 && Cpi % 64 == 0 && Cpo >= 64 && Cpo % 64 == 0, WW_E_INVALID,
               "ww_tq8_conv1d_fwd: padded channel counts %d -> %d must be multiples of 64", Cpi, Cpo);
    WW_REQUIRE(k >= 1 && k <= 8 && dilation >= 1 && dilation <= (1 << 20), WW_E_INVALID, "ww_tq8_conv1d_fwd: k=%d dilation=%d", k,
               dilation);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_tq8_conv1d_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(out) &&
               aligned16(residual), WW_E_INVALID, "ww_tq8_conv1d_fwd: tensors must be 16-byte aligned");
    WW_REQUIRE(in != out && residual != out, WW_E_INVALID, "ww_tq8_conv1d_fwd: in place");
    WW_REQUIRE(!residual || q8_mult_ok(res_mult, res_shift), WW_E_INVALID,
               "ww_tq8_conv1d_fwd: residual multiplier %d / shift %d out of range", res_mult, res_shift);
    const long N = (long)B * T;
    const TqTime geo{in, N, T, Cpi, k, dilation, (zero & 255) * 0x01010101};
    const Q8Chan chan{bias, mult, shift, Cpo};
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope prof(ctx, WW_K_PW_FWD, st);
    // One channel tile's weights are 64 k Cpi bytes.  Up to TQ_SLAB_MAX they are held in LDS; beyond it, or with
    // WW_TQ8_WEIGHTS=stream in the environment (the A/B switch of tools/bench_q8_tcn.py and the tests), they are streamed.
    const size_t slab = (size_t)64 * k * Cpi;
    const char *mode = getenv("WW_TQ8_WEIGHTS");
    const bool lds = slab <= TQ_SLAB_MAX && !(mode && !strcmp(mode, "stream"));
    if (residual) return q8_tap_launch<TqTime, TqEpi<true>, TQ_RT>(ctx, geo, {chan, residual, out, res_mult, res_shift}, w, lds, slab, st);
    return q8_tap_launch<TqTime, TqEpi<false>, TQ_RT>(ctx, geo, {chan, nullptr, out, 0, 0}, w, lds, slab, st);
}

extern "C" int ww_tq8_skip_add_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *h2, long N, int Cp, int zero, int skip_mult,
                                   int skip_shift, int add_mult, int add_shift, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && h2 && out, WW_E_INVALID, "ww_tq8_skip_add_fwd: null argument");
    WW_REQUIRE(N >= 1 && N <= (1l << 40) && Cp >= 64 && Cp % 64 == 0, WW_E_INVALID, "ww_tq8_skip_add_fwd: N=%ld Cp=%d", N, Cp);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_tq8_skip_add_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(q8_mult_ok(skip_mult, skip_shift) && q8_mult_ok(add_mult, add_shift), WW_E_INVALID,
               "ww_tq8_skip_add_fwd: a multiplier or shift out of range");
    WW_REQUIRE(aligned16(in) && aligned16(h2) && aligned16(out), WW_E_INVALID, "ww_tq8_skip_add_fwd: tensors must be 16-byte aligned");
    const long nvec = N * (Cp / 16);
    const int grid = ww_capped_grid(ctx, ww_pass_ew(nvec).grid);
    hipLaunchKernelGGL(k_tq8_skip_add, dim3(grid), dim3(TQ_BLOCK), 0, (hipStream_t)stream, in, h2, nvec, zero, skip_mult, skip_shift,
                       add_mult, add_shift, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_tq8_pool_fc_fwd(ww_ctx *ctx, const int8_t *in, int B, int T, int C, int Cp, int pool_mult, int pool_shift,
                                  const int8_t *fc_w, const int32_t *fc_bias, const float *fc_scale, int num_classes,
                                  int8_t *pool_out, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && fc_w && fc_bias && fc_scale && pool_out && logits, WW_E_INVALID, "ww_tq8_pool_fc_fwd: null argument");
    WW_REQUIRE(B >= 1 && T >= 1 && T <= (1 << 23), WW_E_INVALID, "ww_tq8_pool_fc_fwd: B=%d T=%d", B, T);
    WW_REQUIRE(C >= 1 && Cp == q8_pad64(C) && Cp <= TQ_MAX_CP, WW_E_INVALID, "ww_tq8_pool_fc_fwd: C=%d Cp=%d (Cp = C rounded up to 64, at most %d)",
               C, Cp, TQ_MAX_CP);
    WW_REQUIRE(num_classes >= 2 && num_classes <= 64, WW_E_INVALID, "ww_tq8_pool_fc_fwd: num_classes=%d outside [2, 64]", num_classes);
    WW_REQUIRE(q8_mult_ok(pool_mult, pool_shift), WW_E_INVALID, "ww_tq8_pool_fc_fwd: multiplier %d / shift %d out of range", pool_mult,
               pool_shift);
    WW_REQUIRE(aligned16(in), WW_E_INVALID, "ww_tq8_pool_fc_fwd: the activations must be 16-byte aligned");
    ww_prof_scope prof(ctx, WW_K_GAP_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_tq8_pool_fc, dim3(B), dim3(TQ_BLOCK), 0, (hipStream_t)stream, in, T, C, Cp, pool_mult, pool_shift, fc_w, fc_bias,
                       fc_scale, num_classes, pool_out, logits);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" size_t ww_tq8_tcn_workspace_bytes(int B, int F, int T, int n_blocks, const int32_t *channels) {
    if (B < 1 || F < 1 || T < 1 || n_blocks < 1 || n_blocks > WW_TQ8_MAX_BLOCKS || !channels) return 0;
    long bytes = q8_round256((long)B * T * q8_pad64(F));
    for (int i = 0; i < n_blocks; ++i) {
        if (channels[i] < 1) return 0;
        bytes += 3 * q8_round256((long)B * T * q8_pad64(channels[i]));
    }
    return (size_t)(bytes + q8_round256((long)B * channels[n_blocks - 1]));
}

extern "C" int ww_tq8_tcn_fwd(ww_ctx *ctx, const void *const *tab, const ww_tq8_io *io, const float *x, int B, int T, void *ws,
                              size_t ws_bytes, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && tab && io && x && ws && logits, WW_E_INVALID, "ww_tq8_tcn_fwd: null argument");
    const int nb = io->n_blocks, F = io->input_size, k = io->kernel_size;
    WW_REQUIRE(B >= 1 && T >= 1 && F >= 1, WW_E_INVALID, "ww_tq8_tcn_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(nb >= 1 && nb <= WW_TQ8_MAX_BLOCKS, WW_E_INVALID, "ww_tq8_tcn_fwd: %d blocks", nb);
    const size_t need = ww_tq8_tcn_workspace_bytes(B, F, T, nb, io->channels);
    WW_REQUIRE(need && ws_bytes >= need, WW_E_INVALID, "ww_tq8_tcn_fwd: workspace of %zu bytes, need %zu", ws_bytes, need);
    WW_REQUIRE(aligned16(ws), WW_E_INVALID, "ww_tq8_tcn_fwd: the workspace must be 16-byte aligned");
    auto i8 = [&](int i) { return (const int8_t *)tab[i]; };
    auto i32 = [&](int i) { return (const int32_t *)tab[i]; };
    const long N = (long)B * T;
    int8_t *cur = (int8_t *)ws;
    int Cpi = q8_pad64(F), zin = io->in_zero;
    int rc = ww_tq8_quantize_bt(ctx, x, B, F, T, Cpi, io->in_scale, zin, cur, stream);
    if (rc != WW_OK) return rc;
    int8_t *next = cur + q8_round256(N * Cpi);
    for (int i = 0; i < nb; ++i) {
        const int Cpo = q8_pad64(io->channels[i]), d = 1 << i, p = WW_TQ8_BLOCK_NPTR * i;
        const long act = q8_round256(N * Cpo);
        int8_t *h1 = next, *h2 = next + act, *out = next + 2 * act;
        for (int j = 0; j < 8; ++j) WW_REQUIRE(tab[p + j], WW_E_INVALID, "ww_tq8_tcn_fwd: table entry %d is null", p + j);
        rc = ww_tq8_conv1d_fwd(ctx, cur, i8(p), i32(p + 1), i32(p + 2), i32(p + 3), B, T, Cpi, Cpo, k, d, zin, nullptr, 0, 0, h1, stream);
        if (rc != WW_OK) return rc;
        rc = ww_tq8_conv1d_fwd(ctx, h1, i8(p + 4), i32(p + 5), i32(p + 6), i32(p + 7), B, T, Cpo, Cpo, k, d, -128, nullptr, 0, 0, h2,
                               stream);
        if (rc != WW_OK) return rc;
        if (tab[p + 8]) {
            for (int j = 9; j < 12; ++j) WW_REQUIRE(tab[p + j], WW_E_INVALID, "ww_tq8_tcn_fwd: table entry %d is null", p + j);
            rc = ww_tq8_conv1d_fwd(ctx, cur, i8(p + 8), i32(p + 9), i32(p + 10), i32(p + 11), B, T, Cpi, Cpo, 1, 1, zin, h2,
                                   io->add_mult[i], io->add_shift[i], out, stream);
        } else {
            WW_REQUIRE(Cpi == Cpo, WW_E_INVALID, "ww_tq8_tcn_fwd: block %d has no downsample conv but %d -> %d padded channels", i, Cpi,
                       Cpo);
            rc = ww_tq8_skip_add_fwd(ctx, cur, h2, N, Cpo, zin, io->skip_mult[i], io->skip_shift[i], io->add_mult[i], io->add_shift[i],
                                     out, stream);
        }
        if (rc != WW_OK) return rc;
        cur = out;
        next = out + act;
        Cpi = Cpo;
        zin = -128;
    }
    const int q = WW_TQ8_BLOCK_NPTR * nb;
    for (int j = 0; j < 3; ++j) WW_REQUIRE(tab[q + j], WW_E_INVALID, "ww_tq8_tcn_fwd: table entry %d is null", q + j);
    return ww_tq8_pool_fc_fwd(ctx, cur, B, T, io->channels[nb - 1], Cpi, io->pool_mult, io->pool_shift, i8(q), i32(q + 1),
                              (const float *)tab[q + 2], io->num_classes, (int8_t *)next, logits, stream);
}

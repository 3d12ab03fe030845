// Integer-only inference of an exported int8 TCNWakeword bundle (DESIGN.md "Export", the int8 law, subsection "TCN").
//   k_tq8_quantize_bt : fp32 features (B,F,T) -> int8 rows (B*T, Fp), q = clamp(rne(x / s_x) + z_x), transposed in the same pass
//   k_tq8_conv        : causal dilated Conv1d as a shifted-row GEMM on v_mfma_i32_16x16x64_i8; epilogue (a) requantise + clamp,
//                       (b) R(acc) + R(h2 + 128) + clamp: the downsample conv carrying the block's add and last ReLU
//   k_tq8_skip_add    : the identity-skip form of the add
//   k_tq8_pool_fc     : sum over T, requantise, Linear(C, num_classes), one fp32 multiply per logit
// Activations are int8 rows (B*T, Cp), Cp = the channel count rounded up to 64: every (row, tap) is a whole number of the
// instruction's 64-deep K chunks.  Pad channels hold the tensor's zero point and meet zero weights; pad OUTPUT channels have zero
// weights, a zero bias and m = 2^30, sh = 31, so they come out as -128, the zero point of every tensor a conv writes.
//
// The product, under the lane map of k_q8_pw (ww_q8.hip; DESIGN.md mfma_i8_map): D = A x B, A = weights (row = output channel),
// B = time rows (column = row l & 15 of the tile).  Lane l supplies, for tap j and K chunk kc, the 16 bytes [64 kc + 16 g,
// + 16), g = l >> 4, of the displaced row t - (k-1-j) d -- or 16 bytes of the zero point where that time is negative -- and
// the same 16 k of weight row 16 (i >> 2) + 4 m + (i & 3), i = l & 15, for product m = 0..3: the lane ends with the sixteen
// consecutive channels 64 ct + 16 g .. + 15 of its row and stores one 16-byte vector.  A wave holds TQ_RT tiles of 16 rows at
// once, so a weight fragment it loaded meets TQ_RT row fragments.  The weights of a channel tile (64 k Cpi bytes) are held in LDS
// in fragment order (k_tq8_conv_lds, the default up to 64 KB: measured 1.11 x faster over the default model's forward, DESIGN.md
// 5.6) or streamed through L2 (k_tq8_conv: larger tiles, and WW_TQ8_WEIGHTS=stream in the environment, the A/B switch).
//
// bias arguments are the EFFECTIVE bias q_b - z_in * sum(q_w) (host, once per bundle), so "a source time below 0", "a pad
// channel" and "a row past the end" are all a vector of z_in bytes.  All adds that may wrap are unsigned.
#include "ww_internal.h"

#include <cstdlib>
#include <cstring>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
constexpr int TQ_BLOCK = 256;
constexpr int TQ_WAVES = TQ_BLOCK / 64;
constexpr int TQ_RT = 4;                       // 16-row tiles a wave holds at once
constexpr int TQ_ROWS = 16 * TQ_RT;
constexpr int TQ_MAX_CP = 1024;                // widest tensor k_tq8_pool_fc sums (its LDS image)
constexpr size_t TQ_SLAB_MAX = 64 * 1024;      // largest weight image of one channel tile k_tq8_conv_lds keeps in LDS

// R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh, arithmetic shift; |a| < 2^31, 2^30 <= m < 2^31, 1 <= sh <= 62
__device__ __forceinline__ long long tq8_round(int a, int m, int sh) {
    return ((long long)a * (long long)m + (1ll << (sh - 1))) >> sh;
}

__device__ __forceinline__ int tq8_clamp(long long r) {       // clamp(-128 + r, -128, 127)
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    return (int)r - 128;
}

template <int J> __device__ __forceinline__ int tq8_byte(int d) { return (int)(signed char)((unsigned)d >> (8 * J)); }

__device__ __forceinline__ int tq8_pack4(int a, int b, int c, int d) {
    return (int)((unsigned)(a & 255) | ((unsigned)(b & 255) << 8) | ((unsigned)(c & 255) << 16) | ((unsigned)(d & 255) << 24));
}

__device__ __forceinline__ void tq8_unpack4(int d, int (&q)[4]) {
    q[0] = tq8_byte<0>(d); q[1] = tq8_byte<1>(d); q[2] = tq8_byte<2>(d); q[3] = tq8_byte<3>(d);
}

struct tq8_conv_args {
    const int8_t *in, *w;                      // in (N, Cpi); w (Cpo, k, Cpi) [out][tap][in]
    const int *bias, *mult, *shift;            // (Cpo) each
    const int8_t *res;                         // ADD: the residual tensor h2 (N, Cpo)
    int8_t *out;                               // (N, Cpo)
    long N;
    int T, Cpi, Cpo, k, dil, zfill, res_m, res_sh;
};

// One item: TQ_ROWS rows from row0 on, output channels [64 ct, 64 ct + 64).  SLAB: the weight fragments come from the workgroup's
// LDS image of channel tile ct (k_tq8_conv_lds lays it out), else from global memory.
template <bool ADD, bool SLAB>
__device__ __forceinline__ void tq8_conv_item(const tq8_conv_args &a, int ct, long row0, int lane, const v4i *slab) {
    const int p = lane & 15, g = lane >> 4;
    const int kcn = a.Cpi / 64;
    const v4i zvec = {a.zfill, a.zfill, a.zfill, a.zfill};
    const long wstride = (long)a.k * a.Cpi;
    {
        long n[TQ_RT];
        int t[TQ_RT];
#pragma unroll
        for (int r = 0; r < TQ_RT; ++r) {
            n[r] = row0 + 16 * r + p;
            t[r] = n[r] < a.N ? (int)(n[r] % a.T) : -1;        // a row past the end has no valid source time
        }
        const int8_t *wrow[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) wrow[m] = a.w + (long)(64 * ct + 16 * (p >> 2) + 4 * m + (p & 3)) * wstride + 16 * g;
        v4i acc[TQ_RT][4];
#pragma unroll
        for (int r = 0; r < TQ_RT; ++r)
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[r][m] = v4i{0, 0, 0, 0};
        for (int j = 0; j < a.k; ++j) {
            const long off = (long)(a.k - 1 - j) * a.dil;
            const int8_t *src[TQ_RT];
            bool live[TQ_RT];
#pragma unroll
            for (int r = 0; r < TQ_RT; ++r) {
                live[r] = (long)t[r] - off >= 0;
                src[r] = a.in + (n[r] - off) * a.Cpi + 16 * g;  // dereferenced only where live
            }
            for (int kc = 0; kc < kcn; ++kc) {
                v4i wa[4];
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    wa[m] = SLAB ? slab[((j * kcn + kc) * 4 + m) * 64 + lane] : *(const v4i *)(wrow[m] + (long)j * a.Cpi + 64 * kc);
#pragma unroll
                for (int r = 0; r < TQ_RT; ++r) {
                    v4i bq = zvec;
                    if (live[r]) bq = *(const v4i *)(src[r] + 64 * kc);
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc[r][m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[m], bq, acc[r][m], 0, 0, 0);
                }
            }
        }
        const int c0 = 64 * ct + 16 * g;
#pragma unroll
        for (int r = 0; r < TQ_RT; ++r) {
            if (n[r] >= a.N) continue;
            v4i hv = {0, 0, 0, 0};
            if (ADD) hv = *(const v4i *)(a.res + n[r] * a.Cpo + c0);
            v4i ov;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const v4i b = *(const v4i *)(a.bias + c0 + 4 * m);
                const v4i mu = *(const v4i *)(a.mult + c0 + 4 * m);
                const v4i sh = *(const v4i *)(a.shift + c0 + 4 * m);
                int h[4], q[4];
                tq8_unpack4(hv[m], h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    long long v = tq8_round((int)((unsigned)acc[r][m][e] + (unsigned)b[e]), mu[e], sh[e]);
                    if (ADD) v += tq8_round(h[e] + 128, a.res_m, a.res_sh);
                    q[e] = tq8_clamp(v);
                }
                ov[m] = tq8_pack4(q[0], q[1], q[2], q[3]);
            }
            *(v4i *)(a.out + n[r] * a.Cpo + c0) = ov;
        }
    }
}

// weights streamed through L2: persistent over (row group, channel tile) items, one per wave and trip
template <bool ADD> __global__ __launch_bounds__(TQ_BLOCK) void k_tq8_conv(tq8_conv_args a) {
    const int ctn = a.Cpo / 64;
    const long items = (a.N + TQ_ROWS - 1) / TQ_ROWS * ctn;
    for (long item = (long)blockIdx.x * TQ_WAVES + (threadIdx.x >> 6); item < items; item += (long)gridDim.x * TQ_WAVES)
        tq8_conv_item<ADD, false>(a, (int)(item % ctn), item / ctn * TQ_ROWS, threadIdx.x & 63, nullptr);
}

// weights of one channel tile resident in LDS, in FRAGMENT order: vector ((j kcn + kc) 4 + m) 64 + l is what lane l feeds product m
// of tap j, K chunk kc -- any 16 lanes of a ds_read_b128 group read 16 distinct 16-byte slots, so the reads are conflict-free.
// The grid is ctstep x (row workgroups): ctstep == Cpo / 64 gives a workgroup ONE channel tile for its life, ctstep == 1 (a grid
// smaller than that, or not a multiple of it) makes every workgroup walk all the tiles.  Persistent over row groups.
template <bool ADD> __global__ __launch_bounds__(TQ_BLOCK) void k_tq8_conv_lds(tq8_conv_args a, int ctstep) {
    extern __shared__ v4i tq8_slab[];
    const int ctn = a.Cpo / 64, nvec = a.k * (a.Cpi / 64) * 256;
    const long groups = (a.N + TQ_ROWS - 1) / TQ_ROWS, wstride = (long)a.k * a.Cpi;
    const int rwg = blockIdx.x / ctstep, nrwg = gridDim.x / ctstep;
    for (int ct = blockIdx.x % ctstep; ct < ctn; ct += ctstep) {
        __syncthreads();                                        // every wave is done with the previous tile's image
        for (int idx = threadIdx.x; idx < nvec; idx += TQ_BLOCK) {
            const int l = idx & 63, m = (idx >> 6) & 3, chunk = idx >> 8;           // chunk = j kcn + kc: 64 bytes of a weight row
            const int row = 64 * ct + 16 * ((l & 15) >> 2) + 4 * m + (l & 3);
            tq8_slab[idx] = *(const v4i *)(a.w + row * wstride + 64 * chunk + 16 * (l >> 4));
        }
        __syncthreads();
        for (long grp = (long)rwg * TQ_WAVES + (threadIdx.x >> 6); grp < groups; grp += (long)nrwg * TQ_WAVES)
            tq8_conv_item<ADD, true>(a, ct, grp * TQ_ROWS, threadIdx.x & 63, tq8_slab);
    }
}

// out = clamp(-128 + R(q_in - z_in, m_i, sh_i) + R(q_h2 + 128, m_a, sh_a)) over nvec 16-byte vectors
__global__ __launch_bounds__(TQ_BLOCK) void k_tq8_skip_add(const int8_t *__restrict__ in, const int8_t *__restrict__ h2, long nvec,
                                                           int z_in, int m_i, int sh_i, int m_a, int sh_a, int8_t *__restrict__ out) {
    for (long i = (long)blockIdx.x * TQ_BLOCK + threadIdx.x; i < nvec; i += (long)gridDim.x * TQ_BLOCK) {
        const v4i x = *(const v4i *)(in + 16 * i), h = *(const v4i *)(h2 + 16 * i);
        v4i o;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int xs[4], hs[4], q[4];
            tq8_unpack4(x[d], xs);
            tq8_unpack4(h[d], hs);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = tq8_clamp(tq8_round(xs[e] - z_in, m_i, sh_i) + tq8_round(hs[e] + 128, m_a, sh_a));
            o[d] = tq8_pack4(q[0], q[1], q[2], q[3]);
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
        *(int *)(out + (b * T + t) * Fp + 4 * fq) = tq8_pack4(q[0], q[1], q[2], q[3]);
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
            tq8_unpack4(*(const int *)(img + (long)t * Cp + 4 * col), q);
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
        const int pq = tq8_clamp(tq8_round(S, pool_m, pool_sh));
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

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline long tq8_round256(long n) { return (n + 255) / 256 * 256; }
inline int tq8_pad64(int c) { return (c + 63) / 64 * 64; }
inline bool tq8_mult_ok(int m, int sh) { return m >= (1 << 30) && sh >= 1 && sh <= 62; }

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
    WW_REQUIRE(!residual || tq8_mult_ok(res_mult, res_shift), WW_E_INVALID,
               "ww_tq8_conv1d_fwd: residual multiplier %d / shift %d out of range", res_mult, res_shift);
    const long N = (long)B * T;
    tq8_conv_args a{in, w, bias, mult, shift, residual, out, N, T, Cpi, Cpo, k, dilation, (zero & 255) * 0x01010101, res_mult, res_shift};
    const long items = (N + TQ_ROWS - 1) / TQ_ROWS * (Cpo / 64);
    const long want = (items + TQ_WAVES - 1) / TQ_WAVES;
    ww_prof_scope prof(ctx, WW_K_PW_FWD, (hipStream_t)stream);
    // One channel tile's weights are 64 k Cpi bytes.  Up to TQ_SLAB_MAX they are held in LDS (the launch asks for the next
    // multiple of 16 KB, so the occupancy query sees few distinct sizes); beyond it, or with WW_TQ8_WEIGHTS=stream in the
    // environment (the A/B switch of tools/bench_q8_tcn.py and the tests), they are streamed.
    const size_t slab = (size_t)64 * k * Cpi;
    const char *mode = getenv("WW_TQ8_WEIGHTS");
    if (slab <= TQ_SLAB_MAX && !(mode && !strcmp(mode, "stream"))) {
        const size_t smem = (slab + 16383) / 16384 * 16384;
        const int ctn = Cpo / 64;
        const long groups = (N + TQ_ROWS - 1) / TQ_ROWS;
        const long want_lds = (groups + TQ_WAVES - 1) / TQ_WAVES * ctn;
        const void *fn = residual ? (const void *)k_tq8_conv_lds<true> : (const void *)k_tq8_conv_lds<false>;
        int grid = ww_conv_grid(ctx, fn, TQ_BLOCK, smem, want_lds, 1 << 20);
        const int ctstep = grid >= ctn ? ctn : 1;
        grid -= grid % ctstep;
        if (residual)
            hipLaunchKernelGGL(k_tq8_conv_lds<true>, dim3(grid), dim3(TQ_BLOCK), smem, (hipStream_t)stream, a, ctstep);
        else
            hipLaunchKernelGGL(k_tq8_conv_lds<false>, dim3(grid), dim3(TQ_BLOCK), smem, (hipStream_t)stream, a, ctstep);
        WW_LAUNCH_CHECK();
        return WW_OK;
    }
    if (residual) {
        const int grid = ww_conv_grid(ctx, (const void *)k_tq8_conv<true>, TQ_BLOCK, 0, want, 1 << 20);
        hipLaunchKernelGGL(k_tq8_conv<true>, dim3(grid), dim3(TQ_BLOCK), 0, (hipStream_t)stream, a);
    } else {
        const int grid = ww_conv_grid(ctx, (const void *)k_tq8_conv<false>, TQ_BLOCK, 0, want, 1 << 20);
        hipLaunchKernelGGL(k_tq8_conv<false>, dim3(grid), dim3(TQ_BLOCK), 0, (hipStream_t)stream, a);
    }
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_tq8_skip_add_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *h2, long N, int Cp, int zero, int skip_mult,
                                   int skip_shift, int add_mult, int add_shift, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && h2 && out, WW_E_INVALID, "ww_tq8_skip_add_fwd: null argument");
    WW_REQUIRE(N >= 1 && N <= (1l << 40) && Cp >= 64 && Cp % 64 == 0, WW_E_INVALID, "ww_tq8_skip_add_fwd: N=%ld Cp=%d", N, Cp);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_tq8_skip_add_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(tq8_mult_ok(skip_mult, skip_shift) && tq8_mult_ok(add_mult, add_shift), WW_E_INVALID,
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
    WW_REQUIRE(C >= 1 && Cp == tq8_pad64(C) && Cp <= TQ_MAX_CP, WW_E_INVALID, "ww_tq8_pool_fc_fwd: C=%d Cp=%d (Cp = C rounded up to 64, at most %d)",
               C, Cp, TQ_MAX_CP);
    WW_REQUIRE(num_classes >= 2 && num_classes <= 64, WW_E_INVALID, "ww_tq8_pool_fc_fwd: num_classes=%d outside [2, 64]", num_classes);
    WW_REQUIRE(tq8_mult_ok(pool_mult, pool_shift), WW_E_INVALID, "ww_tq8_pool_fc_fwd: multiplier %d / shift %d out of range", pool_mult,
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
    long bytes = tq8_round256((long)B * T * tq8_pad64(F));
    for (int i = 0; i < n_blocks; ++i) {
        if (channels[i] < 1) return 0;
        bytes += 3 * tq8_round256((long)B * T * tq8_pad64(channels[i]));
    }
    return (size_t)(bytes + tq8_round256((long)B * channels[n_blocks - 1]));
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
    int Cpi = tq8_pad64(F), zin = io->in_zero;
    int rc = ww_tq8_quantize_bt(ctx, x, B, F, T, Cpi, io->in_scale, zin, cur, stream);
    if (rc != WW_OK) return rc;
    int8_t *next = cur + tq8_round256(N * Cpi);
    for (int i = 0; i < nb; ++i) {
        const int Cpo = tq8_pad64(io->channels[i]), d = 1 << i, p = WW_TQ8_BLOCK_NPTR * i;
        const long act = tq8_round256(N * Cpo);
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

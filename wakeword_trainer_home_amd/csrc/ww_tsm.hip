// On-GPU time-stretch and pitch-shift of waveform clips: time-domain WSOLA followed by a windowed-sinc resampler.
// Spec: DESIGN.md "Time-stretch / pitch-shift spec" (the reference's AudioAugmentation source is absent; the law is this
// build's own).  The output is linear in x once the grain positions are fixed, so it is held to fp32 round-off.
//
// k_tsm_wsola    : one workgroup per selected clip, grains in order (p_{m-1} -> p_m is a serial chain).  Per grain the span
//                  x[a_m - 128, a_m + 896) sits in LDS: its first 768 samples are the search region, and the NEXT grain's
//                  template x[p_m + 256, p_m + 768) lies inside it whatever d_m turns out to be, so the chain never waits
//                  on global memory -- the span of grain m+1 (a_{m+1} does not depend on the search) is fetched into
//                  registers while grain m is searched.  The 257 correlations of 512 terms are register-tiled: thread
//                  (dg, p) owns d = 8 dg - 128 ... 8 dg - 120 (nine candidates, the ninth is the next group's first and only
//                  group 31's is used) over the terms i = 64 s + 8 p + k; per step 6 ds_read_b128 feed 72 FMAs.  The eight
//                  partial sums of a candidate sit in neighbouring lanes (fixed-order butterfly), the argmax is a
//                  fixed-order scan that keeps the smallest d on ties.  Hop m of z is written as soon as d_m is known.
// k_tsm_resample : grid (256-sample output tiles, clips).  The z span a tile reads goes through LDS; each output sums
//                  2 half + 2 taps of h(u) = c sinc(c u) (0.5 + 0.5 cos(pi c u / 8)); sinpif / cospif four times per output and
//                  per tap of the clip, angle addition in between.  Clips with neither effect are copied.
#include "ww_internal.h"
#include <math.h>

namespace {

constexpr int LW = 512, HS = 256, DELTA = 128, ZC = 8;
constexpr int SPAN = 1024;                 // staged samples per grain: x[a - DELTA, a - DELTA + SPAN)
constexpr int FQ_ONE = 1 << 20;
constexpr int ZT = 576;                    // z samples a 256-output tile reads: <= 255 * 2 + 1 + 2 * 16 + 2 = 545
constexpr uint32_t TAG_AUDIO = 2u;

struct TsmParams {
    int B, N, Zmax, max_grains;
    uint64_t stretch_thresh, pitch_thresh;
    float rate_min, rate_max;
    int semis_min, semis_max;
    uint32_t seed_lo, seed_hi, step_lo, step_hi;
    uint64_t sample_offset;
    const ww_step_ctl *ctl;
    int32_t fq[25];                        // f_q of -12 ... +12 semitones (host, double)
};
struct TsmChoice { int stretch, semis, fq, half, Z, G; float rate; long long rho_q; bool on; };

__host__ __device__ inline int tsm_half(int fq) { return fq <= FQ_ONE ? ZC : (int)(((long long)ZC * fq + FQ_ONE - 1) >> 20); }
__host__ __device__ inline int tsm_z(int N, int fq) { return (int)(((long long)(N - 1) * fq) >> 20) + tsm_half(fq) + 2; }

__device__ __forceinline__ TsmChoice tsm_choice(const TsmParams &p, int b) {
    const uint32_t g = (uint32_t)(p.sample_offset + (uint64_t)b);
    uint32_t r[4], slo, shi;
    ww_step_resolve(p.ctl, p.step_lo, p.step_hi, slo, shi);
    ww_philox(slo, shi, g, (TAG_AUDIO << 24) | 2u, p.seed_lo, p.seed_hi, r);
    TsmChoice c;
    c.stretch = (uint64_t)r[0] < p.stretch_thresh;
    const float u = (float)(r[1] >> 8) * 5.9604644775390625e-08f;   // 2^-24, exact
    c.rate = c.stretch ? fmaf(u, p.rate_max - p.rate_min, p.rate_min) : 1.0f;
    c.semis = ((uint64_t)r[2] < p.pitch_thresh) ? p.semis_min + (int)(r[3] % (uint32_t)(p.semis_max - p.semis_min + 1)) : 0;
    c.fq = p.fq[c.semis + 12];
    c.rho_q = (long long)floor((double)c.rate / ((double)c.fq * 9.5367431640625e-07) * 65536.0 + 0.5);   // fq * 2^-20
    c.half = tsm_half(c.fq);
    c.Z = tsm_z(p.N, c.fq);
    c.G = (c.Z - 1) / HS;
    c.on = c.stretch || c.semis != 0;
    return c;
}

__global__ __launch_bounds__(256) void k_tsm_wsola(const float *__restrict__ x, TsmParams p, float *__restrict__ zbuf,
                                                   int32_t *__restrict__ choice_out, int16_t *__restrict__ delta_out) {
    __shared__ __align__(16) float span[2][SPAN];
    __shared__ __align__(16) float tau[LW];
    __shared__ float best_v[32];
    __shared__ int best_j[32];
    const int tid = threadIdx.x, b = blockIdx.x, N = p.N;
    const TsmChoice c = tsm_choice(p, b);
    if (choice_out && tid == 0) {
        choice_out[3 * b] = c.stretch; choice_out[3 * b + 1] = __float_as_int(c.rate); choice_out[3 * b + 2] = c.semis;
    }
    if (!c.on) return;                                          // block-uniform; the resampler copies the clip
    const float *xb = x + (size_t)b * N;
    float *z = zbuf + (size_t)b * p.Zmax;
    auto ld = [&](long long t) { return (t >= 0 && t < (long long)N) ? xb[t] : 0.f; };
    const float w_lo = 0.5f - 0.5f * cospif((float)tid * 0.00390625f);            // w[tid], periodic Hann over 512
    const float w_hi = 0.5f - 0.5f * cospif((float)(tid + HS) * 0.00390625f);     // w[tid + 256]
    {   // grains -1 (p = -HS) and 0 (p = 0): the first hop is x itself
        const float xv = ld(tid);
        if (tid < c.Z) z[tid] = fmaf(w_lo, xv, w_hi * xv);
    }
    tau[tid] = ld(HS + tid);                                    // template of grain 1: x[p_0 + HS + i]
    tau[tid + 256] = ld(HS + 256 + tid);
    long long a = ((long long)HS * c.rho_q) >> 16;
    float pre[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pre[k] = ld(a - DELTA + tid + 256 * k);
    const int p8 = tid & 7, dg = tid >> 3;
    for (int m = 1; m <= c.G; ++m) {
        float *sp = span[m & 1];                                // sp[r] = x[a - DELTA + r]
#pragma unroll
        for (int k = 0; k < 4; ++k) sp[tid + 256 * k] = pre[k];
        __syncthreads();                                        // span and template of grain m are in place
        const long long a_next = ((long long)(m + 1) * HS * c.rho_q) >> 16;
        if (m < c.G) {
#pragma unroll
            for (int k = 0; k < 4; ++k) pre[k] = ld(a_next - DELTA + tid + 256 * k);
        }
        int jbest = 0;                                          // d + DELTA
        if (a - DELTA < (long long)N) {                         // (else the region is empty: every c(d) is 0, d = -DELTA)
            float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            // the reads of step s+1 are issued before the FMAs of step s: with one or two waves per SIMD nothing else hides them
            const float *tp = tau + 8 * p8, *wp = sp + 8 * dg + 8 * p8;
            float4 t0 = *reinterpret_cast<const float4 *>(tp), t1 = *reinterpret_cast<const float4 *>(tp + 4);
            float4 w0 = *reinterpret_cast<const float4 *>(wp), w1 = *reinterpret_cast<const float4 *>(wp + 4);
            float4 w2 = *reinterpret_cast<const float4 *>(wp + 8), w3 = *reinterpret_cast<const float4 *>(wp + 12);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
                const float wv[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
                if (s < 7) {
                    const int i1 = 64 * (s + 1);
                    t0 = *reinterpret_cast<const float4 *>(tp + i1); t1 = *reinterpret_cast<const float4 *>(tp + i1 + 4);
                    w0 = *reinterpret_cast<const float4 *>(wp + i1); w1 = *reinterpret_cast<const float4 *>(wp + i1 + 4);
                    w2 = *reinterpret_cast<const float4 *>(wp + i1 + 8); w3 = *reinterpret_cast<const float4 *>(wp + i1 + 12);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int j = 0; j < 9; ++j) acc[j] = fmaf(tv[k], wv[k + j], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                acc[j] += __shfl_xor(acc[j], 1);
                acc[j] += __shfl_xor(acc[j], 2);
                acc[j] += __shfl_xor(acc[j], 4);
            }
            if (p8 == 0) {
                float bv = acc[0];
                int bj = 0;
#pragma unroll
                for (int j = 1; j < 8; ++j) if (acc[j] > bv) { bv = acc[j]; bj = j; }
                if (dg == 31 && acc[8] > bv) { bv = acc[8]; bj = 8; }
                best_v[dg] = bv; best_j[dg] = 8 * dg + bj;
            }
            __syncthreads();
            float bv = best_v[0];
            jbest = best_j[0];
#pragma unroll
            for (int q = 1; q < 32; ++q) {
                const float v = best_v[q];
                if (v > bv) { bv = v; jbest = best_j[q]; }     // strict: the smallest d wins a tie
            }
        }
        const int n = m * HS + tid;
        if (n < c.Z) z[n] = fmaf(w_lo, sp[jbest + tid], w_hi * tau[tid]);
        if (delta_out && tid == 0) delta_out[(size_t)b * p.max_grains + (m - 1)] = (int16_t)(jbest - DELTA);
        // template of grain m+1: x[p_m + HS + i] = sp[jbest + HS + i]
        const float t0 = sp[jbest + HS + tid], t1 = sp[jbest + HS + 256 + tid];
        __syncthreads();                                        // every read of tau and of best_* is done
        tau[tid] = t0; tau[tid + 256] = t1;
        a = a_next;
    }
}

__global__ __launch_bounds__(256) void k_tsm_resample(const float *__restrict__ x, TsmParams p, const float *__restrict__ zbuf,
                                                      float *__restrict__ out) {
    __shared__ float zt[ZT];
    __shared__ float4 rot[2 * 16 + 2];       // per tap j: cos(pi c j), sin(pi c j), cos(pi c j / 8), sin(pi c j / 8)
    const int tid = threadIdx.x, b = blockIdx.y, N = p.N, n0 = blockIdx.x * 256, n = n0 + tid;
    const TsmChoice c = tsm_choice(p, b);
    if (!c.on) {                                                // block-uniform
        if (n < N) out[(size_t)b * N + n] = x[(size_t)b * N + n];
        return;
    }
    const float PI = 3.14159265358979323846f;
    const float *z = zbuf + (size_t)b * p.Zmax;
    const float cc = c.fq <= FQ_ONE ? 1.0f : 1048576.0f / (float)c.fq;
    const int n1 = min(n0 + 255, N - 1);
    const int kb = (int)(((long long)n0 * c.fq) >> 20) - c.half;             // first and last z index of the tile
    const int ke = (int)(((long long)n1 * c.fq) >> 20) + c.half + 1;
    for (int i = tid; i <= ke - kb; i += 256) {
        const int k = kb + i;
        zt[i] = (k >= 0 && k < c.Z) ? z[k] : 0.f;
    }
    if (tid < 2 * c.half + 2) {
        // c j = hi + lo exactly (c has 24 bits, j five); sinpif / cospif reduce hi exactly, lo (<= 2^-20) enters to first order
        const float fj = (float)(tid - c.half), hi = cc * fj, pl = PI * fmaf(cc, fj, -hi), pl8 = 0.125f * pl;
        const float sh = sinpif(hi), ch = cospif(hi), sw = sinpif(0.125f * hi), cw = cospif(0.125f * hi);
        rot[tid] = make_float4(fmaf(-pl, sh, ch), fmaf(pl, ch, sh), fmaf(-pl8, sw, cw), fmaf(pl8, cw, sw));
    }
    __syncthreads();
    if (n >= N) return;
    const long long P = (long long)n * c.fq;
    const int k0 = (int)(P >> 20);
    const float fr = (float)(int)(P & (FQ_ONE - 1)) * 9.5367431640625e-07f;  // 2^-20, exact
    const float *zp = zt + (k0 - kb);
    // sin(pi c (fr - j)) and cos(pi c (fr - j) / 8) by angle addition from the output's own four values and the tap table: four
    // FMAs per tap where sinpif + cospif took sixty instructions.  The absolute error of that, ~2^-23, is divided by pi |v|, and
    // every tap but the two nearest samples has |v| >= c >= 1/2; those two (j = 0, 1: |v| can be tiny) are evaluated directly.
    const float a = cc * fr;
    const float s0 = sinpif(a), c0 = cospif(a), s0w = sinpif(0.125f * a), c0w = cospif(0.125f * a);
    float acc = 0.f;
    for (int j = -c.half; j <= c.half + 1; ++j) {
        const float v = cc * (fr - (float)j);
        if (fabsf(v) < (float)ZC) {
            const float4 r = rot[j + c.half];
            const bool near = j == 0 || j == 1;
            const float sv = near ? sinpif(v) : s0 * r.x - c0 * r.y;
            const float cwv = near ? cospif(0.125f * v) : fmaf(c0w, r.z, s0w * r.w);
            const float sinc = v == 0.f ? 1.0f : sv / (PI * v);
            acc = fmaf(zp[j], cc * sinc * (0.5f + 0.5f * cwv), acc);
        }
    }
    out[(size_t)b * N + n] = acc;
}

int tsm_fq(int semis) { return (int)llround(exp2((double)semis / 12.0) * 1048576.0); }
// the longest z of a call: a clip without pitch shift has semis = 0, whatever the range
int tsm_zmax(int N, int semis_max) { return tsm_z(N, tsm_fq(semis_max > 0 ? semis_max : 0)); }

}  // namespace

extern "C" int ww_audio_tsm_max_grains(int N, int semis_max) {
    if (N < 1 || semis_max < -12 || semis_max > 12) return 0;
    return (tsm_zmax(N, semis_max) - 1) / HS;
}

extern "C" size_t ww_audio_tsm_scratch_bytes(int B, int N, int semis_max) {
    if (B < 1 || N < 1 || semis_max < -12 || semis_max > 12) return 0;
    return (size_t)B * tsm_zmax(N, semis_max) * sizeof(float);      // z of every clip
}

extern "C" int ww_audio_tsm(ww_ctx *ctx, const float *wave_in, float *wave_out, int B, int N, const ww_audio_tsm_cfg *cfg,
                            uint64_t seed, uint64_t step, uint64_t sample_offset, int32_t *choice_out, int16_t *delta_out,
                            void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && wave_in && wave_out && cfg && scratch, WW_E_INVALID, "ww_audio_tsm: null argument");
    WW_REQUIRE(wave_in != wave_out, WW_E_INVALID, "ww_audio_tsm: in-place operation is not supported");
    WW_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N <= (1 << 28), WW_E_INVALID, "ww_audio_tsm: bad shape (%d,%d)", B, N);
    WW_REQUIRE(cfg->stretch_prob >= 0.f && cfg->stretch_prob <= 1.f && cfg->pitch_prob >= 0.f && cfg->pitch_prob <= 1.f,
               WW_E_INVALID, "ww_audio_tsm: probabilities must be in [0, 1]");
    WW_REQUIRE(0.5f <= cfg->rate_min && cfg->rate_min <= cfg->rate_max && cfg->rate_max <= 2.0f, WW_E_INVALID,
               "ww_audio_tsm: need 0.5 <= rate_min <= rate_max <= 2.0, got (%g, %g)", cfg->rate_min, cfg->rate_max);
    WW_REQUIRE(-12 <= cfg->semis_min && cfg->semis_min <= cfg->semis_max && cfg->semis_max <= 12, WW_E_INVALID,
               "ww_audio_tsm: need -12 <= semis_min <= semis_max <= 12, got (%d, %d)", cfg->semis_min, cfg->semis_max);
    WW_REQUIRE(scratch_bytes >= ww_audio_tsm_scratch_bytes(B, N, cfg->semis_max), WW_E_WORKSPACE, "ww_audio_tsm: scratch too small");
    TsmParams p;
    p.B = B; p.N = N;
    p.Zmax = tsm_zmax(N, cfg->semis_max);
    p.max_grains = (p.Zmax - 1) / HS;
    p.stretch_thresh = ww_prob_threshold((double)cfg->stretch_prob);
    p.pitch_thresh = ww_prob_threshold((double)cfg->pitch_prob);
    p.rate_min = cfg->rate_min; p.rate_max = cfg->rate_max;
    p.semis_min = cfg->semis_min; p.semis_max = cfg->semis_max;
    p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
    p.step_lo = (uint32_t)step; p.step_hi = (uint32_t)(step >> 32);
    p.sample_offset = sample_offset;
    p.ctl = ctx->step_ctl;
    hipStream_t st = (hipStream_t)stream;
    for (int s = -12; s <= 12; ++s) p.fq[s + 12] = tsm_fq(s);
    ww_prof_scope ps_(ctx, WW_K_AUDIO_AUG, st);
    hipLaunchKernelGGL(k_tsm_wsola, dim3(B), dim3(256), 0, st, wave_in, p, (float *)scratch, choice_out, delta_out);
    WW_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsm_resample, dim3((N + 255) / 256, B), dim3(256), 0, st, wave_in, p, (const float *)scratch, wave_out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

// The score stage of evaluation, after the logits, and the window cutter of the recording scan.
//   k_eval_accumulate : softmax confidence, threshold decision, ROC bin and argmax confusion counters of one batch, added to
//                       dataset-long device accumulators -- what src/evaluation/evaluator.py:136-138,220-222,305-307,379-405
//                       and src/evaluation/inference.py:208-210 do on the host after one or more D2H copies per batch.
//   k_wave_windows    : the 50 %-overlap windows of src/evaluation/inference.py:150-153, each divided by its own peak (:190-191).
// Counting is integer only: a workgroup counts into LDS, then adds each non-empty counter to the global 64-bit counters with one
// vector atomic -- the totals do not depend on the order in which the workgroups arrive.
#include "ww_internal.h"

namespace {

constexpr int EVAL_BLOCK = 256;

// exp(l - m), m >= l.  The fp32 difference h = l - m is rounded once |h| >= 2 ulps of the larger operand; left alone, that
// rounding error (up to 2^-24 |h|) becomes a RELATIVE error of the exponential: 32 ulps at |h| = 64.  The residual
// r = (l - m) - h is exact in fp64, and exp(h + r) = exp(h) (1 + r) to first order, so the confidence stays within a few
// ulps of the float64 softmax for any pair of logits.  r = 0 where the difference is exact (the maximum itself, ties).
__device__ __forceinline__ float exp_diff(float l, float m) {
    const float h = l - m;
    const float r = isfinite(h) ? (float)(((double)l - (double)m) - (double)h) : 0.f;
    const float e = expf(h);
    return fmaf(e, r, e);
}

// every comparison is (double)conf >= t, t an fp64 table entry: the float32 / float64 / Python-float comparisons of the
// reference differ only in which table the host passes (DESIGN.md "Evaluation")
__global__ __launch_bounds__(EVAL_BLOCK) void k_eval_accumulate(const float *__restrict__ scores, int kind,
                                                                const int64_t *__restrict__ targets, int B,
                                                                const double *__restrict__ thr, int K, double decision,
                                                                float *__restrict__ conf_out, uint8_t *__restrict__ pred_out,
                                                                int32_t *__restrict__ bin_out,
                                                                unsigned long long *__restrict__ hist,
                                                                unsigned long long *__restrict__ counters) {
    __shared__ double s_thr[WW_EVAL_MAX_THRESHOLDS];
    __shared__ unsigned s_hist[2 * (WW_EVAL_MAX_THRESHOLDS + 1)];
    __shared__ unsigned s_cnt[8];
    const int tid = threadIdx.x, nb = K + 1;
    for (int i = tid; i < K; i += EVAL_BLOCK) s_thr[i] = thr[i];
    for (int i = tid; i < 2 * nb; i += EVAL_BLOCK) s_hist[i] = 0u;
    if (tid < 8) s_cnt[tid] = 0u;
    __syncthreads();
    const int i = blockIdx.x * EVAL_BLOCK + tid;
    if (i < B) {
        float c;
        int amax;
        if (kind == WW_SCORE_LOGITS) {
            const float l0 = scores[(size_t)i * 2], l1 = scores[(size_t)i * 2 + 1];
            const float m = fmaxf(l0, l1);
            c = exp_diff(l1, m);
            c = c / (exp_diff(l0, m) + c);
            // torch.argmax: the first maximum wins a tie, a NaN is a maximum, the first NaN wins
            amax = (l0 == l0) && ((l1 != l1) || l1 > l0);
        } else {
            c = scores[i];
            amax = (double)c >= decision;
        }
        const double cd = (double)c;
        int lo = 0, hi = K;             // number of table entries t with cd >= t (ascending table); NaN -> 0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cd >= s_thr[mid]) lo = mid + 1; else hi = mid;
        }
        conf_out[i] = c;
        pred_out[i] = cd >= decision ? 1 : 0;
        if (bin_out) bin_out[i] = lo;
        atomicAdd(&s_cnt[4], 1u);
        if (c != c) atomicAdd(&s_cnt[6], 1u);
        if (targets) {
            const long long t = targets[i];
            if (t == 0 || t == 1) {
                atomicAdd(&s_hist[(int)t * nb + lo], 1u);
                atomicAdd(&s_cnt[t == 1 ? (amax ? 0 : 3) : (amax ? 2 : 1)], 1u);      // tp fn | fp tn
            } else {
                atomicAdd(&s_cnt[5], 1u);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < 2 * nb; j += EVAL_BLOCK) {
        const unsigned v = s_hist[j];
        if (v) atomicAdd(&hist[j], (unsigned long long)v);
    }
    if (tid < 7) {
        const unsigned v = s_cnt[tid];
        if (v) atomicAdd(&counters[tid], (unsigned long long)v);
    }
}

// The logits form of the kernel above for rows of C columns: conf = softmax(row)[1] with the maximum over all C columns
// subtracted, the predicted class is torch.argmax over C columns.  Targets 2..C-1 are valid and are counted nowhere but in
// `count`: the reference's ROC loop and its four counters look at targets 0 and 1 only.  The row is walked twice from global
// memory (no per-thread array); the exponent sum runs in double over the fp32 terms.
__global__ __launch_bounds__(EVAL_BLOCK) void k_eval_accumulate_classes(const float *__restrict__ logits, int C,
                                                                        const int64_t *__restrict__ targets, int B,
                                                                        const double *__restrict__ thr, int K, double decision,
                                                                        float *__restrict__ conf_out,
                                                                        uint8_t *__restrict__ pred_out,
                                                                        int32_t *__restrict__ bin_out,
                                                                        unsigned long long *__restrict__ hist,
                                                                        unsigned long long *__restrict__ counters) {
    __shared__ double s_thr[WW_EVAL_MAX_THRESHOLDS];
    __shared__ unsigned s_hist[2 * (WW_EVAL_MAX_THRESHOLDS + 1)];
    __shared__ unsigned s_cnt[8];
    const int tid = threadIdx.x, nb = K + 1;
    for (int i = tid; i < K; i += EVAL_BLOCK) s_thr[i] = thr[i];
    for (int i = tid; i < 2 * nb; i += EVAL_BLOCK) s_hist[i] = 0u;
    if (tid < 8) s_cnt[tid] = 0u;
    __syncthreads();
    const int i = blockIdx.x * EVAL_BLOCK + tid;
    if (i < B) {
        const float *__restrict__ z = logits + (size_t)i * C;
        // torch.argmax: the first maximum wins a tie, a NaN is a maximum, the first NaN wins
        float m = z[0], top = z[0];
        int amax = 0;
        for (int j = 1; j < C; ++j) {
            const float v = z[j];
            m = fmaxf(m, v);
            if ((top == top) && ((v != v) || v > top)) {
                top = v;
                amax = j;
            }
        }
        double se = 0.0;
        for (int j = 0; j < C; ++j) se += (double)exp_diff(z[j], m);
        const float c = exp_diff(z[1], m) / (float)se;
        const double cd = (double)c;
        int lo = 0, hi = K;             // number of table entries t with cd >= t (ascending table); NaN -> 0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cd >= s_thr[mid]) lo = mid + 1; else hi = mid;
        }
        conf_out[i] = c;
        pred_out[i] = cd >= decision ? 1 : 0;
        if (bin_out) bin_out[i] = lo;
        atomicAdd(&s_cnt[4], 1u);
        if (c != c) atomicAdd(&s_cnt[6], 1u);
        if (targets) {
            const long long t = targets[i];
            if (t == 0 || t == 1) {
                atomicAdd(&s_hist[(int)t * nb + lo], 1u);
                if (amax == 1) atomicAdd(&s_cnt[t == 1 ? 0 : 2], 1u);                 // tp | fp
                else if (amax == 0) atomicAdd(&s_cnt[t == 1 ? 3 : 1], 1u);            // fn | tn
            } else if (t < 0 || t >= C) {
                atomicAdd(&s_cnt[5], 1u);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < 2 * nb; j += EVAL_BLOCK) {
        const unsigned v = s_hist[j];
        if (v) atomicAdd(&hist[j], (unsigned long long)v);
    }
    if (tid < 7) {
        const unsigned v = s_cnt[tid];
        if (v) atomicAdd(&counters[tid], (unsigned long long)v);
    }
}

constexpr int WIN_BLOCK = 256;

__global__ __launch_bounds__(WIN_BLOCK) void k_wave_windows(const float *__restrict__ wave, int chunk, int half, int W,
                                                            float *__restrict__ out, float *__restrict__ peaks) {
    __shared__ float s_max[WIN_BLOCK];
    __shared__ int s_nan[WIN_BLOCK];
    const int tid = threadIdx.x;
    for (int w = blockIdx.x; w < W; w += gridDim.x) {
        const float *src = wave + (size_t)w * half;
        float *dst = out + (size_t)w * chunk;
        float m = 0.f;
        int nan = 0;
        for (int i = tid; i < chunk; i += WIN_BLOCK) {
            const float a = fabsf(src[i]);
            nan |= a != a;
            m = fmaxf(m, a);           // fmaxf drops a NaN operand: the flag carries it
        }
        s_max[tid] = m;
        s_nan[tid] = nan;
        __syncthreads();
        for (int s = WIN_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) {
                s_max[tid] = fmaxf(s_max[tid], s_max[tid + s]);
                s_nan[tid] |= s_nan[tid + s];
            }
            __syncthreads();
        }
        const float peak = s_max[0];
        const bool any_nan = s_nan[0] != 0;
        __syncthreads();               // s_max / s_nan are rewritten by the next window
        // np.max propagates a NaN and `NaN > 0` is false: such a window, like an all-zero one, is copied unscaled
        const bool scale = !any_nan && peak > 0.f;
        for (int i = tid; i < chunk; i += WIN_BLOCK) {
            const float x = src[i];
            dst[i] = scale ? __fdiv_rn(x, peak) : x;      // a true, correctly rounded division: NumPy's float32 x / peak
        }
        if (tid == 0) peaks[w] = any_nan ? __builtin_nanf("") : peak;
    }
}

}  // namespace

extern "C" int ww_eval_accumulate(ww_ctx *ctx, const float *scores, int score_kind, const int64_t *targets, int B,
                                  const double *thresholds, int K, double decision, float *conf, uint8_t *pred, int32_t *bin,
                                  size_t offset, uint64_t *hist, ww_eval_counters *counters, ww_stream_t stream) {
    WW_REQUIRE(ctx && scores && thresholds && conf && pred && hist && counters, WW_E_INVALID,
               "ww_eval_accumulate: null argument");
    WW_REQUIRE(score_kind == WW_SCORE_LOGITS || score_kind == WW_SCORE_CONF, WW_E_INVALID,
               "ww_eval_accumulate: unknown score_kind %d", score_kind);
    WW_REQUIRE(B >= 1, WW_E_INVALID, "ww_eval_accumulate: B=%d", B);
    WW_REQUIRE(K >= 1 && K <= WW_EVAL_MAX_THRESHOLDS, WW_E_INVALID, "ww_eval_accumulate: K=%d outside [1, %d]", K,
               WW_EVAL_MAX_THRESHOLDS);
    WW_REQUIRE(decision == decision, WW_E_INVALID, "ww_eval_accumulate: the decision threshold is NaN");
    static_assert(sizeof(ww_eval_counters) == 8 * sizeof(uint64_t), "ww_eval_counters is eight 64-bit counters");
    const int grid = (B + EVAL_BLOCK - 1) / EVAL_BLOCK;
    hipLaunchKernelGGL(k_eval_accumulate, dim3(grid), dim3(EVAL_BLOCK), 0, (hipStream_t)stream, scores, score_kind, targets, B,
                       thresholds, K, decision, conf + offset, pred + offset, bin ? bin + offset : nullptr,
                       (unsigned long long *)hist, (unsigned long long *)counters);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_eval_accumulate_classes(ww_ctx *ctx, const float *logits, int num_classes, const int64_t *targets, int B,
                                          const double *thresholds, int K, double decision, float *conf, uint8_t *pred,
                                          int32_t *bin, size_t offset, uint64_t *hist, ww_eval_counters *counters,
                                          ww_stream_t stream) {
    WW_REQUIRE(ctx && logits && thresholds && conf && pred && hist && counters, WW_E_INVALID,
               "ww_eval_accumulate_classes: null argument");
    WW_REQUIRE(num_classes >= 2 && num_classes <= WW_LOSS_MAX_CLASSES, WW_E_INVALID,
               "ww_eval_accumulate_classes: num_classes=%d outside [2, %d]", num_classes, WW_LOSS_MAX_CLASSES);
    WW_REQUIRE(B >= 1, WW_E_INVALID, "ww_eval_accumulate_classes: B=%d", B);
    WW_REQUIRE(K >= 1 && K <= WW_EVAL_MAX_THRESHOLDS, WW_E_INVALID, "ww_eval_accumulate_classes: K=%d outside [1, %d]", K,
               WW_EVAL_MAX_THRESHOLDS);
    WW_REQUIRE(decision == decision, WW_E_INVALID, "ww_eval_accumulate_classes: the decision threshold is NaN");
    const int grid = (B + EVAL_BLOCK - 1) / EVAL_BLOCK;
    hipLaunchKernelGGL(k_eval_accumulate_classes, dim3(grid), dim3(EVAL_BLOCK), 0, (hipStream_t)stream, logits, num_classes,
                       targets, B, thresholds, K, decision, conf + offset, pred + offset, bin ? bin + offset : nullptr,
                       (unsigned long long *)hist, (unsigned long long *)counters);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" long ww_wave_num_windows(long S, int chunk) {
    if (chunk < 2 || S < chunk) return 0;
    return (S - chunk) / (chunk / 2) + 1;
}

extern "C" int ww_wave_windows(ww_ctx *ctx, const float *wave, long S, int chunk, int W, float *out, float *peaks,
                               ww_stream_t stream) {
    WW_REQUIRE(ctx, WW_E_INVALID, "ww_wave_windows: null context");
    WW_REQUIRE(chunk >= 2 && S >= 0, WW_E_INVALID, "ww_wave_windows: chunk=%d S=%ld", chunk, S);
    WW_REQUIRE((long)W == ww_wave_num_windows(S, chunk), WW_E_INVALID,
               "ww_wave_windows: W=%d but %ld samples hold %ld windows of %d", W, S, ww_wave_num_windows(S, chunk), chunk);
    if (W == 0) return WW_OK;
    WW_REQUIRE(wave && out && peaks, WW_E_INVALID, "ww_wave_windows: null argument");
    const int grid = ww_pass_wave_windows(W).grid;
    hipLaunchKernelGGL(k_wave_windows, dim3(grid), dim3(WIN_BLOCK), 0, (hipStream_t)stream, wave, chunk, chunk / 2, W, out,
                       peaks);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

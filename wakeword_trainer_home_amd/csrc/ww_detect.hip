// The dense detection scan: windows of a recording at any hop, windows of a feature map, and the detector that turns the
// per-window confidences into triggers matched against labelled keyword occurrences (DESIGN.md "Evaluation", the laws are
// in include/wwhip.h).
//   k_wave_windows_at : window w0 + i = wave[(w0 + i) * hop .. + chunk), optionally divided by its own peak -- k_wave_windows'
//                       law (ww_eval.hip) at a free hop and for a slab of windows.  One workgroup per window and trip;
//                       k_wave_peak_split / k_wave_scale_split do the same for windows too long for one workgroup.
//   k_feat_windows    : out[i][0][f][t] = feat[f][(w0 + i) * step + t], a bit copy.
//   k_detect          : moving average of the confidences (fp64 sum in ascending order, one fp64 division, one rounding to
//                       fp32), then one sequential trigger machine per threshold: a lane per threshold walks the smoothed
//                       sequence, which the workgroup stages through LDS a tile at a time.
// Counting is integer only; a lane owns its threshold's counters and adds them with one vector atomic each at the end.
#include "ww_internal.h"

namespace {

constexpr int WIN_BLOCK = 256;

// Each window is read twice by the workgroup that writes it: once for its peak, once to scale it.  The slab's samples
// (n * hop + chunk of them) are read from HBM once and then live in the L2; the windows written are chunk / hop times as many
// bytes and go to HBM, so the second read is not what bounds the kernel.
__global__ __launch_bounds__(WIN_BLOCK) void k_wave_windows_at(const float *__restrict__ wave, int chunk, int hop, long w0,
                                                               int n, int normalize, float *__restrict__ out,
                                                               float *__restrict__ peaks) {
    __shared__ float s_max[WIN_BLOCK];
    __shared__ int s_nan[WIN_BLOCK];
    const int tid = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const float *src = wave + (size_t)(w0 + i) * hop;
        float *dst = out + (size_t)i * chunk;
        float m = 0.f;
        int nan = 0;
        for (int j = tid; j < chunk; j += WIN_BLOCK) {
            const float a = fabsf(src[j]);
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
        const bool scale = normalize && !any_nan && peak > 0.f;
        for (int j = tid; j < chunk; j += WIN_BLOCK) {
            const float x = src[j];
            dst[j] = scale ? __fdiv_rn(x, peak) : x;      // a true, correctly rounded division: NumPy's float32 x / peak
        }
        if (tid == 0) peaks[i] = any_nan ? __builtin_nanf("") : peak;
    }
}

// A window longer than WW_WAVE_SPLIT_CHUNK samples (a whole recording divided by its own peak is one window of S samples) is
// not left to one workgroup: it is cut into segments of WIN_SEG samples, one workgroup each, in two launches.  The bits of
// |x| order as unsigned integers, +inf below every NaN, so the peak is an integer atomic maximum into peaks[i] (zeroed
// first); a segment that holds a NaN contributes the canonical quiet NaN, which is above every other contribution.  The
// maximum does not depend on the order and the division is the same, so both forms give the same bits.
constexpr int WIN_SEG = 32 * WIN_BLOCK;

__global__ __launch_bounds__(WIN_BLOCK) void k_wave_peak_split(const float *__restrict__ wave, int chunk, int hop, long w0,
                                                               int segs, float *__restrict__ peaks) {
    __shared__ float s_max[WIN_BLOCK];
    __shared__ int s_nan[WIN_BLOCK];
    const int tid = threadIdx.x, i = blockIdx.x / segs;                      // block = i * segs + segment
    const float *src = wave + (size_t)(w0 + i) * hop;
    const int lo = (blockIdx.x - i * segs) * WIN_SEG, hi = min(chunk, lo + WIN_SEG);      // lo < chunk by the grid
    float m = 0.f;
    int nan = 0;
    for (int j = lo + tid; j < hi; j += WIN_BLOCK) {
        const float a = fabsf(src[j]);
        nan |= a != a;
        m = fmaxf(m, a);
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
    if (tid == 0) atomicMax((unsigned *)peaks + i, s_nan[0] ? 0x7fc00000u : __float_as_uint(s_max[0]));
}

__global__ __launch_bounds__(WIN_BLOCK) void k_wave_scale_split(const float *__restrict__ wave, int chunk, int hop, long w0,
                                                                int segs, int normalize, float *__restrict__ out,
                                                                const float *__restrict__ peaks) {
    const int i = blockIdx.x / segs;
    const float *src = wave + (size_t)(w0 + i) * hop;
    float *dst = out + (size_t)i * chunk;
    const int lo = (blockIdx.x - i * segs) * WIN_SEG, hi = min(chunk, lo + WIN_SEG);
    const float peak = peaks[i];
    const bool scale = normalize && peak > 0.f;          // false for a NaN peak
    for (int j = lo + threadIdx.x; j < hi; j += WIN_BLOCK) {
        const float x = src[j];
        dst[j] = scale ? __fdiv_rn(x, peak) : x;
    }
}

constexpr int FEAT_BLOCK = 256;

constexpr int FEAT_ROWS = FEAT_BLOCK / 64;       // rows (one window's band f: Tw neighbouring floats) per workgroup and trip

// one wave per row and trip: the row's address is worked out once, the lanes copy runs of neighbouring floats
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_windows(const float *__restrict__ feat, int F, long Ttot, int Tw, int step,
                                                             long w0, long rows, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * FEAT_ROWS;
    for (long row = (long)blockIdx.x * FEAT_ROWS + (threadIdx.x >> 6); row < rows; row += stride) {
        const long i = row / F;                  // row = i * F + f
        const int f = (int)(row - i * F);
        const float *src = feat + (size_t)f * Ttot + (w0 + i) * step;
        float *dst = out + (size_t)row * Tw;
        for (int t = lane; t < Tw; t += 64) dst[t] = src[t];
    }
}

constexpr int DET_BLOCK = 256;
constexpr int DET_TILE = WW_DETECT_TILE;
constexpr int DET_HALO = WW_DETECT_MAX_SMOOTH - 1;

// Workgroup g holds the machines of thresholds [g * 256, g * 256 + 256); global lane K is the decision threshold's.  Every
// workgroup smooths every tile for itself (W * M additions: nothing beside the walk), workgroup 0 writes `smoothed`.
__global__ __launch_bounds__(DET_BLOCK) void k_detect(const float *__restrict__ conf, int W, int M, int R,
                                                      const double *__restrict__ thr, int K, double decision,
                                                      const int32_t *__restrict__ events, int E,
                                                      float *__restrict__ smoothed, unsigned long long *__restrict__ counts,
                                                      unsigned long long *__restrict__ decision_counts,
                                                      int32_t *__restrict__ triggers, int max_triggers,
                                                      int32_t *__restrict__ n_triggers) {
    __shared__ float s_conf[DET_HALO + DET_TILE];
    __shared__ __attribute__((aligned(16))) float s_smooth[DET_TILE];      // DET_TILE % 8 == 0: the walk reads it in eights
    const int tid = threadIdx.x;
    const int lane = blockIdx.x * DET_BLOCK + tid;
    const bool active = lane <= K, is_decision = lane == K;
    const double t = active ? (is_decision ? decision : thr[lane]) : 0.0;
    long next_ok = 0;
    int cur = 0, hit_ev = -1;                    // first event that may still hold a trigger; the last event this lane hit
    unsigned n_trig = 0, n_hit = 0, n_fa = 0, n_dup = 0;
    for (int base = 0; base < W; base += DET_TILE) {
        const int len = min(DET_TILE, W - base);
        for (int j = tid; j < DET_HALO + len; j += DET_BLOCK) {
            const int w = base - DET_HALO + j;
            s_conf[j] = w >= 0 ? conf[w] : 0.f;
        }
        __syncthreads();
        for (int j = tid; j < len; j += DET_BLOCK) {
            const int w = base + j;
            const int cnt = min(M, w + 1);
            double acc = 0.0;
            for (int k = cnt - 1; k >= 0; --k) acc += (double)s_conf[DET_HALO + j - k];       // ascending window index
            const float s = (float)(acc / (double)cnt);
            s_smooth[j] = s;
            if (smoothed && blockIdx.x == 0) smoothed[w] = s;
        }
        __syncthreads();
        if (active) {
            // eight windows per trip, fetched with two 16-byte LDS reads before the first is looked at: the walk is a chain of
            // dependent branches, and a 4-byte read per step would put an LDS round trip into every link.  Entries past
            // `len` are stale and are not looked at.
            for (int j0 = 0; j0 < len; j0 += 8) {
                const float4 lo4 = *(const float4 *)&s_smooth[j0], hi4 = *(const float4 *)&s_smooth[j0 + 4];
                const float v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int w = base + j0 + u;
                    if (j0 + u < len && (long)w >= next_ok && (double)v[u] >= t) {      // a NaN compares false
                        next_ok = (long)w + R;
                        while (cur < E && events[2 * cur + 1] < w) ++cur;
                        if (cur < E && events[2 * cur] <= w) {
                            if (hit_ev == cur) ++n_dup;
                            else { ++n_hit; hit_ev = cur; }
                        } else {
                            ++n_fa;
                        }
                        if (is_decision && n_trig < (unsigned)max_triggers) triggers[n_trig] = w;
                        ++n_trig;
                    }
                }
            }
        }
        __syncthreads();               // the next tile overwrites s_conf / s_smooth
    }
    if (active) {
        unsigned long long *dst = is_decision ? decision_counts : counts + (size_t)lane * 4;
        if (n_trig) atomicAdd(&dst[0], (unsigned long long)n_trig);
        if (n_hit) atomicAdd(&dst[1], (unsigned long long)n_hit);
        if (n_fa) atomicAdd(&dst[2], (unsigned long long)n_fa);
        if (n_dup) atomicAdd(&dst[3], (unsigned long long)n_dup);
        if (is_decision) *n_triggers = (int32_t)n_trig;
    }
}

}  // namespace

extern "C" long ww_wave_num_windows_hop(long S, int chunk, int hop) {
    if (hop < 1 || hop > chunk || S < chunk) return 0;
    return (S - chunk) / hop + 1;
}

extern "C" int ww_wave_windows_at(ww_ctx *ctx, const float *wave, long S, int chunk, int hop, long w0, int n, int normalize,
                                  float *out, float *peaks, ww_stream_t stream) {
    WW_REQUIRE(ctx, WW_E_INVALID, "ww_wave_windows_at: null context");
    WW_REQUIRE(hop >= 1 && hop <= chunk && S >= 0, WW_E_INVALID, "ww_wave_windows_at: chunk=%d hop=%d S=%ld (1 <= hop <= chunk)",
               chunk, hop, S);
    WW_REQUIRE(normalize == 0 || normalize == 1, WW_E_INVALID, "ww_wave_windows_at: normalize=%d", normalize);
    const long W = ww_wave_num_windows_hop(S, chunk, hop);
    WW_REQUIRE(w0 >= 0 && n >= 0 && w0 + n <= W, WW_E_INVALID,
               "ww_wave_windows_at: windows [%ld, %ld) but %ld samples hold %ld windows of %d at hop %d", w0, w0 + n, S, W, chunk,
               hop);
    if (n == 0) return WW_OK;
    WW_REQUIRE(wave && out && peaks, WW_E_INVALID, "ww_wave_windows_at: null argument");
    if (chunk > WW_WAVE_SPLIT_CHUNK) {
        const int segs = (chunk + WIN_SEG - 1) / WIN_SEG;
        const long blocks = (long)n * segs;
        WW_REQUIRE(blocks <= 0x7fffffffL, WW_E_INVALID, "ww_wave_windows_at: %d windows of %d samples: cut a smaller slab", n, chunk);
        WW_HIP(hipMemsetAsync(peaks, 0, (size_t)n * sizeof(float), (hipStream_t)stream));
        hipLaunchKernelGGL(k_wave_peak_split, dim3((unsigned)blocks), dim3(WIN_BLOCK), 0, (hipStream_t)stream, wave, chunk, hop, w0,
                           segs, peaks);
        WW_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_wave_scale_split, dim3((unsigned)blocks), dim3(WIN_BLOCK), 0, (hipStream_t)stream, wave, chunk, hop,
                           w0, segs, normalize, out, peaks);
        WW_LAUNCH_CHECK();
        return WW_OK;
    }
    const int grid = ww_capped_grid(ctx, ww_pass_wave_windows(n).grid);
    hipLaunchKernelGGL(k_wave_windows_at, dim3(grid), dim3(WIN_BLOCK), 0, (hipStream_t)stream, wave, chunk, hop, w0, n, normalize,
                       out, peaks);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_feat_windows(ww_ctx *ctx, const float *feat, int F, long Ttot, int Tw, int step, long w0, int n, float *out,
                               ww_stream_t stream) {
    WW_REQUIRE(ctx, WW_E_INVALID, "ww_feat_windows: null context");
    WW_REQUIRE(F >= 1 && Tw >= 1 && step >= 1 && Ttot >= 0, WW_E_INVALID, "ww_feat_windows: F=%d Ttot=%ld Tw=%d step=%d", F, Ttot,
               Tw, step);
    WW_REQUIRE(w0 >= 0 && n >= 0, WW_E_INVALID, "ww_feat_windows: w0=%ld n=%d", w0, n);
    if (n == 0) return WW_OK;
    WW_REQUIRE((w0 + n - 1) * step + Tw <= Ttot, WW_E_INVALID,
               "ww_feat_windows: window %ld ends at column %ld of %ld", w0 + n - 1, (w0 + n - 1) * step + Tw, Ttot);
    WW_REQUIRE(feat && out, WW_E_INVALID, "ww_feat_windows: null argument");
    const long rows = (long)n * F;
    const int grid = ww_capped_grid(ctx, ww_pass_capped(rows, FEAT_ROWS, 4096).grid);
    hipLaunchKernelGGL(k_feat_windows, dim3(grid), dim3(FEAT_BLOCK), 0, (hipStream_t)stream, feat, F, Ttot, Tw, step, w0, rows,
                       out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_detect_accumulate(ww_ctx *ctx, const float *conf, int W, int M, int R, const double *thresholds, int K,
                                    double decision, const int32_t *events, int E, float *smoothed, uint64_t *counts,
                                    uint64_t *decision_counts, int32_t *triggers, int max_triggers, int32_t *n_triggers,
                                    ww_stream_t stream) {
    WW_REQUIRE(ctx, WW_E_INVALID, "ww_detect_accumulate: null context");
    WW_REQUIRE(W >= 0, WW_E_INVALID, "ww_detect_accumulate: W=%d", W);
    WW_REQUIRE(M >= 1 && M <= WW_DETECT_MAX_SMOOTH, WW_E_INVALID, "ww_detect_accumulate: M=%d outside [1, %d]", M,
               WW_DETECT_MAX_SMOOTH);
    WW_REQUIRE(R >= 1, WW_E_INVALID, "ww_detect_accumulate: R=%d", R);
    WW_REQUIRE(K >= 1 && K <= WW_EVAL_MAX_THRESHOLDS, WW_E_INVALID, "ww_detect_accumulate: K=%d outside [1, %d]", K,
               WW_EVAL_MAX_THRESHOLDS);
    WW_REQUIRE(decision == decision, WW_E_INVALID, "ww_detect_accumulate: the decision threshold is NaN");
    WW_REQUIRE(E >= 0 && max_triggers >= 0, WW_E_INVALID, "ww_detect_accumulate: E=%d max_triggers=%d", E, max_triggers);
    if (W == 0) return WW_OK;
    WW_REQUIRE(conf && thresholds && counts && decision_counts && n_triggers && (E == 0 || events) &&
               (max_triggers == 0 || triggers), WW_E_INVALID, "ww_detect_accumulate: null argument");
    const int grid = (K + 1 + DET_BLOCK - 1) / DET_BLOCK;
    hipLaunchKernelGGL(k_detect, dim3(grid), dim3(DET_BLOCK), 0, (hipStream_t)stream, conf, W, M, R, thresholds, K, decision,
                       events, E, smoothed, (unsigned long long *)counts, (unsigned long long *)decision_counts, triggers,
                       max_triggers, n_triggers);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

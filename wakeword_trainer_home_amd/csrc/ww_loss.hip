// 2-class loss + gradient + step counters in one single-block kernel; a second one adds per-class weights
// (src/models/losses.py:89-92, :199-202, :256) and the 'sum' / 'none' reductions (:95-102).
//   CE with label smoothing  : src/models/losses.py:66-98  (eps == 0 -> nn.CrossEntropyLoss, :256)
//   focal                    : src/models/losses.py:170-197
// For C == 2 the smoothed CE is exactly BCE-with-logits on d = z1 - z0 with soft target
// t = y(1-eps) + (1-y)eps, so this is the north_star's "BCE loss/grad".
// Also produces what trainer.py:196-200 / metrics.py:105-116 derive from the logits
// (argmax accuracy and confusion counters) so the step needs ONE small D2H read.
#include "ww_internal.h"

namespace {

// Per-sample loss l_b and gradient g_b = dl_b/dz_b (before any weight, divisor or loss scale) for a target already clamped to
// {0, 1}.  Both kernels below call this one function, so the plain and the weighted entry cannot drift apart.
__device__ __forceinline__ void ce2_sample(float z0, float z1, int y, int kind, float eps, float alpha, float gamma, float &lb,
                                           float &g0, float &g1) {
    const float PT_MIN = 1e-7f, PT_MAX = (float)(1.0 - 1e-7);
    const float m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    const float se = e0 + e1;
    const float lse = m + logf(se);
    const float lp0 = z0 - lse, lp1 = z1 - lse;
    const float p0 = e0 / se, p1 = e1 / se;
    if (kind == WW_LOSS_CE) {
        const float s0 = y == 0 ? 1.0f - eps : eps;
        const float s1 = y == 1 ? 1.0f - eps : eps;
        lb = -(s0 * lp0 + s1 * lp1);
        g0 = p0 - s0;
        g1 = p1 - s1;
    } else {
        const float pt_raw = y == 1 ? p1 : p0;
        const float pt = fminf(fmaxf(pt_raw, PT_MIN), PT_MAX);
        const float om = 1.0f - pt;
        const float fw = gamma == 0.f ? 1.0f : powf(om, gamma);
        const float a_t = y == 1 ? alpha : 1.0f - alpha;
        const float ce = -(y == 1 ? lp1 : lp0);
        lb = a_t * fw * ce;
        const bool inside = pt_raw > PT_MIN && pt_raw < PT_MAX;
        const float dfw = (inside && gamma != 0.f) ? -gamma * powf(om, gamma - 1.0f) : 0.f;
        const float oh0 = y == 0 ? 1.f : 0.f, oh1 = 1.f - oh0;
        const float t = dfw * ce * pt_raw;
        g0 = a_t * (fw * (p0 - oh0) + t * (oh0 - p0));
        g1 = a_t * (fw * (p1 - oh1) + t * (oh1 - p1));
    }
}

// What thread 0 writes once the block has reduced: the loss, the skip flag and the batch counters (shc[k][0]).
__device__ __forceinline__ void ce2_report(float loss, const int (*shc)[1024], int B, float *loss_out, ww_step_stats *stats,
                                           float *found_inf_out) {
    if (loss_out) *loss_out = loss;
    // data parallel: the skip decision travels with the gradients (one extra float at the end of the flat bucket that the
    // all-reduce sums), so every rank skips the step when any rank saw a bad batch
    if (found_inf_out) *found_inf_out = (!isfinite(loss) || shc[5][0]) ? 1.0f : 0.0f;
    if (stats) {
        stats->loss = loss;
        stats->correct = shc[0][0]; stats->tp = shc[1][0]; stats->tn = shc[2][0];
        stats->fp = shc[3][0]; stats->fn = shc[4][0];
        stats->nonfinite = isfinite(loss) ? 0 : 1;
        stats->bad_target = shc[5][0] ? 1 : 0;
        stats->count = B;
        stats->grad_norm = 0.f;
        stats->found_inf = (!isfinite(loss) || shc[5][0]) ? 1.0f : 0.0f;
        stats->reserved = 0;
    }
}

__global__ __launch_bounds__(1024) void k_ce2_loss(const float *__restrict__ logits, const int64_t *__restrict__ targets,
                                                   int B, int kind, float eps, float alpha, float gamma,
                                                   float *__restrict__ loss_out, float *__restrict__ dlogits,
                                                   ww_step_stats *__restrict__ stats, float *__restrict__ found_inf_out,
                                                   const ww_loss_scale *__restrict__ ls, int ls_slot,
                                                   const ww_step_ctl *__restrict__ ctl) {
    __shared__ double shl[1024];
    __shared__ int shc[6][1024];
    // fp16 storage: dL/dlogits leaves this kernel times the dynamic loss scale (GradScaler.scale(loss).backward(),
    // src/training/trainer.py:182); the loss value itself is reported unscaled
    const float gscale = ls ? ls->scale[(ctl ? ctl->parity : ls_slot) & 1] : 1.0f;
    const float invB = gscale / (float)B;
    double lsum = 0.0;
    int correct = 0, tp = 0, tn = 0, fp = 0, fn = 0, bad = 0;
    for (int b = threadIdx.x; b < B; b += 1024) {
        const float z0 = logits[(size_t)b * 2], z1 = logits[(size_t)b * 2 + 1];
        long long yy = targets[b];
        if (yy < 0 || yy > 1) {
            bad = 1;
            yy = yy < 0 ? 0 : 1;
        }
        const int y = (int)yy;
        float lb, g0, g1;
        ce2_sample(z0, z1, y, kind, eps, alpha, gamma, lb, g0, g1);
        dlogits[(size_t)b * 2] = g0 * invB;
        dlogits[(size_t)b * 2 + 1] = g1 * invB;
        lsum += (double)lb;
        const int pred = z1 > z0 ? 1 : 0;  // torch.argmax: first max wins on ties
        correct += pred == y;
        tp += (pred == 1) & (y == 1);
        tn += (pred == 0) & (y == 0);
        fp += (pred == 1) & (y == 0);
        fn += (pred == 0) & (y == 1);
    }
    shl[threadIdx.x] = lsum;
    shc[0][threadIdx.x] = correct; shc[1][threadIdx.x] = tp; shc[2][threadIdx.x] = tn;
    shc[3][threadIdx.x] = fp; shc[4][threadIdx.x] = fn; shc[5][threadIdx.x] = bad;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            shl[threadIdx.x] += shl[threadIdx.x + s];
#pragma unroll
            for (int k = 0; k < 6; ++k) shc[k][threadIdx.x] += shc[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) ce2_report((float)(shl[0] / (double)B), shc, B, loss_out, stats, found_inf_out);
}

// The same block with per-class weights w_b = class_weight[y_b] and a choice of reduction (include/wwhip.h has the table).
// With w = the sample's class weight and s = the loss scale, every gradient element is (g * w) * c with
//   c = s / B (MEAN, DIV_BATCH),  s / sum_b w_b (MEAN, DIV_WEIGHT_SUM),  s (SUM, NONE).
// sum_b w_b is known only after the block reduction, so under DIV_WEIGHT_SUM the first trip stores g * w and every thread
// rescales the elements it wrote itself (same thread, program order: no fence needed) once shw[0] is final.  Weights of
// (1, 1) make g * w == g and c == s / B, weights that are one power of two cancel exactly: hence bit-identical to k_ce2_loss.
__global__ __launch_bounds__(1024) void k_ce2_loss_weighted(const float *__restrict__ logits, const int64_t *__restrict__ targets,
                                                            int B, int kind, float eps, float alpha, float gamma,
                                                            const float *__restrict__ class_weight, int reduction, int divisor,
                                                            float *__restrict__ loss_out, float *__restrict__ loss_vec,
                                                            float *__restrict__ dlogits, ww_step_stats *__restrict__ stats,
                                                            float *__restrict__ found_inf_out,
                                                            const ww_loss_scale *__restrict__ ls, int ls_slot,
                                                            const ww_step_ctl *__restrict__ ctl) {
    __shared__ double shl[1024];
    __shared__ double shw[1024];
    __shared__ int shc[6][1024];
    const float gscale = ls ? ls->scale[(ctl ? ctl->parity : ls_slot) & 1] : 1.0f;
    const float cw0 = class_weight ? class_weight[0] : 1.0f, cw1 = class_weight ? class_weight[1] : 1.0f;
    const bool by_wsum = divisor == WW_DIV_WEIGHT_SUM;
    const bool late = reduction == WW_REDUCE_MEAN && by_wsum;                  // gradient factor known after the reduction
    const float c = late ? 1.0f : (reduction == WW_REDUCE_MEAN ? gscale / (float)B : gscale);
    double lsum = 0.0, wsum = 0.0;
    int correct = 0, tp = 0, tn = 0, fp = 0, fn = 0, bad = 0;
    for (int b = threadIdx.x; b < B; b += 1024) {
        const float z0 = logits[(size_t)b * 2], z1 = logits[(size_t)b * 2 + 1];
        long long yy = targets[b];
        if (yy < 0 || yy > 1) {
            bad = 1;
            yy = yy < 0 ? 0 : 1;
        }
        const int y = (int)yy;
        const float w = y == 1 ? cw1 : cw0;                                    // a clamped target takes the weight of its class
        float lb, g0, g1;
        ce2_sample(z0, z1, y, kind, eps, alpha, gamma, lb, g0, g1);
        dlogits[(size_t)b * 2] = (g0 * w) * c;
        dlogits[(size_t)b * 2 + 1] = (g1 * w) * c;
        if (reduction == WW_REDUCE_NONE) loss_vec[b] = lb * w;
        lsum += (double)lb * (double)w;
        wsum += (double)w;
        const int pred = z1 > z0 ? 1 : 0;  // torch.argmax: first max wins on ties; the counters ignore the weights
        correct += pred == y;
        tp += (pred == 1) & (y == 1);
        tn += (pred == 0) & (y == 0);
        fp += (pred == 1) & (y == 0);
        fn += (pred == 0) & (y == 1);
    }
    shl[threadIdx.x] = lsum;
    shw[threadIdx.x] = wsum;
    shc[0][threadIdx.x] = correct; shc[1][threadIdx.x] = tp; shc[2][threadIdx.x] = tn;
    shc[3][threadIdx.x] = fp; shc[4][threadIdx.x] = fn; shc[5][threadIdx.x] = bad;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {                                        // sum_b w_b in the same fixed order as the loss
        if ((int)threadIdx.x < s) {
            shl[threadIdx.x] += shl[threadIdx.x + s];
            shw[threadIdx.x] += shw[threadIdx.x + s];
#pragma unroll
            for (int k = 0; k < 6; ++k) shc[k][threadIdx.x] += shc[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (late) {
        const float cl = gscale / (float)shw[0];                               // sum_b w_b == 0: inf, and the loss below is NaN
        for (int b = threadIdx.x; b < B; b += 1024) {
            dlogits[(size_t)b * 2] *= cl;
            dlogits[(size_t)b * 2 + 1] *= cl;
        }
    }
    if (threadIdx.x == 0) {
        // NONE reports the MEAN value under the given divisor, so the step statistics stay meaningful
        const double den = reduction == WW_REDUCE_SUM ? 1.0 : (by_wsum ? shw[0] : (double)B);
        ce2_report((float)(shl[0] / den), shc, B, loss_out, stats, found_inf_out);
    }
}

// C classes, 2 <= C <= WW_LOSS_MAX_CLASSES: the weighted block above with a row of C logits per sample, plus an optional
// C x C count of (target, pred).  Thread per sample.  A row is never held in registers -- an array indexed by a run-time
// class would become scratch -- it is walked three times from global memory (at most 256 B, cache-resident after the first
// walk): maximum and argmax, then the exponent sum and the loss terms, then the gradient with exp recomputed.  The row sums
// (sum of exponents, smoothed loss) run in double, so a 64-wide row costs no more round-off than a 2-wide one.
// The (target, pred) pairs are counted with LDS atomics into shm and added to global memory by vector atomics, only when this
// launch leaves found_inf at 0; integer adds, so the matrix does not depend on any order.
// Why not a group of lanes per sample (one column per lane, maximum / argmax / sums by butterflies inside the wave): measured
// slower at every width from 2 to 64 (DESIGN.md "Loss scope") -- every lane of a sample repeats the per-sample logf / expf /
// division (and focal's two powf) that one thread does once here, and the rows hit the cache after their first walk.
__global__ __launch_bounds__(1024) void k_cen_loss(const float *__restrict__ logits, const int64_t *__restrict__ targets, int B,
                                                   int C, int kind, float eps, float alpha, float gamma,
                                                   const float *__restrict__ class_weight, int reduction, int divisor,
                                                   float *__restrict__ loss_out, float *__restrict__ loss_vec,
                                                   float *__restrict__ dlogits, ww_step_stats *__restrict__ stats,
                                                   float *__restrict__ found_inf_out,
                                                   unsigned long long *__restrict__ confusion,
                                                   const ww_loss_scale *__restrict__ ls, int ls_slot,
                                                   const ww_step_ctl *__restrict__ ctl) {
    __shared__ double shl[1024];
    __shared__ double shw[1024];
    __shared__ int shc[6][1024];
    __shared__ unsigned shm[WW_LOSS_MAX_CLASSES * WW_LOSS_MAX_CLASSES];
    const float PT_MIN = 1e-7f, PT_MAX = (float)(1.0 - 1e-7);
    const float gscale = ls ? ls->scale[(ctl ? ctl->parity : ls_slot) & 1] : 1.0f;
    const bool by_wsum = divisor == WW_DIV_WEIGHT_SUM;
    const bool late = reduction == WW_REDUCE_MEAN && by_wsum;                  // gradient factor known after the reduction
    const float c = late ? 1.0f : (reduction == WW_REDUCE_MEAN ? gscale / (float)B : gscale);
    const float s_on = 1.0f - eps, s_off = eps / (float)(C - 1);
    if (confusion) {
        for (int i = threadIdx.x; i < C * C; i += 1024) shm[i] = 0u;
        __syncthreads();
    }
    double lsum = 0.0, wsum = 0.0;
    int correct = 0, tp = 0, tn = 0, fp = 0, fn = 0, bad = 0;
    for (int b = threadIdx.x; b < B; b += 1024) {
        const float *__restrict__ z = logits + (size_t)b * C;
        float *__restrict__ g = dlogits + (size_t)b * C;
        long long yy = targets[b];
        if (yy < 0 || yy >= C) {
            bad = 1;
            yy = yy < 0 ? 0 : C - 1;
        }
        const int y = (int)yy;
        const float w = class_weight ? class_weight[y] : 1.0f;                 // a clamped target takes the weight of its class
        float m = z[0], top = z[0];
        int pred = 0;                                                          // first maximum under >: a NaN never wins
        for (int j = 1; j < C; ++j) {
            const float v = z[j];
            m = fmaxf(m, v);
            if (v > top) {
                top = v;
                pred = j;
            }
        }
        double sed = 0.0, zsum = 0.0;
        for (int j = 0; j < C; ++j) {
            const float v = z[j];
            sed += (double)expf(v - m);
            zsum += (double)v;
        }
        const float se = (float)sed;
        const float lse = m + logf(se);
        const float zy = z[y];
        const float lpy = zy - lse;
        const float py = expf(zy - m) / se;
        float lb;
        if (kind == WW_LOSS_CE) {
            // -sum_j s_j lp_j with lp_j = z_j - lse: the off-target terms together are s_off ((sum_j z_j - z_y) - (C-1) lse)
            const double off = (zsum - (double)zy) - (double)(C - 1) * (double)lse;
            lb = (float)(-((double)s_on * (double)lpy + (s_off != 0.f ? (double)s_off * off : 0.0)));   // eps == 0: no 0 * inf
            for (int j = 0; j < C; ++j) {
                const float p = expf(z[j] - m) / se;
                g[j] = ((p - (j == y ? s_on : s_off)) * w) * c;
            }
        } else {
            const float pt = fminf(fmaxf(py, PT_MIN), PT_MAX);
            const float om = 1.0f - pt;
            const float fw = gamma == 0.f ? 1.0f : powf(om, gamma);
            const float a_t = y == 1 ? alpha : 1.0f - alpha;                   // class 1 is the wakeword for every C
            const float ce = -lpy;
            lb = a_t * fw * ce;
            const bool inside = py > PT_MIN && py < PT_MAX;
            const float dfw = (inside && gamma != 0.f) ? -gamma * powf(om, gamma - 1.0f) : 0.f;
            const float t = dfw * ce * py;
            for (int j = 0; j < C; ++j) {
                const float p = expf(z[j] - m) / se;
                const float oh = j == y ? 1.f : 0.f;
                g[j] = ((a_t * (fw * (p - oh) + t * (oh - p))) * w) * c;
            }
        }
        if (reduction == WW_REDUCE_NONE) loss_vec[b] = lb * w;
        lsum += (double)lb * (double)w;
        wsum += (double)w;
        correct += pred == y;                                                  // the counters ignore the weights
        tp += (pred == 1) & (y == 1);
        tn += (pred == 0) & (y == 0);
        fp += (pred == 1) & (y == 0);
        fn += (pred == 0) & (y == 1);
        if (confusion) atomicAdd(&shm[y * C + pred], 1u);
    }
    shl[threadIdx.x] = lsum;
    shw[threadIdx.x] = wsum;
    shc[0][threadIdx.x] = correct; shc[1][threadIdx.x] = tp; shc[2][threadIdx.x] = tn;
    shc[3][threadIdx.x] = fp; shc[4][threadIdx.x] = fn; shc[5][threadIdx.x] = bad;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {                                        // one fixed order for the loss and sum_b w_b
        if ((int)threadIdx.x < s) {
            shl[threadIdx.x] += shl[threadIdx.x + s];
            shw[threadIdx.x] += shw[threadIdx.x + s];
#pragma unroll
            for (int k = 0; k < 6; ++k) shc[k][threadIdx.x] += shc[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (late) {
        const float cl = gscale / (float)shw[0];                               // sum_b w_b == 0: inf, and the loss below is NaN
        for (int b = threadIdx.x; b < B; b += 1024) {
            float *__restrict__ g = dlogits + (size_t)b * C;
            for (int j = 0; j < C; ++j) g[j] *= cl;
        }
    }
    // NONE reports the MEAN value under the given divisor, so the step statistics stay meaningful
    const double den = reduction == WW_REDUCE_SUM ? 1.0 : (by_wsum ? shw[0] : (double)B);
    const float loss = (float)(shl[0] / den);
    if (confusion && isfinite(loss) && !shc[5][0]) {                           // the batch the reference's tracker sees
        for (int i = threadIdx.x; i < C * C; i += 1024) {
            const unsigned v = shm[i];
            if (v) atomicAdd(&confusion[i], (unsigned long long)v);
        }
    }
    if (threadIdx.x == 0) ce2_report(loss, shc, B, loss_out, stats, found_inf_out);
}

}  // namespace

extern "C" int ww_cen_loss_fwd_bwd(ww_ctx *ctx, const float *logits, const int64_t *targets, int B, int num_classes,
                                   int loss_kind, float label_smoothing, float focal_alpha, float focal_gamma,
                                   const float *class_weight, int reduction, int mean_divisor, float *loss_out,
                                   float *loss_vec, float *dlogits, ww_step_stats *stats, float *found_inf_out,
                                   uint64_t *confusion, const ww_loss_scale *loss_scale, int loss_scale_slot,
                                   ww_stream_t stream) {
    WW_REQUIRE(ctx && logits && targets && dlogits, WW_E_INVALID, "ww_cen_loss_fwd_bwd: null argument");
    WW_REQUIRE(B >= 1, WW_E_INVALID, "ww_cen_loss_fwd_bwd: B=%d", B);
    WW_REQUIRE(num_classes >= 2 && num_classes <= WW_LOSS_MAX_CLASSES, WW_E_INVALID,
               "ww_cen_loss_fwd_bwd: num_classes=%d outside [2, %d]", num_classes, WW_LOSS_MAX_CLASSES);
    WW_REQUIRE(loss_kind == WW_LOSS_CE || loss_kind == WW_LOSS_FOCAL, WW_E_INVALID,
               "ww_cen_loss_fwd_bwd: unknown loss_kind %d", loss_kind);
    WW_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, WW_E_INVALID,
               "Label smoothing must be in [0, 1], got %g", label_smoothing);
    WW_REQUIRE(focal_alpha >= 0.f && focal_alpha <= 1.f, WW_E_INVALID, "Alpha must be in [0, 1], got %g", focal_alpha);
    WW_REQUIRE(focal_gamma >= 0.f, WW_E_INVALID, "Gamma must be non-negative, got %g", focal_gamma);
    WW_REQUIRE(reduction == WW_REDUCE_MEAN || reduction == WW_REDUCE_SUM || reduction == WW_REDUCE_NONE, WW_E_INVALID,
               "ww_cen_loss_fwd_bwd: unknown reduction %d", reduction);
    WW_REQUIRE(mean_divisor == WW_DIV_BATCH || mean_divisor == WW_DIV_WEIGHT_SUM, WW_E_INVALID,
               "ww_cen_loss_fwd_bwd: unknown mean_divisor %d", mean_divisor);
    WW_REQUIRE(reduction != WW_REDUCE_NONE || loss_vec, WW_E_INVALID,
               "ww_cen_loss_fwd_bwd: reduction NONE needs loss_vec (B floats)");
    WW_REQUIRE(loss_scale_slot == 0 || loss_scale_slot == 1, WW_E_INVALID, "ww_cen_loss_fwd_bwd: loss_scale_slot must be 0 or 1");
    ww_prof_scope ps_(ctx, WW_K_HEAD_LOSS, (hipStream_t)stream);
    hipLaunchKernelGGL(k_cen_loss, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, targets, B, num_classes, loss_kind,
                       label_smoothing, focal_alpha, focal_gamma, class_weight, reduction, mean_divisor, loss_out, loss_vec,
                       dlogits, stats, found_inf_out, (unsigned long long *)confusion, loss_scale, loss_scale_slot,
                       ctx->step_ctl);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_ce2_loss_fwd_bwd(ww_ctx *ctx, const float *logits, const int64_t *targets, int B, int loss_kind,
                                   float label_smoothing, float focal_alpha, float focal_gamma, float *loss_out,
                                   float *dlogits, ww_step_stats *stats, float *found_inf_out, const ww_loss_scale *loss_scale,
                                   int loss_scale_slot, ww_stream_t stream) {
    WW_REQUIRE(ctx && logits && targets && dlogits, WW_E_INVALID, "ww_ce2_loss_fwd_bwd: null argument");
    WW_REQUIRE(B >= 1, WW_E_INVALID, "ww_ce2_loss_fwd_bwd: B=%d", B);
    WW_REQUIRE(loss_kind == WW_LOSS_CE || loss_kind == WW_LOSS_FOCAL, WW_E_INVALID,
               "ww_ce2_loss_fwd_bwd: unknown loss_kind %d", loss_kind);
    // same range checks as the reference constructors (losses.py:36-37, 132-135)
    WW_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, WW_E_INVALID,
               "Label smoothing must be in [0, 1], got %g", label_smoothing);
    WW_REQUIRE(focal_alpha >= 0.f && focal_alpha <= 1.f, WW_E_INVALID, "Alpha must be in [0, 1], got %g", focal_alpha);
    WW_REQUIRE(focal_gamma >= 0.f, WW_E_INVALID, "Gamma must be non-negative, got %g", focal_gamma);
    WW_REQUIRE(loss_scale_slot == 0 || loss_scale_slot == 1, WW_E_INVALID, "ww_ce2_loss_fwd_bwd: loss_scale_slot must be 0 or 1");
    ww_prof_scope ps_(ctx, WW_K_HEAD_LOSS, (hipStream_t)stream);
    hipLaunchKernelGGL(k_ce2_loss, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, targets, B, loss_kind,
                       label_smoothing, focal_alpha, focal_gamma, loss_out, dlogits, stats, found_inf_out, loss_scale,
                       loss_scale_slot, ctx->step_ctl);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_ce2_loss_weighted_fwd_bwd(ww_ctx *ctx, const float *logits, const int64_t *targets, int B, int loss_kind,
                                            float label_smoothing, float focal_alpha, float focal_gamma,
                                            const float *class_weight, int reduction, int mean_divisor, float *loss_out,
                                            float *loss_vec, float *dlogits, ww_step_stats *stats, float *found_inf_out,
                                            const ww_loss_scale *loss_scale, int loss_scale_slot, ww_stream_t stream) {
    WW_REQUIRE(ctx && logits && targets && dlogits, WW_E_INVALID, "ww_ce2_loss_weighted_fwd_bwd: null argument");
    WW_REQUIRE(B >= 1, WW_E_INVALID, "ww_ce2_loss_weighted_fwd_bwd: B=%d", B);
    WW_REQUIRE(loss_kind == WW_LOSS_CE || loss_kind == WW_LOSS_FOCAL, WW_E_INVALID,
               "ww_ce2_loss_weighted_fwd_bwd: unknown loss_kind %d", loss_kind);
    WW_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, WW_E_INVALID,
               "Label smoothing must be in [0, 1], got %g", label_smoothing);
    WW_REQUIRE(focal_alpha >= 0.f && focal_alpha <= 1.f, WW_E_INVALID, "Alpha must be in [0, 1], got %g", focal_alpha);
    WW_REQUIRE(focal_gamma >= 0.f, WW_E_INVALID, "Gamma must be non-negative, got %g", focal_gamma);
    WW_REQUIRE(reduction == WW_REDUCE_MEAN || reduction == WW_REDUCE_SUM || reduction == WW_REDUCE_NONE, WW_E_INVALID,
               "ww_ce2_loss_weighted_fwd_bwd: unknown reduction %d", reduction);
    WW_REQUIRE(mean_divisor == WW_DIV_BATCH || mean_divisor == WW_DIV_WEIGHT_SUM, WW_E_INVALID,
               "ww_ce2_loss_weighted_fwd_bwd: unknown mean_divisor %d", mean_divisor);
    WW_REQUIRE(reduction != WW_REDUCE_NONE || loss_vec, WW_E_INVALID,
               "ww_ce2_loss_weighted_fwd_bwd: reduction NONE needs loss_vec (B floats)");
    WW_REQUIRE(loss_scale_slot == 0 || loss_scale_slot == 1, WW_E_INVALID,
               "ww_ce2_loss_weighted_fwd_bwd: loss_scale_slot must be 0 or 1");
    ww_prof_scope ps_(ctx, WW_K_HEAD_LOSS, (hipStream_t)stream);
    hipLaunchKernelGGL(k_ce2_loss_weighted, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, targets, B, loss_kind,
                       label_smoothing, focal_alpha, focal_gamma, class_weight, reduction, mean_divisor, loss_out, loss_vec,
                       dlogits, stats, found_inf_out, loss_scale, loss_scale_slot, ctx->step_ctl);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

// Integer-only inference of an exported int8 LSTMWakeword bundle (DESIGN.md "Export", the int8 law, subsection "LSTM").
//   the projection : the input projection of both directions over all B*T rows: the one-segment geometry of the int8 tap-GEMM
//                 core (ww_q8_tap_gemm.h) with the epilogue LqInt16 -- effective bias, R, the int16 clamp; it stores
//                 u (B*T, nd*512) int16, Q8 gate pre-activations
//   k_lq8_lstm  : the recurrence of one layer, both directions in one launch (gridDim.y): T dependent steps of
//                 MFMA over K = 128 -> gate arithmetic in integer C++ -> the int8 output row -> LDS -> barrier
//   k_lq8_head  : hcat = [forward q_h[T-1], reverse q_h[0]], Linear(nd*128, num_classes), one fp32 multiply per logit
// Quantisation is ww_tq8_quantize_bt (ww_q8_tcn.hip): (B,F,T) fp32 -> (B*T, Fp) int8 rows, Fp = F rounded up to 64, the pad
// channels holding z_x and meeting zero weights.
//
// The recurrence.  A workgroup owns LQ_RB = 16 batch rows (the instruction's 16 columns) of one direction for all T steps and
// walks further row groups persistently.  Its eight waves split the 128 hidden units: wave w owns units 16 w .. 16 w + 15 and
// keeps the 64 rows of W_hh that feed them -- gates i, f, g, o of those units, 64 x 128 bytes -- in 32 registers for the whole
// launch, as the A operands of 4 gates x 2 K chunks.  The B operand is q_h of the 16 batch rows, int8 in LDS (two buffers, so a
// step needs ONE barrier: a step reads one and writes the other).  Under the lane map of k_q8_pw (DESIGN.md mfma_i8_map) lane l,
// p = l & 15, g = l >> 4, ends with D rows 4 g + e, e = 0..3, of column p: with A row r = unit 16 w + r of gate G, the four
// products leave the lane with all four gates of units 16 w + 4 g + e of batch row p -- the thread OWNS those four cells, c lives
// in its registers, and no gate value crosses lanes.  u of the next step is loaded before the current step's products are issued.
// The sigmoid and tanh tables (2 x 4096 int16, from the bundle) are copied to LDS once per launch (k_lq8_lstm<true>, the
// default) or read through the caches (k_lq8_lstm<false>, WW_LQ8_TABLES=global in the environment: the A/B switch of
// tools/bench_q8_lstm.py and the tests); both give the same bits.
//
// All adds that may wrap are unsigned; the law's refusal bounds keep every true sum inside int32.
#include "ww_q8_tap_gemm.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int LQ_H = 128;                      // hidden size: the implemented size of LSTMWakeword
constexpr int LQ_G = 4 * LQ_H;                 // gate rows of one direction, torch's order i, f, g, o
constexpr int LQ_BLOCK = 512;                  // the recurrence: 8 waves x 16 hidden units
constexpr int LQ_RB = 16;                      // batch rows a workgroup owns
constexpr int LQ_HROW = LQ_H + 16;             // LDS row of q_h: 144 bytes, so the 16 rows of a ds_read_b128 group spread over banks
constexpr int LQ_TAB = 4096;
constexpr int PJ_RT = 4;                       // the projection: a wave's item is 64 rows x 64 gate rows

// u = clamp(R(acc + bias, m, sh), -32768, 32767): the lane's sixteen gate rows c0 .. c0 + 15 of row n, two 16-byte stores
struct LqInt16 : Q8Chan {
    int16_t *u;                                // (N, G)
    __device__ void store(const v4i (&acc)[4], long n, int c0) const {
        int q[16];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const v4i b = *(const v4i *)(bias + c0 + 4 * m);
            const v4i mu = *(const v4i *)(mult + c0 + 4 * m);
            const v4i sh = *(const v4i *)(shift + c0 + 4 * m);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long v = q8_round((int)((unsigned)acc[m][e] + (unsigned)b[e]), mu[e], sh[e]);
                q[4 * m + e] = v < -32768 ? -32768 : (v > 32767 ? 32767 : (int)v);
            }
        }
        int16_t *dst = u + n * Cout + c0;
        *(v4i *)dst = v4i{q8_pack16(q[0], q[1]), q8_pack16(q[2], q[3]), q8_pack16(q[4], q[5]), q8_pack16(q[6], q[7])};
        *(v4i *)(dst + 8) = v4i{q8_pack16(q[8], q[9]), q8_pack16(q[10], q[11]), q8_pack16(q[12], q[13]), q8_pack16(q[14], q[15])};
    }
};

struct lq8_rec_args {
    const int16_t *u;                          // (B*T, nd*512)
    const int8_t *w_hh;                        // (nd*512, 128)
    const int *bias, *mult, *shift;            // (nd*512) each; bias is the law's q_bh (the zero point of q_h is 0)
    const int16_t *tab_sigmoid, *tab_tanh;     // (4096) each
    int8_t *y;                                 // (B*T, nd*128)
    int16_t *c_n;                              // (B, nd*128)
    int B, T, nd;
};

template <bool TAB_LDS> __global__ __launch_bounds__(LQ_BLOCK) void k_lq8_lstm(lq8_rec_args a) {
    __shared__ __attribute__((aligned(16))) int8_t s_h[2][LQ_RB * LQ_HROW];
    extern __shared__ int16_t s_tab[];         // TAB_LDS: sigmoid, then tanh
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = lane & 15, g = lane >> 4;
    const int dir = blockIdx.y, unit0 = 16 * wv + 4 * g;
    const int16_t *sig = a.tab_sigmoid, *tnh = a.tab_tanh;
    if (TAB_LDS) {
        for (int i = tid; i < LQ_TAB; i += LQ_BLOCK) {
            s_tab[i] = a.tab_sigmoid[i];
            s_tab[LQ_TAB + i] = a.tab_tanh[i];
        }
        sig = s_tab;
        tnh = s_tab + LQ_TAB;
    }
    // the wave's 64 rows of W_hh as A fragments: A row i = l & 15 of the product of gate G is unit 16 wv + i of that gate
    v4i wa[4][2], bq[4], mq[4], sq[4];
#pragma unroll
    for (int G = 0; G < 4; ++G) {
        const int row = dir * LQ_G + G * LQ_H + 16 * wv;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) wa[G][kc] = *(const v4i *)(a.w_hh + (long)(row + p) * LQ_H + 64 * kc + 16 * g);
        bq[G] = *(const v4i *)(a.bias + row + 4 * g);
        mq[G] = *(const v4i *)(a.mult + row + 4 * g);
        sq[G] = *(const v4i *)(a.shift + row + 4 * g);
    }
    const int groups = (a.B + LQ_RB - 1) / LQ_RB;
    const long ustride = (long)a.nd * LQ_G, ystride = (long)a.nd * LQ_H;
    const int t0 = dir ? a.T - 1 : 0, dt = dir ? -1 : 1;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int b = grp * LQ_RB + p;
        const bool live = b < a.B;
        for (int i = tid; i < LQ_RB * LQ_HROW / 4; i += LQ_BLOCK) ((int *)s_h[0])[i] = 0;      // q_h = 0 before the first step
        __syncthreads();                        // (and the tables are in place)
        const int16_t *ub = a.u + (long)(live ? b : 0) * a.T * ustride + dir * LQ_G + unit0;
        int8_t *yb = a.y + (long)(live ? b : 0) * a.T * ystride + dir * LQ_H + unit0;
        int c[4] = {0, 0, 0, 0};
        v2i un[4];
#pragma unroll
        for (int G = 0; G < 4; ++G) un[G] = live ? *(const v2i *)(ub + t0 * ustride + G * LQ_H) : v2i{0, 0};
        for (int s = 0; s < a.T; ++s) {
            const int t = t0 + s * dt;
            v2i uc[4];
#pragma unroll
            for (int G = 0; G < 4; ++G) uc[G] = un[G];
            if (live && s + 1 < a.T) {
#pragma unroll
                for (int G = 0; G < 4; ++G) un[G] = *(const v2i *)(ub + (t + dt) * ustride + G * LQ_H);
            }
            const int8_t *hp = s_h[s & 1] + p * LQ_HROW + 16 * g;
            const v4i h0 = *(const v4i *)hp, h1 = *(const v4i *)(hp + 64);
            v4i acc[4];
#pragma unroll
            for (int G = 0; G < 4; ++G) {
                acc[G] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[G][0], h0, v4i{0, 0, 0, 0}, 0, 0, 0);
                acc[G] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[G][1], h1, acc[G], 0, 0, 0);
            }
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                long long pre[4];
#pragma unroll
                for (int G = 0; G < 4; ++G) {
                    const int uu = (e & 1) ? q8_hi16(uc[G][e >> 1]) : q8_lo16(uc[G][e >> 1]);
                    pre[G] = uu + q8_round((int)((unsigned)acc[G][e] + (unsigned)bq[G][e]), mq[G][e], sq[G][e]);
                }
                const int gi = q8_look(sig, pre[0]), gf = q8_look(sig, pre[1]), gg = q8_look(tnh, pre[2]), go = q8_look(sig, pre[3]);
                int cn = (gf * c[e] + ((gi * gg + 8) >> 4) + (1 << 14)) >> 15;      // |.| < 2^30 + 2^26 + 2^14: inside int32
                cn = cn < -32768 ? -32768 : (cn > 32767 ? 32767 : cn);
                c[e] = cn;
                const int h16 = (go * q8_look(tnh, (cn + 4) >> 3) + (1 << 14)) >> 15;
                const int qh = (h16 + 128) >> 8;
                q[e] = qh < -128 ? -128 : (qh > 127 ? 127 : qh);
            }
            const int packed = q8_pack4(q[0], q[1], q[2], q[3]);
            *(int *)(s_h[(s + 1) & 1] + p * LQ_HROW + unit0) = packed;
            if (live) *(int *)(yb + t * ystride) = packed;
            __syncthreads();                    // q_h[t] is whole before any wave's next product reads it
        }
        if (live) *(v2i *)(a.c_n + (long)b * ystride + dir * LQ_H + unit0) = v2i{q8_pack16(c[0], c[1]), q8_pack16(c[2], c[3])};
    }
}

// one workgroup per sample and trip: hcat, then one thread per class
__global__ __launch_bounds__(64) void k_lq8_head(const int8_t *__restrict__ y, int B, int T, int nd, const int8_t *__restrict__ fc_w,
                                                 const int *__restrict__ fc_b, const float *__restrict__ fc_scale, int nc,
                                                 int8_t *__restrict__ hcat, float *__restrict__ logits) {
    __shared__ int s_h[2 * LQ_H];
    const int C = nd * LQ_H, tid = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        for (int c = tid; c < C; c += 64) {
            const int t = c >= LQ_H ? 0 : T - 1;                    // forward: the last step; reverse: its last step, t = 0
            const int8_t v = y[((long)b * T + t) * C + c];
            hcat[(long)b * C + c] = v;
            s_h[c] = v;
        }
        __syncthreads();
        if (tid < nc) {
            unsigned acc = (unsigned)fc_b[tid];
            for (int c = 0; c < C; ++c) acc += (unsigned)((int)fc_w[(long)tid * C + c] * s_h[c]);
            logits[(long)b * nc + tid] = (float)(int)acc * fc_scale[tid];
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int ww_lq8_proj_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                               const int32_t *shift, long N, int Kp, int G, int16_t *u, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w && bias && mult && shift && u, WW_E_INVALID, "ww_lq8_proj_fwd: null argument");
    WW_REQUIRE(N >= 1 && N <= (1l << 40), WW_E_INVALID, "ww_lq8_proj_fwd: N=%ld", N);
    WW_REQUIRE(Kp >= 64 && Kp % 64 == 0 && Kp <= (1 << 16), WW_E_INVALID, "ww_lq8_proj_fwd: Kp=%d must be a multiple of 64", Kp);
    WW_REQUIRE(G == LQ_G || G == 2 * LQ_G || G == 3 * LQ_H || G == 6 * LQ_H, WW_E_INVALID,
               "ww_lq8_proj_fwd: G=%d gate rows, expected %d or %d (LSTM), %d or %d (GRU)", G, LQ_G, 2 * LQ_G, 3 * LQ_H, 6 * LQ_H);
    WW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(u), WW_E_INVALID,
               "ww_lq8_proj_fwd: tensors must be 16-byte aligned");
    // the pad columns of w are zero and a row past the end is not stored, so the fill value never reaches an output
    const Q8Rows geo{in, N, Kp, 0};
    const LqInt16 epi{{bias, mult, shift, G}, u};
    ww_prof_scope prof(ctx, WW_K_LINEAR, (hipStream_t)stream);
    return q8_tap_launch_stream<Q8Rows, LqInt16, PJ_RT>(ctx, geo, epi, w, (hipStream_t)stream);
}

extern "C" int ww_lq8_lstm_layer_fwd(ww_ctx *ctx, const int16_t *u, const int8_t *w_hh, const int32_t *bias, const int32_t *mult,
                                     const int32_t *shift, const int16_t *tab_sigmoid, const int16_t *tab_tanh, int B, int T,
                                     int num_directions, int8_t *y, int16_t *c_n, ww_stream_t stream) {
    WW_REQUIRE(ctx && u && w_hh && bias && mult && shift && tab_sigmoid && tab_tanh && y && c_n, WW_E_INVALID,
               "ww_lq8_lstm_layer_fwd: null argument");
    WW_REQUIRE(B >= 1 && T >= 1 && (long)B * T <= (1l << 31), WW_E_INVALID, "ww_lq8_lstm_layer_fwd: B=%d T=%d", B, T);
    WW_REQUIRE(num_directions == 1 || num_directions == 2, WW_E_INVALID, "ww_lq8_lstm_layer_fwd: %d directions", num_directions);
    WW_REQUIRE(aligned16(u) && aligned16(w_hh) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(y) &&
               aligned16(c_n), WW_E_INVALID, "ww_lq8_lstm_layer_fwd: tensors must be 16-byte aligned");
    lq8_rec_args a{u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh, y, c_n, B, T, num_directions};
    const int groups = (B + LQ_RB - 1) / LQ_RB;
    const char *mode = getenv("WW_LQ8_TABLES");
    const bool lds = !(mode && !strcmp(mode, "global"));
    const size_t smem = lds ? 2 * LQ_TAB * sizeof(int16_t) : 0;
    const void *fn = lds ? (const void *)k_lq8_lstm<true> : (const void *)k_lq8_lstm<false>;
    const int grid = ww_conv_grid(ctx, fn, LQ_BLOCK, smem, groups, 1 << 20);
    ww_prof_scope prof(ctx, WW_K_LSTM, (hipStream_t)stream);
    if (lds)
        hipLaunchKernelGGL(k_lq8_lstm<true>, dim3(grid, num_directions), dim3(LQ_BLOCK), smem, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_lq8_lstm<false>, dim3(grid, num_directions), dim3(LQ_BLOCK), smem, (hipStream_t)stream, a);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_lq8_head_fwd(ww_ctx *ctx, const int8_t *y, int B, int T, int num_directions, const int8_t *fc_w,
                               const int32_t *fc_bias, const float *fc_scale, int num_classes, int8_t *hcat, float *logits,
                               ww_stream_t stream) {
    WW_REQUIRE(ctx && y && fc_w && fc_bias && fc_scale && hcat && logits, WW_E_INVALID, "ww_lq8_head_fwd: null argument");
    WW_REQUIRE(B >= 1 && T >= 1, WW_E_INVALID, "ww_lq8_head_fwd: B=%d T=%d", B, T);
    WW_REQUIRE(num_directions == 1 || num_directions == 2, WW_E_INVALID, "ww_lq8_head_fwd: %d directions", num_directions);
    WW_REQUIRE(num_classes >= 2 && num_classes <= 64, WW_E_INVALID, "ww_lq8_head_fwd: num_classes=%d outside [2, 64]", num_classes);
    const int grid = ww_capped_grid(ctx, B < 4096 ? B : 4096);
    hipLaunchKernelGGL(k_lq8_head, dim3(grid), dim3(64), 0, (hipStream_t)stream, y, B, T, num_directions, fc_w, fc_bias, fc_scale,
                       num_classes, hcat, logits);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" size_t ww_lq8_lstm_workspace_bytes(int B, int T, int input_size, int num_layers, int num_directions) {
    if (B < 1 || T < 1 || input_size < 1 || num_layers < 1 || num_layers > WW_LQ8_MAX_LAYERS || num_directions < 1 ||
        num_directions > 2)
        return 0;
    const long N = (long)B * T;
    const long layer = q8_round256(N * num_directions * LQ_G * 2) + q8_round256(N * num_directions * LQ_H) +
                       q8_round256((long)B * num_directions * LQ_H * 2);
    return (size_t)(q8_round256(N * q8_pad64(input_size)) + num_layers * layer + q8_round256((long)B * num_directions * LQ_H));
}

extern "C" int ww_lq8_lstm_fwd(ww_ctx *ctx, const void *const *tab, const ww_lq8_io *io, const float *x, int B, int T, void *ws,
                               size_t ws_bytes, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && tab && io && x && ws && logits, WW_E_INVALID, "ww_lq8_lstm_fwd: null argument");
    const int L = io->num_layers, nd = io->num_directions, F = io->input_size;
    WW_REQUIRE(B >= 1 && T >= 1 && F >= 1, WW_E_INVALID, "ww_lq8_lstm_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(L >= 1 && L <= WW_LQ8_MAX_LAYERS && (nd == 1 || nd == 2), WW_E_INVALID, "ww_lq8_lstm_fwd: %d layers, %d directions", L, nd);
    const size_t need = ww_lq8_lstm_workspace_bytes(B, T, F, L, nd);
    WW_REQUIRE(need && ws_bytes >= need, WW_E_INVALID, "ww_lq8_lstm_fwd: workspace of %zu bytes, need %zu", ws_bytes, need);
    WW_REQUIRE(aligned16(ws), WW_E_INVALID, "ww_lq8_lstm_fwd: the workspace must be 16-byte aligned");
    const int np = WW_LQ8_LAYER_NPTR * L;
    for (int j = 0; j < np + WW_LQ8_TAIL_NPTR; ++j) WW_REQUIRE(tab[j], WW_E_INVALID, "ww_lq8_lstm_fwd: table entry %d is null", j);
    auto i8 = [&](int i) { return (const int8_t *)tab[i]; };
    auto i32 = [&](int i) { return (const int32_t *)tab[i]; };
    const long N = (long)B * T;
    int8_t *cur = (int8_t *)ws;
    int Kp = q8_pad64(F);
    int rc = ww_tq8_quantize_bt(ctx, x, B, F, T, Kp, io->in_scale, io->in_zero, cur, stream);
    if (rc != WW_OK) return rc;
    int8_t *next = cur + q8_round256(N * Kp);
    for (int k = 0; k < L; ++k) {
        const int p = WW_LQ8_LAYER_NPTR * k;
        int16_t *u = (int16_t *)next;
        int8_t *y = next + q8_round256(N * nd * LQ_G * 2);
        int16_t *c_n = (int16_t *)(y + q8_round256(N * nd * LQ_H));
        rc = ww_lq8_proj_fwd(ctx, cur, i8(p), i32(p + 1), i32(p + 2), i32(p + 3), N, Kp, nd * LQ_G, u, stream);
        if (rc != WW_OK) return rc;
        rc = ww_lq8_lstm_layer_fwd(ctx, u, i8(p + 4), i32(p + 5), i32(p + 6), i32(p + 7), (const int16_t *)tab[np + 3],
                                   (const int16_t *)tab[np + 4], B, T, nd, y, c_n, stream);
        if (rc != WW_OK) return rc;
        cur = y;
        Kp = nd * LQ_H;
        next = (int8_t *)c_n + q8_round256((long)B * nd * LQ_H * 2);
    }
    return ww_lq8_head_fwd(ctx, cur, B, T, nd, i8(np), i32(np + 1), (const float *)tab[np + 2], io->num_classes, next, logits, stream);
}

// The int8 recurrent frame shared by ww_q8_lstm.hip and ww_q8_crnn.hip (DESIGN.md "Export", the int8 law, subsections "LSTM" and
// "GRU"): one recurrence kernel, one layer launcher, one per-layer workspace formula and one stack walk.  What differs between the
// cells is a `Cell` struct: its gate count NG (gate rows of a direction in torch's order: i, f, g, o / r, z, n) and the integer
// arithmetic of one step.
//
// The recurrence.  A workgroup owns QR_RB = 16 batch rows (the instruction's 16 columns) of one direction (blockIdx.y) for all T
// steps and walks further row groups persistently.  Its eight waves split the 128 hidden units: wave w owns units 16 w .. 16 w + 15
// and keeps the 16 NG rows of W_hh that feed them -- every gate of those units, 16 NG x 128 bytes -- in 8 NG registers for the
// whole launch, as the A operands of NG gates x 2 K chunks of v_mfma_i32_16x16x64_i8.  The B operand is q_h of the 16 batch rows,
// int8 in LDS (two buffers, so a step needs ONE barrier: a step reads one and writes the other).  Under the lane map of k_q8_pw
// (DESIGN.md mfma_i8_map) lane l, p = l & 15, g = l >> 4, ends with D rows 4 g + e, e = 0..3, of column p: with A row i = unit
// 16 w + i of gate G, the 2 NG products leave the lane with every gate of units 16 w + 4 g + e of batch row p -- the thread OWNS
// those four units, their state (the LSTM's c, the GRU's h16) lives in its registers, and no gate value crosses lanes.  u of the
// next step is loaded before the current step's products are issued.  The sigmoid and tanh tables (2 x 4096 int16, from the
// bundle) are copied to dynamic LDS once per launch (TAB_LDS) or read through the caches; both give the same bits.
//
// All adds that may wrap are unsigned; the law's refusal bounds keep every true sum inside int32.
#pragma once
#include "ww_q8_common.h"

namespace {

constexpr int QR_H = 128;                      // hidden size: the implemented size of both recurrent stacks
constexpr int QR_BLOCK = 512;                  // the recurrence: 8 waves x 16 hidden units
constexpr int QR_RB = 16;                      // batch rows a workgroup owns
constexpr int QR_HROW = QR_H + 16;             // LDS row of q_h: 144 bytes, so the 16 rows of a ds_read_b128 group spread over banks
constexpr int QR_TAB = 4096;
constexpr size_t QR_TAB_BYTES = 2 * QR_TAB * sizeof(int16_t);       // the dynamic LDS of a TAB_LDS launch

struct q8_rnn_args {
    const int16_t *u;                          // (B*T, nd*NG*128)
    const int8_t *w_hh;                        // (nd*NG*128, 128)
    const int *bias, *mult, *shift;            // (nd*NG*128) each; bias is the law's q_bh (the zero point of q_h is 0)
    const int16_t *tab_sigmoid, *tab_tanh;     // (4096) each
    int8_t *y;                                 // (B*T, nd*128)
    int16_t *s_n;                              // (B, nd*128): the final state, the entries' c_n / h_n
    int B, T, nd;
};

// Cell::step(sig, tnh, uu, v, state) -> h16: uu[G] the Q8 input pre-activation of gate G, v[G] = R(W_hh q_h + q_bh) of gate G;
// it updates the unit's state and returns the Q15 hidden value, which the frame rounds to the int8 q_h.
template <class Cell, bool TAB_LDS> __global__ __launch_bounds__(QR_BLOCK) void k_q8_rnn(q8_rnn_args a) {
    constexpr int NG = Cell::NG, GR = NG * QR_H;
    __shared__ __attribute__((aligned(16))) int8_t s_h[2][QR_RB * QR_HROW];
    extern __shared__ int16_t s_tab[];         // TAB_LDS: sigmoid, then tanh
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = lane & 15, g = lane >> 4;
    const int dir = blockIdx.y, unit0 = 16 * wv + 4 * g;
    const int16_t *sig = a.tab_sigmoid, *tnh = a.tab_tanh;
    if (TAB_LDS) {
        for (int i = tid; i < QR_TAB; i += QR_BLOCK) {
            s_tab[i] = a.tab_sigmoid[i];
            s_tab[QR_TAB + i] = a.tab_tanh[i];
        }
        sig = s_tab;
        tnh = s_tab + QR_TAB;
    }
    // the wave's 16 NG rows of W_hh as A fragments: A row i = l & 15 of the product of gate G is unit 16 wv + i of that gate
    v4i wa[NG][2], bq[NG], mq[NG], sq[NG];
#pragma unroll
    for (int G = 0; G < NG; ++G) {
        const int row = dir * GR + G * QR_H + 16 * wv;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) wa[G][kc] = *(const v4i *)(a.w_hh + (long)(row + p) * QR_H + 64 * kc + 16 * g);
        bq[G] = *(const v4i *)(a.bias + row + 4 * g);
        mq[G] = *(const v4i *)(a.mult + row + 4 * g);
        sq[G] = *(const v4i *)(a.shift + row + 4 * g);
    }
    const int groups = (a.B + QR_RB - 1) / QR_RB;
    const long ustride = (long)a.nd * GR, ystride = (long)a.nd * QR_H;
    const int t0 = dir ? a.T - 1 : 0, dt = dir ? -1 : 1;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int b = grp * QR_RB + p;
        const bool live = b < a.B;
        for (int i = tid; i < QR_RB * QR_HROW / 4; i += QR_BLOCK) ((int *)s_h[0])[i] = 0;      // q_h = 0 before the first step
        __syncthreads();                        // (and the tables are in place)
        const int16_t *ub = a.u + (long)(live ? b : 0) * a.T * ustride + dir * GR + unit0;
        int8_t *yb = a.y + (long)(live ? b : 0) * a.T * ystride + dir * QR_H + unit0;
        int st[4] = {0, 0, 0, 0};               // the state is 0 before the first step
        v2i un[NG];
#pragma unroll
        for (int G = 0; G < NG; ++G) un[G] = live ? *(const v2i *)(ub + t0 * ustride + G * QR_H) : v2i{0, 0};
        for (int s = 0; s < a.T; ++s) {
            const int t = t0 + s * dt;
            v2i uc[NG];
#pragma unroll
            for (int G = 0; G < NG; ++G) uc[G] = un[G];
            if (live && s + 1 < a.T) {
#pragma unroll
                for (int G = 0; G < NG; ++G) un[G] = *(const v2i *)(ub + (t + dt) * ustride + G * QR_H);
            }
            const int8_t *hp = s_h[s & 1] + p * QR_HROW + 16 * g;
            const v4i h0 = *(const v4i *)hp, h1 = *(const v4i *)(hp + 64);
            v4i acc[NG];
#pragma unroll
            for (int G = 0; G < NG; ++G) {
                acc[G] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[G][0], h0, v4i{0, 0, 0, 0}, 0, 0, 0);
                acc[G] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[G][1], h1, acc[G], 0, 0, 0);
            }
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                long long uu[NG], v[NG];
#pragma unroll
                for (int G = 0; G < NG; ++G) {
                    uu[G] = (e & 1) ? q8_hi16(uc[G][e >> 1]) : q8_lo16(uc[G][e >> 1]);
                    v[G] = q8_round((int)((unsigned)acc[G][e] + (unsigned)bq[G][e]), mq[G][e], sq[G][e]);
                }
                const int qh = (Cell::step(sig, tnh, uu, v, st[e]) + 128) >> 8;
                q[e] = qh < -128 ? -128 : (qh > 127 ? 127 : qh);
            }
            const int packed = q8_pack4(q[0], q[1], q[2], q[3]);
            *(int *)(s_h[(s + 1) & 1] + p * QR_HROW + unit0) = packed;
            if (live) *(int *)(yb + t * ystride) = packed;
            __syncthreads();                    // q_h[t] is whole before any wave's next product reads it
        }
        if (live) *(v2i *)(a.s_n + (long)b * ystride + dir * QR_H + unit0) = v2i{q8_pack16(st[0], st[1]), q8_pack16(st[2], st[3])};
    }
}

// ---- host side
// the recurrence of one layer, all directions in one launch: the checks, the grid, the timing class and the launch of an entry
// point `name`; fn is the entry's instantiation of k_q8_rnn, tab_lds whether it is a TAB_LDS one
int q8_rnn_layer_launch(ww_ctx *ctx, const char *name, void (*fn)(q8_rnn_args), bool tab_lds, int prof, const q8_rnn_args &a,
                        hipStream_t stream) {
    WW_REQUIRE(ctx && a.u && a.w_hh && a.bias && a.mult && a.shift && a.tab_sigmoid && a.tab_tanh && a.y && a.s_n, WW_E_INVALID,
               "%s: null argument", name);
    WW_REQUIRE(a.B >= 1 && a.T >= 1 && (long)a.B * a.T <= (1l << 31), WW_E_INVALID, "%s: B=%d T=%d", name, a.B, a.T);
    WW_REQUIRE(a.nd == 1 || a.nd == 2, WW_E_INVALID, "%s: %d directions", name, a.nd);
    WW_REQUIRE(aligned16(a.u) && aligned16(a.w_hh) && aligned16(a.bias) && aligned16(a.mult) && aligned16(a.shift) && aligned16(a.y) &&
               aligned16(a.s_n), WW_E_INVALID, "%s: tensors must be 16-byte aligned", name);
    const size_t smem = tab_lds ? QR_TAB_BYTES : 0;
    const int grid = ww_conv_grid(ctx, (const void *)fn, QR_BLOCK, smem, (a.B + QR_RB - 1) / QR_RB, 1 << 20);
    ww_prof_scope scope(ctx, prof, stream);
    hipLaunchKernelGGL(fn, dim3(grid, a.nd), dim3(QR_BLOCK), smem, stream, a);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

// a layer's region of the workspace: u int16 (N, nd*NG*128) | y int8 (N, nd*128) | final state int16 (B, nd*128), N = B*T
struct Q8RnnLayerWs {
    long u, y, s;                              // bytes, each rounded up to 256
    Q8RnnLayerWs(long B, long T, long nd, int NG)
        : u(q8_round256(B * T * nd * NG * QR_H * 2)), y(q8_round256(B * T * nd * QR_H)), s(q8_round256(B * nd * QR_H * 2)) {}
    long bytes() const { return u + y + s; }
};

typedef int (*q8_rnn_layer_fn)(ww_ctx *, const int16_t *, const int8_t *, const int32_t *, const int32_t *, const int32_t *,
                               const int16_t *, const int16_t *, int, int, int, int8_t *, int16_t *, ww_stream_t);

// L layers of NG-gate cells over cur (B*T, Kp) int8 rows: per layer the projection (ww_lq8_proj_fwd), then the recurrence (the
// model's entry point `layer`).  lt: a layer's 8 pointers [w_ih, bias, mult, shift, w_hh, bias, mult, shift], L times; tabs: the
// sigmoid and tanh tables.  On return cur is the last layer's y and ws the first byte past the last layer's region.
int q8_rnn_stack_fwd(ww_ctx *ctx, q8_rnn_layer_fn layer, int NG, const void *const *lt, const void *const *tabs, int L, int nd,
                     int B, int T, const int8_t *&cur, int Kp, int8_t *&ws, ww_stream_t stream) {
    static_assert(WW_LQ8_LAYER_NPTR == 8 && WW_CQ8_LAYER_NPTR == 8, "a layer is eight pointers in both models");
    const Q8RnnLayerWs r(B, T, nd, NG);
    for (int k = 0; k < L; ++k, lt += 8) {
        int16_t *u = (int16_t *)ws;
        int8_t *y = ws + r.u;
        int16_t *s_n = (int16_t *)(y + r.y);
        int rc = ww_lq8_proj_fwd(ctx, cur, (const int8_t *)lt[0], (const int32_t *)lt[1], (const int32_t *)lt[2], (const int32_t *)lt[3],
                                 (long)B * T, Kp, nd * NG * QR_H, u, stream);
        if (rc != WW_OK) return rc;
        rc = layer(ctx, u, (const int8_t *)lt[4], (const int32_t *)lt[5], (const int32_t *)lt[6], (const int32_t *)lt[7],
                   (const int16_t *)tabs[0], (const int16_t *)tabs[1], B, T, nd, y, s_n, stream);
        if (rc != WW_OK) return rc;
        cur = y;
        Kp = nd * QR_H;
        ws += r.bytes();
    }
    return WW_OK;
}

}  // namespace

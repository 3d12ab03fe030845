// Integer-only inference of an exported int8 CRNNWakeword bundle (DESIGN.md "Export", the int8 law, subsections "GRU" and "CRNN").
//   k_cq8_fmean : the frequency mean that joins the conv stack to the GRU stack: (B,H',W',64) int8 -> (B*W', 64) int8 rows
//   k_cq8_gru   : the recurrence of one GRU layer, both directions in one launch (gridDim.y): T dependent steps of
//                 MFMA over K = 128 -> gate arithmetic in integer C++ -> the int8 output row -> LDS -> barrier
// The conv stack is cnn_small's (ww_q8.hip: ww_q8_quantize, ww_q8_stem_fwd, ww_q8_dwpw_fwd), the input projection and the head are
// the LSTM's (ww_q8_lstm.hip: ww_lq8_proj_fwd at G = nd*384, ww_lq8_head_fwd).
//
// The recurrence has the structure of k_lq8_lstm.  A workgroup owns CQ_RB = 16 batch rows (the instruction's 16 columns) of one
// direction for all T steps and walks further row groups persistently.  Its eight waves split the 128 hidden units: wave w owns
// units 16 w .. 16 w + 15 and keeps the 48 rows of W_hh that feed them -- gates r, z, n of those units, 48 x 128 bytes -- in 24
// registers for the whole launch, as the A operands of 3 gates x 2 K chunks of v_mfma_i32_16x16x64_i8.  The B operand is q_h of
// the 16 batch rows, int8 in LDS (two buffers, so a step needs ONE barrier: a step reads one and writes the other).  Under the
// lane map of k_q8_pw (DESIGN.md mfma_i8_map) lane l, p = l & 15, g = l >> 4, ends with D rows 4 g + e, e = 0..3, of column p: with
// A row i = unit 16 w + i of gate G, the six products leave the lane with all three gates of units 16 w + 4 g + e of batch row p
// -- the thread OWNS those four hidden values, h16 (int16 range, Q15) lives in its registers, and no gate value crosses lanes.
// u of the next step is loaded before the current step's products are issued.  The sigmoid and tanh tables (2 x 4096 int16, from
// the bundle) are copied to LDS once per launch.
//
// All adds that may wrap are unsigned; the law's refusal bounds keep every true sum inside int32.  R and r v_n are 64-bit.
#include "ww_q8_common.h"

namespace {

constexpr int CQ_H = 128;                      // hidden size: the implemented size of the GRU stack
constexpr int CQ_G = 3 * CQ_H;                 // gate rows of one direction, torch's order r, z, n
constexpr int CQ_BLOCK = 512;                  // the recurrence: 8 waves x 16 hidden units
constexpr int CQ_RB = 16;                      // batch rows a workgroup owns
constexpr int CQ_HROW = CQ_H + 16;             // LDS row of q_h: 144 bytes, so the 16 rows of a ds_read_b128 group spread over banks
constexpr int CQ_TAB = 4096;
constexpr int FM_BLOCK = 256;                  // the frequency mean: 4 waves, each a tile of 16 rows per trip
constexpr int FM_WAVES = FM_BLOCK / 64;

// lane l of a wave's tile: output row 16 tile + (l & 15), channels [16 g, 16 g + 16), g = l >> 4 -- the q8 lane map
__global__ __launch_bounds__(FM_BLOCK) void k_cq8_fmean(const int8_t *__restrict__ in, int H, int W, long rows, int mult, int shift,
                                                        int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, g = lane >> 4;
    const long tiles = (rows + 15) / 16;
    for (long tile = (long)blockIdx.x * FM_WAVES + (threadIdx.x >> 6); tile < tiles; tile += (long)gridDim.x * FM_WAVES) {
        const long row = tile * 16 + p;        // row = b * W + w
        if (row >= rows) continue;
        const long b = row / W;
        const int w = (int)(row - b * W);
        const int8_t *src = in + ((b * H) * W + w) * 64 + 16 * g;
        int sum[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) sum[c] = 0;
        for (int h = 0; h < H; ++h) {
            const v4i q = *(const v4i *)(src + (long)h * W * 64);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                sum[4 * d + 0] += q8_byte<0>(q[d]) + 128;
                sum[4 * d + 1] += q8_byte<1>(q[d]) + 128;
                sum[4 * d + 2] += q8_byte<2>(q[d]) + 128;
                sum[4 * d + 3] += q8_byte<3>(q[d]) + 128;
            }
        }
        v4i o;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = q8_clamp(q8_round(sum[4 * d + r], mult, shift));
            o[d] = q8_pack4(q[0], q[1], q[2], q[3]);
        }
        *(v4i *)(out + row * 64 + 16 * g) = o;
    }
}

struct cq8_rec_args {
    const int16_t *u;                          // (B*T, nd*384)
    const int8_t *w_hh;                        // (nd*384, 128)
    const int *bias, *mult, *shift;            // (nd*384) each; bias is the law's q_bh (the zero point of q_h is 0)
    const int16_t *tab_sigmoid, *tab_tanh;     // (4096) each
    int8_t *y;                                 // (B*T, nd*128)
    int16_t *h_n;                              // (B, nd*128)
    int B, T, nd;
};

__global__ __launch_bounds__(CQ_BLOCK) void k_cq8_gru(cq8_rec_args a) {
    __shared__ __attribute__((aligned(16))) int8_t s_h[2][CQ_RB * CQ_HROW];
    __shared__ int16_t s_tab[2 * CQ_TAB];      // sigmoid, then tanh
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = lane & 15, g = lane >> 4;
    const int dir = blockIdx.y, unit0 = 16 * wv + 4 * g;
    for (int i = tid; i < CQ_TAB; i += CQ_BLOCK) {
        s_tab[i] = a.tab_sigmoid[i];
        s_tab[CQ_TAB + i] = a.tab_tanh[i];
    }
    const int16_t *sig = s_tab, *tnh = s_tab + CQ_TAB;
    // the wave's 48 rows of W_hh as A fragments: A row i = l & 15 of the product of gate G is unit 16 wv + i of that gate
    v4i wa[3][2], bq[3], mq[3], sq[3];
#pragma unroll
    for (int G = 0; G < 3; ++G) {
        const int row = dir * CQ_G + G * CQ_H + 16 * wv;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) wa[G][kc] = *(const v4i *)(a.w_hh + (long)(row + p) * CQ_H + 64 * kc + 16 * g);
        bq[G] = *(const v4i *)(a.bias + row + 4 * g);
        mq[G] = *(const v4i *)(a.mult + row + 4 * g);
        sq[G] = *(const v4i *)(a.shift + row + 4 * g);
    }
    const int groups = (a.B + CQ_RB - 1) / CQ_RB;
    const long ustride = (long)a.nd * CQ_G, ystride = (long)a.nd * CQ_H;
    const int t0 = dir ? a.T - 1 : 0, dt = dir ? -1 : 1;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int b = grp * CQ_RB + p;
        const bool live = b < a.B;
        for (int i = tid; i < CQ_RB * CQ_HROW / 4; i += CQ_BLOCK) ((int *)s_h[0])[i] = 0;      // q_h = 0 before the first step
        __syncthreads();                        // (and the tables are in place)
        const int16_t *ub = a.u + (long)(live ? b : 0) * a.T * ustride + dir * CQ_G + unit0;
        int8_t *yb = a.y + (long)(live ? b : 0) * a.T * ystride + dir * CQ_H + unit0;
        int h[4] = {0, 0, 0, 0};                // h16 = 0 before the first step
        v2i un[3];
#pragma unroll
        for (int G = 0; G < 3; ++G) un[G] = live ? *(const v2i *)(ub + t0 * ustride + G * CQ_H) : v2i{0, 0};
        for (int s = 0; s < a.T; ++s) {
            const int t = t0 + s * dt;
            v2i uc[3];
#pragma unroll
            for (int G = 0; G < 3; ++G) uc[G] = un[G];
            if (live && s + 1 < a.T) {
#pragma unroll
                for (int G = 0; G < 3; ++G) un[G] = *(const v2i *)(ub + (t + dt) * ustride + G * CQ_H);
            }
            const int8_t *hp = s_h[s & 1] + p * CQ_HROW + 16 * g;
            const v4i h0 = *(const v4i *)hp, h1 = *(const v4i *)(hp + 64);
            v4i acc[3];
#pragma unroll
            for (int G = 0; G < 3; ++G) {
                acc[G] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[G][0], h0, v4i{0, 0, 0, 0}, 0, 0, 0);
                acc[G] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[G][1], h1, acc[G], 0, 0, 0);
            }
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                long long uu[3], v[3];
#pragma unroll
                for (int G = 0; G < 3; ++G) {
                    uu[G] = (e & 1) ? q8_hi16(uc[G][e >> 1]) : q8_lo16(uc[G][e >> 1]);
                    v[G] = q8_round((int)((unsigned)acc[G][e] + (unsigned)bq[G][e]), mq[G][e], sq[G][e]);
                }
                const int gr = q8_look(sig, uu[0] + v[0]), gz = q8_look(sig, uu[1] + v[1]);
                const long long rv = (long long)((unsigned long long)gr * (unsigned long long)v[2]);      // r v_n in 64 bits
                const int gn = q8_look(tnh, uu[2] + ((rv + (1ll << 14)) >> 15));
                // the two weights sum to 2^15 and |n|, |h16| <= 32767: |h16'| <= 32767 and the sum stays below 2^30 + 2^14
                const int hn = ((32768 - gz) * gn + gz * h[e] + (1 << 14)) >> 15;
                h[e] = hn;
                const int qh = (hn + 128) >> 8;
                q[e] = qh < -128 ? -128 : (qh > 127 ? 127 : qh);
            }
            const int packed = q8_pack4(q[0], q[1], q[2], q[3]);
            *(int *)(s_h[(s + 1) & 1] + p * CQ_HROW + unit0) = packed;
            if (live) *(int *)(yb + t * ystride) = packed;
            __syncthreads();                    // q_h[t] is whole before any wave's next product reads it
        }
        if (live) *(v2i *)(a.h_n + (long)b * ystride + dir * CQ_H + unit0) = v2i{q8_pack16(h[0], h[1]), q8_pack16(h[2], h[3])};
    }
}

}  // namespace

extern "C" int ww_cq8_fmean_fwd(ww_ctx *ctx, const int8_t *in, int B, int H, int W, int mult, int shift, int8_t *out,
                                ww_stream_t stream) {
    WW_REQUIRE(ctx && in && out, WW_E_INVALID, "ww_cq8_fmean_fwd: null argument");
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= (1 << 20) && (long)B * H * W <= (1l << 40), WW_E_INVALID,
               "ww_cq8_fmean_fwd: B=%d H=%d W=%d", B, H, W);
    WW_REQUIRE(q8_mult_ok(mult, shift), WW_E_INVALID, "ww_cq8_fmean_fwd: multiplier %d / shift %d out of range",
               mult, shift);
    WW_REQUIRE(aligned16(in) && aligned16(out), WW_E_INVALID, "ww_cq8_fmean_fwd: tensors must be 16-byte aligned");
    WW_REQUIRE(in != out, WW_E_INVALID, "ww_cq8_fmean_fwd: in place");
    const long rows = (long)B * W;
    const long want = ((rows + 15) / 16 + FM_WAVES - 1) / FM_WAVES;
    const int grid = ww_conv_grid(ctx, (const void *)k_cq8_fmean, FM_BLOCK, 0, want, 1 << 20);
    ww_prof_scope prof(ctx, WW_K_GAP_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_cq8_fmean, dim3(grid), dim3(FM_BLOCK), 0, (hipStream_t)stream, in, H, W, rows, mult, shift, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_cq8_gru_layer_fwd(ww_ctx *ctx, const int16_t *u, const int8_t *w_hh, const int32_t *bias, const int32_t *mult,
                                    const int32_t *shift, const int16_t *tab_sigmoid, const int16_t *tab_tanh, int B, int T,
                                    int num_directions, int8_t *y, int16_t *h_n, ww_stream_t stream) {
    WW_REQUIRE(ctx && u && w_hh && bias && mult && shift && tab_sigmoid && tab_tanh && y && h_n, WW_E_INVALID,
               "ww_cq8_gru_layer_fwd: null argument");
    WW_REQUIRE(B >= 1 && T >= 1 && (long)B * T <= (1l << 31), WW_E_INVALID, "ww_cq8_gru_layer_fwd: B=%d T=%d", B, T);
    WW_REQUIRE(num_directions == 1 || num_directions == 2, WW_E_INVALID, "ww_cq8_gru_layer_fwd: %d directions", num_directions);
    WW_REQUIRE(aligned16(u) && aligned16(w_hh) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(y) &&
               aligned16(h_n), WW_E_INVALID, "ww_cq8_gru_layer_fwd: tensors must be 16-byte aligned");
    cq8_rec_args a{u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh, y, h_n, B, T, num_directions};
    const int groups = (B + CQ_RB - 1) / CQ_RB;
    const int grid = ww_conv_grid(ctx, (const void *)k_cq8_gru, CQ_BLOCK, 0, groups, 1 << 20);
    ww_prof_scope prof(ctx, WW_K_GRU, (hipStream_t)stream);
    hipLaunchKernelGGL(k_cq8_gru, dim3(grid, num_directions), dim3(CQ_BLOCK), 0, (hipStream_t)stream, a);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" size_t ww_cq8_crnn_workspace_bytes(int B, int F, int T, int num_layers, int num_directions) {
    if (B < 1 || F < 1 || T < 1 || num_layers < 1 || num_layers > WW_CQ8_MAX_LAYERS || num_directions < 1 || num_directions > 2)
        return 0;
    const long H = (F + 1) / 2, W = (T + 1) / 2, N = (long)B * W, nd = num_directions;
    const long layer = q8_round256(N * nd * CQ_G * 2) + q8_round256(N * nd * CQ_H) + q8_round256((long)B * nd * CQ_H * 2);
    return (size_t)(q8_round256((long)B * F * T) + WW_CQ8_NACT * q8_round256((long)B * H * W * 64) + q8_round256(N * 64) +
                    num_layers * layer + q8_round256((long)B * nd * CQ_H));
}

extern "C" int ww_cq8_crnn_fwd(ww_ctx *ctx, const void *const *tab, const ww_cq8_io *io, const float *x, int B, int F, int T,
                               void *ws, size_t ws_bytes, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && tab && io && x && ws && logits, WW_E_INVALID, "ww_cq8_crnn_fwd: null argument");
    const int L = io->num_layers, nd = io->num_directions;
    WW_REQUIRE(B >= 1 && F >= 1 && T >= 1, WW_E_INVALID, "ww_cq8_crnn_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(L >= 1 && L <= WW_CQ8_MAX_LAYERS && (nd == 1 || nd == 2), WW_E_INVALID, "ww_cq8_crnn_fwd: %d layers, %d directions", L, nd);
    const size_t need = ww_cq8_crnn_workspace_bytes(B, F, T, L, nd);
    WW_REQUIRE(need && ws_bytes >= need, WW_E_INVALID, "ww_cq8_crnn_fwd: workspace of %zu bytes, need %zu", ws_bytes, need);
    WW_REQUIRE(aligned16(ws), WW_E_INVALID, "ww_cq8_crnn_fwd: the workspace must be 16-byte aligned");
    const int np = WW_CQ8_CONV_NPTR + WW_CQ8_LAYER_NPTR * L;
    for (int j = 0; j < np + WW_CQ8_TAIL_NPTR; ++j) WW_REQUIRE(tab[j], WW_E_INVALID, "ww_cq8_crnn_fwd: table entry %d is null", j);
    auto i8 = [&](int i) { return (const int8_t *)tab[i]; };
    auto i32 = [&](int i) { return (const int32_t *)tab[i]; };
    const int H = (F + 1) / 2, W = (T + 1) / 2;
    const long N = (long)B * W, act = q8_round256((long)B * H * W * 64);
    int8_t *xq = (int8_t *)ws;
    int8_t *a0 = xq + q8_round256((long)B * F * T);
    int8_t *seq = a0 + WW_CQ8_NACT * act;
    int rc = ww_q8_quantize(ctx, x, (long)B * F * T, io->in_scale, io->in_zero, xq, stream);
    if (rc != WW_OK) return rc;
    rc = ww_q8_stem_fwd(ctx, xq, i8(0), i32(1), i32(2), i32(3), B, F, T, io->in_zero, a0, stream);
    if (rc != WW_OK) return rc;
    for (int k = 0; k < 4; ++k) {
        const int t = 4 + 8 * k;
        rc = ww_q8_dwpw_fwd(ctx, a0 + k * act, i8(t), i32(t + 1), i32(t + 2), i32(t + 3), i8(t + 4), i32(t + 5), i32(t + 6), i32(t + 7),
                            B, H, W, -128, a0 + (k + 1) * act, stream);
        if (rc != WW_OK) return rc;
    }
    rc = ww_cq8_fmean_fwd(ctx, a0 + 4 * act, B, H, W, io->fmean_mult, io->fmean_shift, seq, stream);
    if (rc != WW_OK) return rc;
    const int8_t *cur = seq;
    int Kp = 64;
    int8_t *next = seq + q8_round256(N * 64);
    for (int k = 0; k < L; ++k) {
        const int p = WW_CQ8_CONV_NPTR + WW_CQ8_LAYER_NPTR * k;
        int16_t *u = (int16_t *)next;
        int8_t *y = next + q8_round256(N * nd * CQ_G * 2);
        int16_t *h_n = (int16_t *)(y + q8_round256(N * nd * CQ_H));
        rc = ww_lq8_proj_fwd(ctx, cur, i8(p), i32(p + 1), i32(p + 2), i32(p + 3), N, Kp, nd * CQ_G, u, stream);
        if (rc != WW_OK) return rc;
        rc = ww_cq8_gru_layer_fwd(ctx, u, i8(p + 4), i32(p + 5), i32(p + 6), i32(p + 7), (const int16_t *)tab[np + 3],
                                  (const int16_t *)tab[np + 4], B, W, nd, y, h_n, stream);
        if (rc != WW_OK) return rc;
        cur = y;
        Kp = nd * CQ_H;
        next = (int8_t *)h_n + q8_round256((long)B * nd * CQ_H * 2);
    }
    return ww_lq8_head_fwd(ctx, cur, B, W, nd, i8(np), i32(np + 1), (const float *)tab[np + 2], io->num_classes, next, logits, stream);
}

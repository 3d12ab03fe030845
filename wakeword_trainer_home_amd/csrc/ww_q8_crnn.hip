// Integer-only inference of an exported int8 CRNNWakeword bundle (DESIGN.md "Export", the int8 law, subsections "GRU" and "CRNN").
//   k_cq8_fmean : the frequency mean that joins the conv stack to the GRU stack: (B,H',W',64) int8 -> (B*W', 64) int8 rows
//   k_q8_rnn<GruQ8, true> : the recurrence of one GRU layer, both directions in one launch: the shared int8 recurrent frame
//                 (ww_q8_rnn.h) around the GRU cell below, the tables in LDS
// The conv stack is cnn_small's (ww_q8.hip: ww_q8_quantize, ww_q8_stem_fwd, ww_q8_dwpw_fwd), the input projection and the head are
// the LSTM's (ww_q8_lstm.hip: ww_lq8_proj_fwd at G = nd*384, ww_lq8_head_fwd).
#include "ww_q8_rnn.h"

namespace {

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

// gates r, z, n; the state is h16 (int16 range, Q15).  R and r v_n are 64-bit.
struct GruQ8 {
    static constexpr int NG = 3;
    static __device__ __forceinline__ int step(const int16_t *sig, const int16_t *tnh, const long long (&uu)[3], const long long (&v)[3],
                                               int &h) {
        const int gr = q8_look(sig, uu[0] + v[0]), gz = q8_look(sig, uu[1] + v[1]);
        const long long rv = (long long)((unsigned long long)gr * (unsigned long long)v[2]);      // r v_n in 64 bits
        const int gn = q8_look(tnh, uu[2] + ((rv + (1ll << 14)) >> 15));
        // the two weights sum to 2^15 and |n|, |h16| <= 32767: |h16'| <= 32767 and the sum stays below 2^30 + 2^14
        h = ((32768 - gz) * gn + gz * h + (1 << 14)) >> 15;
        return h;
    }
};

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
    return q8_rnn_layer_launch(ctx, "ww_cq8_gru_layer_fwd", k_q8_rnn<GruQ8, true>, true, WW_K_GRU,
                               {u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh, y, h_n, B, T, num_directions}, (hipStream_t)stream);
}

extern "C" size_t ww_cq8_crnn_workspace_bytes(int B, int F, int T, int num_layers, int num_directions) {
    if (B < 1 || F < 1 || T < 1 || num_layers < 1 || num_layers > WW_CQ8_MAX_LAYERS || num_directions < 1 || num_directions > 2)
        return 0;
    const long H = (F + 1) / 2, W = (T + 1) / 2, N = (long)B * W, nd = num_directions;
    return (size_t)(q8_round256((long)B * F * T) + WW_CQ8_NACT * q8_round256((long)B * H * W * 64) + q8_round256(N * 64) +
                    num_layers * Q8RnnLayerWs(B, W, nd, GruQ8::NG).bytes() + q8_round256((long)B * nd * QR_H));
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
    int8_t *next = seq + q8_round256(N * 64);
    rc = q8_rnn_stack_fwd(ctx, ww_cq8_gru_layer_fwd, GruQ8::NG, tab + WW_CQ8_CONV_NPTR, tab + np + 3, L, nd, B, W, cur, 64, next, stream);
    if (rc != WW_OK) return rc;
    return ww_lq8_head_fwd(ctx, cur, B, W, nd, i8(np), i32(np + 1), (const float *)tab[np + 2], io->num_classes, next, logits, stream);
}

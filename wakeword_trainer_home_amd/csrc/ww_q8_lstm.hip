// Integer-only inference of an exported int8 LSTMWakeword bundle (DESIGN.md "Export", the int8 law, subsection "LSTM").
//   the projection : the input projection of both directions over all B*T rows: the one-segment geometry of the int8 tap-GEMM
//                 core (ww_q8_tap_gemm.h) with the epilogue LqInt16 -- effective bias, R, the int16 clamp; it stores
//                 u (B*T, nd*512) int16, Q8 gate pre-activations
//   k_q8_rnn<LstmQ8, .> : the recurrence of one layer, both directions in one launch: the shared int8 recurrent frame (ww_q8_rnn.h)
//                 around the LSTM cell below; the tables in LDS (<LstmQ8, true>, the default) or read through the caches
//                 (<LstmQ8, false>, WW_LQ8_TABLES=global in the environment: the A/B switch of tools/bench_q8_lstm.py and the tests)
//   k_lq8_head  : hcat = [forward q_h[T-1], reverse q_h[0]], Linear(nd*128, num_classes), one fp32 multiply per logit
// Quantisation is ww_tq8_quantize_bt (ww_q8_tcn.hip): (B,F,T) fp32 -> (B*T, Fp) int8 rows, Fp = F rounded up to 64, the pad
// channels holding z_x and meeting zero weights.
#include "ww_q8_tap_gemm.h"
#include "ww_q8_rnn.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int LQ_G = 4 * QR_H;                 // gate rows of one direction, torch's order i, f, g, o
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

// gates i, f, g, o; the state is c (int16 range, Q11)
struct LstmQ8 {
    static constexpr int NG = 4;
    static __device__ __forceinline__ int step(const int16_t *sig, const int16_t *tnh, const long long (&uu)[4], const long long (&v)[4],
                                               int &c) {
        long long pre[4];                          // all four sums before the first look-up: the step loop's schedule follows this order
#pragma unroll
        for (int G = 0; G < 4; ++G) pre[G] = uu[G] + v[G];
        const int gi = q8_look(sig, pre[0]), gf = q8_look(sig, pre[1]), gg = q8_look(tnh, pre[2]), go = q8_look(sig, pre[3]);
        int cn = (gf * c + ((gi * gg + 8) >> 4) + (1 << 14)) >> 15;      // |.| < 2^30 + 2^26 + 2^14: inside int32
        cn = cn < -32768 ? -32768 : (cn > 32767 ? 32767 : cn);
        c = cn;
        return (go * q8_look(tnh, (cn + 4) >> 3) + (1 << 14)) >> 15;
    }
};

// one workgroup per sample and trip: hcat, then one thread per class
__global__ __launch_bounds__(64) void k_lq8_head(const int8_t *__restrict__ y, int B, int T, int nd, const int8_t *__restrict__ fc_w,
                                                 const int *__restrict__ fc_b, const float *__restrict__ fc_scale, int nc,
                                                 int8_t *__restrict__ hcat, float *__restrict__ logits) {
    __shared__ int s_h[2 * QR_H];
    const int C = nd * QR_H, tid = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        for (int c = tid; c < C; c += 64) {
            const int t = c >= QR_H ? 0 : T - 1;                    // forward: the last step; reverse: its last step, t = 0
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
    WW_REQUIRE(G == LQ_G || G == 2 * LQ_G || G == 3 * QR_H || G == 6 * QR_H, WW_E_INVALID,
               "ww_lq8_proj_fwd: G=%d gate rows, expected %d or %d (LSTM), %d or %d (GRU)", G, LQ_G, 2 * LQ_G, 3 * QR_H, 6 * QR_H);
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
    const char *mode = getenv("WW_LQ8_TABLES");
    const bool lds = !(mode && !strcmp(mode, "global"));
    return q8_rnn_layer_launch(ctx, "ww_lq8_lstm_layer_fwd", lds ? k_q8_rnn<LstmQ8, true> : k_q8_rnn<LstmQ8, false>, lds, WW_K_LSTM,
                               {u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh, y, c_n, B, T, num_directions}, (hipStream_t)stream);
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
    const long nd = num_directions;
    return (size_t)(q8_round256((long)B * T * q8_pad64(input_size)) + num_layers * Q8RnnLayerWs(B, T, nd, LstmQ8::NG).bytes() +
                    q8_round256(B * nd * QR_H));
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
    const int Kp = q8_pad64(F);
    int8_t *xq = (int8_t *)ws, *next = xq + q8_round256((long)B * T * Kp);
    int rc = ww_tq8_quantize_bt(ctx, x, B, F, T, Kp, io->in_scale, io->in_zero, xq, stream);
    if (rc != WW_OK) return rc;
    const int8_t *cur = xq;
    rc = q8_rnn_stack_fwd(ctx, ww_lq8_lstm_layer_fwd, LstmQ8::NG, tab, tab + np + 3, L, nd, B, T, cur, Kp, next, stream);
    if (rc != WW_OK) return rc;
    return ww_lq8_head_fwd(ctx, cur, B, T, nd, (const int8_t *)tab[np], (const int32_t *)tab[np + 1], (const float *)tab[np + 2],
                           io->num_classes, next, logits, stream);
}

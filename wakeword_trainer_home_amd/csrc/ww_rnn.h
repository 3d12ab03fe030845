// The recurrent-layer frame shared by ww_gru.hip and ww_lstm.hip.  A layer is 1 or 2 directions: per direction the input
// projection of ALL time steps (one GEMM), then ONE persistent recurrent launch for all directions (gridDim.y), then (backward)
// the weight-gradient / bias / dX products per direction on the same stream.  What differs between the cells is data (RnnShape:
// gate count, saved tensors, whether dGh has its own region) plus, per cell, its kernels and kernel-argument structs (a `Cell`
// traits class: see GruCell / LstmCell).  Hidden size 128 only.
#pragma once
#include "ww_internal.h"
#include "ww_layers.h"
#include "ww_act.h"
#include <algorithm>

namespace {

// ---- device helpers of the recurrent kernels
typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int RH = 128;              // hidden size
constexpr int RBT = 16;              // batch rows of the MFMA tile
constexpr int RS_LD = RH + 4;        // fp32 LDS row stride: lane (row i, k) -> bank 4i + k, conflict-free fragment reads
constexpr int RB_LD = RH + 8;        // 16-bit row strides (16-byte aligned 8-element fragments)
// (in the 16-bit matrix modes of the recurrent kernels, ModeH<MODE>, the state, the gates and the updates stay fp32)

// 16-bit matrix modes: v_exp_f32 + v_rcp_f32 forms (1 ulp reciprocal, absolute error ~2e-7 -- far below what the 16-bit operands
// of those modes cost); the IEEE division and libm tanhf of the parity mode are ~50 of the ~80 instructions of a GRU cell, and
// the recurrence is VALU-issue-bound (2 waves per SIMD, no other work to hide behind)
template <bool FAST> __device__ __forceinline__ float gate_sigmoid(float x) {
    if constexpr (FAST) return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
    else return 1.0f / (1.0f + __expf(-x));
}
template <bool FAST> __device__ __forceinline__ float gate_tanh(float x) {
    if constexpr (FAST) return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)), 1.0f);
    else return tanhf(x);
}

// fp32 -> 16-bit copies of the input projection's two operands in ONE launch: x (M rows of I floats, row stride ldx) -> xh (M, I),
// w (Nw*I contiguous) -> wh.  I % 4 == 0; a thread moves float4s in batches of four (unconditional, clamped loads).
template <typename H>
__global__ __launch_bounds__(256) void k_to16_pair(const float *__restrict__ x, long ldx, long M, int I, const float *__restrict__ w,
                                                   long nw, H *__restrict__ xh, H *__restrict__ wh) {
    typedef Act<H> A16;
    const long I4 = I >> 2, nx4 = M * I4, n4 = nx4 + (nw >> 2);
    for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += 4L * gridDim.x * 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long i = min(i0 + (long)u * gridDim.x * 256, n4 - 1);
            const float *src = i < nx4 ? x + (i / I4) * ldx + 4 * (i % I4) : w + 4 * (i - nx4);
            v[u] = *reinterpret_cast<const float4 *>(src);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long i = i0 + (long)u * gridDim.x * 256;
            if (i < n4) {
                H *dst = i < nx4 ? xh + 4 * i : wh + 4 * (i - nx4);
                *reinterpret_cast<uint2 *>(dst) = make_uint2(A16::pack2(v[u].x, v[u].y), A16::pack2(v[u].z, v[u].w));
            }
        }
    }
}

// ---- host side
// what tells the cells apart, as data
struct RnnShape {
    int gates;                       // gate blocks of 128 columns: GRU 3 (r|z|n), LSTM 4 (i|f|g|o)
    int nsaved;                      // (B*T, 128) tensors the forward saves per step; the last one is h_{t-1} (dW_hh's operand)
    bool own_dgh;                    // the backward writes dGh to a region of its own (GRU); else one dG serves both sides (LSTM)
    const char *rows_env;            // A/B override of the rows per workgroup (rnn_rows)
    int prof;                        // timing class (ww_prof_scope)
};
// the (mode, ROWS) instantiations of a recurrent kernel template, indexed [mode][ROWS == 16]
#define WW_RNN_KERNELS(k) {{k<0, 8>, k<0, 16>}, {k<1, 8>, k<1, 16>}, {k<2, 8>, k<2, 16>}}

// per-direction host arguments; s = the recurrent states (h; h, c)
struct RnnFwdHost { const float *w_ih, *w_hh, *b_ih, *b_hh, *s0[2]; float *y, *s_n[2]; char *ws; int reverse; };
struct RnnBwdHost {
    const float *w_ih, *w_hh, *dy, *ds_n[2]; char *ws; float *dw_ih, *dw_hh, *db_ih, *db_hh, *ds0[2]; int reverse;
};

constexpr int RNN_SPLITS = 128;      // workspace bound of the weight-gradient GEMMs' K splits (rnn_bwd picks the count)
struct RnnWs { size_t gi, dgh, sav[8], part, bpart, spare, total; };     // byte offsets; bpart: float offset of the bias partials in part
RnnWs rnn_ws_layout(const RnnShape &c, long B, long T, int I) {
    RnnWs L;
    size_t o = 0;
    auto take = [&](size_t nfloat) { size_t r = o; o += (nfloat * sizeof(float) + 255) & ~(size_t)255; return r; };
    const size_t M = (size_t)B * T, G = (size_t)c.gates * RH;
    L.gi = take(M * G);             // projections, overwritten by dGi (dG) in the backward pass
    L.dgh = c.own_dgh ? take(M * G) : L.gi;
    L.spare = c.own_dgh ? M * G * sizeof(float) : 0;                 // idle in the forward pass
    for (int s = 0; s < c.nsaved; ++s) L.sav[s] = take(M * RH);
    L.bpart = (size_t)RNN_SPLITS * G * std::max(I, RH);
    L.part = take(L.bpart + (size_t)((B + 7) / 8) * 2 * G);           // (8-row workgroups: B/8 bias partials)
    L.total = o;
    return L;
}
size_t rnn_workspace_bytes(const RnnShape &c, int B, int T, int I, int H) {
    return B < 1 || T < 1 || I < 1 || H != RH ? 0 : rnn_ws_layout(c, B, T, I).total;
}

// batch rows per workgroup of the recurrent kernels: 8 while 16-row workgroups would leave more than half of the CUs idle
// (c.rows_env = 8 | 16 overrides, for A/B measurements)
int rnn_rows(const RnnShape &c, int B, int nd) {
    const int forced = ww_env_int(c.rows_env, 0);             // (read per call: the tests switch it inside one process)
    if (forced == 8 || forced == 16) return forced;
    return (long)((B + RBT - 1) / RBT) * nd <= 128 ? 8 : RBT;
}

// what every entry point checks before any launch (nd directions; d[k].ws, the parameters and the cell's own pointers filled)
int rnn_check(const char *who, const RnnShape &c, ww_ctx *ctx, int mode, const float *x, long ldx, int nd, const char *const ws[2],
              int B, int T, int I, int H, size_t ws_bytes) {
    WW_REQUIRE(ctx && x, WW_E_INVALID, "%s: null argument", who);
    WW_REQUIRE(B >= 1 && T >= 1 && I >= 1, WW_E_INVALID, "%s: bad shape B=%d T=%d I=%d", who, B, T, I);
    WW_REQUIRE(H == RH, WW_E_UNSUPPORTED, "%s: hidden size %d not implemented (128 only)", who, H);
    WW_REQUIRE(ws[0] && ws[nd - 1], WW_E_INVALID, "%s: null workspace", who);
    WW_REQUIRE(ws_bytes >= rnn_ws_layout(c, B, T, I).total, WW_E_WORKSPACE, "%s: workspace too small", who);
    WW_REQUIRE((((uintptr_t)ws[0] | (uintptr_t)ws[nd - 1]) & 255) == 0, WW_E_INVALID, "%s: workspace must be 256-byte aligned", who);
    WW_REQUIRE(nd == 1 || ws[0] != ws[1], WW_E_INVALID, "%s: the two directions need their own workspaces", who);
    WW_REQUIRE(mode == WW_ACT_F32 || mode == WW_ACT_BF16 || mode == WW_ACT_F16, WW_E_INVALID, "%s: unknown mode %d", who, mode);
    WW_REQUIRE(ldx >= I, WW_E_INVALID, "%s: x row stride smaller than the input size", who);
    return WW_OK;
}

// Gi[(b,t)][G] = x[(b,t)][:] W_ih^T + b_ih for all time steps at once.  *xh_shared: the 16-bit copy of x another direction of the
// same layer has already made (both directions project the SAME input: only the weights are converted then); set to this
// call's copy when it makes one.
template <class Cell>
int rnn_project(ww_ctx *ctx, int mode, const float *x, long ldx, const RnnFwdHost &d, const RnnWs &L, int B, int T, int I,
                hipStream_t st, const void **xh_shared) {
    constexpr int G = Cell::shape.gates * RH;
    char *w = d.ws;
    const long Mrows = (long)B * T;
    if constexpr (Cell::shape.own_dgh) {
        // 16-bit matrix modes with I a multiple of 64 (the CRNN's 64 conv channels, every second layer's 256): both operands are
        // rounded ONCE into 16-bit copies in the spare region (the dGh region is idle in the forward pass) and the product runs on
        // ww_gemm16_nt's 128 x 128 LDS-DMA tiles with b_ih added in its epilogue -- the same operand roundings as k_gemm's LDS
        // fill, 3-5x faster than its 64 x 64 tiles at these shapes.  (Without a spare region the 16-bit modes round the
        // operands in ww_gemm's staging.)
        const size_t xh_bytes = ((size_t)Mrows * I * 2 + 255) & ~(size_t)255, wh_bytes = (size_t)G * I * 2;
        static const int use_gemm16 = ww_env_int("WW_GRU_GEMM16", 1);      // A/B knob: 0 = the k_gemm path for every shape
        if (use_gemm16 && mode != WW_ACT_F32 && I % 64 == 0 && ldx % 4 == 0 && (((uintptr_t)x | (uintptr_t)d.w_ih) & 15) == 0 &&
            xh_bytes + wh_bytes <= L.spare) {
            void *xh = w + L.dgh, *wh = w + L.dgh + xh_bytes;
            const bool have_x = xh_shared && *xh_shared;
            const long rows = have_x ? 0 : Mrows;                          // rows of x this launch still has to convert
            const long n4 = rows * (I / 4) + (long)G * I / 4;
            const int grid = ww_pass_to16_pair(n4).grid;
            if (mode == WW_ACT_BF16)
                hipLaunchKernelGGL(k_to16_pair<ww_bf16>, dim3(grid), dim3(256), 0, st, x, ldx, rows, I, d.w_ih, (long)G * I, (ww_bf16 *)xh, (ww_bf16 *)wh);
            else
                hipLaunchKernelGGL(k_to16_pair<ww_f16>, dim3(grid), dim3(256), 0, st, x, ldx, rows, I, d.w_ih, (long)G * I, (ww_f16 *)xh, (ww_f16 *)wh);
            WW_LAUNCH_CHECK();
            const void *xa = have_x ? *xh_shared : xh;
            if (xh_shared && !have_x) *xh_shared = xh;
            return ww_gemm16_nt_bias(ctx, mode, xa, wh, w + L.gi, 1, Mrows, G, I, d.b_ih, st);
        }
    }
    return ww_gemm(mode, x, ldx, 1, B * T, d.w_ih, I, 1, G, I, (float *)(w + L.gi), G, d.b_ih, 0, 1, nullptr, st);
}

// Forward of a layer: d[k].y = y + k*128 (y / ldy: the (B,T,nd*128) output).  Cell::fwd_dir fills the kernel's per-direction
// arguments, Cell::fwd[mode][ROWS == 16] is the recurrent kernel.
template <class Cell>
int rnn_fwd(const char *who, ww_ctx *ctx, int mode, const float *x, long ldx, RnnFwdHost *d, int nd, int B, int T, int I, int H,
            float *y, long ldy, size_t ws_bytes, hipStream_t st) {
    const char *ws[2] = {d[0].ws, d[nd - 1].ws};
    int rc = rnn_check(who, Cell::shape, ctx, mode, x, ldx, nd, ws, B, T, I, H, ws_bytes);
    if (rc) return rc;
    WW_REQUIRE(y && ldy >= (long)nd * H, WW_E_INVALID, "%s: null y or y row stride too small", who);
    for (int k = 0; k < nd; ++k) {
        WW_REQUIRE(d[k].w_ih && d[k].w_hh && d[k].b_ih && d[k].b_hh, WW_E_INVALID, "%s: null parameter", who);
        d[k].y = y + (size_t)k * RH;
    }
    ww_prof_scope ps_(ctx, Cell::shape.prof, st);
    const RnnWs L = rnn_ws_layout(Cell::shape, B, T, I);
    const void *xh_shared = nullptr;
    for (int k = 0; k < nd; ++k)
        if ((rc = rnn_project<Cell>(ctx, mode, x, ldx, d[k], L, B, T, I, st, &xh_shared))) return rc;
    typename Cell::FwdDir a[2];
    int y_vec = ldy % 4 == 0;
    for (int k = 0; k < 2; ++k) {
        const RnnFwdHost &h = d[k < nd ? k : 0];
        a[k] = Cell::fwd_dir(h, L);
        y_vec = y_vec && (((uintptr_t)h.y & 15) == 0);
    }
    const int rows = rnn_rows(Cell::shape, B, nd);
    const size_t smem = (size_t)2 * Cell::shape.nsaved * rows * RS_LD * sizeof(float);
    const auto kern = Cell::fwd[mode][rows == 16];
    WW_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3((B + rows - 1) / rows, nd), dim3(512), smem, st, a[0], a[1], B, T, ldy, (long)T * ldy, y_vec);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

// Backward of a layer: d[k].dy = dy + k*128 (dy / ldy: the gradient of the (B,T,nd*128) output, or null); dx (+)= the input
// gradient when given.  Cell::bwd_dir fills the kernel's per-direction arguments (dGi, and dGh when it has its own region).
template <class Cell>
int rnn_bwd(const char *who, ww_ctx *ctx, int mode, const float *x, long ldx, RnnBwdHost *d, int nd, const float *dy, long ldy,
            int B, int T, int I, int H, size_t ws_bytes, float *dx, long lddx, int accumulate_dx, hipStream_t st) {
    constexpr int G = Cell::shape.gates * RH;
    const char *ws[2] = {d[0].ws, d[nd - 1].ws};
    int rc = rnn_check(who, Cell::shape, ctx, mode, x, ldx, nd, ws, B, T, I, H, ws_bytes);
    if (rc) return rc;
    WW_REQUIRE(!dy || ldy >= (long)nd * H, WW_E_INVALID, "%s: dy row stride too small", who);
    WW_REQUIRE(!dx || lddx >= I, WW_E_INVALID, "%s: dx row stride smaller than the input size", who);
    for (int k = 0; k < nd; ++k) {
        WW_REQUIRE(d[k].w_ih && d[k].w_hh && d[k].dw_ih && d[k].dw_hh && d[k].db_ih && d[k].db_hh, WW_E_INVALID,
                   "%s: null parameter / gradient pointer", who);
        WW_REQUIRE(dy || d[k].ds_n[0] || d[k].ds_n[1], WW_E_INVALID, "%s: need dy and/or a final-state gradient", who);
        d[k].dy = dy ? dy + (size_t)k * RH : nullptr;
    }
    if (!dy) ldy = (long)nd * RH;
    ww_prof_scope ps_(ctx, Cell::shape.prof, st);
    const RnnWs L = rnn_ws_layout(Cell::shape, B, T, I);
    const int rows = rnn_rows(Cell::shape, B, nd);
    const int nblk = (B + rows - 1) / rows;
    typename Cell::BwdDir a[2];
    int dy_vec = ldy % 4 == 0;
    for (int k = 0; k < 2; ++k) {
        const RnnBwdHost &h = d[k < nd ? k : 0];
        a[k] = Cell::bwd_dir(h, L, (float *)(h.ws + L.part) + L.bpart);
        dy_vec = dy_vec && (!h.dy || ((uintptr_t)h.dy & 15) == 0);
    }
    hipLaunchKernelGGL(Cell::bwd[mode][rows == 16], dim3(nblk, nd), dim3(512), 0, st, a[0], a[1], ldy, (long)T * ldy, B, T, dy_vec);
    WW_LAUNCH_CHECK();
    const int M = B * T;
    // K splits of the weight-gradient products (contraction over the B*T rows, 12-32 output tiles): as for the 1x1 convolutions
    // a split is a chain of dependent K stages, so more, shallower splits finish sooner -- bounded by the partial traffic
    // (splits x G x max(I, H) floats written and re-read): CRNN B=512 step 2.604 / 2.592 / 2.626 ms at 32 / 64 / 128
    // (profiles/r03_i_*; WW_GRU_SPLITS for measurements)
    const int splits = M >= 4096 ? std::min(RNN_SPLITS, std::max(1, ww_env_int("WW_GRU_SPLITS", 64))) : 1;
    // While the context is deferring (ww_ctx_set_deferred_reduce) the three "sum the partials" launches of a direction are
    // queued: the two weight-gradient products then keep their partials apart (dW_hh in the first, dW_ih in the second part of
    // the region sized for RNN_SPLITS splits), and the bias partials are one 2G-column item when db_ih | db_hh are adjacent
    // (nn.GRU's / nn.LSTM's parameter order, i.e. their slots of a flat gradient bucket)
    const bool defer = ctx->defer_on && splits <= RNN_SPLITS / 2;
    for (int k = 0; k < nd; ++k) {
        const RnnBwdHost &h = d[k];
        float *dgi = (float *)(h.ws + L.gi), *dgh = (float *)(h.ws + L.dgh), *part = (float *)(h.ws + L.part);
        float *part_ih = defer ? part + (size_t)splits * G * RH : part;
        const float *hp = (const float *)(h.ws + L.sav[Cell::shape.nsaved - 1]);
        // dW_hh[c][k] = sum_m dGh[m][c] h_prev[m][k]   ;   dW_ih[c][i] = sum_m dGi[m][c] x[m][i]
        // (16-bit modes: the recurrent kernel left dGi / dGh in the matrix type -- a16)
        if ((rc = ww_gemm(mode, dgh, 1, G, G, hp, 1, RH, RH, M, h.dw_hh, RH, nullptr, 0, splits, part, st, defer ? ctx : nullptr, 1))) return rc;
        if ((rc = ww_gemm(mode, dgi, 1, G, G, x, 1, ldx, I, M, h.dw_ih, I, nullptr, 0, splits, part_ih, st, defer ? ctx : nullptr, 1))) return rc;
        // db_ih | db_hh: fixed-order sum of the per-block partials the recurrent kernel left (one launch for both: 2G columns)
        if (defer && h.db_hh == h.db_ih + G) ww_defer(ctx, part + L.bpart, h.db_ih, 2 * G, nblk, 0);
        else if ((rc = ww_colsum_pair(part + L.bpart, nblk, G, h.db_ih, h.db_hh, st))) return rc;
        // dx[m][i] (+)= sum_c dGi[m][c] W_ih[c][i]   (the second direction adds to the first one's; both directions of a
        // layer: ONE product over the two (dGi, W_ih) pairs below instead)
        if (dx && nd != 2 && (rc = ww_gemm(mode, dgi, G, 1, M, h.w_ih, 1, I, I, G, dx, lddx, nullptr, accumulate_dx || k > 0, 1, nullptr, st, nullptr, 1)))
            return rc;
    }
    if (dx && nd == 2 && (rc = ww_gemm_seg2(mode, (float *)(d[0].ws + L.gi), (float *)(d[1].ws + L.gi), G, M, d[0].w_ih, d[1].w_ih, I, I,
                                            G, dx, lddx, accumulate_dx, st, 1)))
        return rc;
    return WW_OK;
}

}  // namespace

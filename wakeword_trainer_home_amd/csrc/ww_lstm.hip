// LSTM layer (one direction, or both in one launch) forward / backward -- torch.nn.LSTM's cell and parameter layout, which is
// what the reference's LSTMWakeword wraps (src/models/architectures.py: nn.LSTM(input, 128, num_layers=2, batch_first=True,
// bidirectional=True)):
//   G = x W_ih^T + b_ih + h W_hh^T + b_hh          gate order i|f|g|o
//   i = s(G_i)   f = s(G_f)   g = tanh(G_g)   o = s(G_o)      c' = f * c + i * g      h' = o * tanh(c')
// The frame is ww_gru.hip's:
//   * the input projection of ALL time steps is one GEMM  Gi = X W_ih^T + b_ih  (ww_gemm, matrix cores);
//   * the recurrence is ONE persistent kernel per layer (gridDim.y = directions): a block owns ROWS batch rows for all T steps,
//     keeps h in LDS, the cell state c in the registers of the lane that owns the cell, and every wavefront keeps ITS slice of
//     W_hh (16 hidden units x 4 gates x 128) in registers for the whole sequence;
//   * backward mirrors it (dh carried in LDS, dc in registers, W_hh slice by output unit in registers, dG W_hh per step).  One
//     pre-activation gradient dG (4H wide) serves both sides of the cell, so dW_ih = dG^T X, dW_hh = sum_t dG_t^T h_{t-1},
//     db_ih = db_hh = sum dG and dX = dG W_ih are products over a single buffer.
// Register budget (fp32 parity mode): the W_hh slice is 4 x 32 = 128 VGPRs (the GRU's 3 gates: 96).  It fits the 256 a wave of a
// 512-thread block may hold at 2 waves per SIMD without spilling once the per-step inputs are loaded one step ahead instead of
// the GRU's two; the 16-bit modes hold 4 x 4 bf16x8 = 64 and keep the two-step distance.
// Hidden size 128 only.
#include "ww_internal.h"
#include "ww_layers.h"
#include "ww_act.h"
#include <algorithm>

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int LH = 128;              // hidden size
constexpr int L4 = 4 * LH;           // gate columns
constexpr int LBT = 16;              // batch rows of the MFMA tile
constexpr int LS_LD = LH + 4;        // fp32 LDS row stride: lane (row i, k) -> bank 4i + k, conflict-free fragment reads
constexpr int LB_LD = LH + 8;        // 16-bit row strides (16-byte aligned 8-element fragments)
constexpr int DG_LD = L4 + 4;
constexpr int DGB_LD = L4 + 8;
constexpr int NSAV = 7;              // saved per step: i, f, g, o, tanh(c_t), c_{t-1}, h_{t-1}
template <int MODE> struct LModeH { typedef ww_bf16 type; };
template <> struct LModeH<2> { typedef ww_f16 type; };

// the gate functions of ww_gru.hip: exact forms in the fp32 parity mode, v_exp + v_rcp forms in the 16-bit modes
template <bool FAST> __device__ __forceinline__ float lsig(float x) {
    if constexpr (FAST) return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
    else return 1.0f / (1.0f + __expf(-x));
}
template <bool FAST> __device__ __forceinline__ float ltanh(float x) {
    if constexpr (FAST) return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)), 1.0f);
    else return tanhf(x);
}

struct LstmSaved { float *s[NSAV]; };       // (B*T, 128) each
struct LstmFwdDir { const float *gi, *w_hh, *b_hh, *h0, *c0; float *y, *hn_out, *cn_out; LstmSaved sv; int reverse; };
struct LstmBwdDir { const float *w_hh, *dy, *dhn, *dcn; LstmSaved sv; float *dg, *dh0, *dc0, *bias_part; int reverse; };
// (the kernels pick every member with its own select: a reference to one of two by-value kernel arguments would need a copy in
//  private memory)
__device__ __forceinline__ LstmSaved pick(bool second, const LstmSaved &a, const LstmSaved &b) {
    LstmSaved r;
#pragma unroll
    for (int k = 0; k < NSAV; ++k) r.s[k] = second ? b.s[k] : a.s[k];
    return r;
}

// grid (ceil(B/ROWS), directions), block 512 = 8 waves; wave w owns hidden units [16w, 16w+16) of all four gates.  ROWS = 16 (the
// MFMA tile's height) or 8 (twice the workgroups at small batches; lanes 32-63 take over result rows 2, 3 of lanes 0-31 through
// v_permlane32_swap, as in k_gru_fwd).  The saved tensors of a step are staged in LDS and written one step later as float4 along
// the unit axis; the projections are loaded two steps ahead (fp32: one).
template <int MODE, int ROWS>
__global__ __launch_bounds__(512) void k_lstm_fwd(LstmFwdDir d0, LstmFwdDir d1, int B, int T, long ldy, long bsy, int y_vec) {
    constexpr bool HALF = ROWS == 8;
    constexpr int NC = HALF ? 2 : 4;             // cells (batch rows of its unit) per lane
    constexpr bool BF16 = MODE != 0;
    typedef typename LModeH<MODE>::type H;
    typedef typename H16<H>::x8 h16x8;
    constexpr int PF = BF16 ? 2 : 1;             // steps the projections are loaded ahead (fp32: the W_hh slice leaves no room for 2)
    const bool second = blockIdx.y != 0;
    const float *__restrict__ gi = second ? d1.gi : d0.gi, *__restrict__ w_hh = second ? d1.w_hh : d0.w_hh;
    const float *__restrict__ b_hh = second ? d1.b_hh : d0.b_hh, *__restrict__ h0 = second ? d1.h0 : d0.h0;
    const float *__restrict__ c0 = second ? d1.c0 : d0.c0;
    float *__restrict__ y = second ? d1.y : d0.y, *__restrict__ hn_out = second ? d1.hn_out : d0.hn_out;
    float *__restrict__ cn_out = second ? d1.cn_out : d0.cn_out;
    const LstmSaved sv = pick(second, d0.sv, d1.sv);
    const int reverse = second ? d1.reverse : d0.reverse;
    __shared__ __align__(16) float hs[2][LBT][LS_LD];
    __shared__ __align__(16) H hb[BF16 ? 2 : 1][BF16 ? LBT : 1][LB_LD];
    extern __shared__ __align__(16) float lstm_sav[];          // [2][NSAV][ROWS][LS_LD]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 15, kq = l >> 4;
    const int b0 = blockIdx.x * ROWS, u = 16 * w + j;
    const int crow0 = HALF ? 4 * (kq & 1) + 2 * (kq >> 1) : 4 * kq;
    float wreg[BF16 ? 1 : 4][BF16 ? 1 : 32];      // fp32: W_hh[g*128 + u][4kk + kq]
    h16x8 wb[BF16 ? 4 : 1][BF16 ? 4 : 1];         // 16-bit: W_hh[g*128 + u][32kk + 8kq .. +7]
    if constexpr (BF16) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = w_hh[(size_t)(g * LH + u) * LH + 32 * kk + 8 * kq + e];
                wb[g][kk] = ww_pack8<H>(v);
            }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) wreg[g][kk] = w_hh[(size_t)(g * LH + u) * LH + 4 * kk + kq];
    }
    const float bi = b_hh[u], bf = b_hh[LH + u], bg = b_hh[2 * LH + u], bo = b_hh[3 * LH + u];
    for (int e = tid; e < LBT * LH; e += 512) {
        const int row = e >> 7, c = e & 127;
        const float hv = (h0 && row < ROWS && b0 + row < B) ? h0[(size_t)(b0 + row) * LH + c] : 0.f;
        hs[0][row][c] = hv;
        if constexpr (BF16) { hb[0][row][c] = (H)hv; hb[1][row][c] = (H)0.f; }     // (rows >= ROWS stay zero operands)
    }
    float cst[NC];                               // the cell state of this lane's cells: never leaves the lane
#pragma unroll
    for (int reg = 0; reg < NC; ++reg) {
        const int b = b0 + crow0 + reg;
        cst[reg] = (c0 && b < B) ? c0[(size_t)b * LH + u] : 0.f;
    }
    __syncthreads();
    const float *gbase[NC];                      // row (b, t = 0) of this lane's batch rows, at its unit
#pragma unroll
    for (int reg = 0; reg < NC; ++reg) gbase[reg] = gi + (size_t)min(b0 + crow0 + reg, B - 1) * T * L4 + u;
    auto load_gi = [&](int it, float (&gv)[4][NC]) {
        if (it >= T) return;
        const size_t toff = (size_t)(reverse ? T - 1 - it : it) * L4;      // wave-uniform
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) {
            const float *g4 = gbase[reg] + toff;
#pragma unroll
            for (int g = 0; g < 4; ++g) gv[g][reg] = g4[g * LH];
        }
    };
    const int frow = tid >> 5, fc0 = 4 * (tid & 31);
    const bool frow_ok = frow < ROWS && b0 + frow < B;
    const size_t fm0 = (size_t)(b0 + frow) * T * LH + fc0;
    float *const fy0 = y + (size_t)(b0 + frow) * bsy + fc0;
    const float *const fs0 = lstm_sav + frow * LS_LD + fc0;
    auto flush = [&](int it) {                  // step `it` is complete (barrier passed): its tiles -> HBM
        if (!frow_ok) return;
        const int t = reverse ? T - 1 - it : it, par = it & 1;
        const size_t m = fm0 + (size_t)t * LH;
        const float *sp = fs0 + (size_t)par * NSAV * ROWS * LS_LD;
#pragma unroll
        for (int s = 0; s < NSAV; ++s)
            *reinterpret_cast<float4 *>(sv.s[s] + m) = *reinterpret_cast<const float4 *>(sp + s * ROWS * LS_LD);
        const float4 h4 = *reinterpret_cast<const float4 *>(&hs[par ^ 1][frow][fc0]);
        float *yo = fy0 + (size_t)t * ldy;
        if (y_vec) *reinterpret_cast<float4 *>(yo) = h4;
        else { yo[0] = h4.x; yo[1] = h4.y; yo[2] = h4.z; yo[3] = h4.w; }
    };
    auto step = [&](int it, float (&sg)[4][NC]) {
        const int cur = it & 1;
        float gin[4][NC];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int reg = 0; reg < NC; ++reg) gin[g][reg] = sg[g][reg];
        load_gi(it + PF, sg);                   // the set is free again: refill it
        if (it > 0) flush(it - 1);
        floatx4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if constexpr (BF16) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const h16x8 a = *reinterpret_cast<const h16x8 *>(&hb[cur][j][32 * kk + 8 * kq]);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = H16<H>::mfma16(a, wb[g][kk], acc[g]);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) {
                const float a = hs[cur][j][4 * kk + kq];
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wreg[g][kk], acc[g], 0, 0, 0);
            }
        }
        if constexpr (HALF) {                   // lanes 32-63 take over result rows 2, 3 of lanes 0-31 (rows 8-15 are unused)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float keep = acc[g][c], give = acc[g][c + 2];     // (plain float copies: see k_gru_fwd)
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(keep), __float_as_uint(give), false, false);
                    acc[g][c] = __uint_as_float(sw[0]);
                }
        }
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) {    // D[row = crow0 + reg][unit u]
            const int row = crow0 + reg;
            const float ig = lsig<BF16>(gin[0][reg] + acc[0][reg] + bi);
            const float fg = lsig<BF16>(gin[1][reg] + acc[1][reg] + bf);
            const float gg = ltanh<BF16>(gin[2][reg] + acc[2][reg] + bg);
            const float og = lsig<BF16>(gin[3][reg] + acc[3][reg] + bo);
            const float cp = cst[reg];
            const float c = fg * cp + ig * gg;
            const float tc = ltanh<BF16>(c);
            const float h = og * tc;
            cst[reg] = c;
            const float hp = hs[cur][row][u];
            hs[cur ^ 1][row][u] = h;
            if constexpr (BF16) hb[cur ^ 1][row][u] = (H)h;
            float *sp = lstm_sav + (size_t)cur * NSAV * ROWS * LS_LD + row * LS_LD + u;
            sp[0] = ig; sp[ROWS * LS_LD] = fg; sp[2 * ROWS * LS_LD] = gg; sp[3 * ROWS * LS_LD] = og;
            sp[4 * ROWS * LS_LD] = tc; sp[5 * ROWS * LS_LD] = cp; sp[6 * ROWS * LS_LD] = hp;
        }
        __syncthreads();
    };
    {
        float sa[4][NC], sb[PF == 2 ? 4 : 1][PF == 2 ? NC : 1];
        load_gi(0, sa);
        if constexpr (PF == 2) {
            load_gi(1, sb);
            for (int it = 0; it < T; it += 2) {
                step(it, sa);
                if (it + 1 < T) step(it + 1, sb);
            }
        } else {
            for (int it = 0; it < T; ++it) step(it, sa);
        }
        flush(T - 1);
    }
    if (hn_out)
        for (int e = tid; e < ROWS * LH; e += 512) {
            const int row = e >> 7, c = e & 127;
            if (b0 + row < B) hn_out[(size_t)(b0 + row) * LH + c] = hs[T & 1][row][c];
        }
    if (cn_out)
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) {
            const int b = b0 + crow0 + reg;
            if (b < B) cn_out[(size_t)b * LH + u] = cst[reg];
        }
}

// same decomposition; wave w owns OUTPUT units [16w,16w+16) of dh_{t-1} = dG W_hh (contraction over the 512 gate rows).
// Elementwise part: thread = (batch row, 4 consecutive units), which also owns dc of those 4 cells in registers for all steps.
template <int MODE, int ROWS>
__global__ __launch_bounds__(512) void k_lstm_bwd(LstmBwdDir d0, LstmBwdDir d1, long ldy, long bsy, int B, int T, int dy_vec) {
    constexpr bool BF16 = MODE != 0;
    typedef typename LModeH<MODE>::type H;
    typedef typename H16<H>::x8 h16x8;
    constexpr int PF = BF16 ? 2 : 1;             // steps the saved gates are loaded ahead (fp32: the W_hh slice leaves no room for 2)
    const bool second = blockIdx.y != 0;
    const float *__restrict__ w_hh = second ? d1.w_hh : d0.w_hh, *__restrict__ dy = second ? d1.dy : d0.dy;
    const float *__restrict__ dhn = second ? d1.dhn : d0.dhn, *__restrict__ dcn = second ? d1.dcn : d0.dcn;
    const LstmSaved sv = pick(second, d0.sv, d1.sv);
    float *__restrict__ dgo = second ? d1.dg : d0.dg, *__restrict__ dh0 = second ? d1.dh0 : d0.dh0;
    float *__restrict__ dc0 = second ? d1.dc0 : d0.dc0, *__restrict__ bias_part = second ? d1.bias_part : d0.bias_part;
    const int reverse = second ? d1.reverse : d0.reverse;
    __shared__ __align__(16) float dhs[LBT][LS_LD];
    __shared__ __align__(16) float dg[BF16 ? 1 : LBT][DG_LD];      // fp32 operand tile
    __shared__ __align__(16) H dgb[BF16 ? LBT : 1][DGB_LD];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 15, kq = l >> 4;
    const int b0 = blockIdx.x * ROWS, u = 16 * w + j;
    float wreg[BF16 ? 1 : 128];        // fp32: W_hh[4cc + kq][u]
    h16x8 wb[BF16 ? 16 : 1];           // 16-bit: W_hh[32cc + 8kq .. +7][u]
    if constexpr (BF16) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w_hh[(size_t)(32 * cc + 8 * kq + e) * LH + u];
            wb[cc] = ww_pack8<H>(v);
        }
    } else {
#pragma unroll
        for (int cc = 0; cc < 128; ++cc) wreg[cc] = w_hh[(size_t)(4 * cc + kq) * LH + u];
    }
    for (int e = tid; e < LBT * LH; e += 512) {
        const int row = e >> 7, c = e & 127;
        dhs[row][c] = (dhn && row < ROWS && b0 + row < B) ? dhn[(size_t)(b0 + row) * LH + c] : 0.f;
    }
    if constexpr (ROWS < LBT) {                     // operand rows nobody writes stay zero (their result rows are never read)
        for (int e = tid; e < (LBT - ROWS) * L4; e += 512) {
            const int row = ROWS + e / L4, c = e % L4;
            if constexpr (BF16) dgb[row][c] = (H)0.f; else dg[row][c] = 0.f;
        }
    }
    const int erow = tid >> 5, ec0 = 4 * (tid & 31);
    const int eb = min(b0 + erow, B - 1);
    const bool erow_ok = b0 + erow < B;
    const bool ewave = erow < ROWS;                 // wave-uniform (two rows per wave)
    float dc[4] = {0.f, 0.f, 0.f, 0.f};
    if (dcn && ewave && erow_ok) {
        const float4 v = *reinterpret_cast<const float4 *>(dcn + (size_t)eb * LH + ec0);
        dc[0] = v.x; dc[1] = v.y; dc[2] = v.z; dc[3] = v.w;
    }
    __syncthreads();
    const size_t em0 = (size_t)eb * T * LH + ec0;
    const float *const edy0 = dy ? dy + (size_t)eb * bsy + ec0 : nullptr;
    struct Saved { float4 v[NSAV - 1]; float4 dy; };        // i, f, g, o, tanh(c_t), c_{t-1} (h_{t-1} is for dW_hh only)
    auto prefetch = [&](int it, Saved &S) {
        if (it >= T || !ewave) return;
        const int t = reverse ? it : T - 1 - it;        // the forward pass's time order, backwards
        const size_t i = em0 + (size_t)t * LH;
#pragma unroll
        for (int s = 0; s < NSAV - 1; ++s) S.v[s] = *reinterpret_cast<const float4 *>(sv.s[s] + i);
        if (edy0) {
            const float *p = edy0 + (size_t)t * ldy;
            S.dy = dy_vec ? *reinterpret_cast<const float4 *>(p) : make_float4(p[0], p[1], p[2], p[3]);
        } else {
            S.dy = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float bsum[4][4] = {};
    auto step = [&](int it, Saved &S) {
        const int t = reverse ? it : T - 1 - it;
        if (ewave) {
            float sv[NSAV - 1][4], pdy[4];
#pragma unroll
            for (int s = 0; s < NSAV - 1; ++s) { sv[s][0] = S.v[s].x; sv[s][1] = S.v[s].y; sv[s][2] = S.v[s].z; sv[s][3] = S.v[s].w; }
            pdy[0] = S.dy.x; pdy[1] = S.dy.y; pdy[2] = S.dy.z; pdy[3] = S.dy.w;
            prefetch(it + PF, S);                       // the set is free again
            const float4 dh4 = *reinterpret_cast<const float4 *>(&dhs[erow][ec0]);
            const float dhv[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
            float q4[4][4];                             // dG of the four gates
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float dh = erow_ok ? dhv[q] + pdy[q] : 0.f;
                const float ig = sv[0][q], fg = sv[1][q], gg = sv[2][q], og = sv[3][q], tc = sv[4][q], cp = sv[5][q];
                const float dct = erow_ok ? dc[q] + dh * og * (1.0f - tc * tc) : 0.f;
                q4[0][q] = dct * gg * ig * (1.0f - ig);
                q4[1][q] = dct * cp * fg * (1.0f - fg);
                q4[2][q] = dct * ig * (1.0f - gg * gg);
                q4[3][q] = dh * tc * og * (1.0f - og);
                dc[q] = dct * fg;
#pragma unroll
                for (int g = 0; g < 4; ++g) bsum[g][q] += q4[g][q];
            }
            const size_t m4 = ((size_t)(b0 + erow) * T + t) * L4 + ec0;
            if constexpr (BF16) {
                // dG leaves in the matrix type: the weight-gradient and dX products round their operands to it while staging
                // them anyway (ww_gemm, a16), so the results are the same and those products read half the bytes
                typedef Act<H> A16;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint2 pk = make_uint2(A16::pack2(q4[g][0], q4[g][1]), A16::pack2(q4[g][2], q4[g][3]));
                    if (erow_ok) *reinterpret_cast<uint2 *>(reinterpret_cast<H *>(dgo) + m4 + g * LH) = pk;
                    *reinterpret_cast<uint2 *>(&dgb[erow][g * LH + ec0]) = pk;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v = make_float4(q4[g][0], q4[g][1], q4[g][2], q4[g][3]);
                    if (erow_ok) *reinterpret_cast<float4 *>(dgo + m4 + g * LH) = v;
                    *reinterpret_cast<float4 *>(&dg[erow][g * LH + ec0]) = v;
                }
            }
        }
        __syncthreads();
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BF16) {
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                acc = H16<H>::mfma16(*reinterpret_cast<const h16x8 *>(&dgb[j][32 * cc + 8 * kq]), wb[cc], acc);
        } else {
#pragma unroll
            for (int cc = 0; cc < 128; ++cc)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dg[j][4 * cc + kq], wreg[cc], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) dhs[4 * kq + reg][u] = acc[reg];
        __syncthreads();
    };
    {
        Saved A, Bs;
        prefetch(0, A);
        if constexpr (PF == 2) {
            prefetch(1, Bs);
            for (int it = 0; it < T; it += 2) {
                step(it, A);
                if (it + 1 < T) step(it + 1, Bs);
            }
        } else {
            for (int it = 0; it < T; ++it) step(it, A);
        }
    }
    if (dh0)
        for (int e = tid; e < ROWS * LH; e += 512) {
            const int row = e >> 7, c = e & 127;
            if (b0 + row < B) dh0[(size_t)(b0 + row) * LH + c] = dhs[row][c];
        }
    if (dc0 && ewave && erow_ok)
        *reinterpret_cast<float4 *>(dc0 + (size_t)(b0 + erow) * LH + ec0) = make_float4(dc[0], dc[1], dc[2], dc[3]);
    // bias gradients: this block's column sums over its rows and all time steps -> bias_part[block][db_ih(512) | db_hh(512)]
    // (both halves the same sums: nn.LSTM's two biases receive the same gradient; rows added in a fixed order)
    {
        float *o = bias_part + (size_t)blockIdx.x * (2 * L4);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            __syncthreads();
            if (ewave) *reinterpret_cast<float4 *>(&dhs[erow][ec0]) = make_float4(bsum[g][0], bsum[g][1], bsum[g][2], bsum[g][3]);
            __syncthreads();
            if (tid < LH) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) s += dhs[r][tid];
                o[g * LH + tid] = s;
                o[L4 + g * LH + tid] = s;
            }
        }
    }
}

struct LWs { size_t gi, sav[NSAV], part, total; };
constexpr int LSTM_SPLITS = 128;         // workspace bound of the weight-gradient GEMMs' K splits
LWs lws_layout(long B, long T, int I) {
    LWs L;
    size_t o = 0;
    auto take = [&](size_t nfloat) { size_t r = o; o += (nfloat * sizeof(float) + 255) & ~(size_t)255; return r; };
    const size_t M = (size_t)B * T;
    L.gi = take(M * L4);            // projections, overwritten by dG in the backward pass
    for (int s = 0; s < NSAV; ++s) L.sav[s] = take(M * LH);
    L.part = take((size_t)LSTM_SPLITS * L4 * std::max(I, LH) + (size_t)((B + 7) / 8) * 2 * L4);   // (8-row workgroups: B/8 bias partials)
    L.total = o;
    return L;
}
int check_lstm(const char *who, ww_ctx *ctx, int B, int T, int I, int H, const void *ws, size_t ws_bytes) {
    WW_REQUIRE(ctx && ws, WW_E_INVALID, "%s: null argument", who);
    WW_REQUIRE(B >= 1 && T >= 1 && I >= 1, WW_E_INVALID, "%s: bad shape B=%d T=%d I=%d", who, B, T, I);
    WW_REQUIRE(H == LH, WW_E_UNSUPPORTED, "%s: hidden size %d not implemented (128 only)", who, H);
    WW_REQUIRE(ws_bytes >= lws_layout(B, T, I).total, WW_E_WORKSPACE, "%s: workspace too small", who);
    WW_REQUIRE(((uintptr_t)ws & 255) == 0, WW_E_INVALID, "%s: workspace must be 256-byte aligned", who);
    return WW_OK;
}
LstmSaved lsaved(char *w, const LWs &L) {
    LstmSaved s;
    for (int k = 0; k < NSAV; ++k) s.s[k] = (float *)(w + L.sav[k]);
    return s;
}
// batch rows per workgroup: 8 while 16-row workgroups would leave more than half of the CUs idle (WW_LSTM_ROWS = 8 | 16 overrides)
int lstm_rows(int B, int nd) {
    const int forced = ww_env_int("WW_LSTM_ROWS", 0);         // (read per call: the tests switch it inside one process)
    if (forced == 8 || forced == 16) return forced;
    return (long)((B + LBT - 1) / LBT) * nd <= 128 ? 8 : LBT;
}
struct LFwdHost { const float *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0; float *y, *h_n, *c_n; char *ws; int reverse; };
struct LBwdHost {
    const float *w_ih, *w_hh, *dy, *dh_n, *dc_n; char *ws; float *dw_ih, *dw_hh, *db_ih, *db_hh, *dh0, *dc0; int reverse;
};

int lstm_layer_fwd(int mode, const float *x, long ldx, const LFwdHost *d, int nd, int B, int T, int I, long ldy, hipStream_t st) {
    const LWs L = lws_layout(B, T, I);
    int rc;
    // Gi[(b,t)][4H] = x[(b,t)][:] W_ih^T + b_ih for all time steps at once (16-bit modes: operands rounded in the staging)
    for (int k = 0; k < nd; ++k)
        if ((rc = ww_gemm(mode, x, ldx, 1, B * T, d[k].w_ih, I, 1, L4, I, (float *)(d[k].ws + L.gi), L4, d[k].b_ih, 0, 1, nullptr, st)))
            return rc;
    LstmFwdDir a[2];
    int y_vec = ldy % 4 == 0;
    for (int k = 0; k < 2; ++k) {
        const LFwdHost &h = d[k < nd ? k : 0];
        a[k] = LstmFwdDir{(const float *)(h.ws + L.gi), h.w_hh, h.b_hh, h.h0, h.c0, h.y, h.h_n, h.c_n, lsaved(h.ws, L), h.reverse};
        y_vec = y_vec && (((uintptr_t)h.y & 15) == 0);
    }
    const int rows = lstm_rows(B, nd);
    const size_t smem = (size_t)2 * NSAV * rows * LS_LD * sizeof(float);
    auto go = [&](auto kern) -> int {
        WW_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        hipLaunchKernelGGL(kern, dim3((B + rows - 1) / rows, nd), dim3(512), smem, st, a[0], a[1], B, T, ldy, (long)T * ldy, y_vec);
        return WW_OK;
    };
    if (rows == 8) rc = mode == WW_ACT_BF16 ? go(k_lstm_fwd<1, 8>) : mode == WW_ACT_F16 ? go(k_lstm_fwd<2, 8>) : go(k_lstm_fwd<0, 8>);
    else rc = mode == WW_ACT_BF16 ? go(k_lstm_fwd<1, 16>) : mode == WW_ACT_F16 ? go(k_lstm_fwd<2, 16>) : go(k_lstm_fwd<0, 16>);
    if (rc) return rc;
    WW_LAUNCH_CHECK();
    return WW_OK;
}

int lstm_layer_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const LBwdHost *d, int nd, long ldy, int B, int T, int I,
                   float *dx, long lddx, int accumulate_dx, hipStream_t st) {
    const LWs L = lws_layout(B, T, I);
    const int rows = lstm_rows(B, nd);
    const int nblk = (B + rows - 1) / rows;
    const size_t bpart_off = (size_t)LSTM_SPLITS * L4 * std::max(I, LH);
    LstmBwdDir a[2];
    int dy_vec = ldy % 4 == 0;
    for (int k = 0; k < 2; ++k) {
        const LBwdHost &h = d[k < nd ? k : 0];
        a[k] = LstmBwdDir{h.w_hh, h.dy, h.dh_n, h.dc_n, lsaved(h.ws, L), (float *)(h.ws + L.gi), h.dh0, h.dc0,
                          (float *)(h.ws + L.part) + bpart_off, h.reverse};
        dy_vec = dy_vec && (!h.dy || ((uintptr_t)h.dy & 15) == 0);
    }
    const dim3 grid(nblk, nd);
#define WW_LSTM_BWD(M_, R_) hipLaunchKernelGGL((k_lstm_bwd<M_, R_>), grid, dim3(512), 0, st, a[0], a[1], ldy, (long)T * ldy, B, T, dy_vec)
    if (rows == 8) { if (mode == WW_ACT_BF16) WW_LSTM_BWD(1, 8); else if (mode == WW_ACT_F16) WW_LSTM_BWD(2, 8); else WW_LSTM_BWD(0, 8); }
    else { if (mode == WW_ACT_BF16) WW_LSTM_BWD(1, 16); else if (mode == WW_ACT_F16) WW_LSTM_BWD(2, 16); else WW_LSTM_BWD(0, 16); }
#undef WW_LSTM_BWD
    WW_LAUNCH_CHECK();
    const int M = B * T;
    // K splits of the weight-gradient products (contraction over the B*T rows), the GRU's choice (ww_gru.hip)
    const int splits = M >= 4096 ? std::min(LSTM_SPLITS, std::max(1, ww_env_int("WW_GRU_SPLITS", 64))) : 1;
    int rc;
    // deferring (ww_ctx_set_deferred_reduce): the dW_hh / dW_ih partials in the two parts of the region sized for LSTM_SPLITS
    // splits, and ONE 1024-column bias item when db_ih | db_hh are adjacent (nn.LSTM's parameter order)
    const bool defer = ctx && ctx->defer_on && splits <= LSTM_SPLITS / 2;
    for (int k = 0; k < nd; ++k) {
        const LBwdHost &h = d[k];
        float *dgp = (float *)(h.ws + L.gi), *part = (float *)(h.ws + L.part);
        float *part_ih = defer ? part + (size_t)splits * L4 * LH : part;
        const LstmSaved sv = lsaved(h.ws, L);
        // dW_hh[c][k] = sum_m dG[m][c] h_prev[m][k]   ;   dW_ih[c][i] = sum_m dG[m][c] x[m][i]   (16-bit modes: dG is a16)
        if ((rc = ww_gemm(mode, dgp, 1, L4, L4, sv.s[NSAV - 1], 1, LH, LH, M, h.dw_hh, LH, nullptr, 0, splits, part, st, defer ? ctx : nullptr, 1)))
            return rc;
        if ((rc = ww_gemm(mode, dgp, 1, L4, L4, x, 1, ldx, I, M, h.dw_ih, I, nullptr, 0, splits, part_ih, st, defer ? ctx : nullptr, 1)))
            return rc;
        if (defer && h.db_hh == h.db_ih + L4) ww_defer(ctx, part + bpart_off, h.db_ih, 2 * L4, nblk, 0);
        else if ((rc = ww_colsum_pair(part + bpart_off, nblk, L4, h.db_ih, h.db_hh, st))) return rc;
        // dx[m][i] (+)= sum_c dG[m][c] W_ih[c][i]  (both directions of a layer: ONE product over the two (dG, W_ih) pairs below)
        if (dx && nd != 2 && (rc = ww_gemm(mode, dgp, L4, 1, M, h.w_ih, 1, I, I, L4, dx, lddx, nullptr, accumulate_dx || k > 0, 1, nullptr, st, nullptr, 1)))
            return rc;
    }
    if (dx && nd == 2 && (rc = ww_gemm_seg2(mode, (float *)(d[0].ws + L.gi), (float *)(d[1].ws + L.gi), L4, M, d[0].w_ih, d[1].w_ih, I, I,
                                            L4, dx, lddx, accumulate_dx, st, 1)))
        return rc;
    return WW_OK;
}

#define WW_LSTM_MODE_OK(who) \
    WW_REQUIRE(mode == WW_ACT_F32 || mode == WW_ACT_BF16 || mode == WW_ACT_F16, WW_E_INVALID, who ": unknown mode %d", mode)
}  // namespace

extern "C" size_t ww_lstm_workspace_bytes(int B, int T, int I, int H) {
    if (B < 1 || T < 1 || I < 1 || H != LH) return 0;
    return lws_layout(B, T, I).total;
}

extern "C" int ww_lstm_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *b_ih,
                           const float *b_hh, const float *h0, const float *c0, int B, int T, int I, int H, int reverse, float *y,
                           long ldy, float *h_n, float *c_n, void *ws, size_t ws_bytes, ww_stream_t stream) {
    int rc = check_lstm("ww_lstm_fwd", ctx, B, T, I, H, ws, ws_bytes);
    if (rc) return rc;
    WW_LSTM_MODE_OK("ww_lstm_fwd");
    WW_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && y, WW_E_INVALID, "ww_lstm_fwd: null argument");
    WW_REQUIRE(ldx >= I && ldy >= H, WW_E_INVALID, "ww_lstm_fwd: row strides smaller than the feature sizes");
    ww_prof_scope ps_(ctx, WW_K_LSTM, (hipStream_t)stream);
    const LFwdHost d{w_ih, w_hh, b_ih, b_hh, h0, c0, y, h_n, c_n, (char *)ws, reverse};
    return lstm_layer_fwd(mode, x, ldx, &d, 1, B, T, I, ldy, (hipStream_t)stream);
}

extern "C" int ww_lstm_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *dy,
                           long ldy, const float *dh_n, const float *dc_n, int B, int T, int I, int H, int reverse, void *ws,
                           size_t ws_bytes, float *dx, long lddx, int accumulate_dx, float *dw_ih, float *dw_hh, float *db_ih,
                           float *db_hh, float *dh0, float *dc0, ww_stream_t stream) {
    int rc = check_lstm("ww_lstm_bwd", ctx, B, T, I, H, ws, ws_bytes);
    if (rc) return rc;
    WW_LSTM_MODE_OK("ww_lstm_bwd");
    WW_REQUIRE(x && w_ih && w_hh && dw_ih && dw_hh && db_ih && db_hh, WW_E_INVALID, "ww_lstm_bwd: null argument");
    WW_REQUIRE(dy || dh_n || dc_n, WW_E_INVALID, "ww_lstm_bwd: need dy, dh_n and/or dc_n");
    WW_REQUIRE(!dy || ldy >= H, WW_E_INVALID, "ww_lstm_bwd: dy row stride smaller than H");
    WW_REQUIRE(!dx || lddx >= I, WW_E_INVALID, "ww_lstm_bwd: dx row stride smaller than the input size");
    ww_prof_scope ps_(ctx, WW_K_LSTM, (hipStream_t)stream);
    const LBwdHost d{w_ih, w_hh, dy, dh_n, dc_n, (char *)ws, dw_ih, dw_hh, db_ih, db_hh, dh0, dc0, reverse};
    return lstm_layer_bwd(ctx, mode, x, ldx, &d, 1, dy ? ldy : H, B, T, I, dx, lddx, accumulate_dx, (hipStream_t)stream);
}

// Both directions of a bidirectional layer: dir[0] runs t = 0..T-1, dir[1] t = T-1..0; y / dy are (B,T,2H) buffers (row stride
// ldy >= 2H) whose column halves belong to the two directions; ONE recurrent launch (gridDim.y = 2) per pass.
extern "C" int ww_lstm_bidir_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_lstm_dir *dir, int B, int T, int I, int H,
                                 float *y, long ldy, size_t ws_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && dir, WW_E_INVALID, "ww_lstm_bidir_fwd: null argument");
    WW_LSTM_MODE_OK("ww_lstm_bidir_fwd");
    WW_REQUIRE(x && y && ldx >= I && ldy >= 2 * H, WW_E_INVALID, "ww_lstm_bidir_fwd: null x / y or row strides too small");
    LFwdHost d[2];
    for (int k = 0; k < 2; ++k) {
        int rc = check_lstm("ww_lstm_bidir_fwd", ctx, B, T, I, H, dir[k].ws, ws_bytes);
        if (rc) return rc;
        WW_REQUIRE(dir[k].w_ih && dir[k].w_hh && dir[k].b_ih && dir[k].b_hh, WW_E_INVALID, "ww_lstm_bidir_fwd: null parameter");
        d[k] = LFwdHost{dir[k].w_ih, dir[k].w_hh, dir[k].b_ih, dir[k].b_hh, dir[k].h0, dir[k].c0, y + (size_t)k * LH, dir[k].h_n,
                        dir[k].c_n, (char *)dir[k].ws, k};
    }
    WW_REQUIRE(d[0].ws != d[1].ws, WW_E_INVALID, "ww_lstm_bidir_fwd: the two directions need their own workspaces");
    ww_prof_scope ps_(ctx, WW_K_LSTM, (hipStream_t)stream);
    return lstm_layer_fwd(mode, x, ldx, d, 2, B, T, I, ldy, (hipStream_t)stream);
}

extern "C" int ww_lstm_bidir_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_lstm_dir *dir, const float *dy, long ldy,
                                 int B, int T, int I, int H, size_t ws_bytes, float *dx, long lddx, ww_stream_t stream) {
    WW_REQUIRE(ctx && dir && x, WW_E_INVALID, "ww_lstm_bidir_bwd: null argument");
    WW_LSTM_MODE_OK("ww_lstm_bidir_bwd");
    WW_REQUIRE(!dy || ldy >= 2 * H, WW_E_INVALID, "ww_lstm_bidir_bwd: dy row stride smaller than 2H");
    WW_REQUIRE(!dx || lddx >= I, WW_E_INVALID, "ww_lstm_bidir_bwd: dx row stride smaller than the input size");
    LBwdHost d[2];
    for (int k = 0; k < 2; ++k) {
        int rc = check_lstm("ww_lstm_bidir_bwd", ctx, B, T, I, H, dir[k].ws, ws_bytes);
        if (rc) return rc;
        WW_REQUIRE(dir[k].w_ih && dir[k].w_hh && dir[k].dw_ih && dir[k].dw_hh && dir[k].db_ih && dir[k].db_hh, WW_E_INVALID,
                   "ww_lstm_bidir_bwd: null parameter / gradient pointer");
        WW_REQUIRE(dy || dir[k].dh_n || dir[k].dc_n, WW_E_INVALID, "ww_lstm_bidir_bwd: need dy, dh_n and/or dc_n");
        d[k] = LBwdHost{dir[k].w_ih, dir[k].w_hh, dy ? dy + (size_t)k * LH : nullptr, dir[k].dh_n, dir[k].dc_n, (char *)dir[k].ws,
                        dir[k].dw_ih, dir[k].dw_hh, dir[k].db_ih, dir[k].db_hh, dir[k].dh0, dir[k].dc0, k};
    }
    WW_REQUIRE(d[0].ws != d[1].ws, WW_E_INVALID, "ww_lstm_bidir_bwd: the two directions need their own workspaces");
    ww_prof_scope ps_(ctx, WW_K_LSTM, (hipStream_t)stream);
    return lstm_layer_bwd(ctx, mode, x, ldx, d, 2, dy ? ldy : 2 * LH, B, T, I, dx, lddx, 0, (hipStream_t)stream);
}

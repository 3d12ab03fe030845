// LSTM layer (one direction, or both in one launch) forward / backward -- torch.nn.LSTM's cell and parameter layout, which is
// what the reference's LSTMWakeword wraps (src/models/architectures.py: nn.LSTM(input, 128, num_layers=2, batch_first=True,
// bidirectional=True)):
//   G = x W_ih^T + b_ih + h W_hh^T + b_hh          gate order i|f|g|o
//   i = s(G_i)   f = s(G_f)   g = tanh(G_g)   o = s(G_o)      c' = f * c + i * g      h' = o * tanh(c')
// The layer frame is ww_rnn.h's, shared with ww_gru.hip:
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
#include "ww_rnn.h"

namespace {

constexpr int L4 = 4 * RH;           // gate columns
constexpr int DG_LD = L4 + 4;        // LDS row strides of the dG operand tile: fp32, 16-bit
constexpr int DGB_LD = L4 + 8;
constexpr int NSAV = 7;              // saved per step: i, f, g, o, tanh(c_t), c_{t-1}, h_{t-1}

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
    typedef typename ModeH<MODE>::type H;
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
    __shared__ __align__(16) float hs[2][RBT][RS_LD];
    __shared__ __align__(16) H hb[BF16 ? 2 : 1][BF16 ? RBT : 1][RB_LD];
    extern __shared__ __align__(16) float lstm_sav[];          // [2][NSAV][ROWS][RS_LD]
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
                for (int e = 0; e < 8; ++e) v[e] = w_hh[(size_t)(g * RH + u) * RH + 32 * kk + 8 * kq + e];
                wb[g][kk] = ww_pack8<H>(v);
            }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) wreg[g][kk] = w_hh[(size_t)(g * RH + u) * RH + 4 * kk + kq];
    }
    const float bi = b_hh[u], bf = b_hh[RH + u], bg = b_hh[2 * RH + u], bo = b_hh[3 * RH + u];
    for (int e = tid; e < RBT * RH; e += 512) {
        const int row = e >> 7, c = e & 127;
        const float hv = (h0 && row < ROWS && b0 + row < B) ? h0[(size_t)(b0 + row) * RH + c] : 0.f;
        hs[0][row][c] = hv;
        if constexpr (BF16) { hb[0][row][c] = (H)hv; hb[1][row][c] = (H)0.f; }     // (rows >= ROWS stay zero operands)
    }
    float cst[NC];                               // the cell state of this lane's cells: never leaves the lane
#pragma unroll
    for (int reg = 0; reg < NC; ++reg) {
        const int b = b0 + crow0 + reg;
        cst[reg] = (c0 && b < B) ? c0[(size_t)b * RH + u] : 0.f;
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
            for (int g = 0; g < 4; ++g) gv[g][reg] = g4[g * RH];
        }
    };
    const int frow = tid >> 5, fc0 = 4 * (tid & 31);
    const bool frow_ok = frow < ROWS && b0 + frow < B;
    const size_t fm0 = (size_t)(b0 + frow) * T * RH + fc0;
    float *const fy0 = y + (size_t)(b0 + frow) * bsy + fc0;
    const float *const fs0 = lstm_sav + frow * RS_LD + fc0;
    auto flush = [&](int it) {                  // step `it` is complete (barrier passed): its tiles -> HBM
        if (!frow_ok) return;
        const int t = reverse ? T - 1 - it : it, par = it & 1;
        const size_t m = fm0 + (size_t)t * RH;
        const float *sp = fs0 + (size_t)par * NSAV * ROWS * RS_LD;
#pragma unroll
        for (int s = 0; s < NSAV; ++s)
            *reinterpret_cast<float4 *>(sv.s[s] + m) = *reinterpret_cast<const float4 *>(sp + s * ROWS * RS_LD);
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
            const float ig = gate_sigmoid<BF16>(gin[0][reg] + acc[0][reg] + bi);
            const float fg = gate_sigmoid<BF16>(gin[1][reg] + acc[1][reg] + bf);
            const float gg = gate_tanh<BF16>(gin[2][reg] + acc[2][reg] + bg);
            const float og = gate_sigmoid<BF16>(gin[3][reg] + acc[3][reg] + bo);
            const float cp = cst[reg];
            const float c = fg * cp + ig * gg;
            const float tc = gate_tanh<BF16>(c);
            const float h = og * tc;
            cst[reg] = c;
            const float hp = hs[cur][row][u];
            hs[cur ^ 1][row][u] = h;
            if constexpr (BF16) hb[cur ^ 1][row][u] = (H)h;
            float *sp = lstm_sav + (size_t)cur * NSAV * ROWS * RS_LD + row * RS_LD + u;
            sp[0] = ig; sp[ROWS * RS_LD] = fg; sp[2 * ROWS * RS_LD] = gg; sp[3 * ROWS * RS_LD] = og;
            sp[4 * ROWS * RS_LD] = tc; sp[5 * ROWS * RS_LD] = cp; sp[6 * ROWS * RS_LD] = hp;
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
        for (int e = tid; e < ROWS * RH; e += 512) {
            const int row = e >> 7, c = e & 127;
            if (b0 + row < B) hn_out[(size_t)(b0 + row) * RH + c] = hs[T & 1][row][c];
        }
    if (cn_out)
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) {
            const int b = b0 + crow0 + reg;
            if (b < B) cn_out[(size_t)b * RH + u] = cst[reg];
        }
}

// same decomposition; wave w owns OUTPUT units [16w,16w+16) of dh_{t-1} = dG W_hh (contraction over the 512 gate rows).
// Elementwise part: thread = (batch row, 4 consecutive units), which also owns dc of those 4 cells in registers for all steps.
template <int MODE, int ROWS>
__global__ __launch_bounds__(512) void k_lstm_bwd(LstmBwdDir d0, LstmBwdDir d1, long ldy, long bsy, int B, int T, int dy_vec) {
    constexpr bool BF16 = MODE != 0;
    typedef typename ModeH<MODE>::type H;
    typedef typename H16<H>::x8 h16x8;
    constexpr int PF = BF16 ? 2 : 1;             // steps the saved gates are loaded ahead (fp32: the W_hh slice leaves no room for 2)
    const bool second = blockIdx.y != 0;
    const float *__restrict__ w_hh = second ? d1.w_hh : d0.w_hh, *__restrict__ dy = second ? d1.dy : d0.dy;
    const float *__restrict__ dhn = second ? d1.dhn : d0.dhn, *__restrict__ dcn = second ? d1.dcn : d0.dcn;
    const LstmSaved sv = pick(second, d0.sv, d1.sv);
    float *__restrict__ dgo = second ? d1.dg : d0.dg, *__restrict__ dh0 = second ? d1.dh0 : d0.dh0;
    float *__restrict__ dc0 = second ? d1.dc0 : d0.dc0, *__restrict__ bias_part = second ? d1.bias_part : d0.bias_part;
    const int reverse = second ? d1.reverse : d0.reverse;
    __shared__ __align__(16) float dhs[RBT][RS_LD];
    __shared__ __align__(16) float dg[BF16 ? 1 : RBT][DG_LD];      // fp32 operand tile
    __shared__ __align__(16) H dgb[BF16 ? RBT : 1][DGB_LD];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 15, kq = l >> 4;
    const int b0 = blockIdx.x * ROWS, u = 16 * w + j;
    float wreg[BF16 ? 1 : 128];        // fp32: W_hh[4cc + kq][u]
    h16x8 wb[BF16 ? 16 : 1];           // 16-bit: W_hh[32cc + 8kq .. +7][u]
    if constexpr (BF16) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w_hh[(size_t)(32 * cc + 8 * kq + e) * RH + u];
            wb[cc] = ww_pack8<H>(v);
        }
    } else {
#pragma unroll
        for (int cc = 0; cc < 128; ++cc) wreg[cc] = w_hh[(size_t)(4 * cc + kq) * RH + u];
    }
    for (int e = tid; e < RBT * RH; e += 512) {
        const int row = e >> 7, c = e & 127;
        dhs[row][c] = (dhn && row < ROWS && b0 + row < B) ? dhn[(size_t)(b0 + row) * RH + c] : 0.f;
    }
    if constexpr (ROWS < RBT) {                     // operand rows nobody writes stay zero (their result rows are never read)
        for (int e = tid; e < (RBT - ROWS) * L4; e += 512) {
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
        const float4 v = *reinterpret_cast<const float4 *>(dcn + (size_t)eb * RH + ec0);
        dc[0] = v.x; dc[1] = v.y; dc[2] = v.z; dc[3] = v.w;
    }
    __syncthreads();
    const size_t em0 = (size_t)eb * T * RH + ec0;
    const float *const edy0 = dy ? dy + (size_t)eb * bsy + ec0 : nullptr;
    struct Saved { float4 v[NSAV - 1]; float4 dy; };        // i, f, g, o, tanh(c_t), c_{t-1} (h_{t-1} is for dW_hh only)
    auto prefetch = [&](int it, Saved &S) {
        if (it >= T || !ewave) return;
        const int t = reverse ? it : T - 1 - it;        // the forward pass's time order, backwards
        const size_t i = em0 + (size_t)t * RH;
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
                    if (erow_ok) *reinterpret_cast<uint2 *>(reinterpret_cast<H *>(dgo) + m4 + g * RH) = pk;
                    *reinterpret_cast<uint2 *>(&dgb[erow][g * RH + ec0]) = pk;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v = make_float4(q4[g][0], q4[g][1], q4[g][2], q4[g][3]);
                    if (erow_ok) *reinterpret_cast<float4 *>(dgo + m4 + g * RH) = v;
                    *reinterpret_cast<float4 *>(&dg[erow][g * RH + ec0]) = v;
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
        for (int e = tid; e < ROWS * RH; e += 512) {
            const int row = e >> 7, c = e & 127;
            if (b0 + row < B) dh0[(size_t)(b0 + row) * RH + c] = dhs[row][c];
        }
    if (dc0 && ewave && erow_ok)
        *reinterpret_cast<float4 *>(dc0 + (size_t)(b0 + erow) * RH + ec0) = make_float4(dc[0], dc[1], dc[2], dc[3]);
    // bias gradients: this block's column sums over its rows and all time steps -> bias_part[block][db_ih(512) | db_hh(512)]
    // (both halves the same sums: nn.LSTM's two biases receive the same gradient; rows added in a fixed order)
    {
        float *o = bias_part + (size_t)blockIdx.x * (2 * L4);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            __syncthreads();
            if (ewave) *reinterpret_cast<float4 *>(&dhs[erow][ec0]) = make_float4(bsum[g][0], bsum[g][1], bsum[g][2], bsum[g][3]);
            __syncthreads();
            if (tid < RH) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) s += dhs[r][tid];
                o[g * RH + tid] = s;
                o[L4 + g * RH + tid] = s;
            }
        }
    }
}

// the LSTM in the frame of ww_rnn.h: 4 gates, 7 saved tensors, one dG for both sides of the cell (no region of its own for dGh)
struct LstmCell {
    static constexpr RnnShape shape{4, NSAV, false, "WW_LSTM_ROWS", WW_K_LSTM};
    typedef LstmFwdDir FwdDir;
    typedef LstmBwdDir BwdDir;
    static constexpr decltype(&k_lstm_fwd<0, 8>) fwd[3][2] = WW_RNN_KERNELS(k_lstm_fwd);
    static constexpr decltype(&k_lstm_bwd<0, 8>) bwd[3][2] = WW_RNN_KERNELS(k_lstm_bwd);
    static LstmSaved saved(char *w, const RnnWs &L) {
        LstmSaved s;
        for (int k = 0; k < NSAV; ++k) s.s[k] = (float *)(w + L.sav[k]);
        return s;
    }
    static FwdDir fwd_dir(const RnnFwdHost &h, const RnnWs &L) {
        return FwdDir{(const float *)(h.ws + L.gi), h.w_hh, h.b_hh, h.s0[0], h.s0[1], h.y, h.s_n[0], h.s_n[1], saved(h.ws, L), h.reverse};
    }
    static BwdDir bwd_dir(const RnnBwdHost &h, const RnnWs &L, float *bias_part) {
        return BwdDir{h.w_hh, h.dy, h.ds_n[0], h.ds_n[1], saved(h.ws, L), (float *)(h.ws + L.gi), h.ds0[0], h.ds0[1], bias_part,
                      h.reverse};
    }
};

}  // namespace

extern "C" size_t ww_lstm_workspace_bytes(int B, int T, int I, int H) { return rnn_workspace_bytes(LstmCell::shape, B, T, I, H); }

extern "C" int ww_lstm_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *b_ih,
                           const float *b_hh, const float *h0, const float *c0, int B, int T, int I, int H, int reverse, float *y,
                           long ldy, float *h_n, float *c_n, void *ws, size_t ws_bytes, ww_stream_t stream) {
    RnnFwdHost d{w_ih, w_hh, b_ih, b_hh, {h0, c0}, nullptr, {h_n, c_n}, (char *)ws, reverse};
    return rnn_fwd<LstmCell>("ww_lstm_fwd", ctx, mode, x, ldx, &d, 1, B, T, I, H, y, ldy, ws_bytes, (hipStream_t)stream);
}

extern "C" int ww_lstm_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *dy,
                           long ldy, const float *dh_n, const float *dc_n, int B, int T, int I, int H, int reverse, void *ws,
                           size_t ws_bytes, float *dx, long lddx, int accumulate_dx, float *dw_ih, float *dw_hh, float *db_ih,
                           float *db_hh, float *dh0, float *dc0, ww_stream_t stream) {
    RnnBwdHost d{w_ih, w_hh, nullptr, {dh_n, dc_n}, (char *)ws, dw_ih, dw_hh, db_ih, db_hh, {dh0, dc0}, reverse};
    return rnn_bwd<LstmCell>("ww_lstm_bwd", ctx, mode, x, ldx, &d, 1, dy, ldy, B, T, I, H, ws_bytes, dx, lddx, accumulate_dx,
                             (hipStream_t)stream);
}

// Both directions of a bidirectional layer: dir[0] runs t = 0..T-1, dir[1] t = T-1..0; y / dy are (B,T,2H) buffers (row stride
// ldy >= 2H) whose column halves belong to the two directions; ONE recurrent launch (gridDim.y = 2) per pass.
extern "C" int ww_lstm_bidir_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_lstm_dir *dir, int B, int T, int I, int H,
                                 float *y, long ldy, size_t ws_bytes, ww_stream_t stream) {
    WW_REQUIRE(dir, WW_E_INVALID, "ww_lstm_bidir_fwd: null argument");
    RnnFwdHost d[2];
    for (int k = 0; k < 2; ++k)
        d[k] = RnnFwdHost{dir[k].w_ih, dir[k].w_hh, dir[k].b_ih, dir[k].b_hh, {dir[k].h0, dir[k].c0}, nullptr, {dir[k].h_n, dir[k].c_n},
                          (char *)dir[k].ws, k};
    return rnn_fwd<LstmCell>("ww_lstm_bidir_fwd", ctx, mode, x, ldx, d, 2, B, T, I, H, y, ldy, ws_bytes, (hipStream_t)stream);
}

extern "C" int ww_lstm_bidir_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_lstm_dir *dir, const float *dy, long ldy,
                                 int B, int T, int I, int H, size_t ws_bytes, float *dx, long lddx, ww_stream_t stream) {
    WW_REQUIRE(dir, WW_E_INVALID, "ww_lstm_bidir_bwd: null argument");
    RnnBwdHost d[2];
    for (int k = 0; k < 2; ++k)
        d[k] = RnnBwdHost{dir[k].w_ih, dir[k].w_hh, nullptr, {dir[k].dh_n, dir[k].dc_n}, (char *)dir[k].ws, dir[k].dw_ih, dir[k].dw_hh,
                          dir[k].db_ih, dir[k].db_hh, {dir[k].dh0, dir[k].dc0}, k};
    return rnn_bwd<LstmCell>("ww_lstm_bidir_bwd", ctx, mode, x, ldx, d, 2, dy, ldy, B, T, I, H, ws_bytes, dx, lddx, 0,
                             (hipStream_t)stream);
}

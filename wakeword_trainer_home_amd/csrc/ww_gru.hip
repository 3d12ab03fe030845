// GRU layer (one direction) forward / backward -- the recurrent half of SURVEY.md §8f rank 3 (CRNN); cell maths and
// parameter layout are torch.nn.GRU's, which is what the reference's GRUWakeword wraps
// (src/models/architectures.py:228-235: nn.GRU(input, 128, num_layers=2, batch_first=True, bidirectional=True)):
//   r = s(W_ir x + b_ir + W_hr h + b_hr)   z = s(W_iz x + b_iz + W_hz h + b_hz)
//   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))          h' = (1 - z) * n + z * h          gate order r|z|n
// MI355X shape of the computation:
//   * the input projection of ALL time steps is one GEMM  Gi = X W_ih^T + b_ih  (ww_gemm, matrix cores);
//   * the recurrence is ONE persistent kernel per direction: a block owns 16 batch rows for all T steps, keeps h in LDS,
//     and every wavefront keeps ITS slice of W_hh (16 hidden units x 3 gates x 128 = 96 VGPRs) in registers for the whole
//     sequence -- the per-step product h W_hh^T is 96 v_mfma_f32_16x16x4_f32 per wave with no weight traffic at all;
//   * backward mirrors it (dh carried in LDS, W_hh slice by output unit in registers, dGh W_hh per step), and the weight
//     gradients are three large GEMMs over all (batch, time) rows afterwards, split over K with fixed-order sums.
// `mode` selects the matrix type everywhere a matrix core is used: WW_ACT_F32 = exact-fp32 MFMA (parity mode);
// WW_ACT_BF16 = operands rounded to bf16, fp32 accumulation (what autocast does to a GRU) for the big GEMMs (input
// projection, dX, dW_ih, dW_hh) AND for the per-step products of the recurrence (h and W_hh enter the MFMA as bf16; the hidden
// state, the gates and every elementwise step stay fp32).  Hidden size 128 only.
#include "ww_rnn.h"

namespace {

constexpr int DG_LD = 3 * RH + 4;      // LDS row strides of the dG operand tile: fp32, 16-bit
constexpr int DGB_LD = 3 * RH + 8;

struct GruSaved { float *r, *z, *n, *hn, *hp; };    // (B*T, 128) each: gates, W_hn h + b_hn, h_{t-1}
// per-direction arguments of the recurrent kernels: gridDim.y = 2 runs BOTH directions of a bidirectional layer in one launch
// (blockIdx.y picks the set) -- twice the resident workgroups, no second stream, and a captured HIP graph keeps the concurrency
struct GruFwdDir { const float *gi, *w_hh, *b_hh, *h0; float *y, *hn_out; GruSaved sv; int reverse; };
struct GruBwdDir { const float *w_hh, *dy, *dhn; GruSaved sv; float *dgi, *dgh, *dh0, *bias_part; int reverse; };
__device__ __forceinline__ GruSaved pick(bool second, const GruSaved &a, const GruSaved &b) {
    return GruSaved{second ? b.r : a.r, second ? b.z : a.z, second ? b.n : a.n, second ? b.hn : a.hn, second ? b.hp : a.hp};
}

// grid (ceil(B/16), directions), block 512 = 8 waves; wave w owns hidden units [16w, 16w+16).  BF16: h and W_hh enter the MFMA as bf16
// (v_mfma_f32_16x16x32_bf16, 12 instead of 96 matrix instructions per step); h itself, the gates and the update stay fp32.
// ROWS = batch rows a workgroup owns: 16 (the MFMA tile's height) or 8.  The recurrence is bound by the ELEMENTWISE instructions
// a CU issues per time step (gates, saved-tensor traffic), not by its 12 MFMAs, and at the per-GPU batches of data-parallel
// training B/16 workgroups cover a fraction of the 256 CUs -- so with ROWS = 8 twice as many CUs each do half the elementwise
// work (the MFMA tile keeps 16 rows, the lower 8 unused): the 4 result rows of lanes 0-31 are split with lanes 32-63 by
// v_permlane32_swap, every lane then owns 2 cells instead of 4.
template <int MODE, int ROWS>
__global__ __launch_bounds__(512) void k_gru_fwd(GruFwdDir d0, GruFwdDir d1, int B, int T, long ldy, long bsy, int y_vec) {
    constexpr bool HALF = ROWS == 8;
    constexpr int NC = HALF ? 2 : 4;             // cells (batch rows of its unit) per lane
    const bool second = blockIdx.y != 0;
    const float *__restrict__ gi = second ? d1.gi : d0.gi, *__restrict__ w_hh = second ? d1.w_hh : d0.w_hh;
    const float *__restrict__ b_hh = second ? d1.b_hh : d0.b_hh, *__restrict__ h0 = second ? d1.h0 : d0.h0;
    float *__restrict__ y = second ? d1.y : d0.y, *__restrict__ hn_out = second ? d1.hn_out : d0.hn_out;
    const GruSaved sv = pick(second, d0.sv, d1.sv);
    const int reverse = second ? d1.reverse : d0.reverse;
    constexpr bool BF16 = MODE != 0;
    typedef typename ModeH<MODE>::type H;
    typedef typename H16<H>::x8 bf16x8;
    __shared__ __align__(16) float hs[2][RBT][RS_LD];
    __shared__ __align__(16) H hb[BF16 ? 2 : 1][BF16 ? RBT : 1][RB_LD];
    // what the backward needs of a step (r, z, n, W_hn h + b_hn, h_{t-1}) is parked in LDS in the MFMA result layout (a lane
    // holds 4 ROWS of one unit) and written out one step later as float4 along the UNIT axis by thread (row, 4 units):
    // 6 vector stores per thread and step instead of 24 scalar ones -- the store issue, not the MFMAs, bounded a step.
    // Two parities: a tile is rewritten two steps after it was filled, with a barrier in between.
    extern __shared__ __align__(16) float gru_sav[];           // [2][5][ROWS][RS_LD]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 15, kq = l >> 4;
    const int b0 = blockIdx.x * ROWS, u = 16 * w + j;
    const int crow0 = HALF ? 4 * (kq & 1) + 2 * (kq >> 1) : 4 * kq;      // first of this lane's NC consecutive batch rows
    float wreg[BF16 ? 1 : 3][BF16 ? 1 : 32];      // fp32: B operand of k-step kk, gate g: W_hh[g*128 + u][4kk + kq]
    bf16x8 wb[BF16 ? 3 : 1][BF16 ? 4 : 1];        // bf16: W_hh[g*128 + u][32kk + 8kq .. +7]
    if constexpr (BF16) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = w_hh[(size_t)(g * RH + u) * RH + 32 * kk + 8 * kq + e];
                wb[g][kk] = ww_pack8<H>(v);
            }
    } else {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) wreg[g][kk] = w_hh[(size_t)(g * RH + u) * RH + 4 * kk + kq];
    }
    const float bhr = b_hh[u], bhz = b_hh[RH + u], bhn = b_hh[2 * RH + u];
    for (int e = tid; e < RBT * RH; e += 512) {
        const int row = e >> 7, c = e & 127;
        const float hv = (h0 && row < ROWS && b0 + row < B) ? h0[(size_t)(b0 + row) * RH + c] : 0.f;
        hs[0][row][c] = hv;
        if constexpr (BF16) { hb[0][row][c] = (H)hv; hb[1][row][c] = (H)0.f; }     // (rows >= ROWS stay zero operands)
    }
    __syncthreads();
    // input projections of a step are loaded TWO steps ahead (register sets A / B, alternating): a step is ~0.5 us of
    // MFMA + gate work, an HBM/L2 round trip 1-2 us -- loaded at the top of the step that needs them (first version) the
    // latency was most of the step
    const float *gbase[NC];                      // row (b, t = 0) of this lane's batch rows, at its unit
#pragma unroll
    for (int reg = 0; reg < NC; ++reg) gbase[reg] = gi + (size_t)min(b0 + crow0 + reg, B - 1) * T * (3 * RH) + u;
    auto load_gi = [&](int it, float (&gr)[NC], float (&gz)[NC], float (&gn)[NC]) {
        if (it >= T) return;
        const size_t toff = (size_t)(reverse ? T - 1 - it : it) * (3 * RH);      // wave-uniform
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) {
            const float *g3 = gbase[reg] + toff;
            gr[reg] = g3[0]; gz[reg] = g3[RH]; gn[reg] = g3[2 * RH];
        }
    };
    const int frow = tid >> 5, fc0 = 4 * (tid & 31);
    const bool frow_ok = frow < ROWS && b0 + frow < B;           // (ROWS = 8: the upper four waves have nothing to flush)
    const size_t fm0 = (size_t)(b0 + frow) * T * RH + fc0;                 // element (b, t = 0, fc0) of the (B*T, 128) tensors
    float *const fy0 = y + (size_t)(b0 + frow) * bsy + fc0;
    const float *const fs0 = gru_sav + frow * RS_LD + fc0;
    auto flush = [&](int it) {                  // step `it` is complete (barrier passed): its tiles -> HBM
        if (!frow_ok) return;
        const int t = reverse ? T - 1 - it : it, par = it & 1;
        const size_t m = fm0 + (size_t)t * RH;
        const float *sp = fs0 + (size_t)par * 5 * ROWS * RS_LD;
        *reinterpret_cast<float4 *>(sv.r + m) = *reinterpret_cast<const float4 *>(sp);
        *reinterpret_cast<float4 *>(sv.z + m) = *reinterpret_cast<const float4 *>(sp + ROWS * RS_LD);
        *reinterpret_cast<float4 *>(sv.n + m) = *reinterpret_cast<const float4 *>(sp + 2 * ROWS * RS_LD);
        *reinterpret_cast<float4 *>(sv.hn + m) = *reinterpret_cast<const float4 *>(sp + 3 * ROWS * RS_LD);
        *reinterpret_cast<float4 *>(sv.hp + m) = *reinterpret_cast<const float4 *>(sp + 4 * ROWS * RS_LD);
        const float4 h4 = *reinterpret_cast<const float4 *>(&hs[par ^ 1][frow][fc0]);
        float *yo = fy0 + (size_t)t * ldy;
        if (y_vec) *reinterpret_cast<float4 *>(yo) = h4;
        else { yo[0] = h4.x; yo[1] = h4.y; yo[2] = h4.z; yo[3] = h4.w; }
    };
    auto step = [&](int it, float (&sr)[NC], float (&sz)[NC], float (&sn)[NC]) {
        const int cur = it & 1;
        float gir[NC], giz[NC], gin[NC];
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) { gir[reg] = sr[reg]; giz[reg] = sz[reg]; gin[reg] = sn[reg]; }
        load_gi(it + 2, sr, sz, sn);            // the set is free again: refill it for the step after next
        if (it > 0) flush(it - 1);
        floatx4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if constexpr (BF16) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(&hb[cur][j][32 * kk + 8 * kq]);
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = H16<H>::mfma16(a, wb[g][kk], acc[g]);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) {
                const float a = hs[cur][j][4 * kk + kq];
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wreg[g][kk], acc[g], 0, 0, 0);
            }
        }
        if constexpr (HALF) {                   // lanes 32-63 take over result rows 2, 3 of lanes 0-31 (rows 8-15 are unused)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    // (plain float copies first: __builtin_bit_cast applied to a vector ELEMENT reads element 0 with this clang --
                    //  the generated code swapped acc[g][0] with a copy of itself)
                    const float keep = acc[g][c], give = acc[g][c + 2];
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(keep), __float_as_uint(give), false, false);
                    acc[g][c] = __uint_as_float(sw[0]);
                }
        }
#pragma unroll
        for (int reg = 0; reg < NC; ++reg) {    // D[row = crow0 + reg][unit u]
            const int row = crow0 + reg;
            const float hnv = acc[2][reg] + bhn;
            const float r = gate_sigmoid<BF16>(gir[reg] + acc[0][reg] + bhr);
            const float z = gate_sigmoid<BF16>(giz[reg] + acc[1][reg] + bhz);
            const float n = gate_tanh<BF16>(gin[reg] + r * hnv);
            const float hp = hs[cur][row][u];
            const float h = (1.0f - z) * n + z * hp;
            hs[cur ^ 1][row][u] = h;
            if constexpr (BF16) hb[cur ^ 1][row][u] = (H)h;
            float *sp = gru_sav + (size_t)cur * 5 * ROWS * RS_LD + row * RS_LD + u;
            sp[0] = r; sp[ROWS * RS_LD] = z; sp[2 * ROWS * RS_LD] = n; sp[3 * ROWS * RS_LD] = hnv; sp[4 * ROWS * RS_LD] = hp;
        }
        __syncthreads();
    };
    {
        float ar[NC], az[NC], an[NC], br[NC], bz[NC], bn[NC];
        load_gi(0, ar, az, an);
        load_gi(1, br, bz, bn);
        for (int it = 0; it < T; it += 2) {
            step(it, ar, az, an);
            if (it + 1 < T) step(it + 1, br, bz, bn);
        }
        flush(T - 1);
    }
    if (hn_out)
        for (int e = tid; e < ROWS * RH; e += 512) {
            const int row = e >> 7, c = e & 127;
            if (b0 + row < B) hn_out[(size_t)(b0 + row) * RH + c] = hs[T & 1][row][c];
        }
}

// same decomposition; wave w owns OUTPUT units [16w,16w+16) of dh_{t-1} = dh*z + dGh W_hh
template <int MODE, int ROWS>
__global__ __launch_bounds__(512) void k_gru_bwd(GruBwdDir d0, GruBwdDir d1, long ldy, long bsy, int B, int T, int dy_vec) {
    const bool second = blockIdx.y != 0;
    const float *__restrict__ w_hh = second ? d1.w_hh : d0.w_hh, *__restrict__ dy = second ? d1.dy : d0.dy;
    const float *__restrict__ dhn = second ? d1.dhn : d0.dhn;
    const GruSaved sv = pick(second, d0.sv, d1.sv);
    float *__restrict__ dgi = second ? d1.dgi : d0.dgi, *__restrict__ dgh = second ? d1.dgh : d0.dgh;
    float *__restrict__ dh0 = second ? d1.dh0 : d0.dh0, *__restrict__ bias_part = second ? d1.bias_part : d0.bias_part;
    const int reverse = second ? d1.reverse : d0.reverse;
    constexpr bool BF16 = MODE != 0;
    typedef typename ModeH<MODE>::type H;
    typedef typename H16<H>::x8 bf16x8;
    __shared__ __align__(16) float dhs[RBT][RS_LD];
    __shared__ __align__(16) float dg[BF16 ? 1 : RBT][DG_LD];      // fp32 operand tile
    __shared__ __align__(16) H dgb[BF16 ? RBT : 1][DGB_LD];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 15, kq = l >> 4;
    const int b0 = blockIdx.x * ROWS, u = 16 * w + j;
    float wreg[BF16 ? 1 : 96];         // fp32: B operand of k-step cc: W_hh[4cc + kq][u]  (contraction over the 384 gate rows)
    bf16x8 wb[BF16 ? 12 : 1];          // bf16: W_hh[32cc + 8kq .. +7][u]
    if constexpr (BF16) {
#pragma unroll
        for (int cc = 0; cc < 12; ++cc) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w_hh[(size_t)(32 * cc + 8 * kq + e) * RH + u];
            wb[cc] = ww_pack8<H>(v);
        }
    } else {
#pragma unroll
        for (int cc = 0; cc < 96; ++cc) wreg[cc] = w_hh[(size_t)(4 * cc + kq) * RH + u];
    }
    for (int e = tid; e < RBT * RH; e += 512) {
        const int row = e >> 7, c = e & 127;
        dhs[row][c] = (dhn && row < ROWS && b0 + row < B) ? dhn[(size_t)(b0 + row) * RH + c] : 0.f;
    }
    if constexpr (ROWS < RBT) {                     // operand rows nobody writes stay zero (their result rows are never read)
        for (int e = tid; e < (RBT - ROWS) * 3 * RH; e += 512) {
            const int row = ROWS + e / (3 * RH), c = e % (3 * RH);
            if constexpr (BF16) dgb[row][c] = (H)0.f; else dg[row][c] = 0.f;
        }
    }
    __syncthreads();
    // elementwise part: thread = (batch row, 4 consecutive units) -> every tensor moves as ONE float4 per thread and step
    // (5 saved gates + dy in, dGi / dGh (3 gates each) out: 12 vector accesses instead of 48 scalar ones; the recurrence
    // is VALU-issue-bound and two thirds of its instructions were address arithmetic and scalar memory operations).
    // The saved gates of a step are loaded TWO steps ahead (register sets A / B, alternating), as in the forward kernel.
    const int erow = tid >> 5, ec0 = 4 * (tid & 31);
    const int eb = min(b0 + erow, B - 1);
    const bool erow_ok = b0 + erow < B;
    const bool ewave = erow < ROWS;                 // wave-uniform (two rows per wave): ROWS = 8 leaves the elementwise part to waves 0-3
    const size_t em0 = (size_t)eb * T * RH + ec0;                        // (b, t = 0, ec0) of the (B*T, 128) tensors
    const float *const edy0 = dy ? dy + (size_t)eb * bsy + ec0 : nullptr;
    struct Saved { float4 r, z, n, hn, hp, dy; };
    auto prefetch = [&](int it, Saved &S) {
        if (it >= T || !ewave) return;
        const int t = reverse ? it : T - 1 - it;        // the forward pass's time order, backwards
        const size_t i = em0 + (size_t)t * RH;
        S.r = *reinterpret_cast<const float4 *>(sv.r + i);
        S.z = *reinterpret_cast<const float4 *>(sv.z + i);
        S.n = *reinterpret_cast<const float4 *>(sv.n + i);
        S.hn = *reinterpret_cast<const float4 *>(sv.hn + i);
        S.hp = *reinterpret_cast<const float4 *>(sv.hp + i);
        if (edy0) {
            const float *p = edy0 + (size_t)t * ldy;
            S.dy = dy_vec ? *reinterpret_cast<const float4 *>(p) : make_float4(p[0], p[1], p[2], p[3]);
        } else {
            S.dy = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float sar[4] = {0.f, 0.f, 0.f, 0.f}, saz[4] = {0.f, 0.f, 0.f, 0.f}, san[4] = {0.f, 0.f, 0.f, 0.f}, shn[4] = {0.f, 0.f, 0.f, 0.f};
    auto step = [&](int it, Saved &S) {
        const int t = reverse ? it : T - 1 - it;
        if (ewave) {
        const float pr[4] = {S.r.x, S.r.y, S.r.z, S.r.w}, pz[4] = {S.z.x, S.z.y, S.z.z, S.z.w};
        const float pn[4] = {S.n.x, S.n.y, S.n.z, S.n.w}, phn[4] = {S.hn.x, S.hn.y, S.hn.z, S.hn.w};
        const float php[4] = {S.hp.x, S.hp.y, S.hp.z, S.hp.w}, pdy[4] = {S.dy.x, S.dy.y, S.dy.z, S.dy.w};
        prefetch(it + 2, S);                            // the set is free again
        const float4 dh4 = *reinterpret_cast<const float4 *>(&dhs[erow][ec0]);
        const float dhv[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
        float dar[4], daz[4], dan[4], dhn_[4], keep[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float dh = erow_ok ? dhv[q] + pdy[q] : 0.f;
            const float r = pr[q], z = pz[q], n = pn[q], hnv = phn[q], hp = php[q];
            const float dn = dh * (1.0f - z), dz = dh * (hp - n);
            dan[q] = dn * (1.0f - n * n);
            dar[q] = dan[q] * hnv * r * (1.0f - r);
            daz[q] = dz * z * (1.0f - z);
            dhn_[q] = dan[q] * r;
            keep[q] = dh * z;
            sar[q] += dar[q]; saz[q] += daz[q]; san[q] += dan[q]; shn[q] += dhn_[q];
        }
        const size_t m3 = ((size_t)(b0 + erow) * T + t) * (3 * RH) + ec0;
        if constexpr (BF16) {
            // dGi / dGh leave in the matrix type: the weight-gradient and dX products round their operands to it while staging
            // them anyway (ww_gemm, a16), so the results are bit-identical and those HBM-bound products read half the bytes
            typedef Act<H> A16;
            const uint2 qr = make_uint2(A16::pack2(dar[0], dar[1]), A16::pack2(dar[2], dar[3]));
            const uint2 qz = make_uint2(A16::pack2(daz[0], daz[1]), A16::pack2(daz[2], daz[3]));
            const uint2 qn = make_uint2(A16::pack2(dan[0], dan[1]), A16::pack2(dan[2], dan[3]));
            const uint2 qh = make_uint2(A16::pack2(dhn_[0], dhn_[1]), A16::pack2(dhn_[2], dhn_[3]));
            if (erow_ok) {
                H *gi16 = reinterpret_cast<H *>(dgi) + m3, *gh16 = reinterpret_cast<H *>(dgh) + m3;
                *reinterpret_cast<uint2 *>(gi16) = qr;
                *reinterpret_cast<uint2 *>(gi16 + RH) = qz;
                *reinterpret_cast<uint2 *>(gi16 + 2 * RH) = qn;
                *reinterpret_cast<uint2 *>(gh16) = qr;
                *reinterpret_cast<uint2 *>(gh16 + RH) = qz;
                *reinterpret_cast<uint2 *>(gh16 + 2 * RH) = qh;
            }
            *reinterpret_cast<uint2 *>(&dgb[erow][ec0]) = qr;
            *reinterpret_cast<uint2 *>(&dgb[erow][RH + ec0]) = qz;
            *reinterpret_cast<uint2 *>(&dgb[erow][2 * RH + ec0]) = qh;
        } else {
            if (erow_ok) {
                *reinterpret_cast<float4 *>(dgi + m3) = make_float4(dar[0], dar[1], dar[2], dar[3]);
                *reinterpret_cast<float4 *>(dgi + m3 + RH) = make_float4(daz[0], daz[1], daz[2], daz[3]);
                *reinterpret_cast<float4 *>(dgi + m3 + 2 * RH) = make_float4(dan[0], dan[1], dan[2], dan[3]);
                *reinterpret_cast<float4 *>(dgh + m3) = make_float4(dar[0], dar[1], dar[2], dar[3]);
                *reinterpret_cast<float4 *>(dgh + m3 + RH) = make_float4(daz[0], daz[1], daz[2], daz[3]);
                *reinterpret_cast<float4 *>(dgh + m3 + 2 * RH) = make_float4(dhn_[0], dhn_[1], dhn_[2], dhn_[3]);
            }
            *reinterpret_cast<float4 *>(&dg[erow][ec0]) = make_float4(dar[0], dar[1], dar[2], dar[3]);
            *reinterpret_cast<float4 *>(&dg[erow][RH + ec0]) = make_float4(daz[0], daz[1], daz[2], daz[3]);
            *reinterpret_cast<float4 *>(&dg[erow][2 * RH + ec0]) = make_float4(dhn_[0], dhn_[1], dhn_[2], dhn_[3]);
        }
        *reinterpret_cast<float4 *>(&dhs[erow][ec0]) = make_float4(keep[0], keep[1], keep[2], keep[3]);   // this thread's cells only
        }
        __syncthreads();
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BF16) {
#pragma unroll
            for (int cc = 0; cc < 12; ++cc)
                acc = H16<H>::mfma16(*reinterpret_cast<const bf16x8 *>(&dgb[j][32 * cc + 8 * kq]), wb[cc], acc);
        } else {
#pragma unroll
            for (int cc = 0; cc < 96; ++cc)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dg[j][4 * cc + kq], wreg[cc], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) dhs[4 * kq + reg][u] += acc[reg];
        __syncthreads();
    };
    {
        Saved A, Bs;
        prefetch(0, A);
        prefetch(1, Bs);
        for (int it = 0; it < T; it += 2) {
            step(it, A);
            if (it + 1 < T) step(it + 1, Bs);
        }
    }
    if (dh0)
        for (int e = tid; e < ROWS * RH; e += 512) {
            const int row = e >> 7, c = e & 127;
            if (b0 + row < B) dh0[(size_t)(b0 + row) * RH + c] = dhs[row][c];
        }
    // bias gradients: this block's column sums over its 16 rows and all time steps -> bias_part[block][db_ih(384) | db_hh(384)]
    // (thread (row, 4 columns) holds the time sums of its cells; one pass through dhs per gate, rows added in a fixed order)
    {
        float *o = bias_part + (size_t)blockIdx.x * (6 * RH);
        const float *src[4] = {sar, saz, san, shn};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            __syncthreads();
            if (ewave) *reinterpret_cast<float4 *>(&dhs[erow][ec0]) = make_float4(src[k][0], src[k][1], src[k][2], src[k][3]);
            __syncthreads();
            if (tid < 128) {
                float t = 0.f;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) t += dhs[r][tid];
                if (k == 0) { o[tid] = t; o[3 * RH + tid] = t; }
                else if (k == 1) { o[RH + tid] = t; o[4 * RH + tid] = t; }
                else if (k == 2) o[2 * RH + tid] = t;
                else o[5 * RH + tid] = t;
            }
        }
    }
}

// Philox dropout on a (B,T,C) tensor with row-strided rows: out = keep ? x * scale : 0.  Counter field (24 bits):
// stream_id (4) | t (12) | c>>2 (8); lane c&3; sample = global batch index.  Its own backward (apply to the gradient).
__global__ __launch_bounds__(256) void k_dropout_bt(const float *__restrict__ x, long ldx, int B, int T, int C, float scale,
                                                    uint64_t thresh, uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo,
                                                    uint32_t step_hi, uint64_t sample_offset, uint32_t stream_id,
                                                    float *__restrict__ out, long ldo, const ww_step_ctl *__restrict__ ctl) {
    ww_step_resolve(ctl, step_lo, step_hi, step_lo, step_hi);
    const int cq = (C + 3) / 4;
    const long n = (long)B * T * cq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int q = (int)(i % cq);
        const long m = i / cq;
        const int t = (int)(m % T), b = (int)(m / T);
        uint32_t rr[4];
        ww_philox(step_lo, step_hi, (uint32_t)(sample_offset + (uint64_t)b),
                  (WW_TAG_DROPOUT << 24) | (stream_id << 20) | ((uint32_t)t << 8) | (uint32_t)q, seed_lo, seed_hi, rr);
        const float *src = x + m * ldx + 4 * q;
        float *dst = out + m * ldo + 4 * q;
        if (4 * q < C) dst[0] = (uint64_t)rr[0] >= thresh ? src[0] * scale : 0.f;
        if (4 * q + 1 < C) dst[1] = (uint64_t)rr[1] >= thresh ? src[1] * scale : 0.f;
        if (4 * q + 2 < C) dst[2] = (uint64_t)rr[2] >= thresh ? src[2] * scale : 0.f;
        if (4 * q + 3 < C) dst[3] = (uint64_t)rr[3] >= thresh ? src[3] * scale : 0.f;
    }
}

// the GRU in the frame of ww_rnn.h: 3 gates, 5 saved tensors (r, z, n, W_hn h + b_hn, h_{t-1}), dGh apart from dGi (its n block is
// dGn * r, dGi's is dGn)
struct GruCell {
    static constexpr RnnShape shape{3, 5, true, "WW_GRU_ROWS", WW_K_GRU};
    typedef GruFwdDir FwdDir;
    typedef GruBwdDir BwdDir;
    static constexpr decltype(&k_gru_fwd<0, 8>) fwd[3][2] = WW_RNN_KERNELS(k_gru_fwd);
    static constexpr decltype(&k_gru_bwd<0, 8>) bwd[3][2] = WW_RNN_KERNELS(k_gru_bwd);
    static GruSaved saved(char *w, const RnnWs &L) {
        return GruSaved{(float *)(w + L.sav[0]), (float *)(w + L.sav[1]), (float *)(w + L.sav[2]), (float *)(w + L.sav[3]),
                        (float *)(w + L.sav[4])};
    }
    static FwdDir fwd_dir(const RnnFwdHost &h, const RnnWs &L) {
        return FwdDir{(const float *)(h.ws + L.gi), h.w_hh, h.b_hh, h.s0[0], h.y, h.s_n[0], saved(h.ws, L), h.reverse};
    }
    static BwdDir bwd_dir(const RnnBwdHost &h, const RnnWs &L, float *bias_part) {
        return BwdDir{h.w_hh, h.dy, h.ds_n[0], saved(h.ws, L), (float *)(h.ws + L.gi), (float *)(h.ws + L.dgh), h.ds0[0], bias_part,
                      h.reverse};
    }
};

}  // namespace

extern "C" int ww_dropout_bt(ww_ctx *ctx, const float *x, long ldx, int B, int T, int C, float p, uint64_t seed,
                             uint64_t step, uint64_t sample_offset, int stream_id, float *out, long ldo,
                             ww_stream_t stream) {
    WW_REQUIRE(ctx && x && out, WW_E_INVALID, "ww_dropout_bt: null argument");
    WW_REQUIRE(B >= 1 && T >= 1 && C >= 1 && ldx >= C && ldo >= C, WW_E_INVALID, "ww_dropout_bt: bad shape");
    WW_REQUIRE(T <= 4096 && C <= 1024 && stream_id >= 0 && stream_id < 16, WW_E_UNSUPPORTED,
               "ww_dropout_bt: T <= 4096, C <= 1024, stream_id < 16");
    WW_REQUIRE(p >= 0.f && p < 1.f, WW_E_INVALID, "ww_dropout_bt: p=%f not in [0,1)", (double)p);
    const int grid = ww_pass_dropout_bt((long)B * T * ((C + 3) / 4)).grid;
    hipLaunchKernelGGL(k_dropout_bt, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ldx, B, T, C,
                       (float)(1.0 / (1.0 - (double)p)), ww_prob_threshold((double)p), (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)step, (uint32_t)(step >> 32), sample_offset, (uint32_t)stream_id, out, ldo, ctx->step_ctl);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" size_t ww_gru_workspace_bytes(int B, int T, int I, int H) { return rnn_workspace_bytes(GruCell::shape, B, T, I, H); }

extern "C" int ww_gru_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *b_ih,
                          const float *b_hh, const float *h0, int B, int T, int I, int H, int reverse, float *y, long ldy,
                          float *h_n, void *ws, size_t ws_bytes, ww_stream_t stream) {
    RnnFwdHost d{w_ih, w_hh, b_ih, b_hh, {h0}, nullptr, {h_n}, (char *)ws, reverse};
    return rnn_fwd<GruCell>("ww_gru_fwd", ctx, mode, x, ldx, &d, 1, B, T, I, H, y, ldy, ws_bytes, (hipStream_t)stream);
}

extern "C" int ww_gru_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *dy,
                          long ldy, const float *dh_n, int B, int T, int I, int H, int reverse, void *ws, size_t ws_bytes,
                          float *dx, long lddx, int accumulate_dx, float *dw_ih, float *dw_hh, float *db_ih, float *db_hh,
                          float *dh0, ww_stream_t stream) {
    RnnBwdHost d{w_ih, w_hh, nullptr, {dh_n}, (char *)ws, dw_ih, dw_hh, db_ih, db_hh, {dh0}, reverse};
    return rnn_bwd<GruCell>("ww_gru_bwd", ctx, mode, x, ldx, &d, 1, dy, ldy, B, T, I, H, ws_bytes, dx, lddx, accumulate_dx,
                            (hipStream_t)stream);
}

// Both directions of a bidirectional layer: dir[0] runs t = 0..T-1, dir[1] t = T-1..0; y / dy are (B,T,2H) buffers (row stride
// ldy >= 2H) whose column halves belong to the two directions; ONE recurrent launch (gridDim.y = 2) per pass.
extern "C" int ww_gru_bidir_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_gru_dir *dir, int B, int T, int I, int H,
                                float *y, long ldy, size_t ws_bytes, ww_stream_t stream) {
    WW_REQUIRE(dir, WW_E_INVALID, "ww_gru_bidir_fwd: null argument");
    RnnFwdHost d[2];
    for (int k = 0; k < 2; ++k)
        d[k] = RnnFwdHost{dir[k].w_ih, dir[k].w_hh, dir[k].b_ih, dir[k].b_hh, {dir[k].h0}, nullptr, {dir[k].h_n}, (char *)dir[k].ws, k};
    return rnn_fwd<GruCell>("ww_gru_bidir_fwd", ctx, mode, x, ldx, d, 2, B, T, I, H, y, ldy, ws_bytes, (hipStream_t)stream);
}

extern "C" int ww_gru_bidir_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_gru_dir *dir, const float *dy, long ldy,
                                int B, int T, int I, int H, size_t ws_bytes, float *dx, long lddx, ww_stream_t stream) {
    WW_REQUIRE(dir, WW_E_INVALID, "ww_gru_bidir_bwd: null argument");
    RnnBwdHost d[2];
    for (int k = 0; k < 2; ++k)
        d[k] = RnnBwdHost{dir[k].w_ih, dir[k].w_hh, nullptr, {dir[k].dh_n}, (char *)dir[k].ws, dir[k].dw_ih, dir[k].dw_hh,
                          dir[k].db_ih, dir[k].db_hh, {dir[k].dh0}, k};
    return rnn_bwd<GruCell>("ww_gru_bidir_bwd", ctx, mode, x, ldx, d, 2, dy, ldy, B, T, I, H, ws_bytes, dx, lddx, 0,
                            (hipStream_t)stream);
}

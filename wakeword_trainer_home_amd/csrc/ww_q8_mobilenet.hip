// Integer-only inference of an exported int8 MobileNetV3Wakeword bundle (DESIGN.md "Export", the int8 law, subsection "MobileNetV3").
//   the 1x1 conv : expand, project, 96 -> 576, classifier.0 on the pooled rows: the one-segment geometry of the int8 tap-GEMM core
//                (ww_q8_tap_gemm.h: the lane map), one 16-row tile per wave and item, weights streamed, with one of three epilogues:
//                    RELU   out = clamp(-128 + R(acc), -128, 127)
//                    HSWISH u = clamp(z_u + R(acc), -128, 127), out = T[u + 128]      (T: the layer's int8 table)
//                    SIGNED out = clamp(R(acc) [+ R(res, m_r, sh_r)], -128, 127)       (z_out = 0, res signed)
//   k_mq8_dw   : depthwise k x k (k = 3, 5), stride 1 or 2, pad k / 2, and the 3x3 stride-2 one-channel stem: VALU int32, one lane per
//                (output pixel, 16 channels), RELU or HSWISH epilogue
//   k_mq8_se   : squeeze-excitation, one workgroup per image: channel sums through LDS, the pooled vector, fc1 + ReLU, fc2 + the
//                Hardsigmoid gate G (uint8, scale 1 / 255)
//   k_mq8_gate : y = clamp(z_a + R((q_a - z_a) G, m_g, sh_g), -128, 127), a pass over the tensor (the pass form; in the fused form the
//                projection's geometry MqGated applies the same expression to its pixel fragments and y is never stored)
//   k_mq8_pool, k_mq8_fc : the head's pool (one workgroup per image) and classifier.3 (one wave per class)
// Quantisation is ww_q8_quantize.  Activations are int8 NHWC (B,H,W,Cp), Cp = the channel count rounded up to 64: a pixel's channels are
// whole 64-deep K chunks of the instruction.  Pad channels hold the tensor's zero point and meet zero weights; pad OUTPUT channels have
// zero weights, a zero bias and m = 2^30, sh = 31, so they come out as the zero point of the tensor written (T[z_u + 128] = z_out).
// Rows of the 1x1 conv are pixels of the whole batch, so a 16-row tile may span images.
//
// bias arguments of the conv kernels are the EFFECTIVE bias q_b - z_in * sum(q_w) (host, once per bundle), so "a source pixel outside
// the image" and "a pad channel" are both z_in bytes.  k_mq8_se and k_mq8_fc subtract the zero point themselves and take the law's own
// q_b.  All adds that may wrap are unsigned.
#include "ww_q8_tap_gemm.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int MQ_BLOCK = 256;
constexpr int MQ_WAVES = MQ_BLOCK / 64;
constexpr int MQ_MAX_CP = 1024;                // widest tensor the one-workgroup-per-image kernels sum (their LDS image)
constexpr int MQ_MAX_SQ = 256;                 // widest squeeze vector of k_mq8_se
enum { MQ_RELU = 0, MQ_HSWISH = 1, MQ_SIGNED = 2 };
constexpr bool MQ_GATE_FUSED_DEFAULT = false;  // decided by the A/B of tools/bench_q8_mobilenetv3.py (profiles/q8_mobilenetv3_measured.txt)

// the RELU and HSWISH epilogues of one value r = R(acc, m, sh); tab: the layer's table in LDS
template <int EP> __device__ __forceinline__ int mq8_act(long long r, int zu, const signed char *tab) {
    if (EP == MQ_RELU) return q8_clamp(r);
    return (int)tab[q8_clamp_signed(r + zu) + 128];
}

// The fused gate form of the one-segment geometry: `in` is the depthwise output a, not y; the gate multiply
// y = clamp(z_a + R((q_a - z_a) G, m_g, sh_g)) is applied to the pixel fragment as it is loaded, so it stays in registers and no y
// tensor is written or read.  gate: (N / HW, Cin), the row of the image a pixel belongs to.
struct MqGated {
    const int8_t *in;
    long N;
    int Cin, zfill;
    const uint8_t *gate;
    int HW, zero, gate_m, gate_sh;
    struct Row { long n; };
    struct Src { const int8_t *p; const uint8_t *gp; bool live; };
    __device__ int nseg() const { return 1; }
    __device__ int K() const { return Cin; }
    __device__ void row(long n, Row &r) const { r.n = n; }
    __device__ void seg(const Row &r, int, int g, Src &s) const {
        s.live = r.n < N;
        s.p = in + r.n * Cin + 16 * g;                          // both dereferenced only where live
        s.gp = gate + r.n / HW * Cin + 16 * g;
    }
    __device__ v4i load(const Src &s, int kc) const {
        v4i bq = {zfill, zfill, zfill, zfill};
        if (s.live) {
            bq = *(const v4i *)(s.p + 64 * kc);
            const v4i gv = *(const v4i *)(s.gp + 64 * kc);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                int q[4];
                q8_unpack4(bq[d], q);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    q[e] = q8_clamp_signed(zero + q8_round((q[e] - zero) * (int)(((unsigned)gv[d] >> (8 * e)) & 255u), gate_m, gate_sh));
                bq[d] = q8_pack4(q[0], q[1], q[2], q[3]);
            }
        }
        return bq;
    }
};

__shared__ signed char mq8_s_tab[256];         // the Hardswish table of the 1x1 conv a workgroup runs (MqAct<MQ_HSWISH>)

template <int EP> struct MqAct : Q8Chan {      // RELU and HSWISH
    const int8_t *tab;                         // HSWISH: int8 (256)
    int8_t *out;                               // (N, Cout)
    int zu;
    __device__ void begin() const {
        if (EP == MQ_HSWISH) {
            mq8_s_tab[threadIdx.x] = tab[threadIdx.x];
            __syncthreads();
        }
    }
    __device__ void store(const v4i (&acc)[4], long n, int c0) const {
        q8_tap_store(*this, acc, v4i{0, 0, 0, 0}, out, n, c0, [&](long long v, int) { return mq8_act<EP>(v, zu, mq8_s_tab); });
    }
};

struct MqSigned : Q8Chan {                     // out = clamp(R(acc) [+ R(res, m_r, sh_r)]); res: (N, Cout), zero point 0, or null
    const int8_t *res;
    int8_t *out;
    int res_m, res_sh;
    __device__ void store(const v4i (&acc)[4], long n, int c0) const {
        v4i hv = {0, 0, 0, 0};
        if (res) hv = *(const v4i *)(res + n * Cout + c0);
        q8_tap_store(*this, acc, hv, out, n, c0, [&](long long v, int h) {
            if (res) v += q8_round(h, res_m, res_sh);
            return q8_clamp_signed(v);
        });
    }
};

struct mq8_dw_args {
    const int8_t *in, *w;                      // in (B,H,W,Cp) -- STEM: (B,H,W) --; w (k k, Cp) [tap][channel]
    const int *bias, *mult, *shift;            // (Cp) each
    const int8_t *tab;
    int8_t *out;                               // (B,Ho,Wo,Cp)
    long nvec;                                 // B Ho Wo (Cp / 16)
    int H, W, Ho, Wo, Cp, k, stride, zero, zu;
};

// one lane per (output pixel, 16 channels); a window position outside the image reads as the zero point
template <int EP, bool STEM> __global__ __launch_bounds__(MQ_BLOCK) void k_mq8_dw(mq8_dw_args a) {
    __shared__ signed char s_tab[256];
    if (EP == MQ_HSWISH) {
        s_tab[threadIdx.x] = a.tab[threadIdx.x];
        __syncthreads();
    }
    const int cv = a.Cp / 16, pad = a.k / 2;
    const int zfill = (a.zero & 255) * 0x01010101;
    for (long i = (long)blockIdx.x * MQ_BLOCK + threadIdx.x; i < a.nvec; i += (long)gridDim.x * MQ_BLOCK) {
        const int v = (int)(i % cv);
        const long pix = i / cv;
        const long b = pix / ((long)a.Ho * a.Wo);
        const int rem = (int)(pix - b * a.Ho * a.Wo);
        const int h0 = rem / a.Wo * a.stride - pad, w0 = rem % a.Wo * a.stride - pad;
        int acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0;
        for (int kh = 0; kh < a.k; ++kh) {
            const int hi = h0 + kh;
            for (int kw = 0; kw < a.k; ++kw) {
                const int wi = w0 + kw;
                const bool live = hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
                const v4i wv = *(const v4i *)(a.w + (long)(kh * a.k + kw) * a.Cp + 16 * v);
                v4i x = {zfill, zfill, zfill, zfill};
                if (STEM) {
                    if (live) {
                        const int q = (int)a.in[(b * a.H + hi) * a.W + wi] & 255;
                        x = v4i{q * 0x01010101, q * 0x01010101, q * 0x01010101, q * 0x01010101};
                    }
                } else if (live) {
                    x = *(const v4i *)(a.in + ((b * a.H + hi) * a.W + wi) * a.Cp + 16 * v);
                }
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    int q[4], ww[4];
                    q8_unpack4(x[d], q);
                    q8_unpack4(wv[d], ww);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * d + e] += ww[e] * q[e];
                }
            }
        }
        v4i ov;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const v4i bb = *(const v4i *)(a.bias + 16 * v + 4 * d);
            const v4i mu = *(const v4i *)(a.mult + 16 * v + 4 * d);
            const v4i sh = *(const v4i *)(a.shift + 16 * v + 4 * d);
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                q[e] = mq8_act<EP>(q8_round((int)((unsigned)acc[4 * d + e] + (unsigned)bb[e]), mu[e], sh[e]), a.zu, s_tab);
            ov[d] = q8_pack4(q[0], q[1], q[2], q[3]);
        }
        *(v4i *)(a.out + pix * a.Cp + 16 * v) = ov;
    }
}

// The pooled vector of image blockIdx.x into s_pool (Cp ints, as DIFFERENCES p - zero) and, where pool_out is given, to memory:
// p = clamp(zero + R(sum_hw (q - zero), m, sh), -128, 127).  s_part: slots x Cp ints, slots = MQ_BLOCK / (Cp / 4) >= 1.
__device__ __forceinline__ void mq8_pool_image(const int8_t *__restrict__ img, int HW, int Cp, int zero, int pm, int psh, int *s_part,
                                               int *s_pool, int8_t *__restrict__ pool_out) {
    const int tid = threadIdx.x, ncol = Cp / 4, slots = MQ_BLOCK / ncol;
    if (tid < slots * ncol) {
        const int col = tid % ncol, slot = tid / ncol;
        int sum[4] = {0, 0, 0, 0};
        for (int t = slot; t < HW; t += slots) {
            int q[4];
            q8_unpack4(*(const int *)(img + (long)t * Cp + 4 * col), q);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] += q[e] - zero;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s_part[slot * Cp + 4 * col + e] = sum[e];
    }
    __syncthreads();
    for (int c = tid; c < Cp; c += MQ_BLOCK) {
        int S = 0;
        for (int s = 0; s < slots; ++s) S += s_part[s * Cp + c];
        const int pq = q8_clamp_signed(zero + q8_round(S, pm, psh));
        if (pool_out) pool_out[(long)blockIdx.x * Cp + c] = (int8_t)pq;
        s_pool[c] = pq - zero;
    }
    __syncthreads();
}

__global__ __launch_bounds__(MQ_BLOCK) void k_mq8_pool(const int8_t *__restrict__ in, int HW, int Cp, int zero, int pm, int psh,
                                                       int8_t *__restrict__ pool_out) {
    __shared__ int s_part[MQ_MAX_CP];
    __shared__ int s_pool[MQ_MAX_CP];
    mq8_pool_image(in + (long)blockIdx.x * HW * Cp, HW, Cp, zero, pm, psh, s_part, s_pool, pool_out);
}

struct mq8_se_args {
    const int8_t *in;                          // (B, HW, Cp)
    const int8_t *w1, *w2;                     // fc1 (Csq, C), fc2 (C, Csq), unpadded rows
    const int *b1, *m1, *sh1, *b2, *m2, *sh2;  // the law's q_b (not the effective bias), mult, shift: (Csq) and (C)
    int8_t *pool, *h;                          // (B, Cp), (B, Csq)
    uint8_t *gate;                             // (B, Cp); the pad channels get 0
    int HW, C, Cp, Csq, zero, pm, psh;
};

__global__ __launch_bounds__(MQ_BLOCK) void k_mq8_se(mq8_se_args a) {
    __shared__ int s_part[MQ_MAX_CP];
    __shared__ int s_pool[MQ_MAX_CP];
    __shared__ int s_h[MQ_MAX_SQ];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    mq8_pool_image(a.in + b * a.HW * a.Cp, a.HW, a.Cp, a.zero, a.pm, a.psh, s_part, s_pool, a.pool);
    for (int j = tid; j < a.Csq; j += MQ_BLOCK) {
        unsigned acc = (unsigned)a.b1[j];
        const int8_t *w = a.w1 + (long)j * a.C;
        for (int c = 0; c < a.C; ++c) acc += (unsigned)((int)w[c] * s_pool[c]);
        const int hq = q8_clamp_signed(q8_round((int)acc, a.m1[j], a.sh1[j]) - 128);
        a.h[b * a.Csq + j] = (int8_t)hq;
        s_h[j] = hq + 128;
    }
    __syncthreads();
    for (int c = tid; c < a.Cp; c += MQ_BLOCK) {
        int gq = 0;
        if (c < a.C) {
            unsigned acc = (unsigned)a.b2[c];
            const int8_t *w = a.w2 + (long)c * a.Csq;
            for (int j = 0; j < a.Csq; ++j) acc += (unsigned)((int)w[j] * s_h[j]);
            const long long r = q8_round((int)acc, a.m2[c], a.sh2[c]);
            gq = (int)(r < 0 ? 0 : (r > 255 ? 255 : r));
        }
        a.gate[b * a.Cp + c] = (uint8_t)gq;
    }
}

// y = clamp(zero + R((q - zero) G, gm, gsh), -128, 127): one thread per 16 channels of a pixel
__global__ __launch_bounds__(MQ_BLOCK) void k_mq8_gate(const int8_t *__restrict__ in, const uint8_t *__restrict__ gate, long nvec, int HW,
                                                       int Cp, int zero, int gm, int gsh, int8_t *__restrict__ out) {
    const int cv = Cp / 16;
    for (long i = (long)blockIdx.x * MQ_BLOCK + threadIdx.x; i < nvec; i += (long)gridDim.x * MQ_BLOCK) {
        const int v = (int)(i % cv);
        const long pix = i / cv, b = pix / HW;
        const v4i x = *(const v4i *)(in + pix * Cp + 16 * v);
        const v4i gv = *(const v4i *)(gate + b * Cp + 16 * v);
        v4i ov;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int q[4], y[4];
            q8_unpack4(x[d], q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int G = (int)(((unsigned)gv[d] >> (8 * e)) & 255u);
                y[e] = q8_clamp_signed(zero + q8_round((q[e] - zero) * G, gm, gsh));
            }
            ov[d] = q8_pack4(y[0], y[1], y[2], y[3]);
        }
        *(v4i *)(out + pix * Cp + 16 * v) = ov;
    }
}

// classifier.3: logits[b, c] = float(sum_k w[c, k] (q[b, k] - zero) + bias[c]) * scale[c]; one workgroup per image, one wave per class
__global__ __launch_bounds__(MQ_BLOCK) void k_mq8_fc(const int8_t *__restrict__ hid, int K, int zero, const int8_t *__restrict__ w,
                                                     const int *__restrict__ bias, const float *__restrict__ scale, int nc,
                                                     float *__restrict__ logits) {
    const int lane = threadIdx.x & 63;
    const int8_t *q = hid + (long)blockIdx.x * K;
    for (int c = threadIdx.x >> 6; c < nc; c += MQ_WAVES) {
        unsigned acc = 0;
        for (int k = lane; k < K; k += 64) acc += (unsigned)((int)w[(long)c * K + k] * ((int)q[k] - zero));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += (unsigned)__shfl_xor((int)acc, off, 64);
        if (lane == 0) logits[(long)blockIdx.x * nc + c] = (float)(int)(acc + (unsigned)bias[c]) * scale[c];
    }
}

inline int mq8_half(int n) { return (n - 1) / 2 + 1; }           // floor((n + 2 p - k) / 2) + 1 for (k, p) = (3, 1) and (5, 2)
inline bool mq8_zero_ok(int z) { return z >= -128 && z <= 127; }

template <int EP, bool STEM> int mq8_launch_dw(ww_ctx *ctx, const mq8_dw_args &a, hipStream_t st) {
    const int grid = ww_capped_grid(ctx, ww_pass_ew(a.nvec).grid);
    hipLaunchKernelGGL((k_mq8_dw<EP, STEM>), dim3(grid), dim3(MQ_BLOCK), 0, st, a);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

// mobilenet_v3_small: cin, k, exp, cout, squeeze width (0: no squeeze-excitation), Hardswish, stride
struct mq8_block { int cin, k, exp, cout, sq, hs, stride; };
const mq8_block MQ_CONF[WW_MQ8_BLOCKS] = {{16, 3, 16, 16, 8, 0, 2},   {16, 3, 72, 24, 0, 0, 2},    {24, 3, 88, 24, 0, 0, 1},
                                          {24, 5, 96, 40, 24, 1, 2},  {40, 5, 240, 40, 64, 1, 1},  {40, 5, 240, 40, 64, 1, 1},
                                          {40, 5, 120, 48, 32, 1, 1}, {48, 5, 144, 48, 40, 1, 1},  {48, 5, 288, 96, 72, 1, 2},
                                          {96, 5, 576, 96, 144, 1, 1}, {96, 5, 576, 96, 144, 1, 1}};

struct mq8_plan {                              // byte offsets of every tensor the launches write, -1 where a block has none
    long xq, stem, expand[WW_MQ8_BLOCKS], dw[WW_MQ8_BLOCKS], sepool[WW_MQ8_BLOCKS], h[WW_MQ8_BLOCKS], gate[WW_MQ8_BLOCKS],
        y[WW_MQ8_BLOCKS], out[WW_MQ8_BLOCKS], last, pool, hidden, total;
    int Hin[WW_MQ8_BLOCKS], Win[WW_MQ8_BLOCKS], H[WW_MQ8_BLOCKS], W[WW_MQ8_BLOCKS];
};

bool mq8_make_plan(int B, int F, int T, mq8_plan *p) {
    if (B < 1 || F < 1 || T < 1 || (long)B * F * T > (1l << 28)) return false;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += q8_round256(bytes); return at; };
    int H = mq8_half(F), W = mq8_half(T);
    p->xq = take((long)B * F * T);
    p->stem = take((long)B * H * W * 64);
    for (int i = 0; i < WW_MQ8_BLOCKS; ++i) {
        const mq8_block &c = MQ_CONF[i];
        const int ep = q8_pad64(c.exp);
        p->Hin[i] = H; p->Win[i] = W;
        p->expand[i] = c.exp != c.cin ? take((long)B * H * W * ep) : -1;
        if (c.stride == 2) { H = mq8_half(H); W = mq8_half(W); }
        p->H[i] = H; p->W[i] = W;
        p->dw[i] = take((long)B * H * W * ep);
        p->sepool[i] = c.sq ? take((long)B * ep) : -1;
        p->h[i] = c.sq ? take((long)B * c.sq) : -1;
        p->gate[i] = c.sq ? take((long)B * ep) : -1;
        p->y[i] = c.sq ? take((long)B * H * W * ep) : -1;
        p->out[i] = take((long)B * H * W * q8_pad64(c.cout));
    }
    p->last = take((long)B * H * W * WW_MQ8_LAST);
    p->pool = take((long)B * WW_MQ8_LAST);
    p->hidden = take((long)B * WW_MQ8_HIDDEN);
    p->total = off;
    return true;
}

}  // namespace

extern "C" int ww_mq8_conv1x1_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                                  const int32_t *shift, long N, int Cin, int Cout, int zero, int epilogue, int zero_u, const int8_t *tab,
                                  const int8_t *residual, int res_mult, int res_shift, const uint8_t *gate, int HW, int gate_mult,
                                  int gate_shift, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w && bias && mult && shift && out, WW_E_INVALID, "ww_mq8_conv1x1_fwd: null argument");
    WW_REQUIRE(!gate || (epilogue == WW_MQ8_SIGNED && HW >= 1 && N % HW == 0 && q8_mult_ok(gate_mult, gate_shift) && aligned16(gate)),
               WW_E_INVALID, "ww_mq8_conv1x1_fwd: a gate goes with the signed epilogue, HW = %d dividing N, multiplier %d / shift %d", HW,
               gate_mult, gate_shift);
    WW_REQUIRE(N >= 1 && N <= (1l << 31), WW_E_INVALID, "ww_mq8_conv1x1_fwd: N=%ld", N);
    WW_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cout >= 64 && Cout % 64 == 0 && Cin <= 4096 && Cout <= 4096, WW_E_INVALID,
               "ww_mq8_conv1x1_fwd: channel counts %d -> %d must be multiples of 64 (at most 4096)", Cin, Cout);
    WW_REQUIRE(mq8_zero_ok(zero) && mq8_zero_ok(zero_u), WW_E_INVALID, "ww_mq8_conv1x1_fwd: zero points %d / %d outside int8", zero, zero_u);
    WW_REQUIRE(epilogue == WW_MQ8_RELU || epilogue == WW_MQ8_HSWISH || epilogue == WW_MQ8_SIGNED, WW_E_INVALID,
               "ww_mq8_conv1x1_fwd: epilogue %d", epilogue);
    WW_REQUIRE((epilogue == WW_MQ8_HSWISH) == (tab != nullptr), WW_E_INVALID,
               "ww_mq8_conv1x1_fwd: the Hardswish epilogue, and only it, takes a table");
    WW_REQUIRE(!residual || epilogue == WW_MQ8_SIGNED, WW_E_INVALID, "ww_mq8_conv1x1_fwd: only the signed epilogue takes a residual");
    WW_REQUIRE(!residual || q8_mult_ok(res_mult, res_shift), WW_E_INVALID,
               "ww_mq8_conv1x1_fwd: residual multiplier %d / shift %d out of range", res_mult, res_shift);
    WW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(out) &&
               aligned16(residual), WW_E_INVALID, "ww_mq8_conv1x1_fwd: tensors must be 16-byte aligned");
    WW_REQUIRE(in != out && residual != out, WW_E_INVALID, "ww_mq8_conv1x1_fwd: in place");
    const Q8Rows geo{in, N, Cin, (zero & 255) * 0x01010101};
    const Q8Chan chan{bias, mult, shift, Cout};
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope prof(ctx, WW_K_PW_FWD, st);
    if (epilogue == WW_MQ8_RELU) return q8_tap_launch_stream<Q8Rows, MqAct<MQ_RELU>, 1>(ctx, geo, {chan, tab, out, zero_u}, w, st);
    if (epilogue == WW_MQ8_HSWISH) return q8_tap_launch_stream<Q8Rows, MqAct<MQ_HSWISH>, 1>(ctx, geo, {chan, tab, out, zero_u}, w, st);
    const MqSigned epi{chan, residual, out, res_mult, res_shift};
    if (gate) {
        const MqGated gated{in, N, Cin, geo.zfill, gate, HW, zero, gate_mult, gate_shift};
        return q8_tap_launch_stream<MqGated, MqSigned, 1>(ctx, gated, epi, w, st);
    }
    return q8_tap_launch_stream<Q8Rows, MqSigned, 1>(ctx, geo, epi, w, st);
}

extern "C" int ww_mq8_dwconv_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                                 const int32_t *shift, int B, int H, int W, int Cp, int k, int stride, int zero, int epilogue, int zero_u,
                                 const int8_t *tab, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w && bias && mult && shift && out, WW_E_INVALID, "ww_mq8_dwconv_fwd: null argument");
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= (1l << 31), WW_E_INVALID, "ww_mq8_dwconv_fwd: B=%d H=%d W=%d", B, H, W);
    WW_REQUIRE(Cp >= 16 && Cp % 16 == 0 && Cp <= 4096, WW_E_INVALID, "ww_mq8_dwconv_fwd: %d channels (a multiple of 16, at most 4096)", Cp);
    WW_REQUIRE((k == 3 || k == 5) && (stride == 1 || stride == 2), WW_E_INVALID, "ww_mq8_dwconv_fwd: k=%d stride=%d", k, stride);
    WW_REQUIRE(mq8_zero_ok(zero) && mq8_zero_ok(zero_u), WW_E_INVALID, "ww_mq8_dwconv_fwd: zero points %d / %d outside int8", zero, zero_u);
    WW_REQUIRE(epilogue == WW_MQ8_RELU || epilogue == WW_MQ8_HSWISH, WW_E_INVALID, "ww_mq8_dwconv_fwd: epilogue %d", epilogue);
    WW_REQUIRE((epilogue == WW_MQ8_HSWISH) == (tab != nullptr), WW_E_INVALID,
               "ww_mq8_dwconv_fwd: the Hardswish epilogue, and only it, takes a table");
    WW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(out) && in != out,
               WW_E_INVALID, "ww_mq8_dwconv_fwd: tensors must be 16-byte aligned, not in place");
    const int Ho = stride == 2 ? mq8_half(H) : H, Wo = stride == 2 ? mq8_half(W) : W;
    mq8_dw_args a{in, w, bias, mult, shift, tab, out, (long)B * Ho * Wo * (Cp / 16), H, W, Ho, Wo, Cp, k, stride, zero, zero_u};
    ww_prof_scope prof(ctx, WW_K_DW_FWD, (hipStream_t)stream);
    return epilogue == WW_MQ8_RELU ? mq8_launch_dw<MQ_RELU, false>(ctx, a, (hipStream_t)stream)
                                   : mq8_launch_dw<MQ_HSWISH, false>(ctx, a, (hipStream_t)stream);
}

extern "C" int ww_mq8_stem_fwd(ww_ctx *ctx, const int8_t *xq, const int8_t *w, const int32_t *bias, const int32_t *mult,
                               const int32_t *shift, int B, int F, int T, int Cp, int zero, int zero_u, const int8_t *tab, int8_t *out,
                               ww_stream_t stream) {
    WW_REQUIRE(ctx && xq && w && bias && mult && shift && tab && out, WW_E_INVALID, "ww_mq8_stem_fwd: null argument");
    WW_REQUIRE(B >= 1 && F >= 1 && T >= 1 && (long)B * F * T <= (1l << 31), WW_E_INVALID, "ww_mq8_stem_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(Cp >= 16 && Cp % 16 == 0 && Cp <= 4096, WW_E_INVALID, "ww_mq8_stem_fwd: %d channels (a multiple of 16, at most 4096)", Cp);
    WW_REQUIRE(mq8_zero_ok(zero) && mq8_zero_ok(zero_u), WW_E_INVALID, "ww_mq8_stem_fwd: zero points %d / %d outside int8", zero, zero_u);
    WW_REQUIRE(aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(out), WW_E_INVALID,
               "ww_mq8_stem_fwd: weights, vectors and output must be 16-byte aligned");
    const int Ho = mq8_half(F), Wo = mq8_half(T);
    mq8_dw_args a{xq, w, bias, mult, shift, tab, out, (long)B * Ho * Wo * (Cp / 16), F, T, Ho, Wo, Cp, 3, 2, zero, zero_u};
    ww_prof_scope prof(ctx, WW_K_STEM_FWD, (hipStream_t)stream);
    return mq8_launch_dw<MQ_HSWISH, true>(ctx, a, (hipStream_t)stream);
}

extern "C" int ww_mq8_se_fwd(ww_ctx *ctx, const int8_t *in, int B, int HW, int C, int Cp, int Csq, int zero, int pool_mult, int pool_shift,
                             const int8_t *w1, const int32_t *b1, const int32_t *m1, const int32_t *sh1, const int8_t *w2,
                             const int32_t *b2, const int32_t *m2, const int32_t *sh2, int8_t *pool_out, int8_t *h_out, uint8_t *gate_out,
                             ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w1 && b1 && m1 && sh1 && w2 && b2 && m2 && sh2 && pool_out && h_out && gate_out, WW_E_INVALID,
               "ww_mq8_se_fwd: null argument");
    WW_REQUIRE(B >= 1 && HW >= 1 && HW <= (1 << 22), WW_E_INVALID, "ww_mq8_se_fwd: B=%d HW=%d", B, HW);
    WW_REQUIRE(C >= 1 && Cp == q8_pad64(C) && Cp <= MQ_MAX_CP && Csq >= 1 && Csq <= MQ_MAX_SQ, WW_E_INVALID,
               "ww_mq8_se_fwd: C=%d Cp=%d Csq=%d (Cp = C rounded up to 64, at most %d; Csq at most %d)", C, Cp, Csq, MQ_MAX_CP, MQ_MAX_SQ);
    WW_REQUIRE(mq8_zero_ok(zero) && q8_mult_ok(pool_mult, pool_shift), WW_E_INVALID,
               "ww_mq8_se_fwd: zero point %d / multiplier %d / shift %d out of range", zero, pool_mult, pool_shift);
    WW_REQUIRE(aligned16(in) && aligned16(gate_out), WW_E_INVALID, "ww_mq8_se_fwd: the activations and the gate must be 16-byte aligned");
    mq8_se_args a{in, w1, w2, b1, m1, sh1, b2, m2, sh2, pool_out, h_out, gate_out, HW, C, Cp, Csq, zero, pool_mult, pool_shift};
    ww_prof_scope prof(ctx, WW_K_NHWC, (hipStream_t)stream);
    hipLaunchKernelGGL(k_mq8_se, dim3(B), dim3(MQ_BLOCK), 0, (hipStream_t)stream, a);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_mq8_gate_fwd(ww_ctx *ctx, const int8_t *in, const uint8_t *gate, int B, int HW, int Cp, int zero, int gate_mult,
                               int gate_shift, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && gate && out, WW_E_INVALID, "ww_mq8_gate_fwd: null argument");
    WW_REQUIRE(B >= 1 && HW >= 1 && (long)B * HW <= (1l << 31) && Cp >= 16 && Cp % 16 == 0, WW_E_INVALID,
               "ww_mq8_gate_fwd: B=%d HW=%d Cp=%d", B, HW, Cp);
    WW_REQUIRE(mq8_zero_ok(zero) && q8_mult_ok(gate_mult, gate_shift), WW_E_INVALID,
               "ww_mq8_gate_fwd: zero point %d / multiplier %d / shift %d out of range", zero, gate_mult, gate_shift);
    WW_REQUIRE(aligned16(in) && aligned16(gate) && aligned16(out), WW_E_INVALID, "ww_mq8_gate_fwd: tensors must be 16-byte aligned");
    const long nvec = (long)B * HW * (Cp / 16);
    const int grid = ww_capped_grid(ctx, ww_pass_ew(nvec).grid);
    ww_prof_scope prof(ctx, WW_K_NHWC, (hipStream_t)stream);
    hipLaunchKernelGGL(k_mq8_gate, dim3(grid), dim3(MQ_BLOCK), 0, (hipStream_t)stream, in, gate, nvec, HW, Cp, zero, gate_mult, gate_shift,
                       out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_mq8_head_fwd(ww_ctx *ctx, const int8_t *in, int B, int HW, int zero, int pool_mult, int pool_shift, const int8_t *w0,
                               const int32_t *b0, const int32_t *m0, const int32_t *sh0, int zero_u, const int8_t *tab, int zero_h,
                               const int8_t *fc_w, const int32_t *fc_bias, const float *fc_scale, int num_classes, int8_t *pool_out,
                               int8_t *hidden_out, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w0 && b0 && m0 && sh0 && tab && fc_w && fc_bias && fc_scale && pool_out && hidden_out && logits, WW_E_INVALID,
               "ww_mq8_head_fwd: null argument");
    WW_REQUIRE(B >= 1 && HW >= 1 && HW <= (1 << 22), WW_E_INVALID, "ww_mq8_head_fwd: B=%d HW=%d", B, HW);
    WW_REQUIRE(num_classes >= 2 && num_classes <= 64, WW_E_INVALID, "ww_mq8_head_fwd: num_classes=%d outside [2, 64]", num_classes);
    WW_REQUIRE(mq8_zero_ok(zero) && mq8_zero_ok(zero_h) && q8_mult_ok(pool_mult, pool_shift), WW_E_INVALID,
               "ww_mq8_head_fwd: zero points %d / %d, multiplier %d / shift %d out of range", zero, zero_h, pool_mult, pool_shift);
    WW_REQUIRE(aligned16(in) && aligned16(pool_out), WW_E_INVALID, "ww_mq8_head_fwd: the activations must be 16-byte aligned");
    {
        ww_prof_scope prof(ctx, WW_K_GAP_FWD, (hipStream_t)stream);
        hipLaunchKernelGGL(k_mq8_pool, dim3(B), dim3(MQ_BLOCK), 0, (hipStream_t)stream, in, HW, WW_MQ8_LAST, zero, pool_mult, pool_shift,
                           pool_out);
        WW_LAUNCH_CHECK();
    }
    // classifier.0 is a 1x1 conv over the B pooled rows: (B, 576) x (1024, 576)^T on the matrix cores, Hardswish epilogue
    const int rc = ww_mq8_conv1x1_fwd(ctx, pool_out, w0, b0, m0, sh0, B, WW_MQ8_LAST, WW_MQ8_HIDDEN, zero, WW_MQ8_HSWISH, zero_u, tab,
                                      nullptr, 0, 0, nullptr, 0, 0, 0, hidden_out, stream);
    if (rc != WW_OK) return rc;
    ww_prof_scope prof(ctx, WW_K_HEAD_LOSS, (hipStream_t)stream);
    hipLaunchKernelGGL(k_mq8_fc, dim3(B), dim3(MQ_BLOCK), 0, (hipStream_t)stream, hidden_out, WW_MQ8_HIDDEN, zero_h, fc_w, fc_bias, fc_scale,
                       num_classes, logits);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" size_t ww_mq8_mobilenetv3_workspace_bytes(int B, int F, int T) {
    mq8_plan p;
    return mq8_make_plan(B, F, T, &p) ? (size_t)p.total : 0;
}

extern "C" int ww_mq8_mobilenetv3_fwd(ww_ctx *ctx, const void *const *tab, const ww_mq8_io *io, const float *x, int B, int F, int T,
                                      void *ws, size_t ws_bytes, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && tab && io && x && ws && logits, WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: null argument");
    mq8_plan p;
    WW_REQUIRE(mq8_make_plan(B, F, T, &p), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(ws_bytes >= (size_t)p.total, WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: workspace of %zu bytes, need %ld", ws_bytes, p.total);
    WW_REQUIRE(aligned16(ws), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: the workspace must be 16-byte aligned");
    auto i8 = [&](int i) { return (const int8_t *)tab[i]; };
    auto i32 = [&](int i) { return (const int32_t *)tab[i]; };
    auto have = [&](int first, int n) {
        for (int j = first; j < first + n; ++j)
            if (!tab[j]) return false;
        return true;
    };
    int8_t *base = (int8_t *)ws;
    // the two gate forms give the same bits; WW_MQ8_GATE=pass | fused in the environment, read at every launch, picks one (the A/B
    // switch of tools/bench_q8_mobilenetv3.py and the tests).  The default is the pass form: see MQ_GATE_FUSED_DEFAULT.
    const char *gate_form = getenv("WW_MQ8_GATE");
    bool fused = MQ_GATE_FUSED_DEFAULT;
    if (gate_form && !strcmp(gate_form, "fused")) fused = true;
    if (gate_form && !strcmp(gate_form, "pass")) fused = false;
    int rc = ww_q8_quantize(ctx, x, (long)B * F * T, io->in_scale, io->in_zero, base + p.xq, stream);
    if (rc != WW_OK) return rc;
    WW_REQUIRE(have(0, 5), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: a stem table entry is null");
    rc = ww_mq8_stem_fwd(ctx, base + p.xq, i8(0), i32(1), i32(2), i32(3), B, F, T, 64, io->in_zero, io->stem_zu, i8(4), base + p.stem, stream);
    if (rc != WW_OK) return rc;
    const int8_t *cur = base + p.stem;
    int zcur = io->stem_zo;
    for (int i = 0; i < WW_MQ8_BLOCKS; ++i) {
        const mq8_block &c = MQ_CONF[i];
        const int t = 5 + WW_MQ8_BLOCK_NPTR * i, cinp = q8_pad64(c.cin), ep = q8_pad64(c.exp), ntab = c.hs ? 5 : 4;
        const int act = c.hs ? WW_MQ8_HSWISH : WW_MQ8_RELU;
        const int8_t *block_in = cur;
        if (c.exp != c.cin) {
            WW_REQUIRE(have(t, ntab), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: block %d: an expand table entry is null", i);
            rc = ww_mq8_conv1x1_fwd(ctx, cur, i8(t), i32(t + 1), i32(t + 2), i32(t + 3), (long)B * p.Hin[i] * p.Win[i], cinp, ep, zcur, act,
                                    c.hs ? io->exp_zu[i] : 0, c.hs ? i8(t + 4) : nullptr, nullptr, 0, 0, nullptr, 0, 0, 0, base + p.expand[i],
                                    stream);
            if (rc != WW_OK) return rc;
            cur = base + p.expand[i];
            zcur = c.hs ? io->exp_zo[i] : -128;
        }
        WW_REQUIRE(have(t + 5, ntab), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: block %d: a depthwise table entry is null", i);
        rc = ww_mq8_dwconv_fwd(ctx, cur, i8(t + 5), i32(t + 6), i32(t + 7), i32(t + 8), B, p.Hin[i], p.Win[i], ep, c.k, c.stride, zcur, act,
                               c.hs ? io->dw_zu[i] : 0, c.hs ? i8(t + 9) : nullptr, base + p.dw[i], stream);
        if (rc != WW_OK) return rc;
        cur = base + p.dw[i];
        zcur = c.hs ? io->dw_zo[i] : -128;
        const int HW = p.H[i] * p.W[i];
        const uint8_t *gate = nullptr;
        if (c.sq) {
            WW_REQUIRE(have(t + 10, 8), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: block %d: a squeeze-excitation table entry is null", i);
            rc = ww_mq8_se_fwd(ctx, cur, B, HW, c.exp, ep, c.sq, zcur, io->sepool_mult[i], io->sepool_shift[i], i8(t + 10), i32(t + 11),
                               i32(t + 12), i32(t + 13), i8(t + 14), i32(t + 15), i32(t + 16), i32(t + 17), base + p.sepool[i],
                               base + p.h[i], (uint8_t *)(base + p.gate[i]), stream);
            if (rc != WW_OK) return rc;
            if (fused) {
                gate = (const uint8_t *)(base + p.gate[i]);           // the projection conv gates its own pixel fragments: no y tensor
            } else {
                rc = ww_mq8_gate_fwd(ctx, cur, (const uint8_t *)(base + p.gate[i]), B, HW, ep, zcur, io->gate_mult[i], io->gate_shift[i],
                                     base + p.y[i], stream);
                if (rc != WW_OK) return rc;
                cur = base + p.y[i];
            }
        }
        WW_REQUIRE(have(t + 18, 4), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: block %d: a projection table entry is null", i);
        const bool res = c.stride == 1 && c.cin == c.cout;
        rc = ww_mq8_conv1x1_fwd(ctx, cur, i8(t + 18), i32(t + 19), i32(t + 20), i32(t + 21), (long)B * HW, ep, q8_pad64(c.cout), zcur,
                                WW_MQ8_SIGNED, 0, nullptr, res ? block_in : nullptr, io->res_mult[i], io->res_shift[i], gate, HW,
                                io->gate_mult[i], io->gate_shift[i], base + p.out[i], stream);
        if (rc != WW_OK) return rc;
        cur = base + p.out[i];
        zcur = 0;
    }
    const int t = 5 + WW_MQ8_BLOCK_NPTR * WW_MQ8_BLOCKS, HW = p.H[WW_MQ8_BLOCKS - 1] * p.W[WW_MQ8_BLOCKS - 1];
    WW_REQUIRE(have(t, 13), WW_E_INVALID, "ww_mq8_mobilenetv3_fwd: a table entry of the last conv or the head is null");
    rc = ww_mq8_conv1x1_fwd(ctx, cur, i8(t), i32(t + 1), i32(t + 2), i32(t + 3), (long)B * HW, 128, WW_MQ8_LAST, 0, WW_MQ8_HSWISH,
                            io->last_zu, i8(t + 4), nullptr, 0, 0, nullptr, 0, 0, 0, base + p.last, stream);
    if (rc != WW_OK) return rc;
    return ww_mq8_head_fwd(ctx, base + p.last, B, HW, io->last_zo, io->pool_mult, io->pool_shift, i8(t + 5), i32(t + 6), i32(t + 7),
                           i32(t + 8), io->cls_zu, i8(t + 9), io->cls_zo, i8(t + 10), i32(t + 11), (const float *)tab[t + 12],
                           io->num_classes, base + p.pool, base + p.hidden, logits, stream);
}

// Integer-only inference of an exported int8 ResNet18Wakeword bundle (DESIGN.md "Export", the int8 law, subsection "ResNet18").
//   k_rq8_stem    : 7x7 s2 p3, 1 -> 64 channels, on the matrix pipe: the 49-tap window padded to 64 is one K chunk
//   k_rq8_maxpool : 3x3 s2 p1 maximum over the window positions inside the image; nothing is rounded
//   the conv      : dense k x k (k = 1, 3), stride 1 or 2, pad k / 2 Conv2d as an implicit GEMM, the RqPixel geometry of the int8
//                   tap-GEMM core (ww_q8_tap_gemm.h: the lane map, the row tiles, the LDS weight slab), with one of three epilogues:
//                       RELU   out = clamp(-128 + R(acc), -128, 127)            (z_out = -128)
//                       SIGNED out = clamp(R(acc), -128, 127)                   (z_out = 0: the downsample)
//                       ADD    out = clamp(-128 + R(acc) + R(res - z_res, m_r, sh_r), -128, 127)   (conv2)
// Quantisation is ww_q8_quantize, pooling and the classifier are ww_tq8_pool_fc_fwd (T = H W, C = Cp = 512).
// Activations are int8 NHWC (B,H,W,C), C a multiple of 64: a pixel's channels are whole 64-deep K chunks of the instruction.
//
// The pixel index is per row, so a 16-row tile may span images.  A wave holds RT tiles of 16 rows at once (RT = 4, or 1 for
// launches with few rows, so that the (row group x channel tile) grid still fills the machine).  The weights of a channel tile
// (64 k k Cin bytes, re-laid (Cout, k k, Cin) by the host) are held in LDS or streamed through L2; WW_RQ8_WEIGHTS=stream | lds in
// the environment forces one form (lds: wherever the tile fits LDS).
//
// bias arguments are the EFFECTIVE bias q_b - z_in * sum(q_w) (host, once per bundle), so "a source pixel outside the image" and
// "a row past the end" are both a vector of z_in bytes.  All adds that may wrap are unsigned.
#include "ww_q8_tap_gemm.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int RQ_BLOCK = 256;
constexpr int RQ_WAVES = RQ_BLOCK / 64;
// the largest weight image of a channel tile held in LDS by default is the largest that fits (Cin = 256 at k = 3): measured per
// launch (profiles/q8_resnet18_measured.txt), the LDS form is the faster one at every shape of the model whose tile fits, the
// one-workgroup-a-CU 144 KB tiles of stage 3 included
constexpr size_t RQ_SLAB_DEFAULT = Q8T_SLAB_FITS;
constexpr long RQ_RT4_ITEMS = 1024;            // 64-row items from which a wave takes 64 rows: one per SIMD of the machine (256 CUs x 4)
enum { RQ_RELU = 0, RQ_SIGNED = 1, RQ_ADD = 2 };

// row n = output pixel (b, ho, wo) of (B,Ho,Wo); tap j = (kh, kw) reads pixel (ho s - p + kh, wo s - p + kw) of image b of
// (B,H,W,Cin), or the zero point where that pixel lies outside the image
struct RqPixel {
    const int8_t *in;
    long N;
    int H, W, Ho, Wo, Cin, k, stride, zfill;
    struct Row { long n, img; int h0, w0; };   // the window's first source pixel; a row past the end has none inside the image
    struct Src { const int8_t *p; bool live; };
    __device__ int nseg() const { return k * k; }
    __device__ int K() const { return Cin; }
    __device__ void row(long n, Row &r) const {
        const int pad = k / 2;
        const long b = n / ((long)Ho * Wo);
        const int rem = (int)(n - b * Ho * Wo);
        const bool ok = n < N;
        r.n = n;
        r.img = b * H;
        r.h0 = ok ? rem / Wo * stride - pad : -(1 << 20);
        r.w0 = ok ? rem % Wo * stride - pad : -(1 << 20);
    }
    __device__ void seg(const Row &r, int j, int g, Src &s) const {
        const int kh = j / k, kw = j - kh * k;
        const int hi = r.h0 + kh, wi = r.w0 + kw;
        s.live = hi >= 0 && hi < H && wi >= 0 && wi < W;
        s.p = in + ((r.img + hi) * W + wi) * Cin + 16 * g;      // dereferenced only where live
    }
    __device__ v4i load(const Src &s, int kc) const {
        v4i bq = {zfill, zfill, zfill, zfill};
        if (s.live) bq = *(const v4i *)(s.p + 64 * kc);
        return bq;
    }
};

template <int EP> struct RqEpi : Q8Chan {
    const int8_t *res;                         // ADD: the residual tensor (N, Cout)
    int8_t *out;                               // (N, Cout), N = B Ho Wo
    int res_zero, res_m, res_sh;
    __device__ void store(const v4i (&acc)[4], long n, int c0) const {
        v4i hv = {0, 0, 0, 0};
        if (EP == RQ_ADD) hv = *(const v4i *)(res + n * Cout + c0);
        q8_tap_store(*this, acc, hv, out, n, c0, [&](long long v, int h) {
            if (EP == RQ_ADD) v += q8_round(h - res_zero, res_m, res_sh);
            return EP == RQ_SIGNED ? q8_clamp_signed(v) : q8_clamp(v);
        });
    }
};

// The stem on the matrix pipe: a pixel's 49-byte window, padded to 64, is exactly one K chunk.  Persistent over 16-pixel tiles, one
// per wave and trip, under the conv kernel's lane map: lane l gathers the taps [16 g, 16 g + 16) of the window of pixel l & 15 --
// the input's zero point where the tap lies outside the image, anything (here 0) for the pad taps 49..63, whose weights are zero --
// and holds the 64 x 64 weights' four fragments for its life.  w is (64, 64) [channel][tap], tap = kh 7 + kw.
__global__ __launch_bounds__(RQ_BLOCK) void k_rq8_stem(const int8_t *__restrict__ xq, const int8_t *__restrict__ w,
                                                       const int *__restrict__ bias, const int *__restrict__ mult,
                                                       const int *__restrict__ shift, int F, int T, int Ho, int Wo, long N, int zero,
                                                       int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, g = lane >> 4;
    v4i wa[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) wa[m] = *(const v4i *)(w + (16 * (p >> 2) + 4 * m + (p & 3)) * 64 + 16 * g);
    const long tiles = (N + 15) / 16;
    for (long tile = (long)blockIdx.x * RQ_WAVES + (threadIdx.x >> 6); tile < tiles; tile += (long)gridDim.x * RQ_WAVES) {
        const long n = tile * 16 + p;
        const bool ok = n < N;
        const long b = n / ((long)Ho * Wo);
        const int rem = (int)(n - b * Ho * Wo);
        const int h0 = rem / Wo * 2 - 3, w0 = rem % Wo * 2 - 3;
        const int8_t *img = xq + b * F * T;
        v4i bq;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tap = 16 * g + 4 * d + e, kh = tap / 7, kw = tap - 7 * kh;
                const int hi = h0 + kh, wi = w0 + kw;
                q[e] = tap < 49 ? zero : 0;
                if (ok && tap < 49 && hi >= 0 && hi < F && wi >= 0 && wi < T) q[e] = img[(long)hi * T + wi];
            }
            bq[d] = q8_pack4(q[0], q[1], q[2], q[3]);
        }
        v4i acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[m], bq, v4i{0, 0, 0, 0}, 0, 0, 0);
        if (!ok) continue;
        v4i ov;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const v4i bb = *(const v4i *)(bias + 16 * g + 4 * m);
            const v4i mu = *(const v4i *)(mult + 16 * g + 4 * m);
            const v4i sh = *(const v4i *)(shift + 16 * g + 4 * m);
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = q8_clamp(q8_round((int)((unsigned)acc[m][e] + (unsigned)bb[e]), mu[e], sh[e]));
            ov[m] = q8_pack4(q[0], q[1], q[2], q[3]);
        }
        *(v4i *)(out + n * 64 + 16 * g) = ov;
    }
}

// one thread per (output pixel, 16 channels): the maximum over the window positions inside the image (there is always one)
__global__ __launch_bounds__(RQ_BLOCK) void k_rq8_maxpool(const int8_t *__restrict__ in, int H, int W, int Ho, int Wo, int C, long nvec,
                                                          int8_t *__restrict__ out) {
    const int cv = C / 16;
    for (long i = (long)blockIdx.x * RQ_BLOCK + threadIdx.x; i < nvec; i += (long)gridDim.x * RQ_BLOCK) {
        const int v = (int)(i % cv);
        const long pix = i / cv;
        const long b = pix / ((long)Ho * Wo);
        const int rem = (int)(pix - b * Ho * Wo);
        const int h0 = rem / Wo * 2 - 1, w0 = rem % Wo * 2 - 1;
        int best[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) best[e] = -128;
        for (int kh = 0; kh < 3; ++kh) {
            const int hi = h0 + kh;
            if (hi < 0 || hi >= H) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int wi = w0 + kw;
                if (wi < 0 || wi >= W) continue;
                const v4i x = *(const v4i *)(in + ((b * H + hi) * W + wi) * C + 16 * v);
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    int q[4];
                    q8_unpack4(x[d], q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) best[4 * d + e] = q[e] > best[4 * d + e] ? q[e] : best[4 * d + e];
                }
            }
        }
        v4i o;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = q8_pack4(best[4 * d], best[4 * d + 1], best[4 * d + 2], best[4 * d + 3]);
        *(v4i *)(out + pix * C + 16 * v) = o;
    }
}

inline int rq8_half(int n) { return (n - 1) / 2 + 1; }          // floor((n + 2 p - k) / 2) + 1 for (k, p) = (7, 3), (3, 1), (1, 0)

template <int EP>
int rq8_launch_rt(ww_ctx *ctx, const RqPixel &geo, const RqEpi<EP> &epi, const int8_t *w, bool lds, size_t slab, hipStream_t st) {
    // 64-row groups x channel tiles are the waves' work items: below one per SIMD of the machine a wave takes 16 rows, so that four
    // times as many waves share the launch (measured per launch: 16 rows win at every shape below the threshold, 64 rows at or
    // above it except two stride-2 convs by 5 and 12 %).  WW_RQ8_ROWTILE=1 | 4 in the environment forces one: the tests' shapes are
    // all below the threshold.
    const long items4 = (geo.N + 63) / 64 * (epi.Cout / 64);
    const char *rt = getenv("WW_RQ8_ROWTILE");
    bool small = items4 < RQ_RT4_ITEMS;
    if (rt && !strcmp(rt, "1")) small = true;
    if (rt && !strcmp(rt, "4")) small = false;
    return small ? q8_tap_launch<RqPixel, RqEpi<EP>, 1>(ctx, geo, epi, w, lds, slab, st)
                 : q8_tap_launch<RqPixel, RqEpi<EP>, 4>(ctx, geo, epi, w, lds, slab, st);
}

}  // namespace

extern "C" int ww_rq8_conv2d_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                                 const int32_t *shift, int B, int H, int W, int Cin, int Cout, int k, int stride, int zero,
                                 int epilogue, const int8_t *residual, int res_zero, int res_mult, int res_shift, int8_t *out,
                                 ww_stream_t stream) {
    WW_REQUIRE(ctx && in && w && bias && mult && shift && out, WW_E_INVALID, "ww_rq8_conv2d_fwd: null argument");
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= (1l << 31), WW_E_INVALID, "ww_rq8_conv2d_fwd: B=%d H=%d W=%d", B, H, W);
    WW_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cout >= 64 && Cout % 64 == 0 && Cin <= 4096 && Cout <= 4096, WW_E_INVALID,
               "ww_rq8_conv2d_fwd: channel counts %d -> %d must be multiples of 64 (at most 4096)", Cin, Cout);
    WW_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), WW_E_INVALID, "ww_rq8_conv2d_fwd: k=%d stride=%d", k, stride);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_rq8_conv2d_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(epilogue == WW_RQ8_RELU || epilogue == WW_RQ8_SIGNED || epilogue == WW_RQ8_ADD, WW_E_INVALID,
               "ww_rq8_conv2d_fwd: epilogue %d", epilogue);
    WW_REQUIRE((epilogue == WW_RQ8_ADD) == (residual != nullptr), WW_E_INVALID,
               "ww_rq8_conv2d_fwd: the add epilogue, and only it, takes a residual tensor");
    WW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(out) &&
               aligned16(residual), WW_E_INVALID, "ww_rq8_conv2d_fwd: tensors must be 16-byte aligned");
    WW_REQUIRE(in != out && residual != out, WW_E_INVALID, "ww_rq8_conv2d_fwd: in place");
    WW_REQUIRE(!residual || (q8_mult_ok(res_mult, res_shift) && res_zero >= -128 && res_zero <= 127), WW_E_INVALID,
               "ww_rq8_conv2d_fwd: residual multiplier %d / shift %d / zero point %d out of range", res_mult, res_shift, res_zero);
    const int Ho = stride == 2 ? rq8_half(H) : H, Wo = stride == 2 ? rq8_half(W) : W;
    const long N = (long)B * Ho * Wo;
    const RqPixel geo{in, N, H, W, Ho, Wo, Cin, k, stride, (zero & 255) * 0x01010101};
    const Q8Chan chan{bias, mult, shift, Cout};
    ww_prof_scope prof(ctx, WW_K_PW_FWD, (hipStream_t)stream);
    // One channel tile's weights are 64 k k Cin bytes.  Up to RQ_SLAB_DEFAULT they are held in LDS, beyond it streamed; the
    // environment's WW_RQ8_WEIGHTS (the A/B switch of tools/bench_q8_resnet18.py and the tests) forces a form.
    const size_t slab = (size_t)64 * k * k * Cin;
    const char *mode = getenv("WW_RQ8_WEIGHTS");
    bool lds = slab <= RQ_SLAB_DEFAULT;
    if (mode && !strcmp(mode, "stream")) lds = false;
    if (mode && !strcmp(mode, "lds")) lds = slab <= Q8T_SLAB_FITS;
    hipStream_t st = (hipStream_t)stream;
    if (epilogue == WW_RQ8_RELU) return rq8_launch_rt<RQ_RELU>(ctx, geo, {chan, residual, out, res_zero, res_mult, res_shift}, w, lds, slab, st);
    if (epilogue == WW_RQ8_SIGNED) return rq8_launch_rt<RQ_SIGNED>(ctx, geo, {chan, residual, out, res_zero, res_mult, res_shift}, w, lds, slab, st);
    return rq8_launch_rt<RQ_ADD>(ctx, geo, {chan, residual, out, res_zero, res_mult, res_shift}, w, lds, slab, st);
}

extern "C" int ww_rq8_stem_fwd(ww_ctx *ctx, const int8_t *xq, const int8_t *w, const int32_t *bias, const int32_t *mult,
                               const int32_t *shift, int B, int F, int T, int zero, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && xq && w && bias && mult && shift && out, WW_E_INVALID, "ww_rq8_stem_fwd: null argument");
    WW_REQUIRE(B >= 1 && F >= 1 && T >= 1 && (long)B * F * T <= (1l << 40), WW_E_INVALID, "ww_rq8_stem_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(zero >= -128 && zero <= 127, WW_E_INVALID, "ww_rq8_stem_fwd: zero point %d outside int8", zero);
    WW_REQUIRE(aligned16(w) && aligned16(bias) && aligned16(mult) && aligned16(shift) && aligned16(out), WW_E_INVALID,
               "ww_rq8_stem_fwd: weights, vectors and output must be 16-byte aligned");
    const int Ho = rq8_half(F), Wo = rq8_half(T);
    const long N = (long)B * Ho * Wo, tiles = (N + 15) / 16;
    const int grid = ww_conv_grid(ctx, (const void *)k_rq8_stem, RQ_BLOCK, 0, (tiles + RQ_WAVES - 1) / RQ_WAVES, 1 << 20);
    ww_prof_scope prof(ctx, WW_K_STEM_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_rq8_stem, dim3(grid), dim3(RQ_BLOCK), 0, (hipStream_t)stream, xq, w, bias, mult, shift, F, T, Ho, Wo, N, zero,
                       out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_rq8_maxpool_fwd(ww_ctx *ctx, const int8_t *in, int B, int H, int W, int C, int8_t *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && in && out, WW_E_INVALID, "ww_rq8_maxpool_fwd: null argument");
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 16 && C % 16 == 0, WW_E_INVALID, "ww_rq8_maxpool_fwd: B=%d H=%d W=%d C=%d", B, H, W, C);
    WW_REQUIRE(aligned16(in) && aligned16(out) && in != out, WW_E_INVALID, "ww_rq8_maxpool_fwd: tensors must be 16-byte aligned, not in place");
    const int Ho = rq8_half(H), Wo = rq8_half(W);
    const long nvec = (long)B * Ho * Wo * (C / 16);
    const int grid = ww_capped_grid(ctx, ww_pass_ew(nvec).grid);
    hipLaunchKernelGGL(k_rq8_maxpool, dim3(grid), dim3(RQ_BLOCK), 0, (hipStream_t)stream, in, H, W, Ho, Wo, C, nvec, out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

namespace {
struct rq8_plan {                              // byte offsets of every stage tensor in the workspace, and the stage sizes
    long xq, stem, pool0, h1[8], ds[8], out[8], pool, total;
    int H[6], W[6];                            // 0: stem output, 1: after the max pool = stage 1, 2..4: stages 2..4
};
const int RQ_PLANES[4] = {64, 128, 256, 512};

bool rq8_make_plan(int B, int F, int T, rq8_plan *p) {
    if (B < 1 || F < 1 || T < 1 || (long)B * F * T > (1l << 31)) return false;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += q8_round256(bytes); return at; };
    p->H[0] = rq8_half(F); p->W[0] = rq8_half(T);
    p->H[1] = rq8_half(p->H[0]); p->W[1] = rq8_half(p->W[0]);
    for (int s = 1; s < 4; ++s) { p->H[s + 1] = rq8_half(p->H[s]); p->W[s + 1] = rq8_half(p->W[s]); }
    p->xq = take((long)B * F * T);
    p->stem = take((long)B * p->H[0] * p->W[0] * 64);
    p->pool0 = take((long)B * p->H[1] * p->W[1] * 64);
    for (int i = 0; i < 8; ++i) {
        const int s = i / 2;
        const long act = (long)B * p->H[s + 1] * p->W[s + 1] * RQ_PLANES[s];
        p->h1[i] = take(act);
        p->ds[i] = (s > 0 && i % 2 == 0) ? take(act) : -1;
        p->out[i] = take(act);
    }
    p->pool = take((long)B * 512);
    p->total = off;
    return true;
}
}  // namespace

extern "C" size_t ww_rq8_resnet18_workspace_bytes(int B, int F, int T) {
    rq8_plan p;
    return rq8_make_plan(B, F, T, &p) ? (size_t)p.total : 0;
}

extern "C" int ww_rq8_resnet18_fwd(ww_ctx *ctx, const void *const *tab, const ww_rq8_io *io, const float *x, int B, int F, int T,
                                   void *ws, size_t ws_bytes, float *logits, ww_stream_t stream) {
    WW_REQUIRE(ctx && tab && io && x && ws && logits, WW_E_INVALID, "ww_rq8_resnet18_fwd: null argument");
    rq8_plan p;
    WW_REQUIRE(rq8_make_plan(B, F, T, &p), WW_E_INVALID, "ww_rq8_resnet18_fwd: B=%d F=%d T=%d", B, F, T);
    WW_REQUIRE(ws_bytes >= (size_t)p.total, WW_E_INVALID, "ww_rq8_resnet18_fwd: workspace of %zu bytes, need %ld", ws_bytes, p.total);
    WW_REQUIRE(aligned16(ws), WW_E_INVALID, "ww_rq8_resnet18_fwd: the workspace must be 16-byte aligned");
    for (int j = 0; j < WW_RQ8_NPTR; ++j) {
        const int blk = (j - 4) / 12, down = j >= 4 && j < 100 && (j - 4) % 12 >= 8;
        const bool optional = down && !(blk >= 2 && blk % 2 == 0);
        WW_REQUIRE(optional ? !tab[j] : tab[j] != nullptr, WW_E_INVALID, "ww_rq8_resnet18_fwd: table entry %d is %s", j,
                   optional ? "not null" : "null");
    }
    auto i8 = [&](int i) { return (const int8_t *)tab[i]; };
    auto i32 = [&](int i) { return (const int32_t *)tab[i]; };
    int8_t *base = (int8_t *)ws;
    int rc = ww_q8_quantize(ctx, x, (long)B * F * T, io->in_scale, io->in_zero, base + p.xq, stream);
    if (rc != WW_OK) return rc;
    rc = ww_rq8_stem_fwd(ctx, base + p.xq, i8(0), i32(1), i32(2), i32(3), B, F, T, io->in_zero, base + p.stem, stream);
    if (rc != WW_OK) return rc;
    rc = ww_rq8_maxpool_fwd(ctx, base + p.stem, B, p.H[0], p.W[0], 64, base + p.pool0, stream);
    if (rc != WW_OK) return rc;
    const int8_t *cur = base + p.pool0;
    int cin = 64;
    for (int i = 0; i < 8; ++i) {
        const int s = i / 2, t = 4 + 12 * i, planes = RQ_PLANES[s];
        const bool down = p.ds[i] >= 0;
        const int stride = down ? 2 : 1;
        const int Hin = down ? p.H[s] : p.H[s + 1], Win = down ? p.W[s] : p.W[s + 1];
        int8_t *h1 = base + p.h1[i], *out = base + p.out[i];
        rc = ww_rq8_conv2d_fwd(ctx, cur, i8(t), i32(t + 1), i32(t + 2), i32(t + 3), B, Hin, Win, cin, planes, 3, stride, -128, WW_RQ8_RELU,
                               nullptr, 0, 0, 0, h1, stream);
        if (rc != WW_OK) return rc;
        const int8_t *res = cur;
        int res_zero = -128;
        if (down) {
            int8_t *ds = base + p.ds[i];
            rc = ww_rq8_conv2d_fwd(ctx, cur, i8(t + 8), i32(t + 9), i32(t + 10), i32(t + 11), B, Hin, Win, cin, planes, 1, 2, -128,
                                   WW_RQ8_SIGNED, nullptr, 0, 0, 0, ds, stream);
            if (rc != WW_OK) return rc;
            res = ds;
            res_zero = 0;
        }
        rc = ww_rq8_conv2d_fwd(ctx, h1, i8(t + 4), i32(t + 5), i32(t + 6), i32(t + 7), B, p.H[s + 1], p.W[s + 1], planes, planes, 3, 1,
                               -128, WW_RQ8_ADD, res, res_zero, io->res_mult[i], io->res_shift[i], out, stream);
        if (rc != WW_OK) return rc;
        cur = out;
        cin = planes;
    }
    return ww_tq8_pool_fc_fwd(ctx, cur, B, p.H[4] * p.W[4], 512, 512, io->pool_mult, io->pool_shift, i8(100), i32(101),
                              (const float *)tab[102], io->num_classes, base + p.pool, logits, stream);
}

// Dense k x k Conv2d on the matrix cores, the one-channel k x k stem and MaxPool2d(3, 2, 1): the layers ResNet18Wakeword is made of
// (torchvision's resnet18 with the reference's Conv2d(1, 64, 7, 2, 3) in front).  Channels-last, bias-free, padding p = k / 2:
//   fwd : y[b,ho,wo,n]  = sum_{r,s,c} x[b, ho st + r - p, wo st + s - p, c] w[n,c,r,s]      (pixels outside the image read as 0)
//   dX  : dx[b,hi,wi,c] = sum_{r,s,n} dy[b, (hi + p - r) / st, (wi + p - s) / st, n] w[n,c,r,s]   (exact quotients in range only)
//   dW  : dw[n,c,r,s]   = sum_{b,ho,wo} dy[b,ho,wo,n] x[b, ho st + r - p, wo st + s - p, c]
// The three products are the tap GEMM of ww_tap_gemm.h with the geometry of an image: an implicit GEMM whose M is the pixels of the
// tensor being written and whose k*k K-segments (the taps, r k + s) read the displaced pixels of the tensor being read -- taken only
// while the displaced (h, w) stays inside the row's own image, so an M tile that spans image rows or samples never reads a
// neighbour as "padding".  No patch matrix exists in memory.  The stages' sums are added per tap and the taps at the end
// (SumBlocked); the rows kernel has no epilogue.  The partial products of the dW pixel ranges are summed in a fixed order (or
// queued with ww_defer).
#include "ww_tap_gemm.h"

namespace {

// ---- the image.  m = (b, oh, ow) on the (OH, OW) grid of the tensor being written, A lies on the (SH, SW) grid of the tensor read.
//   DX == false: src = (b, oh st + r - p, ow st + s - p)                    -- the forward product (A = x, C = y)
//   DX == true : src = (b, (oh + p - r) / st, (ow + p - s) / st), exact only -- the input gradient (A = dy, C = dx)
// A row without a source in its own image contributes 0; a dx pixel no output read is therefore WRITTEN as 0.
constexpr int NO_ROW = -(1 << 24);       // "oh" of a row past M: every bounds test below fails on it
struct ImageTap { int tr, ts; };           // (r, s) of segment r k + s
template <bool DX>
struct ImageRows {
    typedef ImageTap Tap;
    struct Row { int oh, ow, img; };     // img = b SH SW: the first source pixel of the row's own image
    int OH, OW, SH, SW, k, stride, pad;
    __device__ Row row(long m, int M) const {
        if (m >= M) return Row{NO_ROW, 0, 0};
        const unsigned per = (unsigned)OH * OW, um = (unsigned)m, b = um / per, rem = um - b * per;
        const int oh = (int)(rem / (unsigned)OW);
        return Row{oh, (int)(rem - (unsigned)oh * OW), (int)b * SH * SW};
    }
    __device__ Tap tap(int seg) const { const int tr = seg / k; return Tap{tr, seg - tr * k}; }
    __device__ bool src(const Row &p, long, Tap t, long &at) const {
        const int tr = t.tr, ts = t.ts, sh1 = stride - 1;                 // stride 1 | 2: a shift by 0 | 1
        int sh, sw;
        bool ok;
        if constexpr (DX) {
            const int th = p.oh + pad - tr, tw = p.ow + pad - ts;
            sh = th >> sh1; sw = tw >> sh1;
            ok = th >= 0 && tw >= 0 && ((th | tw) & sh1) == 0 && sh < SH && sw < SW;
        } else {
            sh = p.oh * stride + tr - pad; sw = p.ow * stride + ts - pad;
            ok = sh >= 0 && sh < SH && sw >= 0 && sw < SW;
        }
        at = (long)p.img + sh * SW + sw;
        return ok;
    }
};
// dW: the output pixel m = (b, ho, wo) of dy meets the source pixel of the forward product
struct ImageDw {
    int Ho, Wo, H, W, k, stride, pad;
    typedef ImageTap Tap;
    __device__ Tap tap(int seg) const { const int tr = seg / k; return Tap{tr, seg - tr * k}; }
    __device__ bool src(int m, Tap t, long &at) const {
        const int tr = t.tr, ts = t.ts, sh1 = stride - 1;
        const unsigned per = (unsigned)Ho * Wo, um = (unsigned)m, b = um / per, rem = um - b * per, ho = rem / (unsigned)Wo, wo = rem - ho * Wo;
        const int hi = ((int)ho << sh1) + tr - pad, wi = ((int)wo << sh1) + ts - pad;
        at = ((long)b * H + hi) * W + wi;
        return hi >= 0 && hi < H && wi >= 0 && wi < W;
    }
};
template <bool DX> using RowArgs = RowsArgs<ImageRows<DX>, EpiNone>;      // {A, W, C, {}, M, CA, N, nseg, accumulate, {OH, OW, SH, SW, k, stride, pad}}

// ---- the one-channel stem, a direct convolution: x (B,H,W), w (C,1,k,k) -> y (B,Ho,Wo,C).  Threads = (pixel lane, channel quad);
// the weights sit in LDS as [tap][channel], so a pixel lane's quads read neighbouring float4s and the image sample is a broadcast.
struct StemArgs { int B, H, W, C, k, stride, pad, Ho, Wo; };
constexpr int STEM_W_MAX = 128 * 49;
__global__ __launch_bounds__(256) void k_conv2d_stem_fwd(const float *__restrict__ x, const float *__restrict__ w, StemArgs g,
                                                         float *__restrict__ y) {
    __shared__ __align__(16) float wl[STEM_W_MAX];
    const int kk = g.k * g.k;
    for (int i = threadIdx.x; i < g.C * kk; i += 256) {
        const int c = i / kk, t = i - c * kk;
        wl[t * g.C + c] = w[i];
    }
    __syncthreads();
    const int C4 = g.C >> 2, cq = threadIdx.x % C4, lane = threadIdx.x / C4, L = 256 / C4;
    if (lane >= L) return;
    const unsigned P = (unsigned)g.B * g.Ho * g.Wo, per = (unsigned)g.Ho * g.Wo;
    for (unsigned p = blockIdx.x * L + lane; p < P; p += gridDim.x * L) {
        const unsigned b = p / per, rem = p - b * per;
        const int ho = (int)(rem / (unsigned)g.Wo), wo = (int)(rem - (unsigned)ho * g.Wo);
        const float *xb = x + (size_t)b * g.H * g.W;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int tr = 0; tr < g.k; ++tr) {
            const int hi = ho * g.stride + tr - g.pad;
            if (hi < 0 || hi >= g.H) continue;
            for (int ts = 0; ts < g.k; ++ts) {
                const int wi = wo * g.stride + ts - g.pad;
                if (wi < 0 || wi >= g.W) continue;
                const float v = xb[hi * g.W + wi];
                const float4 wq = *reinterpret_cast<const float4 *>(wl + (tr * g.k + ts) * g.C + 4 * cq);
                o.x = fmaf(v, wq.x, o.x); o.y = fmaf(v, wq.y, o.y); o.z = fmaf(v, wq.z, o.z); o.w = fmaf(v, wq.w, o.w);
            }
        }
        *reinterpret_cast<float4 *>(y + (size_t)p * g.C + 4 * cq) = o;
    }
}
// dW of the stem: part[block][c][r][s] = sum over the block's pixels of dy[p][c] x[patch(p, r, s)].  grid = (pixel blocks, k): a
// workgroup takes ONE kernel row r, so a thread carries k <= 7 float4 sums; they meet in LDS in a fixed order.
constexpr int STEM_DW_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_conv2d_stem_dw(const float *__restrict__ x, const float *__restrict__ dy, StemArgs g,
                                                        float *__restrict__ part) {
    __shared__ float red[256][29];
    const int C4 = g.C >> 2, cq = threadIdx.x % C4, lane = threadIdx.x / C4, L = 256 / C4, tr = blockIdx.y;
    const unsigned P = (unsigned)g.B * g.Ho * g.Wo, per = (unsigned)g.Ho * g.Wo;
    float4 acc[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < L)
        for (unsigned p = blockIdx.x * L + lane; p < P; p += gridDim.x * L) {
            const unsigned b = p / per, rem = p - b * per;
            const int ho = (int)(rem / (unsigned)g.Wo), wo = (int)(rem - (unsigned)ho * g.Wo);
            const int hi = ho * g.stride + tr - g.pad;
            if (hi < 0 || hi >= g.H) continue;
            const float4 d = *reinterpret_cast<const float4 *>(dy + (size_t)p * g.C + 4 * cq);
            const float *xr = x + ((size_t)b * g.H + hi) * g.W;
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int wi = wo * g.stride + s - g.pad;
                const float v = (s < g.k && wi >= 0 && wi < g.W) ? xr[wi] : 0.f;
                acc[s].x = fmaf(d.x, v, acc[s].x); acc[s].y = fmaf(d.y, v, acc[s].y);
                acc[s].z = fmaf(d.z, v, acc[s].z); acc[s].w = fmaf(d.w, v, acc[s].w);
            }
        }
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        red[threadIdx.x][4 * s + 0] = acc[s].x; red[threadIdx.x][4 * s + 1] = acc[s].y;
        red[threadIdx.x][4 * s + 2] = acc[s].z; red[threadIdx.x][4 * s + 3] = acc[s].w;
    }
    __syncthreads();
    // C*k outputs of this kernel row, each the fixed-order sum over the L pixel lanes of its channel quad
    for (int o = threadIdx.x; o < g.C * g.k; o += 256) {
        const int c = o / g.k, s = o - c * g.k, q4 = c >> 2, e = c & 3;
        float sum = 0.f;
        for (int q = 0; q < L; ++q) sum += red[q * C4 + q4][4 * s + e];
        part[((size_t)blockIdx.x * g.C + c) * g.k * g.k + tr * g.k + s] = sum;
    }
}

// ---- MaxPool2d(3, 2, 1) on (B,H,W,C): padding never wins; of equal values the FIRST in row-major order holds the maximum (a NaN
// takes it from whatever came before, as torch's max_pool2d has it).  Threads = (output | input pixel, channel quad).
struct PoolArgs { int B, H, W, C, Ho, Wo; };
__device__ __forceinline__ void pool_take(float v, int idx, float &m, int &at) {
    if (v > m || v != v) { m = v; at = idx; }
}
// the window (ho, wo): per channel of the quad its maximum and the flat index hi W + wi where it sits
__device__ __forceinline__ void pool_window(const float *__restrict__ xb, const PoolArgs &g, int ho, int wo, int c, float4 &m, int (&at)[4]) {
    const float ninf = -__builtin_huge_valf();
    m = make_float4(ninf, ninf, ninf, ninf);
    at[0] = at[1] = at[2] = at[3] = -1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int hi = 2 * ho + r - 1;
        if (hi < 0 || hi >= g.H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int wi = 2 * wo + s - 1;
            if (wi < 0 || wi >= g.W) continue;
            const int idx = hi * g.W + wi;
            const float4 v = *reinterpret_cast<const float4 *>(xb + (size_t)idx * g.C + c);
            pool_take(v.x, idx, m.x, at[0]); pool_take(v.y, idx, m.y, at[1]); pool_take(v.z, idx, m.z, at[2]); pool_take(v.w, idx, m.w, at[3]);
        }
    }
}
__global__ __launch_bounds__(256) void k_maxpool_fwd(const float *__restrict__ x, PoolArgs g, float *__restrict__ y) {
    const int C4 = g.C >> 2;
    const long n = (long)g.B * g.Ho * g.Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int cq = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % g.Wo); p /= g.Wo;
        const int ho = (int)(p % g.Ho);
        const long b = p / g.Ho;
        float4 m;
        int at[4];
        pool_window(x + (size_t)b * g.H * g.W * g.C, g, ho, wo, 4 * cq, m, at);
        *reinterpret_cast<float4 *>(y + (size_t)(i / C4) * g.C + 4 * cq) = m;
    }
}
// a gather per INPUT pixel over the (at most 4) windows that contain it, in row-major window order: no atomics
__global__ __launch_bounds__(256) void k_maxpool_bwd(const float *__restrict__ x, const float *__restrict__ dy, PoolArgs g,
                                                     float *__restrict__ dx) {
    const int C4 = g.C >> 2;
    const long n = (long)g.B * g.H * g.W * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int cq = (int)(i % C4);
        long p = i / C4;
        const int wi = (int)(p % g.W); p /= g.W;
        const int hi = (int)(p % g.H);
        const long b = p / g.H;
        const float *xb = x + (size_t)b * g.H * g.W * g.C;
        const int me = hi * g.W + wi;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        // windows with 2 ho - 1 <= hi <= 2 ho + 1
        for (int ho = hi >> 1; ho <= min((hi + 1) >> 1, g.Ho - 1); ++ho)
            for (int wo = wi >> 1; wo <= min((wi + 1) >> 1, g.Wo - 1); ++wo) {
                float4 m;
                int at[4];
                pool_window(xb, g, ho, wo, 4 * cq, m, at);
                const float4 gq = *reinterpret_cast<const float4 *>(dy + (((size_t)b * g.Ho + ho) * g.Wo + wo) * g.C + 4 * cq);
                if (at[0] == me) d.x += gq.x;
                if (at[1] == me) d.y += gq.y;
                if (at[2] == me) d.z += gq.z;
                if (at[3] == me) d.w += gq.w;
            }
        *reinterpret_cast<float4 *>(dx + (size_t)(i / C4) * g.C + 4 * cq) = d;
    }
}

int out_size(int n, int k, int stride) { return (n + 2 * (k / 2) - k) / stride + 1; }

struct Layout { size_t wp, dwp, total; };      // float offsets of the scratch regions
Layout layout(long M, int Cin, int Cout, int k) {
    Layout l;
    l.wp = 0;
    l.dwp = (size_t)k * k * Cin * Cout;
    l.total = l.dwp + (size_t)dw_splits(M, Cin, Cout, k * k) * Cout * Cin * k * k;
    return l;
}
bool shape_ok(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    return B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= 0x7fffffffL && Cin >= 4 && Cout >= 4 && Cin % 4 == 0 && Cout % 4 == 0 &&
           k >= 1 && k <= 7 && (k & 1) && (stride == 1 || stride == 2);
}
int check_shape(const char *who, int mode, int B, int H, int W, int Cin, int Cout, int k, int stride) {
    WW_REQUIRE(mode == WW_ACT_F32 || mode == WW_ACT_BF16 || mode == WW_ACT_F16, WW_E_INVALID, "%s: unknown mode %d", who, mode);
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= 0x7fffffffL, WW_E_INVALID, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    WW_REQUIRE(Cin >= 4 && Cout >= 4 && Cin % 4 == 0 && Cout % 4 == 0, WW_E_INVALID,
               "%s: channel counts must be positive multiples of 4, got Cin=%d Cout=%d", who, Cin, Cout);
    WW_REQUIRE(k >= 1 && k <= 7 && (k & 1), WW_E_INVALID, "%s: kernel_size=%d is not an odd number in 1..7", who, k);
    WW_REQUIRE(stride == 1 || stride == 2, WW_E_INVALID, "%s: stride=%d is not 1 or 2", who, stride);
    return WW_OK;
}
int check_stem(const char *who, int B, int H, int W, int C, int k, int stride, StemArgs *g) {
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1, WW_E_INVALID, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    WW_REQUIRE(C >= 4 && C % 4 == 0 && C <= 128, WW_E_INVALID, "%s: channel count must be a multiple of 4 in 4..128, got C=%d", who, C);
    WW_REQUIRE(k >= 1 && k <= 7 && (k & 1), WW_E_INVALID, "%s: kernel_size=%d is not an odd number in 1..7", who, k);
    WW_REQUIRE(stride == 1 || stride == 2, WW_E_INVALID, "%s: stride=%d is not 1 or 2", who, stride);
    *g = StemArgs{B, H, W, C, k, stride, k / 2, out_size(H, k, stride), out_size(W, k, stride)};
    WW_REQUIRE((long)B * H * W < (1L << 31) && (long)B * g->Ho * g->Wo * C < (1L << 31), WW_E_INVALID,
               "%s: tensor too large for 32-bit indices", who);
    return WW_OK;
}
int stem_blocks(const StemArgs &g, int cap) {
    const long P = (long)g.B * g.Ho * g.Wo;
    const int L = 256 / (g.C / 4);
    return (int)std::max<long>(1, std::min<long>(cap, (P + L - 1) / L));
}
int check_pool(const char *who, int B, int H, int W, int C, PoolArgs *g) {
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, WW_E_INVALID,
               "%s: bad shape B=%d H=%d W=%d C=%d (C must be a positive multiple of 4)", who, B, H, W, C);
    WW_REQUIRE((long)H * W < (1L << 31), WW_E_INVALID, "%s: image too large for 32-bit indices", who);
    *g = PoolArgs{B, H, W, C, (H - 1) / 2 + 1, (W - 1) / 2 + 1};
    return WW_OK;
}

}  // namespace

extern "C" size_t ww_conv2d_scratch_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    if (!shape_ok(B, H, W, Cin, Cout, k, stride)) return 0;
    return layout((long)B * out_size(H, k, stride) * out_size(W, k, stride), Cin, Cout, k).total * sizeof(float);
}

extern "C" int ww_conv2d_fwd(ww_ctx *ctx, int mode, const float *x, const float *w, int B, int H, int W, int Cin, int Cout, int k,
                             int stride, float *y, void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && y && scratch, WW_E_INVALID, "ww_conv2d_fwd: null argument");
    int rc = check_shape("ww_conv2d_fwd", mode, B, H, W, Cin, Cout, k, stride);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y) && al16(scratch), WW_E_INVALID, "ww_conv2d_fwd: tensors must be 16-byte aligned");
    const int Ho = out_size(H, k, stride), Wo = out_size(W, k, stride);
    const long M = (long)B * Ho * Wo;
    WW_REQUIRE(scratch_bytes >= layout(M, Cin, Cout, k).total * sizeof(float), WW_E_WORKSPACE, "ww_conv2d_fwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    float *wp = (float *)scratch;
    hipLaunchKernelGGL(k_tap_pack, dim3(ew_grid((long)k * k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k * k, 0, wp);
    WW_LAUNCH_CHECK();
    const RowArgs<false> a{x, wp, y, {}, (int)M, Cin, Cout, k * k, 0, {Ho, Wo, H, W, k, stride, k / 2}};
    tap_launch_rows<SumBlocked>(mode, a, st);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_conv2d_bwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *dy, int B, int H, int W, int Cin,
                             int Cout, int k, int stride, float *dx, int accumulate_dx, float *dw, void *scratch, size_t scratch_bytes,
                             ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && dy && dw && scratch, WW_E_INVALID, "ww_conv2d_bwd: null argument");
    int rc = check_shape("ww_conv2d_bwd", mode, B, H, W, Cin, Cout, k, stride);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(dy) && al16(dx) && al16(scratch), WW_E_INVALID, "ww_conv2d_bwd: tensors must be 16-byte aligned");
    const int Ho = out_size(H, k, stride), Wo = out_size(W, k, stride), kk = k * k;
    const long M = (long)B * Ho * Wo;
    const Layout l = layout(M, Cin, Cout, k);
    WW_REQUIRE(scratch_bytes >= l.total * sizeof(float), WW_E_WORKSPACE, "ww_conv2d_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    float *base = (float *)scratch;
    if (dx) {
        float *wp = base + l.wp;
        hipLaunchKernelGGL(k_tap_pack, dim3(ew_grid((long)kk * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, kk, 1, wp);
        WW_LAUNCH_CHECK();
        const RowArgs<true> a{dy, wp, dx, {}, (int)((long)B * H * W), Cout, Cin, kk, accumulate_dx != 0, {H, W, Ho, Wo, k, stride, k / 2}};
        tap_launch_rows<SumBlocked>(mode, a, st);
        WW_LAUNCH_CHECK();
    }
    return tap_dw<SumBlocked>(ctx, mode, dy, x, ImageDw{Ho, Wo, H, W, k, stride, k / 2}, M, Cin, Cout, kk, base + l.dwp, dw, st);
}

extern "C" size_t ww_conv2d_stem_scratch_bytes(int C, int k) {
    if (C < 4 || C % 4 || C > 128 || k < 1 || k > 7 || !(k & 1)) return 0;
    return (size_t)STEM_DW_BLOCKS * C * k * k * sizeof(float);
}

extern "C" int ww_conv2d_stem_fwd(ww_ctx *ctx, const float *x, const float *w, int B, int H, int W, int C, int k, int stride, float *y,
                                  ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && y, WW_E_INVALID, "ww_conv2d_stem_fwd: null argument");
    StemArgs g;
    int rc = check_stem("ww_conv2d_stem_fwd", B, H, W, C, k, stride, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(y), WW_E_INVALID, "ww_conv2d_stem_fwd: y must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    hipLaunchKernelGGL(k_conv2d_stem_fwd, dim3(stem_blocks(g, 2048)), dim3(256), 0, st, x, w, g, y);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_conv2d_stem_bwd_dw(ww_ctx *ctx, const float *x, const float *dy, int B, int H, int W, int C, int k, int stride,
                                     float *dw, void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && dy && dw && scratch, WW_E_INVALID, "ww_conv2d_stem_bwd_dw: null argument");
    StemArgs g;
    int rc = check_stem("ww_conv2d_stem_bwd_dw", B, H, W, C, k, stride, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(dy), WW_E_INVALID, "ww_conv2d_stem_bwd_dw: dy must be 16-byte aligned");
    WW_REQUIRE(scratch_bytes >= ww_conv2d_stem_scratch_bytes(C, k), WW_E_WORKSPACE, "ww_conv2d_stem_bwd_dw: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    const int blocks = stem_blocks(g, STEM_DW_BLOCKS);
    const long n = (long)C * k * k;
    float *part = (float *)scratch;
    hipLaunchKernelGGL(k_conv2d_stem_dw, dim3(blocks, k), dim3(256), 0, st, x, dy, g, blocks > 1 ? part : dw);
    WW_LAUNCH_CHECK();
    if (blocks > 1 && !ww_defer(ctx, part, dw, n, blocks, 0)) {
        hipLaunchKernelGGL(k_tap_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, blocks, dw);
        WW_LAUNCH_CHECK();
    }
    return WW_OK;
}

extern "C" int ww_maxpool3x3s2_fwd(ww_ctx *ctx, const float *x, int B, int H, int W, int C, float *y, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && y, WW_E_INVALID, "ww_maxpool3x3s2_fwd: null argument");
    PoolArgs g;
    int rc = check_pool("ww_maxpool3x3s2_fwd", B, H, W, C, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y), WW_E_INVALID, "ww_maxpool3x3s2_fwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    hipLaunchKernelGGL(k_maxpool_fwd, dim3(ew_grid((long)B * g.Ho * g.Wo * (C / 4))), dim3(256), 0, st, x, g, y);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_maxpool3x3s2_bwd(ww_ctx *ctx, const float *x, const float *dy, int B, int H, int W, int C, float *dx,
                                   ww_stream_t stream) {
    WW_REQUIRE(ctx && x && dy && dx, WW_E_INVALID, "ww_maxpool3x3s2_bwd: null argument");
    PoolArgs g;
    int rc = check_pool("ww_maxpool3x3s2_bwd", B, H, W, C, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(dy) && al16(dx), WW_E_INVALID, "ww_maxpool3x3s2_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    hipLaunchKernelGGL(k_maxpool_bwd, dim3(ew_grid((long)B * H * W * (C / 4))), dim3(256), 0, st, x, dy, g, dx);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

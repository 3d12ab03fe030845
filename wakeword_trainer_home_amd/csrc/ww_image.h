// The image geometry of the dense Conv2d tap GEMMs, the one-channel k x k stem and MaxPool2d(3, 2, 1), shared by ww_conv2d.hip (fp32
// activations in HBM) and ww_conv2d16.hip (bf16 / fp16 activations in HBM).  The stem and pool kernels are templated on the
// storage type T of the (B,H,W,C) tensors (ww_act.h): arithmetic is fp32, a value is rounded where it is stored.
#pragma once
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
template <typename T>
__global__ __launch_bounds__(256) void k_conv2d_stem_fwd(const float *__restrict__ x, const float *__restrict__ w, StemArgs g,
                                                         T *__restrict__ y) {
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
        Act<T>::st4(y + (size_t)p * g.C + 4 * cq, o);
    }
}
// dW of the stem: part[block][c][r][s] = sum over the block's pixels of dy[p][c] x[patch(p, r, s)].  grid = (pixel blocks, k): a
// workgroup takes ONE kernel row r, so a thread carries k <= 7 float4 sums; they meet in LDS in a fixed order.
constexpr int STEM_DW_BLOCKS = 256;
template <typename T>
__global__ __launch_bounds__(256) void k_conv2d_stem_dw(const float *__restrict__ x, const T *__restrict__ dy, StemArgs g,
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
            const float4 d = Act<T>::cvt4(Act<T>::ldraw4(dy + (size_t)p * g.C + 4 * cq));
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
template <typename T>
__device__ __forceinline__ void pool_window(const T *__restrict__ xb, const PoolArgs &g, int ho, int wo, int c, float4 &m, int (&at)[4]) {
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
            const float4 v = Act<T>::cvt4(Act<T>::ldraw4(xb + (size_t)idx * g.C + c));
            pool_take(v.x, idx, m.x, at[0]); pool_take(v.y, idx, m.y, at[1]); pool_take(v.z, idx, m.z, at[2]); pool_take(v.w, idx, m.w, at[3]);
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_maxpool_fwd(const T *__restrict__ x, PoolArgs g, T *__restrict__ y) {
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
        Act<T>::st4(y + (size_t)(i / C4) * g.C + 4 * cq, m);
    }
}
// a gather per INPUT pixel over the (at most 4) windows that contain it, in row-major window order: no atomics; the fp32 sum is
// rounded once, where it is stored
template <typename T>
__global__ __launch_bounds__(256) void k_maxpool_bwd(const T *__restrict__ x, const T *__restrict__ dy, PoolArgs g,
                                                     T *__restrict__ dx) {
    const int C4 = g.C >> 2;
    const long n = (long)g.B * g.H * g.W * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int cq = (int)(i % C4);
        long p = i / C4;
        const int wi = (int)(p % g.W); p /= g.W;
        const int hi = (int)(p % g.H);
        const long b = p / g.H;
        const T *xb = x + (size_t)b * g.H * g.W * g.C;
        const int me = hi * g.W + wi;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        // windows with 2 ho - 1 <= hi <= 2 ho + 1
        for (int ho = hi >> 1; ho <= min((hi + 1) >> 1, g.Ho - 1); ++ho)
            for (int wo = wi >> 1; wo <= min((wi + 1) >> 1, g.Wo - 1); ++wo) {
                float4 m;
                int at[4];
                pool_window(xb, g, ho, wo, 4 * cq, m, at);
                const float4 gq = Act<T>::cvt4(Act<T>::ldraw4(dy + (((size_t)b * g.Ho + ho) * g.Wo + wo) * g.C + 4 * cq));
                if (at[0] == me) d.x += gq.x;
                if (at[1] == me) d.y += gq.y;
                if (at[2] == me) d.z += gq.z;
                if (at[3] == me) d.w += gq.w;
            }
        Act<T>::st4(dx + (size_t)(i / C4) * g.C + 4 * cq, d);
    }
}

int out_size(int n, int k, int stride) { return (n + 2 * (k / 2) - k) / stride + 1; }

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

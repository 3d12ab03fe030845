// Dense k x k Conv2d on the matrix cores, the one-channel k x k stem and MaxPool2d(3, 2, 1): the layers ResNet18Wakeword is made of
// (torchvision's resnet18 with the reference's Conv2d(1, 64, 7, 2, 3) in front).  Channels-last, bias-free, padding p = k / 2:
//   fwd : y[b,ho,wo,n]  = sum_{r,s,c} x[b, ho st + r - p, wo st + s - p, c] w[n,c,r,s]      (pixels outside the image read as 0)
//   dX  : dx[b,hi,wi,c] = sum_{r,s,n} dy[b, (hi + p - r) / st, (wi + p - s) / st, n] w[n,c,r,s]   (exact quotients in range only)
//   dW  : dw[n,c,r,s]   = sum_{b,ho,wo} dy[b,ho,wo,n] x[b, ho st + r - p, wo st + s - p, c]
// fwd and dX are one implicit GEMM (k_conv2d_rows): M = the pixels of the tensor being written, k*k K-segments (the taps) whose A
// rows are the displaced pixels of the tensor being read -- taken only while the displaced (h, w) stays inside the row's own image,
// so an M tile that spans image rows or samples never reads a neighbour as "padding".  No patch matrix exists in memory.  The
// weights are first re-laid per tap (k_conv2d_pack: nn.Conv2d's (Cout,Cin,k,k) has the tap as its fastest index).  dW
// (k_conv2d_dw) contracts over the output pixels, split into ranges whose partial products are summed in a fixed order (or queued
// with ww_defer).  Tile shape, LDS strides and fragments are those of ww_tconv.hip: 64 x 64 block tiles, 4 wavefronts x one 32x32
// MFMA tile; WW_ACT_F32: v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain per LDS stage, the parity mode); WW_ACT_BF16 / WW_ACT_F16:
// operands rounded when they are staged into LDS, v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation.  The stages' sums are added per
// tap and the taps at the end (blocked summation).  All tensors are fp32 in HBM.
#include "ww_internal.h"
#include "ww_act.h"
#include "ww_mfma_stage.h"
#include <algorithm>

namespace {

// ---- the implicit GEMM:  C[m][n] (+)= sum_{(r,s)} sum_c A[src(m, r, s)][c] W[r k + s][n][c]
// m = (b, oh, ow) on the (OH, OW) grid of the tensor being written, A lies on the (SH, SW) grid of the tensor being read.
//   DX == false: src = (b, oh st + r - p, ow st + s - p)                    -- the forward product (A = x, C = y)
//   DX == true : src = (b, (oh + p - r) / st, (ow + p - s) / st), exact only -- the input gradient (A = dy, C = dx)
// A row without a source in its own image contributes 0; a dx pixel no output read is therefore WRITTEN as 0.  CA, N multiples of 4.
struct RowArgs {
    const float *A;      // (B, SH, SW, CA)
    const float *W;      // (k*k, N, CA): k_conv2d_pack
    float *C;            // (M, N)
    int M, OH, OW, SH, SW, CA, N, k, stride, pad, accumulate;
};
constexpr int NO_ROW = -(1 << 24);       // "oh" of a row past M: every bounds test below fails on it
template <int MODE, bool DX>
__global__ __launch_bounds__(256) void k_conv2d_rows(RowArgs a) {
    typedef typename ModeH<MODE>::type H;
    constexpr int KT = MODE ? 64 : 32;             // K per LDS stage: 16 fp32 MFMAs (2 k each) / 4 16-bit ones (16 k each)
    constexpr int NV = 64 * KT / 1024;             // float4 per thread and operand tile
    constexpr int F4 = KT / 4;                     // float4 per tile row
    constexpr int LD = MODE ? KT + 8 : KT + 4;     // [row][k] LDS stride (elements)
    constexpr int TILE_BYTES = 64 * LD * (MODE ? 2 : 4);
    __shared__ __align__(16) unsigned char lds[2 * TILE_BYTES];
    void *As = lds, *Bs = lds + TILE_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 31, h = lane >> 5, rh = wv >> 1, nh = wv & 1;
    const long m0 = (long)blockIdx.y * 64;
    const int n0 = blockIdx.x * 64;
    // the rows this thread stages are the same in every stage: their pixel is worked out once
    int oh[NV], ow[NV], img[NV];                   // img = b SH SW: the first source pixel of the row's own image
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long m = m0 + (tid + 256 * j) / F4;
        oh[j] = NO_ROW; ow[j] = 0; img[j] = 0;
        if (m < a.M) {
            const unsigned per = (unsigned)a.OH * a.OW, um = (unsigned)m, b = um / per, rem = um - b * per;
            oh[j] = (int)(rem / (unsigned)a.OW);
            ow[j] = (int)(rem - (unsigned)oh[j] * a.OW);
            img[j] = (int)b * a.SH * a.SW;
        }
    }
    const int nk = (a.CA + KT - 1) / KT, stages = a.k * a.k * nk, sh1 = a.stride - 1;      // stride 1 | 2: a shift by 0 | 1
    float4 va[NV], vb[NV];
    auto fetch = [&](int it) {
        const int seg = it / nk, k0 = (it - seg * nk) * KT, tr = seg / a.k, ts = seg - tr * a.k;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, kk = k0 + 4 * (q % F4), n = n0 + q / F4;
            int sh, sw;
            bool ok;
            if constexpr (DX) {
                const int th = oh[j] + a.pad - tr, tw = ow[j] + a.pad - ts;
                sh = th >> sh1; sw = tw >> sh1;
                ok = th >= 0 && tw >= 0 && ((th | tw) & sh1) == 0 && sh < a.SH && sw < a.SW;
            } else {
                sh = oh[j] * a.stride + tr - a.pad; sw = ow[j] * a.stride + ts - a.pad;
                ok = sh >= 0 && sh < a.SH && sw >= 0 && sw < a.SW;
            }
            ok = ok && kk < a.CA;
            va[j] = ok ? *reinterpret_cast<const float4 *>(a.A + ((long)img[j] + sh * a.SW + sw) * a.CA + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool okb = n < a.N && kk < a.CA;
            vb[j] = okb ? *reinterpret_cast<const float4 *>(a.W + ((long)seg * a.N + n) * a.CA + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    floatx16 acc = floatx16{0.f}, tap = floatx16{0.f};
    int in_tap = 0;
    fetch(0);
    for (int it = 0; it < stages; ++it) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, off = (q / F4) * LD + 4 * (q % F4);
            put4<MODE>(As, off, va[j]);
            put4<MODE>(Bs, off, vb[j]);
        }
        __syncthreads();
        if (it + 1 < stages) fetch(it + 1);        // the next stage in flight under the MFMAs
        // blocked summation: a stage's KT products are one chain, the stages of a tap are summed per tap, the taps at the end --
        // chains of KT, Cin / KT and k k terms instead of one of k k Cin (4608 in the last ResNet stage)
        floatx16 part = floatx16{0.f};
        if constexpr (MODE != 0) {
            typedef typename H16<H>::x8 x8;
            const H *pa = reinterpret_cast<const H *>(As) + (32 * rh + r) * LD + 8 * h;
            const H *pb = reinterpret_cast<const H *>(Bs) + (32 * nh + r) * LD + 8 * h;
#pragma unroll
            for (int t = 0; t < KT / 16; ++t)
                part = H16<H>::mfma32(*reinterpret_cast<const x8 *>(pa + 16 * t), *reinterpret_cast<const x8 *>(pb + 16 * t), part);
        } else {
            const float *pa = reinterpret_cast<const float *>(As) + (32 * rh + r) * LD + h;
            const float *pb = reinterpret_cast<const float *>(Bs) + (32 * nh + r) * LD + h;
#pragma unroll
            for (int t = 0; t < KT / 2; ++t) part = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t], pb[2 * t], part, 0, 0, 0);
        }
        tap += part;
        if (++in_tap == nk) { acc += tap; tap = floatx16{0.f}; in_tap = 0; }
    }
    const int col = n0 + 32 * nh + r;
    if (col >= a.N) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const long row = m0 + 32 * rh + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (row >= a.M) continue;
        float v = acc[reg];
        if (a.accumulate) v += a.C[row * a.N + col];
        a.C[row * a.N + col] = v;
    }
}
template <bool DX>
void launch_rows(int mode, const RowArgs &a, hipStream_t st) {
    const dim3 grid((a.N + 63) / 64, (unsigned)((a.M + 63) / 64));
    if (mode == WW_ACT_BF16) hipLaunchKernelGGL((k_conv2d_rows<1, DX>), grid, dim3(256), 0, st, a);
    else if (mode == WW_ACT_F16) hipLaunchKernelGGL((k_conv2d_rows<2, DX>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv2d_rows<0, DX>), grid, dim3(256), 0, st, a);
}

// ---- the weight gradient:  out[z][n][c][r k + s] = sum_{m in range z} G[m][n] X[src(m, r, s)][c]   (src as the forward's)
// grid: x = c tiles, y = n tiles, z = tap * nsplit + range.  Both operands are row-contiguous ([k][row] tiles in LDS).
struct DwArgs {
    const float *G;      // dy (M, N), M = B Ho Wo
    const float *X;      // (B, H, W, C)
    float *out;          // (nsplit, N, C, k, k)
    int M, Ho, Wo, H, W, N, C, k, stride, pad, rps, nsplit;
};
template <int MODE>
__global__ __launch_bounds__(256) void k_conv2d_dw(DwArgs a) {
    typedef typename ModeH<MODE>::type H;
    constexpr int KT = MODE ? 64 : 32;
    constexpr int NV = 64 * KT / 1024;
    constexpr int LD = MODE ? 64 + 8 : 64 + 4;     // [k][row] LDS stride (elements)
    constexpr int TILE_BYTES = KT * LD * (MODE ? 2 : 4);
    __shared__ __align__(16) unsigned char lds[2 * TILE_BYTES];
    void *As = lds, *Bs = lds + TILE_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 31, h = lane >> 5, rh = wv >> 1, nh = wv & 1;
    const int c0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int seg = blockIdx.z / a.nsplit, z = blockIdx.z - seg * a.nsplit;
    const int tr = seg / a.k, ts = seg - tr * a.k, sh1 = a.stride - 1;
    const int mb = (int)min((long)a.M, (long)z * a.rps), me = (int)min((long)a.M, (long)mb + a.rps);
    const unsigned per = (unsigned)a.Ho * a.Wo;
    float4 va[NV], vb[NV];
    auto fetch = [&](int mk0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, m = mk0 + q / 16, e = 4 * (q % 16);
            const bool okm = m < me;
            const bool oka = okm && n0 + e < a.N;
            va[j] = oka ? *reinterpret_cast<const float4 *>(a.G + (long)m * a.N + n0 + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            const unsigned um = okm ? (unsigned)m : 0u, b = um / per, rem = um - b * per, ho = rem / (unsigned)a.Wo, wo = rem - ho * a.Wo;
            const int hi = ((int)ho << sh1) + tr - a.pad, wi = ((int)wo << sh1) + ts - a.pad;
            const bool okb = okm && c0 + e < a.C && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
            vb[j] = okb ? *reinterpret_cast<const float4 *>(a.X + (((long)b * a.H + hi) * a.W + wi) * a.C + c0 + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    floatx16 acc = floatx16{0.f};
    if (mb < me) fetch(mb);
    for (int mk0 = mb; mk0 < me; mk0 += KT) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, off = (q / 16) * LD + 4 * (q % 16);
            put4<MODE>(As, off, va[j]);
            put4<MODE>(Bs, off, vb[j]);
        }
        __syncthreads();
        if (mk0 + KT < me) fetch(mk0 + KT);
        floatx16 part = floatx16{0.f};             // blocked summation, as in k_conv2d_rows: a chain per stage, then the stages
        if constexpr (MODE != 0) {
            const H *pa = reinterpret_cast<const H *>(As), *pb = reinterpret_cast<const H *>(Bs);
#pragma unroll
            for (int t = 0; t < KT / 16; ++t)
                part = H16<H>::mfma32(tr_frag(pa, LD, 16 * t, 32 * rh, lane), tr_frag(pb, LD, 16 * t, 32 * nh, lane), part);
        } else {
            const float *pa = reinterpret_cast<const float *>(As) + h * LD + 32 * rh + r;
            const float *pb = reinterpret_cast<const float *>(Bs) + h * LD + 32 * nh + r;
#pragma unroll
            for (int t = 0; t < KT / 2; ++t) part = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t * LD], pb[2 * t * LD], part, 0, 0, 0);
        }
        acc += part;
    }
    const int c = c0 + 32 * nh + r;
    if (c >= a.C) return;
    const int kk = a.k * a.k;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + 32 * rh + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (n < a.N) a.out[(((long)z * a.N + n) * a.C + c) * kk + seg] = acc[reg];
    }
}

// out[t][n][c] = w[n][c][t] (transpose == 0: the forward's taps) or out[t][c][n] = w[n][c][t] (the dX product's); t = r k + s
__global__ __launch_bounds__(256) void k_conv2d_pack(const float *__restrict__ w, int Cout, int Cin, int kk, int transpose,
                                                     float *__restrict__ out) {
    const long per = (long)Cout * Cin, n_all = per * kk;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_all; i += (long)gridDim.x * 256) {
        const int t = (int)(i / per);
        const long rem = i - (long)t * per;
        int n, c;
        if (transpose) { c = (int)(rem / Cout); n = (int)(rem - (long)c * Cout); }
        else { n = (int)(rem / Cin); c = (int)(rem - (long)n * Cin); }
        out[i] = w[((long)n * Cin + c) * kk + t];
    }
}
// dst[i] = sum_z part[z*n + i], z in order (the immediate form of the deferred reduction)
__global__ __launch_bounds__(256) void k_conv2d_sum(const float *__restrict__ part, long n, int splits, float *__restrict__ dst) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        double s = 0.0;
        for (int z = 0; z < splits; ++z) s += (double)part[(long)z * n + i];
        dst[i] = (float)s;
    }
}

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

int ew_grid(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 4096)); }
int out_size(int n, int k, int stride) { return (n + 2 * (k / 2) - k) / stride + 1; }

// ranges of the weight-gradient contraction: enough of them for ~1024 workgroups, each at least 128 pixels deep, at most 256
int dw_splits(long M, int Cin, int Cout, int kk) {
    const long tiles = (long)((Cout + 63) / 64) * ((Cin + 63) / 64) * kk;
    long s = (1024 + tiles - 1) / tiles;
    s = std::min<long>(s, M / 128);
    return (int)std::max<long>(1, std::min<long>(s, 256));
}
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
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

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
    hipLaunchKernelGGL(k_conv2d_pack, dim3(ew_grid((long)k * k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k * k, 0, wp);
    WW_LAUNCH_CHECK();
    const RowArgs a{x, wp, y, (int)M, Ho, Wo, H, W, Cin, Cout, k, stride, k / 2, 0};
    launch_rows<false>(mode, a, st);
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
        hipLaunchKernelGGL(k_conv2d_pack, dim3(ew_grid((long)kk * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, kk, 1, wp);
        WW_LAUNCH_CHECK();
        const RowArgs a{dy, wp, dx, (int)((long)B * H * W), H, W, Ho, Wo, Cout, Cin, k, stride, k / 2, accumulate_dx != 0};
        launch_rows<true>(mode, a, st);
        WW_LAUNCH_CHECK();
    }
    const int kt = mode == WW_ACT_F32 ? 32 : 64;
    const int want = dw_splits(M, Cin, Cout, kk);
    const long rps = ((M + want - 1) / want + kt - 1) / kt * kt;      // whole K stages per range
    const int nz = (int)((M + rps - 1) / rps);                         // <= want
    const long n = (long)Cout * Cin * kk;
    float *part = base + l.dwp;
    const DwArgs a{dy, x, nz > 1 ? part : dw, (int)M, Ho, Wo, H, W, Cout, Cin, k, stride, k / 2, (int)rps, nz};
    const dim3 grid((Cin + 63) / 64, (Cout + 63) / 64, kk * nz);
    if (mode == WW_ACT_BF16) hipLaunchKernelGGL(k_conv2d_dw<1>, grid, dim3(256), 0, st, a);
    else if (mode == WW_ACT_F16) hipLaunchKernelGGL(k_conv2d_dw<2>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_conv2d_dw<0>, grid, dim3(256), 0, st, a);
    WW_LAUNCH_CHECK();
    if (nz > 1 && !ww_defer(ctx, part, dw, n, nz, 0)) {
        hipLaunchKernelGGL(k_conv2d_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, nz, dw);
        WW_LAUNCH_CHECK();
    }
    return WW_OK;
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
        hipLaunchKernelGGL(k_conv2d_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, blocks, dw);
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

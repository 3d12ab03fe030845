// Causal dilated Conv1d on the matrix cores: the layer TCNWakeword is made of (the reference's TemporalBlock pads both sides by
// (k-1) d, convolves and keeps the first T outputs -- on those outputs exactly a causal convolution).  Channels-last:
//   fwd : y[b,t,n]   = bias[n] + sum_j sum_c x[b, t - (k-1-j) d, c] w[n,c,j]      (rows before t = 0 read as 0)
//   dX  : dx[b,s,c]  = sum_j sum_n dpre[b, s + (k-1-j) d, n] w[n,c,j]             (rows from T on read as 0)
//   dW  : dw[n,c,j]  = sum_{b,t} dpre[b,t,n] x[b, t - (k-1-j) d, c] ;  db[n] = sum_{b,t} dpre[b,t,n]
// with dpre = dy * scale * [y != 0] * [y2 != 0] (the ReLU and dropout masks of the layer, read off its saved outputs).
// fwd and dX are one "shifted-row GEMM" (k_tconv_rows): k K-segments whose A rows are displaced by a per-segment row offset that
// never leaves the sample; the weights are first re-laid per tap (k_tconv_pack: (Cout,Cin,k), nn.Conv1d's own layout, has the tap
// as its fastest index).  dW (k_tconv_dw) contracts over the B*T rows, split into row ranges whose partial products are summed
// in a fixed order (or queued with ww_defer).  64 x 64 block tiles, 4 wavefronts x one 32x32 MFMA tile;  mode WW_ACT_F32:
// v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain, the parity mode); WW_ACT_BF16 / WW_ACT_F16: operands rounded when they are staged
// into LDS, v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation.  All tensors are fp32 in HBM.
#include "ww_internal.h"
#include "ww_act.h"
#include "ww_mfma_stage.h"
#include <algorithm>

namespace {

// ---- the shifted-row GEMM:  C[m][n] (+)= sum_s sum_c A[m + (nseg-1-s) dstep][c] W[s][n][c]  (+ bias, + residual, ReLU)
// m = b*T + t; a displaced row is read only while t + (nseg-1-s) dstep stays in [0, T) -- an M tile that spans two samples never
// takes the neighbouring sample's rows for "before t = 0".  dstep = -d (forward) or +d (dX).  CA, N multiples of 4.
struct RowArgs {
    const float *A;      // (M, CA)
    const float *W;      // (nseg, N, CA): k_tconv_pack
    float *C;            // (M, N)
    const float *bias;   // (N) nullable
    const float *res;    // (M, N) nullable: added before the ReLU
    int M, T, CA, N, nseg, dstep, relu, accumulate;
};
// (A 128 x 128 form of this kernel -- each staged byte feeding twice the MFMA work, 224 VGPRs -- was measured and dropped: the
// B = 512 step read 2.27 ms against 2.16 in the 16-bit modes and 3.17 against 3.08 in fp32.)
template <int MODE>
__global__ __launch_bounds__(256) void k_tconv_rows(RowArgs a) {
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
    // the rows this thread stages are the same in every stage: their time index is worked out once (-1: past the last row)
    int tA[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long m = m0 + (tid + 256 * j) / F4;
        tA[j] = m < a.M ? (int)(m % a.T) : -1;
    }
    const int nk = (a.CA + KT - 1) / KT, stages = a.nseg * nk;
    float4 va[NV], vb[NV];
    auto fetch = [&](int it) {
        const int s = it / nk, k0 = (it - s * nk) * KT;
        const long off = (long)(a.nseg - 1 - s) * a.dstep;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, kk = k0 + 4 * (q % F4), n = n0 + q / F4;
            const long tt = (long)tA[j] + off;
            const bool oka = tA[j] >= 0 && tt >= 0 && tt < a.T && kk < a.CA;
            va[j] = oka ? *reinterpret_cast<const float4 *>(a.A + (m0 + q / F4 + off) * a.CA + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool okb = n < a.N && kk < a.CA;
            vb[j] = okb ? *reinterpret_cast<const float4 *>(a.W + ((long)s * a.N + n) * a.CA + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    floatx16 acc = floatx16{0.f};
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
        if constexpr (MODE != 0) {
            typedef typename H16<H>::x8 x8;
            const H *pa = reinterpret_cast<const H *>(As) + (32 * rh + r) * LD + 8 * h;
            const H *pb = reinterpret_cast<const H *>(Bs) + (32 * nh + r) * LD + 8 * h;
#pragma unroll
            for (int t = 0; t < KT / 16; ++t)
                acc = H16<H>::mfma32(*reinterpret_cast<const x8 *>(pa + 16 * t), *reinterpret_cast<const x8 *>(pb + 16 * t), acc);
        } else {
            const float *pa = reinterpret_cast<const float *>(As) + (32 * rh + r) * LD + h;
            const float *pb = reinterpret_cast<const float *>(Bs) + (32 * nh + r) * LD + h;
#pragma unroll
            for (int t = 0; t < KT / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t], pb[2 * t], acc, 0, 0, 0);
        }
    }
    const int col = n0 + 32 * nh + r;
    if (col >= a.N) return;
    const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const long row = m0 + 32 * rh + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (row >= a.M) continue;
        float v = acc[reg] + bias;
        if (a.res) v += a.res[row * a.N + col];
        if (a.relu) v = v < 0.f ? 0.f : v;         // (a NaN stays a NaN: the step's non-finite check must see it)
        if (a.accumulate) v += a.C[row * a.N + col];
        a.C[row * a.N + col] = v;
    }
}
void launch_rows(int mode, const RowArgs &a, hipStream_t st) {
    const dim3 grid((a.N + 63) / 64, (unsigned)((a.M + 63) / 64));
    if (mode == WW_ACT_BF16) hipLaunchKernelGGL(k_tconv_rows<1>, grid, dim3(256), 0, st, a);
    else if (mode == WW_ACT_F16) hipLaunchKernelGGL(k_tconv_rows<2>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_tconv_rows<0>, grid, dim3(256), 0, st, a);
}

// ---- the weight gradient:  out[z][n][c][s] = sum_{m in split z} G[m][n] X[m - (k-1-s) d][c]   (rows with t(m) < (k-1-s) d read as 0)
// grid: x = c tiles, y = n tiles, z = tap * nsplit + split.  Both operands are row-contiguous ([k][row] tiles in LDS).
struct DwArgs {
    const float *G;      // dpre (M, N)
    const float *X;      // (M, C)
    float *out;          // (nsplit, N, C, k)
    int M, T, N, C, k, d, rps, nsplit;
};
template <int MODE>
__global__ __launch_bounds__(256) void k_tconv_dw(DwArgs a) {
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
    const int s = blockIdx.z / a.nsplit, z = blockIdx.z - s * a.nsplit;
    const long shift = (long)(a.k - 1 - s) * a.d;
    const int mb = (int)min((long)a.M, (long)z * a.rps), me = (int)min((long)a.M, (long)mb + a.rps);
    float4 va[NV], vb[NV];
    auto fetch = [&](int mk0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, m = mk0 + q / 16, e = 4 * (q % 16);
            const bool okm = m < me;
            const bool oka = okm && n0 + e < a.N;
            va[j] = oka ? *reinterpret_cast<const float4 *>(a.G + (long)m * a.N + n0 + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool okb = okm && c0 + e < a.C && (long)(m % a.T) >= shift;
            vb[j] = okb ? *reinterpret_cast<const float4 *>(a.X + ((long)m - shift) * a.C + c0 + e) : make_float4(0.f, 0.f, 0.f, 0.f);
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
        if constexpr (MODE != 0) {
            const H *pa = reinterpret_cast<const H *>(As), *pb = reinterpret_cast<const H *>(Bs);
#pragma unroll
            for (int t = 0; t < KT / 16; ++t)
                acc = H16<H>::mfma32(tr_frag(pa, LD, 16 * t, 32 * rh, lane), tr_frag(pb, LD, 16 * t, 32 * nh, lane), acc);
        } else {
            const float *pa = reinterpret_cast<const float *>(As) + h * LD + 32 * rh + r;
            const float *pb = reinterpret_cast<const float *>(Bs) + h * LD + 32 * nh + r;
#pragma unroll
            for (int t = 0; t < KT / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t * LD], pb[2 * t * LD], acc, 0, 0, 0);
        }
    }
    const int c = c0 + 32 * nh + r;
    if (c >= a.C) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + 32 * rh + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (n < a.N) a.out[(((long)z * a.N + n) * a.C + c) * a.k + s] = acc[reg];
    }
}

// out[s][n][c] = w[n][c][s] (transpose == 0: the forward's taps) or out[s][c][n] = w[n][c][s] (the dX product's)
__global__ __launch_bounds__(256) void k_tconv_pack(const float *__restrict__ w, int Cout, int Cin, int k, int transpose,
                                                    float *__restrict__ out) {
    const long per = (long)Cout * Cin, n_all = per * k;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_all; i += (long)gridDim.x * 256) {
        const int s = (int)(i / per);
        const long rem = i - (long)s * per;
        int n, c;
        if (transpose) { c = (int)(rem / Cout); n = (int)(rem - (long)c * Cout); }
        else { n = (int)(rem / Cin); c = (int)(rem - (long)n * Cin); }
        out[i] = w[((long)n * Cin + c) * k + s];
    }
}
// dpre = dy * scale where the saved outputs are non-zero (n4 float4s)
__global__ __launch_bounds__(256) void k_tconv_dpre(const float4 *__restrict__ dy, const float4 *__restrict__ y, const float4 *__restrict__ y2,
                                                    float scale, long n4, float4 *__restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 g = dy[i];
        float4 m = make_float4(scale, scale, scale, scale);
        if (y) { const float4 v = y[i]; m.x = v.x != 0.f ? m.x : 0.f; m.y = v.y != 0.f ? m.y : 0.f; m.z = v.z != 0.f ? m.z : 0.f; m.w = v.w != 0.f ? m.w : 0.f; }
        if (y2) { const float4 v = y2[i]; m.x = v.x != 0.f ? m.x : 0.f; m.y = v.y != 0.f ? m.y : 0.f; m.z = v.z != 0.f ? m.z : 0.f; m.w = v.w != 0.f ? m.w : 0.f; }
        // (a masked entry is 0 whatever the gradient holds there, as autograd's ReLU backward has it)
        g.x = m.x != 0.f ? g.x * m.x : 0.f; g.y = m.y != 0.f ? g.y * m.y : 0.f; g.z = m.z != 0.f ? g.z * m.z : 0.f; g.w = m.w != 0.f ? g.w * m.w : 0.f;
        out[i] = g;
    }
}
// dst[i] = sum_z part[z*n + i], z in order (the immediate form of the deferred reduction)
__global__ __launch_bounds__(256) void k_tconv_sum(const float *__restrict__ part, long n, int splits, float *__restrict__ dst) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        double s = 0.0;
        for (int z = 0; z < splits; ++z) s += (double)part[(long)z * n + i];
        dst[i] = (float)s;
    }
}
// y = relu(a + b);  dx = dy where y != 0
__global__ __launch_bounds__(256) void k_add_relu(const float *__restrict__ a, const float *__restrict__ b, long n, float *__restrict__ y) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = a[i] + b[i];
        y[i] = v < 0.f ? 0.f : v;
    }
}
__global__ __launch_bounds__(256) void k_relu_mask(const float *__restrict__ dy, const float *__restrict__ y, long n, float *__restrict__ dx) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dx[i] = y[i] != 0.f ? dy[i] : 0.f;
}

int ew_grid(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 4096)); }

// row ranges of the weight-gradient contraction: enough of them for ~1024 workgroups, each at least 128 rows deep, at most 256
int dw_splits(long M, int Cin, int Cout, int k) {
    const long tiles = (long)((Cout + 63) / 64) * ((Cin + 63) / 64) * k;
    long s = (1024 + tiles - 1) / tiles;
    s = std::min<long>(s, M / 128);
    return (int)std::max<long>(1, std::min<long>(s, 256));
}
constexpr int DB_CHUNKS = 64;

struct Layout { size_t wp, dpre, dwp, dbp, total; };      // float offsets of the scratch regions
Layout layout(long M, int Cin, int Cout, int k) {
    Layout l;
    l.wp = 0;
    l.dpre = (size_t)k * Cin * Cout;
    l.dwp = l.dpre + (size_t)M * Cout;
    l.dbp = l.dwp + (size_t)dw_splits(M, Cin, Cout, k) * Cout * Cin * k;
    l.total = l.dbp + (size_t)DB_CHUNKS * Cout;
    return l;
}

int check_shape(const char *who, int mode, int B, int T, int Cin, int Cout, int k, int d) {
    WW_REQUIRE(mode == WW_ACT_F32 || mode == WW_ACT_BF16 || mode == WW_ACT_F16, WW_E_INVALID, "%s: unknown mode %d", who, mode);
    WW_REQUIRE(B >= 1 && T >= 1 && (long)B * T <= 0x7fffffffL, WW_E_INVALID, "%s: bad shape B=%d T=%d", who, B, T);
    WW_REQUIRE(Cin >= 4 && Cout >= 4 && Cin % 4 == 0 && Cout % 4 == 0, WW_E_INVALID,
               "%s: channel counts must be positive multiples of 4, got Cin=%d Cout=%d", who, Cin, Cout);
    WW_REQUIRE(k >= 1 && k <= 8, WW_E_INVALID, "%s: kernel_size=%d not in 1..8", who, k);
    WW_REQUIRE(d >= 1, WW_E_INVALID, "%s: dilation=%d must be >= 1", who, d);
    return WW_OK;
}
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t ww_tconv1d_scratch_bytes(int B, int T, int Cin, int Cout, int k) {
    if (B < 1 || T < 1 || Cin < 4 || Cout < 4 || Cin % 4 || Cout % 4 || k < 1 || k > 8 || (long)B * T > 0x7fffffffL) return 0;
    return layout((long)B * T, Cin, Cout, k).total * sizeof(float);
}

extern "C" int ww_tconv1d_fwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *bias, int B, int T, int Cin, int Cout,
                              int k, int dilation, int relu, const float *residual, float *y, void *scratch, size_t scratch_bytes,
                              ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && bias && y && scratch, WW_E_INVALID, "ww_tconv1d_fwd: null argument");
    int rc = check_shape("ww_tconv1d_fwd", mode, B, T, Cin, Cout, k, dilation);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y) && al16(scratch) && al16(residual), WW_E_INVALID, "ww_tconv1d_fwd: tensors must be 16-byte aligned");
    const long M = (long)B * T;
    WW_REQUIRE(scratch_bytes >= layout(M, Cin, Cout, k).total * sizeof(float), WW_E_WORKSPACE, "ww_tconv1d_fwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    float *wp = (float *)scratch;
    hipLaunchKernelGGL(k_tconv_pack, dim3(ew_grid((long)k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k, 0, wp);
    WW_LAUNCH_CHECK();
    // a dilation of T or more displaces every tap but the last out of the sample, as T itself does
    const RowArgs a{x, wp, y, bias, residual, (int)M, T, Cin, Cout, k, -std::min(dilation, T), relu != 0, 0};
    launch_rows(mode, a, st);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_tconv1d_bwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *y, const float *y2, float mask_scale,
                              const float *dy, int B, int T, int Cin, int Cout, int k, int dilation, float *dx, int accumulate_dx,
                              float *dw, float *db, void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && dy && dw && db && scratch, WW_E_INVALID, "ww_tconv1d_bwd: null argument");
    int rc = check_shape("ww_tconv1d_bwd", mode, B, T, Cin, Cout, k, dilation);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y) && al16(y2) && al16(dy) && al16(dx) && al16(scratch), WW_E_INVALID,
               "ww_tconv1d_bwd: tensors must be 16-byte aligned");
    const long M = (long)B * T;
    const Layout l = layout(M, Cin, Cout, k);
    WW_REQUIRE(scratch_bytes >= l.total * sizeof(float), WW_E_WORKSPACE, "ww_tconv1d_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    float *base = (float *)scratch;
    const int d = std::min(dilation, T);
    const float *dpre = dy;
    if (y || y2 || mask_scale != 1.f) {
        const long n4 = M * Cout / 4;
        hipLaunchKernelGGL(k_tconv_dpre, dim3(ew_grid(n4)), dim3(256), 0, st, (const float4 *)dy, (const float4 *)y, (const float4 *)y2,
                           mask_scale, n4, (float4 *)(base + l.dpre));
        WW_LAUNCH_CHECK();
        dpre = base + l.dpre;
    }
    if (dx) {
        float *wp = base + l.wp;
        hipLaunchKernelGGL(k_tconv_pack, dim3(ew_grid((long)k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k, 1, wp);
        WW_LAUNCH_CHECK();
        const RowArgs a{dpre, wp, dx, nullptr, nullptr, (int)M, T, Cout, Cin, k, d, 0, accumulate_dx != 0};
        launch_rows(mode, a, st);
        WW_LAUNCH_CHECK();
    }
    {
        const int kt = mode == WW_ACT_F32 ? 32 : 64;
        const int want = dw_splits(M, Cin, Cout, k);
        const long rps = ((M + want - 1) / want + kt - 1) / kt * kt;      // whole K stages per split
        const int nz = (int)((M + rps - 1) / rps);                         // <= want
        const long n = (long)Cout * Cin * k;
        float *part = base + l.dwp;
        const DwArgs a{dpre, x, nz > 1 ? part : dw, (int)M, T, Cout, Cin, k, d, (int)rps, nz};
        const dim3 grid((Cin + 63) / 64, (Cout + 63) / 64, k * nz);
        if (mode == WW_ACT_BF16) hipLaunchKernelGGL(k_tconv_dw<1>, grid, dim3(256), 0, st, a);
        else if (mode == WW_ACT_F16) hipLaunchKernelGGL(k_tconv_dw<2>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_tconv_dw<0>, grid, dim3(256), 0, st, a);
        WW_LAUNCH_CHECK();
        if (nz > 1 && !ww_defer(ctx, part, dw, n, nz, 0)) {
            hipLaunchKernelGGL(k_tconv_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, nz, dw);
            WW_LAUNCH_CHECK();
        }
    }
    if (M <= 1024) return ww_colsum_rows_small(dpre, (int)M, Cout, db, st);
    return ww_colsum_rows(dpre, M, Cout, db, base + l.dbp, DB_CHUNKS, st);
}

extern "C" int ww_add_relu_fwd(ww_ctx *ctx, const float *a, const float *b, size_t n, float *y, ww_stream_t stream) {
    WW_REQUIRE(ctx && a && b && y, WW_E_INVALID, "ww_add_relu_fwd: null argument");
    if (n == 0) return WW_OK;
    hipLaunchKernelGGL(k_add_relu, dim3(ew_grid((long)n)), dim3(256), 0, (hipStream_t)stream, a, b, (long)n, y);
    WW_LAUNCH_CHECK();
    return WW_OK;
}
extern "C" int ww_relu_mask_bwd(ww_ctx *ctx, const float *dy, const float *y, size_t n, float *dx, ww_stream_t stream) {
    WW_REQUIRE(ctx && dy && y && dx, WW_E_INVALID, "ww_relu_mask_bwd: null argument");
    if (n == 0) return WW_OK;
    hipLaunchKernelGGL(k_relu_mask, dim3(ew_grid((long)n)), dim3(256), 0, (hipStream_t)stream, dy, y, (long)n, dx);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

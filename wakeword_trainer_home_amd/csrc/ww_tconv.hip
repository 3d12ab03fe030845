// Causal dilated Conv1d on the matrix cores: the layer TCNWakeword is made of (the reference's TemporalBlock pads both sides by
// (k-1) d, convolves and keeps the first T outputs -- on those outputs exactly a causal convolution).  Channels-last:
//   fwd : y[b,t,n]   = bias[n] + sum_j sum_c x[b, t - (k-1-j) d, c] w[n,c,j]      (rows before t = 0 read as 0)
//   dX  : dx[b,s,c]  = sum_j sum_n dpre[b, s + (k-1-j) d, n] w[n,c,j]             (rows from T on read as 0)
//   dW  : dw[n,c,j]  = sum_{b,t} dpre[b,t,n] x[b, t - (k-1-j) d, c] ;  db[n] = sum_{b,t} dpre[b,t,n]
// with dpre = dy * scale * [y != 0] * [y2 != 0] (the ReLU and dropout masks of the layer, read off its saved outputs).
// The three products are the tap GEMM of ww_tap_gemm.h with the geometry of a time axis: k K-segments whose A rows are displaced
// by a per-segment row offset that never leaves the sample, summed as one MFMA chain (SumChain); bias, residual and ReLU are the
// epilogue of the rows kernel.  The partial products of the dW row ranges are summed in a fixed order (or queued with ww_defer).
#include "ww_tap_gemm.h"

namespace {

// ---- the time axis.  m = b*T + t; segment s displaces a row by (k-1-s) dstep, dstep = -d (forward) or +d (dX), and the displaced
// row is read only while t + (k-1-s) dstep stays in [0, T) -- an M tile that spans two samples never takes the neighbouring
// sample's rows for "before t = 0".
struct TimeRows {
    typedef int Row;     // t, or -1 past the last row
    int T, k, dstep;
    __device__ Row row(long m, int M) const { return m < M ? (int)(m % T) : -1; }
    typedef long Tap;    // the row offset of a segment
    __device__ Tap tap(int seg) const { return (long)(k - 1 - seg) * dstep; }
    __device__ bool src(Row t, long m, Tap off, long &at) const {
        const long tt = (long)t + off;
        at = m + off;
        return t >= 0 && tt >= 0 && tt < T;
    }
};
// dW: row m of dpre meets x[m - (k-1-s) d]   (rows with t(m) < (k-1-s) d read as 0)
struct TimeDw {
    int T, k, d;
    typedef long Tap;
    __device__ Tap tap(int seg) const { return (long)(k - 1 - seg) * d; }
    __device__ bool src(int m, Tap shift, long &at) const {
        at = (long)m - shift;
        return (long)(m % T) >= shift;
    }
};
// sum + bias, + residual, ReLU
struct TimeEpi {
    const float *bias;   // (N) nullable
    const float *res;    // (M, N) nullable: added before the ReLU
    int relu;
    __device__ float column(int col) const { return bias ? bias[col] : 0.f; }
    __device__ float operator()(float v, float b, long at) const {
        v += b;
        if (res) v += res[at];
        if (relu) v = v < 0.f ? 0.f : v;           // (a NaN stays a NaN: the step's non-finite check must see it)
        return v;
    }
};
typedef RowsArgs<TimeRows, TimeEpi> RowArgs;      // {A, W, C, {bias, res, relu}, M, CA, N, nseg, accumulate, {T, k, dstep}}

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
    hipLaunchKernelGGL(k_tap_pack, dim3(ew_grid((long)k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k, 0, wp);
    WW_LAUNCH_CHECK();
    // a dilation of T or more displaces every tap but the last out of the sample, as T itself does
    const RowArgs a{x, wp, y, {bias, residual, relu != 0}, (int)M, Cin, Cout, k, 0, {T, k, -std::min(dilation, T)}};
    tap_launch_rows<SumChain>(mode, a, st);
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
        hipLaunchKernelGGL(k_tap_pack, dim3(ew_grid((long)k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k, 1, wp);
        WW_LAUNCH_CHECK();
        const RowArgs a{dpre, wp, dx, {nullptr, nullptr, 0}, (int)M, Cout, Cin, k, accumulate_dx != 0, {T, k, d}};
        tap_launch_rows<SumChain>(mode, a, st);
        WW_LAUNCH_CHECK();
    }
    rc = tap_dw<SumChain>(ctx, mode, dpre, x, TimeDw{T, k, d}, M, Cin, Cout, k, base + l.dwp, dw, st);
    if (rc) return rc;
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

// Causal dilated Conv1d on the matrix cores: the layer TCNWakeword is made of (the reference's TemporalBlock pads both sides by
// (k-1) d, convolves and keeps the first T outputs -- on those outputs exactly a causal convolution).  Channels-last:
//   fwd : y[b,t,n]   = bias[n] + sum_j sum_c x[b, t - (k-1-j) d, c] w[n,c,j]      (rows before t = 0 read as 0)
//   dX  : dx[b,s,c]  = sum_j sum_n dpre[b, s + (k-1-j) d, n] w[n,c,j]             (rows from T on read as 0)
//   dW  : dw[n,c,j]  = sum_{b,t} dpre[b,t,n] x[b, t - (k-1-j) d, c] ;  db[n] = sum_{b,t} dpre[b,t,n]
// with dpre = dy * scale * [y != 0] * [y2 != 0] (the ReLU and dropout masks of the layer, read off its saved outputs).
// The three products are the tap GEMM of ww_tap_gemm.h with the geometry of a time axis: k K-segments whose A rows are displaced
// by a per-segment row offset that never leaves the sample, summed as one MFMA chain (SumChain); bias, residual and ReLU are the
// epilogue of the rows kernel.  The partial products of the dW row ranges are summed in a fixed order (or queued with ww_defer).
// The second half of the file is the same layer with bf16 / fp16 ACTIVATION STORAGE (the `_st` entry points).
#include "ww_tap_gemm16.h"

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

// ============================================================================================================================
// 16-bit activation storage: every (B, T, C) tensor of the TCN -- the rounded input features, h1, h2, out of each block and every
// gradient of one -- is S = bf16 | fp16 in HBM, S = the matrix mode.  Arithmetic is fp32; a value is rounded (RNE, Act<S>::pack2)
// exactly where a tensor is stored and nowhere else; weights, their gradients, the bias and its gradient stay fp32.  The three
// products are the 16-bit tap GEMM of ww_tap_gemm16.h with the time geometry above, one MFMA chain (SumChain) and, for rows, the
// epilogue below inside the pair-exchange store.  Channel counts are multiples of 8.
namespace {

// (sum + bias, + residual, ReLU) of a column pair; the residual is an S tensor, widened
template <typename H>
struct TimeEpi16 {
    const float *bias;   // (N) nullable
    const H *res;        // (M, N) nullable: added before the ReLU
    int relu;
    __device__ float2 column(int col) const { return bias ? make_float2(bias[col], bias[col + 1]) : make_float2(0.f, 0.f); }
    __device__ float2 operator()(float2 v, float2 b, long at) const {
        v.x += b.x; v.y += b.y;
        if (res) {
            const float2 r = Act<H>::cvt2(Act<H>::ldraw2(res + at));
            v.x += r.x; v.y += r.y;
        }
        if (relu) { v.x = v.x < 0.f ? 0.f : v.x; v.y = v.y < 0.f ? 0.f : v.y; }      // (a NaN stays a NaN)
        return v;
    }
};
template <typename H> using TimeRows16 = Rows16<H, TimeRows, TimeEpi16<H>, Tail16None>;

// a 16-bit value is zero when its 15 low bits are: 0xffff / 0xffff0000 where the halves of v are non-zero
__device__ __forceinline__ uint32_t nz_pair(uint32_t v) { return (v & 0x7fffu ? 0xffffu : 0u) | (v & 0x7fff0000u ? 0xffff0000u : 0u); }

// dpre = S(dy * scale) where the STORED outputs are non-zero, else 0 (n8 vectors of 8 elements)
template <typename T>
__global__ __launch_bounds__(256) void k_tconv_dpre16(uint32_t n8, const uint4 *__restrict__ dy, const uint4 *__restrict__ y,
                                                      const uint4 *__restrict__ y2, float scale, uint4 *__restrict__ out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const uint4 g = dy[i];
        uint4 m = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (y) { const uint4 v = y[i]; m.x &= nz_pair(v.x); m.y &= nz_pair(v.y); m.z &= nz_pair(v.z); m.w &= nz_pair(v.w); }
        if (y2) { const uint4 v = y2[i]; m.x &= nz_pair(v.x); m.y &= nz_pair(v.y); m.z &= nz_pair(v.z); m.w &= nz_pair(v.w); }
        // (a masked entry is 0 whatever the gradient holds there, as autograd's ReLU backward has it)
        auto one = [&](uint32_t gw, uint32_t mw) {
            const float2 f = Act<T>::cvt2(gw);
            return Act<T>::pack2(f.x * scale, f.y * scale) & mw;
        };
        out[i] = make_uint4(one(g.x, m.x), one(g.y, m.y), one(g.z, m.z), one(g.w, m.w));
    }
}
// y = S(relu(a + b))
template <typename T>
__global__ __launch_bounds__(256) void k_add_relu16(uint32_t n8, const T *__restrict__ a, const T *__restrict__ b, T *__restrict__ y) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        float u[8], v[8];
        ld8(a + (size_t)i * 8, u); ld8(b + (size_t)i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float s = u[e] + v[e]; u[e] = s < 0.f ? 0.f : s; }
        st8(y + (size_t)i * 8, u);
    }
}
// k_dropout_bt (ww_gru.hip) on contiguous rows of C 16-bit elements: out = S(keep ? x * scale : 0), the same Philox law.  A counter
// word serves 4 channels, so a 16-byte access takes the two words c>>2 = 2j, 2j + 1 (C % 8 == 0: no tail word).  out may be x.
template <typename T>
__global__ __launch_bounds__(256) void k_dropout_bt16(uint32_t n8, const T *x, int T_, int C8, float scale, uint64_t thresh,
                                                      uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi,
                                                      uint64_t sample_offset, uint32_t stream_id, T *out,
                                                      const ww_step_ctl *__restrict__ ctl) {
    ww_step_resolve(ctl, step_lo, step_hi, step_lo, step_hi);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const uint32_t j = i % (uint32_t)C8, m = i / (uint32_t)C8;
        const uint32_t t = m % (uint32_t)T_, b = m / (uint32_t)T_;
        float v[8];
        ld8(x + (size_t)i * 8, v);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            uint32_t rr[4];
            ww_philox(step_lo, step_hi, (uint32_t)(sample_offset + (uint64_t)b),
                      (WW_TAG_DROPOUT << 24) | (stream_id << 20) | (t << 8) | (2 * j + w), seed_lo, seed_hi, rr);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * w + e] = (uint64_t)rr[e] >= thresh ? v[4 * w + e] * scale : 0.f;
        }
        st8(out + (size_t)i * 8, v);
    }
}
// the network input: out (B, T, F) = S(x), x (B, F, T) fp32.  One workgroup per (32 steps, 64 features, sample): coalesced reads
// along T into an LDS tile, 16-byte writes along F (F % 8 == 0: an octet of features is inside F or outside)
template <typename T>
__global__ __launch_bounds__(256) void k_seq_round_t16(const float *__restrict__ x, int F, int T_, T *__restrict__ out) {
    __shared__ float tile[64][33];
    const int t0 = blockIdx.x * 32, f0 = blockIdx.y * 64;
    const size_t b = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = f0 + ty + 8 * i, t = t0 + tx;
        tile[ty + 8 * i][tx] = (f < F && t < T_) ? x[(b * F + f) * T_ + t] : 0.f;
    }
    __syncthreads();
    const int tl = threadIdx.x >> 3, o = threadIdx.x & 7;
    if (t0 + tl >= T_ || f0 + 8 * o >= F) return;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[8 * o + e][tl];
    st8(out + (b * T_ + t0 + tl) * F + f0 + 8 * o, v);
}
// the same for an input that already is (B, T, F): n8 vectors of 8 elements
template <typename T>
__global__ __launch_bounds__(256) void k_seq_round16(uint32_t n8, const float *__restrict__ x, T *__restrict__ out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        float v[8];
        ld8(x + (size_t)i * 8, v);
        st8(out + (size_t)i * 8, v);
    }
}
// the bias gradient: column sums of a 16-bit (M, C) matrix.  Workgroup (64 columns, row chunk): thread = (column pair, one of 32 row
// lanes), fp64 accumulators that meet in LDS in a fixed order; part[chunk][C] fp32
template <typename T>
__global__ __launch_bounds__(1024) void k_colsum_chunk16(const T *__restrict__ a, long M, int C, long rows_per_chunk, float *__restrict__ part) {
    __shared__ double sh[32][64];
    const int cp = threadIdx.x & 31, rl = threadIdx.x >> 5, col = blockIdx.x * 64 + 2 * cp;
    const long r0 = (long)blockIdx.y * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    double s0 = 0.0, s1 = 0.0;
    if (col < C) {
#pragma unroll 4
        for (long r = r0 + rl; r < r1; r += 32) {
            const float2 v = Act<T>::cvt2(Act<T>::ldraw2(a + (size_t)r * C + col));
            s0 += (double)v.x; s1 += (double)v.y;
        }
    }
    sh[rl][2 * cp] = s0; sh[rl][2 * cp + 1] = s1;
    __syncthreads();
    if (threadIdx.x < 64 && blockIdx.x * 64 + threadIdx.x < C) {
        double tsum = 0.0;
#pragma unroll
        for (int i = 0; i < 32; ++i) tsum += sh[i][threadIdx.x];
        part[(size_t)blockIdx.y * C + blockIdx.x * 64 + threadIdx.x] = (float)tsum;
    }
}

// scratch of one layer call, in bytes: [packed 16-bit weights | 16-bit dpre | fp32 dW partials | fp32 db partials], each 16-aligned
struct LayoutSt { size_t wp, dpre, dwp, dbp, total; };
size_t up16(size_t n) { return (n + 15) / 16 * 16; }
LayoutSt layout_st(long M, int Cin, int Cout, int k) {
    LayoutSt l;
    l.wp = 0;
    l.dpre = up16((size_t)k * Cin * Cout * 2);
    l.dwp = l.dpre + up16((size_t)M * Cout * 2);
    l.dbp = l.dwp + (size_t)dw_splits(M, Cin, Cout, k) * Cout * Cin * k * sizeof(float);
    l.total = l.dbp + (size_t)DB_CHUNKS * Cout * sizeof(float);
    return l;
}
bool shape_st_ok(int B, int T, int Cin, int Cout, int k) {
    return B >= 1 && T >= 1 && (long)B * T <= 0x7fffffffL && Cin >= 8 && Cout >= 8 && Cin % 8 == 0 && Cout % 8 == 0 && k >= 1 && k <= 8;
}
int check_shape_st(const char *who, int st, int B, int T, int Cin, int Cout, int k, int d) {
    ST_REQUIRE_STORAGE(who, st);
    WW_REQUIRE(B >= 1 && T >= 1 && (long)B * T <= 0x7fffffffL, WW_E_INVALID, "%s: bad shape B=%d T=%d", who, B, T);
    WW_REQUIRE(Cin >= 8 && Cout >= 8 && Cin % 8 == 0 && Cout % 8 == 0, WW_E_INVALID,
               "%s: channel counts must be positive multiples of 8, got Cin=%d Cout=%d", who, Cin, Cout);
    WW_REQUIRE(k >= 1 && k <= 8, WW_E_INVALID, "%s: kernel_size=%d not in 1..8", who, k);
    WW_REQUIRE(d >= 1, WW_E_INVALID, "%s: dilation=%d must be >= 1", who, d);
    WW_REQUIRE(ew8_ok((long)B * T * Cin) && ew8_ok((long)B * T * Cout), WW_E_INVALID, "%s: tensor too large for 32-bit vector indices", who);
    return WW_OK;
}

}  // namespace

extern "C" size_t ww_tconv1d_st_scratch_bytes(int storage, int B, int T, int Cin, int Cout, int k) {
    if (!storage_ok(storage) || !shape_st_ok(B, T, Cin, Cout, k)) return 0;
    return layout_st((long)B * T, Cin, Cout, k).total;
}

extern "C" int ww_tconv1d_st_fwd(ww_ctx *ctx, int storage, const void *x, const float *w, const float *bias, int B, int T, int Cin,
                                 int Cout, int k, int dilation, int relu, const void *residual, void *y, void *scratch,
                                 size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && bias && y && scratch, WW_E_INVALID, "ww_tconv1d_st_fwd: null argument");
    int rc = check_shape_st("ww_tconv1d_st_fwd", storage, B, T, Cin, Cout, k, dilation);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y) && al16(scratch) && al16(residual), WW_E_INVALID, "ww_tconv1d_st_fwd: tensors must be 16-byte aligned");
    const long M = (long)B * T;
    WW_REQUIRE(scratch_bytes >= layout_st(M, Cin, Cout, k).total, WW_E_WORKSPACE, "ww_tconv1d_st_fwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    const dim3 grid((Cout + 63) / 64, (unsigned)((M + 63) / 64));
    with_mode16(storage, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        typedef typename ModeH<MODE>::type H;
        hipLaunchKernelGGL(k_tap_pack16<H>, dim3(ew_grid((long)k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k, 0, (H *)scratch);
        // a dilation of T or more displaces every tap but the last out of the sample, as T itself does
        const TimeRows16<H> a{(const H *)x, (const H *)scratch, (H *)y, {}, (int)M, Cin, Cout, k, 0, {T, k, -std::min(dilation, T)},
                              {bias, (const H *)residual, relu != 0}};
        hipLaunchKernelGGL((k_tap_rows16<MODE, TimeRows, SumChain, TimeEpi16<H>, Tail16None>), grid, dim3(256), 0, st, a);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_tconv1d_st_bwd(ww_ctx *ctx, int storage, const void *x, const float *w, const void *y, const void *y2, float mask_scale,
                                 const void *dy, int B, int T, int Cin, int Cout, int k, int dilation, void *dx, int accumulate_dx,
                                 float *dw, float *db, void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && dy && dw && db && scratch, WW_E_INVALID, "ww_tconv1d_st_bwd: null argument");
    int rc = check_shape_st("ww_tconv1d_st_bwd", storage, B, T, Cin, Cout, k, dilation);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y) && al16(y2) && al16(dy) && al16(dx) && al16(scratch), WW_E_INVALID,
               "ww_tconv1d_st_bwd: tensors must be 16-byte aligned");
    const long M = (long)B * T;
    const LayoutSt l = layout_st(M, Cin, Cout, k);
    WW_REQUIRE(scratch_bytes >= l.total, WW_E_WORKSPACE, "ww_tconv1d_st_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    unsigned char *base = (unsigned char *)scratch;
    const int d = std::min(dilation, T);
    const void *dpre = dy;
    float *part = (float *)(base + l.dwp), *dbp = (float *)(base + l.dbp);
    const DwRanges rg = dw_ranges16(M, Cin, Cout, k);
    const long n = (long)Cout * Cin * k;
    // the bias gradient's row chunks: at least 32 rows (one per row lane) each
    const int chunks = (int)std::max<long>(1, std::min<long>(DB_CHUNKS, M / 32));
    with_mode16(storage, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        typedef typename ModeH<MODE>::type H;
        if (y || y2 || mask_scale != 1.f) {
            const uint32_t n8 = (uint32_t)(M * Cout / 8);
            hipLaunchKernelGGL(k_tconv_dpre16<H>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, (const uint4 *)dy, (const uint4 *)y,
                               (const uint4 *)y2, mask_scale, (uint4 *)(base + l.dpre));
            dpre = base + l.dpre;
        }
        if (dx) {
            hipLaunchKernelGGL(k_tap_pack16<H>, dim3(ew_grid((long)k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k, 1, (H *)(base + l.wp));
            const TimeRows16<H> a{(const H *)dpre, (const H *)(base + l.wp), (H *)dx, {}, (int)M, Cout, Cin, k, accumulate_dx != 0,
                                  {T, k, d}, {nullptr, nullptr, 0}};
            hipLaunchKernelGGL((k_tap_rows16<MODE, TimeRows, SumChain, TimeEpi16<H>, Tail16None>),
                               dim3((Cin + 63) / 64, (unsigned)((M + 63) / 64)), dim3(256), 0, st, a);
        }
        const Dw16<H, TimeDw> g{(const H *)dpre, (const H *)x, rg.nz > 1 ? part : dw, (int)M, Cout, Cin, k, (int)rg.rps, rg.nz, {T, k, d}};
        hipLaunchKernelGGL((k_tap_dw16<MODE, TimeDw, SumChain>), dim3((Cin + 63) / 64, (Cout + 63) / 64, k * rg.nz), dim3(256), 0, st, g);
        hipLaunchKernelGGL(k_colsum_chunk16<H>, dim3((Cout + 63) / 64, chunks), dim3(1024), 0, st, (const H *)dpre, M, Cout,
                           (M + chunks - 1) / chunks, chunks > 1 ? dbp : db);
    });
    WW_LAUNCH_CHECK();
    if (chunks > 1 && (rc = ww_colsum_rows_small(dbp, chunks, Cout, db, st))) return rc;
    if (rg.nz > 1 && !ww_defer(ctx, part, dw, n, rg.nz, 0)) {
        hipLaunchKernelGGL(k_tap_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, rg.nz, dw);
        WW_LAUNCH_CHECK();
    }
    return WW_OK;
}

extern "C" int ww_dropout_bt_st(ww_ctx *ctx, int storage, const void *x, int B, int T, int C, float p, uint64_t seed, uint64_t step,
                                uint64_t sample_offset, int stream_id, void *out, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && out, WW_E_INVALID, "ww_dropout_bt_st: null argument");
    ST_REQUIRE_STORAGE("ww_dropout_bt_st", storage);
    WW_REQUIRE(B >= 1 && T >= 1 && C >= 8 && C % 8 == 0 && ew8_ok((long)B * T * C), WW_E_INVALID,
               "ww_dropout_bt_st: bad shape (%d,%d,%d): C must be a multiple of 8", B, T, C);
    WW_REQUIRE(T <= 4096 && C <= 1024 && stream_id >= 0 && stream_id < 16, WW_E_UNSUPPORTED,
               "ww_dropout_bt_st: T <= 4096, C <= 1024, stream_id < 16");
    WW_REQUIRE(p >= 0.f && p < 1.f, WW_E_INVALID, "ww_dropout_bt_st: p=%f not in [0,1)", (double)p);
    WW_REQUIRE(al16(x) && al16(out), WW_E_INVALID, "ww_dropout_bt_st: tensors must be 16-byte aligned");
    const uint32_t n8 = (uint32_t)((long)B * T * C / 8);
    with_mode16(storage, [&](auto m) {
        typedef typename ModeH<decltype(m)::value>::type H;
        hipLaunchKernelGGL(k_dropout_bt16<H>, dim3(ew_grid(n8)), dim3(256), 0, (hipStream_t)stream, n8, (const H *)x, T, C / 8,
                           (float)(1.0 / (1.0 - (double)p)), ww_prob_threshold((double)p), (uint32_t)seed, (uint32_t)(seed >> 32),
                           (uint32_t)step, (uint32_t)(step >> 32), sample_offset, (uint32_t)stream_id, (H *)out, ctx->step_ctl);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_add_relu_st_fwd(ww_ctx *ctx, int storage, const void *a, const void *b, size_t n, void *y, ww_stream_t stream) {
    WW_REQUIRE(ctx && a && b && y, WW_E_INVALID, "ww_add_relu_st_fwd: null argument");
    ST_REQUIRE_STORAGE("ww_add_relu_st_fwd", storage);
    WW_REQUIRE(ew8_ok((long)n), WW_E_INVALID, "ww_add_relu_st_fwd: n=%zu must be a positive multiple of 8", n);
    WW_REQUIRE(al16(a) && al16(b) && al16(y), WW_E_INVALID, "ww_add_relu_st_fwd: tensors must be 16-byte aligned");
    const uint32_t n8 = (uint32_t)(n / 8);
    with_mode16(storage, [&](auto m) {
        typedef typename ModeH<decltype(m)::value>::type H;
        hipLaunchKernelGGL(k_add_relu16<H>, dim3(ew_grid(n8)), dim3(256), 0, (hipStream_t)stream, n8, (const H *)a, (const H *)b, (H *)y);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_seq_round_st(ww_ctx *ctx, int storage, const float *x, int B, int T, int F, int transposed, void *out,
                               ww_stream_t stream) {
    WW_REQUIRE(ctx && x && out, WW_E_INVALID, "ww_seq_round_st: null argument");
    ST_REQUIRE_STORAGE("ww_seq_round_st", storage);
    WW_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && F >= 8 && F % 8 == 0 && ew8_ok((long)B * T * F), WW_E_INVALID,
               "ww_seq_round_st: bad shape B=%d T=%d F=%d: F must be a multiple of 8, B <= 65535", B, T, F);
    WW_REQUIRE(al16(out) && (transposed || al16(x)), WW_E_INVALID, "ww_seq_round_st: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n8 = (uint32_t)((long)B * T * F / 8);
    with_mode16(storage, [&](auto m) {
        typedef typename ModeH<decltype(m)::value>::type H;
        if (transposed)
            hipLaunchKernelGGL(k_seq_round_t16<H>, dim3((T + 31) / 32, (F + 63) / 64, B), dim3(256), 0, st, x, F, T, (H *)out);
        else
            hipLaunchKernelGGL(k_seq_round16<H>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, x, (H *)out);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

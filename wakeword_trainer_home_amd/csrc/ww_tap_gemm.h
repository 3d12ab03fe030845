// The 64 x 64-tile "tap GEMM" on the matrix cores that ww_tconv.hip (causal dilated Conv1d) and ww_conv2d.hip (dense Conv2d) are
// two sets of instantiations of.  A convolution over channels-last tensors is nseg K-segments (the taps), each a GEMM whose A rows
// are DISPLACED rows of the tensor being read:
//   rows : C[m][n] (+)= epilogue( sum_seg sum_c A[src(m, seg)][c] W[seg][n][c] )       -- the forward and the dX product
//   dW   : out[z][n][c][seg] = sum_{m in range z} G[m][n] X[src(m, seg)][c]            -- the weight gradient, one tap per workgroup
// A row without a source contributes 0.  What a layer brings, all of it at compile time: a GEOMETRY (what a row is, and where -- if
// anywhere -- segment seg finds its source), a SUMMATION policy (SumChain | SumBlocked) and, for rows, an EPILOGUE.  Everything else
// is here, once: 64 x 64 block tiles, 4 wavefronts x one 32x32 MFMA tile; mode WW_ACT_F32: v_mfma_f32_32x32x2_f32 (an exact fp32
// fma chain, the parity mode); WW_ACT_BF16 / WW_ACT_F16: operands rounded when they are staged into LDS,
// v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation.  All tensors are fp32 in HBM; channel counts are multiples of 4 and buffers
// 16-byte aligned (al16), so every global access is a float4 and a K tail is whole float4s of zeros.  (ww_tap_gemm16.h has the rows / dW
// forms whose operands are ALREADY 16-bit in HBM: the same tiles, lane map, MFMA stage and summation, a staging loop of their own.)
// (A 128 x 128 form of the rows kernel -- each staged byte feeding twice the MFMA work, 224 VGPRs -- was measured on the Conv1d
// layer and dropped: the B = 512 step read 2.27 ms against 2.16 in the 16-bit modes and 3.17 against 3.08 in fp32.)
#pragma once
#include "ww_internal.h"
#include "ww_act.h"
#include <algorithm>
#include <type_traits>

namespace {

typedef short short4v __attribute__((ext_vector_type(4)));

// ---- tile constants of a matrix mode
template <int MODE> struct TapTile {
    static constexpr int KT = MODE ? 64 : 32;                     // K per LDS stage: 16 fp32 MFMAs (2 k each) / 4 16-bit ones (16 k each)
    static constexpr int NV = 64 * KT / 1024;                     // float4 per thread and operand tile
    static constexpr int ES = MODE ? 2 : 4;                       // bytes of an LDS element
    static constexpr int LD_ROWS = MODE ? KT + 8 : KT + 4;        // [row][k] LDS stride (elements): the rows kernel
    static constexpr int LD_DW = MODE ? 64 + 8 : 64 + 4;          // [k][row] LDS stride (elements): the dW kernel
    static constexpr int ROWS_BYTES = 64 * LD_ROWS * ES, DW_BYTES = KT * LD_DW * ES;      // one operand tile
};

// four consecutive elements of an operand tile, rounded to the matrix type on the way into LDS
template <int MODE>
__device__ __forceinline__ void put4(void *lds, int off, float4 v) {
    if constexpr (MODE == 0) {
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(lds) + off) = v;
    } else {
        typedef typename ModeH<MODE>::type H;
        *reinterpret_cast<uint2 *>(reinterpret_cast<H *>(lds) + off) = make_uint2(Act<H>::pack2(v.x, v.y), Act<H>::pack2(v.z, v.w));
    }
}
// 16-bit MFMA operand (rows row0 + lane&31, k = k0 + 8*(lane>>5) .. +7) from a [k][row] tile of stride ld: transposing LDS reads
template <typename H>
__device__ __forceinline__ typename H16<H>::x8 tr_frag(const H *tile, int ld, int k0, int row0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
    const H *base = tile + (k0 + 8 * (g >> 1) + q) * ld + row0 + 16 * (g & 1) + 4 * pp;
    typedef short4v __attribute__((address_space(3))) * lds_p;
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(base));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(base + 4 * ld));
    return __builtin_bit_cast(typename H16<H>::x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- a thread's place in the block tile: wavefront (rh, nh) owns the 32x32 tile at (32 rh, 32 nh), lane = (r, h)
struct TapLane {
    int lane, r, h, rh, nh;
    __device__ TapLane() : lane(threadIdx.x & 63), r(lane & 31), h(lane >> 5), rh(threadIdx.x >> 7), nh((threadIdx.x >> 6) & 1) {}
    __device__ int d_col() const { return 32 * nh + r; }      // the tile column this lane's 16 accumulator registers hold
};
// the D layout of v_mfma_f32_32x32: register reg of lane (r, h) is the element (tap_d_row(reg), d_col()) of the block tile
__device__ __forceinline__ int tap_d_row(const TapLane &t, int reg) { return 32 * t.rh + (reg & 3) + 8 * (reg >> 2) + 4 * t.h; }

// ---- one LDS stage through the matrix cores: acc + A B^T over the stage's KT values of k
// [row][k] tiles (the rows kernel): a fragment is 8 (16-bit) or 1 (fp32) consecutive k of a row
template <int MODE>
__device__ __forceinline__ floatx16 tap_mfma_rows(const void *As, const void *Bs, const TapLane &t, floatx16 acc) {
    constexpr int KT = TapTile<MODE>::KT, LD = TapTile<MODE>::LD_ROWS;
    if constexpr (MODE != 0) {
        typedef typename ModeH<MODE>::type H;
        typedef typename H16<H>::x8 x8;
        const H *pa = reinterpret_cast<const H *>(As) + (32 * t.rh + t.r) * LD + 8 * t.h;
        const H *pb = reinterpret_cast<const H *>(Bs) + (32 * t.nh + t.r) * LD + 8 * t.h;
#pragma unroll
        for (int i = 0; i < KT / 16; ++i)
            acc = H16<H>::mfma32(*reinterpret_cast<const x8 *>(pa + 16 * i), *reinterpret_cast<const x8 *>(pb + 16 * i), acc);
    } else {
        const float *pa = reinterpret_cast<const float *>(As) + (32 * t.rh + t.r) * LD + t.h;
        const float *pb = reinterpret_cast<const float *>(Bs) + (32 * t.nh + t.r) * LD + t.h;
#pragma unroll
        for (int i = 0; i < KT / 2; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * i], pb[2 * i], acc, 0, 0, 0);
    }
    return acc;
}
// [k][row] tiles (the dW kernel: both operands are row-contiguous in memory); the 16-bit modes read them back transposed
template <int MODE>
__device__ __forceinline__ floatx16 tap_mfma_dw(const void *As, const void *Bs, const TapLane &t, floatx16 acc) {
    constexpr int KT = TapTile<MODE>::KT, LD = TapTile<MODE>::LD_DW;
    if constexpr (MODE != 0) {
        typedef typename ModeH<MODE>::type H;
        const H *pa = reinterpret_cast<const H *>(As), *pb = reinterpret_cast<const H *>(Bs);
#pragma unroll
        for (int i = 0; i < KT / 16; ++i)
            acc = H16<H>::mfma32(tr_frag(pa, LD, 16 * i, 32 * t.rh, t.lane), tr_frag(pb, LD, 16 * i, 32 * t.nh, t.lane), acc);
    } else {
        const float *pa = reinterpret_cast<const float *>(As) + t.h * LD + 32 * t.rh + t.r;
        const float *pb = reinterpret_cast<const float *>(Bs) + t.h * LD + 32 * t.nh + t.r;
#pragma unroll
        for (int i = 0; i < KT / 2; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * i * LD], pb[2 * i * LD], acc, 0, 0, 0);
    }
    return acc;
}

// ---- how the stages' sums are combined: a stage's MFMAs start from in() and their result goes to out()
// one MFMA chain through all stages (Conv1d: K = k Cin <= 768 in the model)
struct SumChain {
    floatx16 acc = floatx16{0.f};
    __device__ floatx16 in() const { return acc; }
    __device__ void out(floatx16 s) { acc = s; }
    __device__ void end_tap() {}
    __device__ floatx16 total() const { return acc; }
};
// blocked summation (Conv2d): a stage's KT products are one chain from zero, the stages of a tap are summed per tap, the taps at the
// end -- chains of KT, Cin / KT and k k terms instead of one of k k Cin (4608 in the last ResNet stage), for 16 v_add_f32 per stage
struct SumBlocked {
    floatx16 acc = floatx16{0.f}, tap = floatx16{0.f};
    __device__ floatx16 in() const { return floatx16{0.f}; }
    __device__ void out(floatx16 s) { tap += s; }
    __device__ void end_tap() { acc += tap; tap = floatx16{0.f}; }
    __device__ floatx16 total() const { return acc; }
};

// ---- the stage loop, double-buffered in registers: fetch(it, va, vb) loads stage it of both operands from global memory (NV float4
// each; thread q's float4 is row q / F4, elements 4 (q % F4) .. + 3 of the LDS tile), mfma() consumes the stage in LDS.  Two
// barriers per stage; stage it + 1 is in flight under the MFMAs of stage it.  A fetch zero-fills its registers, then loads under the
// condition with the address formed inside it, and the first fetch is unconditional (every load in it is guarded): in this form all
// loads of a stage are issued before the first is waited for, in the prologue too, and every instantiation stays within the VGPRs
// of its waves-per-SIMD bracket -- the tightest is the fp32 dW kernel of Conv2d, 80 VGPRs + 16 AGPRs = the 96 of five waves.
template <int MODE, int F4, int LD, class Fetch, class Mfma>
__device__ __forceinline__ void tap_stages(void *As, void *Bs, int stages, Fetch &&fetch, Mfma &&mfma) {
    constexpr int NV = TapTile<MODE>::NV;
    const int tid = threadIdx.x;
    float4 va[NV], vb[NV];
    fetch(0, va, vb);
    for (int it = 0; it < stages; ++it) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, off = (q / F4) * LD + 4 * (q % F4);
            put4<MODE>(As, off, va[j]);
            put4<MODE>(Bs, off, vb[j]);
        }
        __syncthreads();
        if (it + 1 < stages) fetch(it + 1, va, vb);
        mfma();
    }
}

// ---- the rows kernel.  grid: x = N tiles, y = M tiles.  CA, N multiples of 4.
//   Geo::Row row(m, M)                 the descriptor of output row m (m >= M: a row that finds no source anywhere), worked out once
//                                      per thread: the rows a thread stages are the same in every stage
//   Geo::Tap tap(seg)                  what segment seg displaces a row by, worked out once per stage
//   bool src(row, m, tap, &at)         whether that segment of the row has a source row, and which row of A it is
//   Epi: auto column(col)              what the epilogue holds per output column;  float operator()(sum, column, index into C)
template <class Geo, class Epi>
struct RowsArgs {
    const float *A;      // the tensor being read, rows of CA floats
    const float *W;      // (nseg, N, CA): k_tap_pack
    float *C;            // (M, N)
    Epi epi;
    int M, CA, N, nseg, accumulate;
    Geo g;
};
template <int MODE, class Geo, class Sum, class Epi>
__global__ __launch_bounds__(256) void k_tap_rows(RowsArgs<Geo, Epi> a) {
    typedef TapTile<MODE> TT;
    constexpr int KT = TT::KT, NV = TT::NV, F4 = KT / 4;           // F4: float4 per tile row
    __shared__ __align__(16) unsigned char lds[2 * TT::ROWS_BYTES];
    void *As = lds, *Bs = lds + TT::ROWS_BYTES;
    const int tid = threadIdx.x;
    const TapLane t;
    const long m0 = (long)blockIdx.y * 64;
    const int n0 = blockIdx.x * 64;
    typename Geo::Row row[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) row[j] = a.g.row(m0 + (tid + 256 * j) / F4, a.M);
    const int nk = (a.CA + KT - 1) / KT;
    auto fetch = [&](int it, float4(&va)[NV], float4(&vb)[NV]) {
        const int seg = it / nk, k0 = (it - seg * nk) * KT;
        const auto tap = a.g.tap(seg);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, kk = k0 + 4 * (q % F4), n = n0 + q / F4;
            va[j] = vb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            long at = 0;
            // (& not &&: the geometry's tests and the K bound make ONE exec-masked region around the load)
            if (a.g.src(row[j], m0 + q / F4, tap, at) & (kk < a.CA)) va[j] = *reinterpret_cast<const float4 *>(a.A + at * a.CA + kk);
            if (n < a.N && kk < a.CA) vb[j] = *reinterpret_cast<const float4 *>(a.W + ((long)seg * a.N + n) * a.CA + kk);
        }
    };
    Sum sum;
    int in_tap = 0;
    tap_stages<MODE, F4, TT::LD_ROWS>(As, Bs, a.nseg * nk, fetch, [&] {
        sum.out(tap_mfma_rows<MODE>(As, Bs, t, sum.in()));
        if (++in_tap == nk) { sum.end_tap(); in_tap = 0; }
    });
    const int col = n0 + t.d_col();
    if (col >= a.N) return;
    const auto ec = a.epi.column(col);
    const floatx16 acc = sum.total();
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const long row = m0 + tap_d_row(t, reg);
        if (row >= a.M) continue;
        float v = a.epi(acc[reg], ec, row * a.N + col);
        if (a.accumulate) v += a.C[row * a.N + col];
        a.C[row * a.N + col] = v;
    }
}
// an epilogue that adds nothing (not even a "+ 0" bias, which would turn a -0 sum into +0)
struct EpiNone {
    struct Col {};
    __device__ Col column(int) const { return Col{}; }
    __device__ float operator()(float v, Col, long) const { return v; }
};

// ---- the dW kernel.  grid: x = c tiles, y = n tiles, z = seg * nsplit + range; range z is the rows [z rps, (z + 1) rps) of M.
//   Geo::Tap tap(seg)                  the displacement of the workgroup's segment
//   bool src(m, tap, &at)              whether row m of G meets a row of X in that segment, and which row of X it is
template <class Geo>
struct DwArgs {
    const float *G;      // the output gradient (M, N)
    const float *X;      // the layer input, rows of C floats
    float *out;          // (nsplit, N, C, nseg)
    int M, N, C, nseg, rps, nsplit;
    Geo g;
};
template <int MODE, class Geo, class Sum>
__global__ __launch_bounds__(256) void k_tap_dw(DwArgs<Geo> a) {
    typedef TapTile<MODE> TT;
    constexpr int KT = TT::KT, NV = TT::NV;
    __shared__ __align__(16) unsigned char lds[2 * TT::DW_BYTES];
    void *As = lds, *Bs = lds + TT::DW_BYTES;
    const int tid = threadIdx.x;
    const TapLane t;
    const int c0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int seg = blockIdx.z / a.nsplit, z = blockIdx.z - seg * a.nsplit;
    const int mb = (int)min((long)a.M, (long)z * a.rps), me = (int)min((long)a.M, (long)mb + a.rps);
    const auto tap = a.g.tap(seg);
    auto fetch = [&](int it, float4(&va)[NV], float4(&vb)[NV]) {
        const int mk0 = mb + it * KT;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = tid + 256 * j, m = mk0 + q / 16, e = 4 * (q % 16);
            const bool okm = m < me;
            va[j] = vb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (okm && n0 + e < a.N) va[j] = *reinterpret_cast<const float4 *>(a.G + (long)m * a.N + n0 + e);
            long at = 0;      // a row past the range looks up row 0, not m: that holds the fp32 Conv2d instantiation at its 80 VGPRs
            const bool hit = a.g.src(okm ? m : 0, tap, at);
            if (okm && c0 + e < a.C && hit) vb[j] = *reinterpret_cast<const float4 *>(a.X + at * a.C + c0 + e);
        }
    };
    Sum sum;
    tap_stages<MODE, 16, TT::LD_DW>(As, Bs, (me - mb + KT - 1) / KT, fetch,
                                    [&] { sum.out(tap_mfma_dw<MODE>(As, Bs, t, sum.in())); });
    sum.end_tap();
    const int c = c0 + t.d_col();
    if (c >= a.C) return;
    const floatx16 acc = sum.total();
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + tap_d_row(t, reg);
        if (n < a.N) a.out[(((long)z * a.N + n) * a.C + c) * a.nseg + seg] = acc[reg];
    }
}

// ---- the weights re-laid per tap, (Cout, Cin, nseg) -- nn.Conv1d's / nn.Conv2d's own layout has the tap as its fastest index:
// out[s][n][c] = w[n][c][s] (transpose == 0: the forward's taps) or out[s][c][n] = w[n][c][s] (the dX product's)
__global__ __launch_bounds__(256) void k_tap_pack(const float *__restrict__ w, int Cout, int Cin, int nseg, int transpose,
                                                  float *__restrict__ out) {
    const long per = (long)Cout * Cin, n_all = per * nseg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_all; i += (long)gridDim.x * 256) {
        const int s = (int)(i / per);
        const long rem = i - (long)s * per;
        int n, c;
        if (transpose) { c = (int)(rem / Cout); n = (int)(rem - (long)c * Cout); }
        else { n = (int)(rem / Cin); c = (int)(rem - (long)n * Cin); }
        out[i] = w[((long)n * Cin + c) * nseg + s];
    }
}
// dst[i] = sum_z part[z*n + i], z in order (the immediate form of the deferred reduction)
__global__ __launch_bounds__(256) void k_tap_sum(const float *__restrict__ part, long n, int splits, float *__restrict__ dst) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        double s = 0.0;
        for (int z = 0; z < splits; ++z) s += (double)part[(long)z * n + i];
        dst[i] = (float)s;
    }
}

// ---- host side
int ew_grid(long n) { return ww_pass_ew(n).grid; }      // (ww_internal.h: what ww_pass_plan reports)
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// f(std::integral_constant<int, MODE>) for the MODE template parameter of a matrix mode
template <class F>
void with_mode(int mode, F &&f) {
    if (mode == WW_ACT_BF16) f(std::integral_constant<int, 1>{});
    else if (mode == WW_ACT_F16) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 0>{});
}
template <class Sum, class Geo, class Epi>
void tap_launch_rows(int mode, const RowsArgs<Geo, Epi> &a, hipStream_t st) {
    const dim3 grid((a.N + 63) / 64, (unsigned)((a.M + 63) / 64));
    with_mode(mode, [&](auto m) { hipLaunchKernelGGL((k_tap_rows<decltype(m)::value, Geo, Sum, Epi>), grid, dim3(256), 0, st, a); });
}
// row ranges of the weight-gradient contraction: enough of them for ~1024 workgroups, each at least 128 rows deep, at most 256
int dw_splits(long M, int Cin, int Cout, int nseg) {
    const long tiles = (long)((Cout + 63) / 64) * ((Cin + 63) / 64) * nseg;
    long s = (1024 + tiles - 1) / tiles;
    s = std::min<long>(s, M / 128);
    return (int)std::max<long>(1, std::min<long>(s, 256));
}
// dw (Cout, Cin, nseg) = the dW product of G (M, Cout) and X: one range writes dw itself; more leave partial products in part
// (dw_splits(...) * Cout * Cin * nseg floats) that are summed in range order, here or -- queued with ww_defer -- by the one flush
template <class Sum, class Geo>
int tap_dw(ww_ctx *ctx, int mode, const float *G, const float *X, const Geo &g, long M, int Cin, int Cout, int nseg, float *part,
           float *dw, hipStream_t st) {
    const int kt = mode == WW_ACT_F32 ? 32 : 64;
    const int want = dw_splits(M, Cin, Cout, nseg);
    const long rps = ((M + want - 1) / want + kt - 1) / kt * kt;      // whole K stages per range
    const int nz = (int)((M + rps - 1) / rps);                         // <= want
    const long n = (long)Cout * Cin * nseg;
    const DwArgs<Geo> a{G, X, nz > 1 ? part : dw, (int)M, Cout, Cin, nseg, (int)rps, nz, g};
    const dim3 grid((Cin + 63) / 64, (Cout + 63) / 64, nseg * nz);
    with_mode(mode, [&](auto m) { hipLaunchKernelGGL((k_tap_dw<decltype(m)::value, Geo, Sum>), grid, dim3(256), 0, st, a); });
    WW_LAUNCH_CHECK();
    if (nz > 1 && !ww_defer(ctx, part, dw, n, nz, 0)) {
        hipLaunchKernelGGL(k_tap_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, nz, dw);
        WW_LAUNCH_CHECK();
    }
    return WW_OK;
}

}  // namespace

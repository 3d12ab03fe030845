// The tap GEMM of ww_tap_gemm.h in the forms whose operands are ALREADY 16-bit in HBM (activation storage S = bf16 | fp16 = the matrix
// mode): the same tiles, lane map, MFMA stage and summation policies, and a staging loop of its own -- KT = 64, so an operand tile
// is 64 rows x 8 uint4 = two 16-byte loads per thread whose halves go into the LDS tile as they are: no conversion in the staging
// loop.  The weights are rounded once, by the per-tap packing pass.  ww_conv2d16.hip (image geometry, SumBlocked, no epilogue, a
// BatchNorm-statistics tail) and ww_tconv16.hip (time geometry, SumChain, bias | residual | ReLU epilogue, no tail) are two sets of
// instantiations of this text.  Channel counts are multiples of 8: a 16-byte access is 8 elements.
//   rows : C[m][n] = S( epi( sum_seg sum_c A[src(m, seg)][c] W[seg][n][c] ) (+ float(C[m][n])) )
//   dW   : out[z][n][c][seg] = sum_{m in range z} G[m][n] X[src(m, seg)][c], fp32
#pragma once
#include "ww_tap_gemm.h"

namespace {

constexpr int KT16 = 64;
template <class Fetch, class Mfma>
__device__ __forceinline__ void stages16(void *As, void *Bs, int ld, int stages, Fetch &&fetch, Mfma &&mfma) {
    const int tid = threadIdx.x;
    uint4 va[2], vb[2];
    fetch(0, va, vb);
    for (int it = 0; it < stages; ++it) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = tid + 256 * j, off = ((q >> 3) * ld + 8 * (q & 7)) * 2;      // bytes
            *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(As) + off) = va[j];
            *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(Bs) + off) = vb[j];
        }
        __syncthreads();
        if (it + 1 < stages) fetch(it + 1, va, vb);
        mfma();
    }
}

// ---- what a rows instantiation brings besides its geometry and summation
//   Epi : auto column(col)                       what the epilogue holds for the column PAIR (col, col + 1), col even
//         float2 operator()(sums, column, at)    the pair's values from its sums; at = the index of (row, col) in C
//   Tail: void run<MODE>(acc, lane, m0, n0, M, N, tile row)   work on the whole accumulator tile ahead of the store (uniform)
struct Epi16None {
    struct Col {};
    __device__ Col column(int) const { return Col{}; }
    __device__ float2 operator()(float2 v, Col, long) const { return v; }
};
struct Tail16None {
    template <int MODE> __device__ void run(const floatx16 &, const TapLane &, long, int, int, int, int) const {}
};
// forward statistics from the epilogue: per column the fp32 sums of the 64 rows' STORED values and of their squares, in a fixed
// order -- the lane's 16 registers, then the two lane halves (rows 4h .. of each group of 8), then the two row wavefronts through
// LDS.  Rows past M and columns past N hold zeros.  (part is uniform: every thread of the grid takes the same branch.)
struct Tail16Stats {
    float *part;     // nullable: [M tile][sum (N) | sum of squares (N)] of the ROUNDED values of the tile's rows (BatchNorm's statistics)
    template <int MODE> __device__ void run(const floatx16 &acc, const TapLane &t, long m0, int n0, int M, int N, int tile) const {
        typedef typename ModeH<MODE>::type H;
        if (part) {
            __shared__ float sh[2][2][64];
            const int tid = threadIdx.x;
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v = Act<H>::round1(acc[reg]);
                if (m0 + tap_d_row(t, reg) < M) { s += v; q = fmaf(v, v, q); }
            }
            const float s1 = __shfl_xor(s, 32), q1 = __shfl_xor(q, 32);
            if (t.h == 0) { sh[0][t.rh][t.d_col()] = s + s1; sh[1][t.rh][t.d_col()] = q + q1; }
            __syncthreads();
            if (tid < 64 && n0 + tid < N) {
                float *p = part + (long)tile * 2 * N + n0 + tid;
                p[0] = sh[0][0][tid] + sh[0][1][tid];
                p[N] = sh[1][0][tid] + sh[1][1][tid];
            }
        }
    }
};

// ---- rows.  grid: x = N tiles, y = M tiles.
template <typename H, class Geo, class Epi, class Tail>
struct Rows16 {
    const H *A;      // the tensor being read, rows of CA elements
    const H *W;      // (nseg, N, CA): k_tap_pack16
    H *C;            // (M, N)
    Tail tail;
    int M, CA, N, nseg, accumulate;
    Geo g;
    Epi epi;
};
template <int MODE, class Geo, class Sum, class Epi, class Tail>
__global__ __launch_bounds__(256) void k_tap_rows16(Rows16<typename ModeH<MODE>::type, Geo, Epi, Tail> a) {
    typedef TapTile<MODE> TT;
    typedef typename ModeH<MODE>::type H;
    __shared__ __align__(16) unsigned char lds[2 * TT::ROWS_BYTES];
    void *As = lds, *Bs = lds + TT::ROWS_BYTES;
    const int tid = threadIdx.x;
    const TapLane t;
    const long m0 = (long)blockIdx.y * 64;
    const int n0 = blockIdx.x * 64;
    typename Geo::Row row[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) row[j] = a.g.row(m0 + ((tid + 256 * j) >> 3), a.M);
    const int nk = (a.CA + KT16 - 1) / KT16;
    auto fetch = [&](int it, uint4(&va)[2], uint4(&vb)[2]) {
        const int seg = it / nk, k0 = (it - seg * nk) * KT16;
        const auto tap = a.g.tap(seg);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = tid + 256 * j, kk = k0 + 8 * (q & 7), n = n0 + (q >> 3);
            va[j] = vb[j] = make_uint4(0u, 0u, 0u, 0u);
            long at = 0;
            if (a.g.src(row[j], m0 + (q >> 3), tap, at) & (kk < a.CA)) va[j] = *reinterpret_cast<const uint4 *>(a.A + at * a.CA + kk);
            if (n < a.N && kk < a.CA) vb[j] = *reinterpret_cast<const uint4 *>(a.W + ((long)seg * a.N + n) * a.CA + kk);
        }
    };
    Sum sum;
    int in_tap = 0;
    stages16(As, Bs, TT::LD_ROWS, a.nseg * nk, fetch, [&] {
        sum.out(tap_mfma_rows<MODE>(As, Bs, t, sum.in()));
        if (++in_tap == nk) { sum.end_tap(); in_tap = 0; }
    });
    // a lane holds ONE column of 16 rows; neighbouring lanes hold neighbouring columns.  Lanes (2i, 2i + 1) trade every other register,
    // after which the even lane holds both columns of the even registers' rows and the odd lane those of the odd registers' rows: eight
    // 4-byte stores per lane instead of sixteen 2-byte ones
    const floatx16 acc = sum.total();
    a.tail.template run<MODE>(acc, t, m0, n0, a.M, a.N, (int)blockIdx.y);
    const int odd = t.lane & 1;
    float lo[8], hi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float got = __shfl_xor(odd ? acc[2 * i] : acc[2 * i + 1], 1);
        lo[i] = odd ? got : acc[2 * i];
        hi[i] = odd ? acc[2 * i + 1] : got;
    }
    const int col = n0 + (t.d_col() & ~1);
    if (col >= a.N) return;                        // (N is even: both columns of a pair are in range or neither is)
    const auto ec = a.epi.column(col);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long r = m0 + tap_d_row(t, 2 * i + odd);
        if (r >= a.M) continue;
        H *p = a.C + r * a.N + col;
        float2 v = a.epi(make_float2(lo[i], hi[i]), ec, r * a.N + col);
        if (a.accumulate) {
            const float2 o = Act<H>::cvt2(Act<H>::ldraw2(p));
            v.x += o.x; v.y += o.y;
        }
        Act<H>::st2(p, v);
    }
}

// ---- dW.  grid: x = c tiles, y = n tiles, z = seg * nsplit + range
template <typename H, class Geo>
struct Dw16 {
    const H *G;      // the output gradient (M, N)
    const H *X;      // the layer input, rows of C elements
    float *out;      // (nsplit, N, C, nseg)
    int M, N, C, nseg, rps, nsplit;
    Geo g;
};
template <int MODE, class Geo, class Sum>
__global__ __launch_bounds__(256) void k_tap_dw16(Dw16<typename ModeH<MODE>::type, Geo> a) {
    typedef TapTile<MODE> TT;
    __shared__ __align__(16) unsigned char lds[2 * TT::DW_BYTES];
    void *As = lds, *Bs = lds + TT::DW_BYTES;
    const int tid = threadIdx.x;
    const TapLane t;
    const int c0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int seg = blockIdx.z / a.nsplit, z = blockIdx.z - seg * a.nsplit;
    const int mb = (int)min((long)a.M, (long)z * a.rps), me = (int)min((long)a.M, (long)mb + a.rps);
    const auto tap = a.g.tap(seg);
    auto fetch = [&](int it, uint4(&va)[2], uint4(&vb)[2]) {
        const int mk0 = mb + it * KT16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = tid + 256 * j, m = mk0 + (q >> 3), e = 8 * (q & 7);
            const bool okm = m < me;
            va[j] = vb[j] = make_uint4(0u, 0u, 0u, 0u);
            if (okm && n0 + e < a.N) va[j] = *reinterpret_cast<const uint4 *>(a.G + (long)m * a.N + n0 + e);
            long at = 0;
            const bool hit = a.g.src(okm ? m : 0, tap, at);
            if (okm && c0 + e < a.C && hit) vb[j] = *reinterpret_cast<const uint4 *>(a.X + at * a.C + c0 + e);
        }
    };
    Sum sum;
    stages16(As, Bs, TT::LD_DW, (me - mb + KT16 - 1) / KT16, fetch, [&] { sum.out(tap_mfma_dw<MODE>(As, Bs, t, sum.in())); });
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

// k_tap_pack with the weights rounded to the matrix type on the way: out[s][n][c] | out[s][c][n] = S(w[n][c][s])
template <typename H>
__global__ __launch_bounds__(256) void k_tap_pack16(const float *__restrict__ w, int Cout, int Cin, int nseg, int transpose,
                                                    H *__restrict__ out) {
    const long per = (long)Cout * Cin, n_all = per * nseg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_all; i += (long)gridDim.x * 256) {
        const int s = (int)(i / per);
        const long rem = i - (long)s * per;
        int n, c;
        if (transpose) { c = (int)(rem / Cout); n = (int)(rem - (long)c * Cout); }
        else { n = (int)(rem / Cin); c = (int)(rem - (long)n * Cin); }
        reinterpret_cast<uint16_t *>(out)[i] = (uint16_t)Act<H>::pack2(w[((long)n * Cin + c) * nseg + s], 0.f);
    }
}

// ---- 8 consecutive elements of a 16-bit (or fp32) tensor
template <typename T> __device__ __forceinline__ void ld8(const T *p, float (&v)[8]) {
    const uint4 r = *reinterpret_cast<const uint4 *>(p);
    const float2 a = Act<T>::cvt2(r.x), b = Act<T>::cvt2(r.y), c = Act<T>::cvt2(r.z), d = Act<T>::cvt2(r.w);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y; v[6] = d.x; v[7] = d.y;
}
__device__ __forceinline__ void ld8(const float *p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T> __device__ __forceinline__ void st8(T *p, const float (&v)[8]) {
    Act<T>::st8(p, make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
}

// ---- host side
// f(std::integral_constant<int, MODE>), MODE = 1 | 2, for a storage code the caller has checked
template <class F>
void with_mode16(int st, F &&f) {
    if (st == WW_ACT_BF16) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}
bool storage_ok(int st) { return st == WW_ACT_BF16 || st == WW_ACT_F16; }
#define ST_REQUIRE_STORAGE(who, st) \
    WW_REQUIRE(storage_ok(st), WW_E_INVALID, "%s: storage must be WW_ACT_BF16 or WW_ACT_F16, got %d", who, st)
// elementwise launches: n elements, 8 per thread, at most 4096 workgroups
bool ew8_ok(long n) { return n >= 8 && n % 8 == 0 && n / 8 < (1L << 31); }
// the dW row ranges of tap_dw (ww_tap_gemm.h) for a 16-bit launch: whole K stages per range
struct DwRanges { long rps; int nz; };
DwRanges dw_ranges16(long M, int Cin, int Cout, int nseg) {
    const int want = dw_splits(M, Cin, Cout, nseg);
    const long rps = ((M + want - 1) / want + KT16 - 1) / KT16 * KT16;
    return DwRanges{rps, (int)((M + rps - 1) / rps)};
}

}  // namespace

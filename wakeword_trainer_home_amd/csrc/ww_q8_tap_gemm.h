// The int8 "tap GEMM" on v_mfma_i32_16x16x64_i8 that the TCN's Conv1d (ww_q8_tcn.hip), the ResNet's Conv2d (ww_q8_resnet.hip), the
// LSTM / GRU input projection (ww_q8_lstm.hip) and MobileNetV3's 1x1 convs (ww_q8_mobilenet.hip) are instantiations of -- the int8
// counterpart of ww_tap_gemm.h.  A layer is nseg K-segments (the taps), each a GEMM over K = geo.K() input channels, a multiple of
// 64, whose B rows are DISPLACED rows of the tensor being read; weights are (Cout, nseg, K) int8 [out][tap][in].  What a layer
// brings, all of it at compile time:
//   a GEOMETRY  N, nseg(), K(); Row: what row n is (Row::n is the row, past the end included); Src: where -- if anywhere -- segment
//               j of a row finds its source; load(): the 16-byte B fragment of K chunk kc, or the input's zero point where the row
//               has no source (a displaced time or pixel outside the tensor, a row past the end).  The geometry owns the load, so a
//               transform of the fragment (MobileNetV3's fused squeeze-excitation gate) is a geometry like any other.
//   an EPILOGUE derived from Q8Chan: begin(), once per workgroup (a table into LDS), and store(acc, n, c0): the lane's 16 sums of
//               the LIVE row n, channels c0 .. c0 + 15, to memory.  q8_tap_store is the frame of the int8 ones.
//   RT          16-row tiles a wave holds at once: a weight fragment it loaded meets RT row fragments
//   SLAB        the weights of a channel tile come from the workgroup's LDS image (k_q8_tap_lds) or stream through L2 (k_q8_tap)
//
// The lane map (DESIGN.md mfma_i8_map): D = A x B, A = weights (row = output channel), B = rows (column = row l & 15 of the tile).
// Lane l, p = l & 15, g = l >> 4, supplies, for segment j and K chunk kc, the 16 bytes [64 kc + 16 g, + 16) of the source of ITS
// row, and the same 16 k of weight row 16 (p >> 2) + 4 m + (p & 3) for product m = 0..3.  The accumulator puts D rows 4 g .. 4 g + 3
// of column p in lane l, so the lane ends with the sixteen consecutive channels 64 ct + 16 g .. + 15 of its row: one 16-byte store
// of int8.  bias is the EFFECTIVE bias q_b - z_in * sum(q_w) (host, once per bundle), which is what makes "no source" a vector of
// z_in bytes.  All adds that may wrap are unsigned.
#pragma once
#include "ww_q8_common.h"

namespace {

constexpr int Q8T_BLOCK = 256;
constexpr int Q8T_WAVES = Q8T_BLOCK / 64;
constexpr size_t Q8T_SLAB_FITS = 144 * 1024;   // largest weight image of a channel tile k_q8_tap_lds can hold (K = 256 at 9 taps)

struct Q8Chan {                                // what every epilogue reads: (Cout) int32 each, and the row stride of the output
    const int *bias, *mult, *shift;
    int Cout;
    __device__ void begin() const {}
};

// The int8 epilogues' frame: q = fin(R(acc + bias, mult, shift), h) per channel, h the byte of hv (a residual vector, or anything)
// at that channel; one 16-byte store.
template <class FIN>
__device__ __forceinline__ void q8_tap_store(const Q8Chan &c, const v4i (&acc)[4], v4i hv, int8_t *out, long n, int c0, FIN fin) {
    v4i ov;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const v4i b = *(const v4i *)(c.bias + c0 + 4 * m);
        const v4i mu = *(const v4i *)(c.mult + c0 + 4 * m);
        const v4i sh = *(const v4i *)(c.shift + c0 + 4 * m);
        int h[4], q[4];
        q8_unpack4(hv[m], h);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = fin(q8_round((int)((unsigned)acc[m][e] + (unsigned)b[e]), mu[e], sh[e]), h[e]);
        ov[m] = q8_pack4(q[0], q[1], q[2], q[3]);
    }
    *(v4i *)(out + n * c.Cout + c0) = ov;
}

// The one-segment geometry: row n of the product reads row n of `in` (N, K).
struct Q8Rows {
    const int8_t *in;
    long N;
    int Kin, zfill;                            // zfill: the input's zero point in all four bytes
    struct Row { long n; };
    struct Src { const int8_t *p; bool live; };
    __device__ int nseg() const { return 1; }
    __device__ int K() const { return Kin; }
    __device__ void row(long n, Row &r) const { r.n = n; }
    __device__ void seg(const Row &r, int, int g, Src &s) const {
        s.live = r.n < N;
        s.p = in + r.n * Kin + 16 * g;         // dereferenced only where live
    }
    __device__ v4i load(const Src &s, int kc) const {
        v4i bq = {zfill, zfill, zfill, zfill};
        if (s.live) bq = *(const v4i *)(s.p + 64 * kc);
        return bq;
    }
};

// One item: 16 RT rows from row0 on, output channels [64 ct, 64 ct + 64).
template <class GEO, class EPI, int RT, bool SLAB>
__device__ __forceinline__ void q8_tap_item(const GEO &geo, const EPI &epi, const int8_t *w, int ct, long row0, int lane,
                                            const v4i *slab) {
    const int p = lane & 15, g = lane >> 4;
    const int nseg = geo.nseg(), K = geo.K(), kcn = K / 64;
    const long wstride = (long)nseg * K;
    typename GEO::Row row[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) geo.row(row0 + 16 * r + p, row[r]);
    const int8_t *wrow[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) wrow[m] = w + (long)(64 * ct + 16 * (p >> 2) + 4 * m + (p & 3)) * wstride + 16 * g;
    v4i acc[RT][4];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[r][m] = v4i{0, 0, 0, 0};
    for (int j = 0; j < nseg; ++j) {
        typename GEO::Src src[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) geo.seg(row[r], j, g, src[r]);
        for (int kc = 0; kc < kcn; ++kc) {
            v4i wa[4];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                wa[m] = SLAB ? slab[((j * kcn + kc) * 4 + m) * 64 + lane] : *(const v4i *)(wrow[m] + (long)j * K + 64 * kc);
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const v4i bq = geo.load(src[r], kc);
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[r][m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[m], bq, acc[r][m], 0, 0, 0);
            }
        }
    }
    const int c0 = 64 * ct + 16 * g;
#pragma unroll
    for (int r = 0; r < RT; ++r)
        if (row[r].n < geo.N) epi.store(acc[r], row[r].n, c0);
}

// weights streamed through L2: persistent over (row group, channel tile) items, one per wave and trip
template <class GEO, class EPI, int RT> __global__ __launch_bounds__(Q8T_BLOCK) void k_q8_tap(GEO geo, EPI epi, const int8_t *w) {
    epi.begin();
    const int ctn = epi.Cout / 64;
    const long items = (geo.N + 16 * RT - 1) / (16 * RT) * ctn;
    for (long item = (long)blockIdx.x * Q8T_WAVES + (threadIdx.x >> 6); item < items; item += (long)gridDim.x * Q8T_WAVES)
        q8_tap_item<GEO, EPI, RT, false>(geo, epi, w, (int)(item % ctn), item / ctn * (16 * RT), threadIdx.x & 63, nullptr);
}

// weights of one channel tile resident in LDS, in FRAGMENT order: vector ((j kcn + kc) 4 + m) 64 + l is what lane l feeds product m
// of segment j, K chunk kc -- any 16 lanes of a ds_read_b128 group read 16 distinct 16-byte slots, so the reads are conflict-free.
// The grid is ctstep x (row workgroups): ctstep == Cout / 64 gives a workgroup ONE channel tile for its life, ctstep == 1 (a grid
// smaller than that) makes every workgroup walk all the tiles.  Persistent over row groups.
template <class GEO, class EPI, int RT>
__global__ __launch_bounds__(Q8T_BLOCK) void k_q8_tap_lds(GEO geo, EPI epi, const int8_t *w, int ctstep) {
    extern __shared__ v4i q8_slab[];
    epi.begin();
    const int ctn = epi.Cout / 64, nvec = geo.nseg() * (geo.K() / 64) * 256;
    const long groups = (geo.N + 16 * RT - 1) / (16 * RT), wstride = (long)geo.nseg() * geo.K();
    const int rwg = blockIdx.x / ctstep, nrwg = gridDim.x / ctstep;
    for (int ct = blockIdx.x % ctstep; ct < ctn; ct += ctstep) {
        __syncthreads();                                        // every wave is done with the previous tile's image
        for (int idx = threadIdx.x; idx < nvec; idx += Q8T_BLOCK) {
            const int l = idx & 63, m = (idx >> 6) & 3, chunk = idx >> 8;           // chunk = j kcn + kc: 64 bytes of a weight row
            const int wr = 64 * ct + 16 * ((l & 15) >> 2) + 4 * m + (l & 3);
            q8_slab[idx] = *(const v4i *)(w + wr * wstride + 64 * chunk + 16 * (l >> 4));
        }
        __syncthreads();
        for (long grp = (long)rwg * Q8T_WAVES + (threadIdx.x >> 6); grp < groups; grp += (long)nrwg * Q8T_WAVES)
            q8_tap_item<GEO, EPI, RT, true>(geo, epi, w, ct, grp * (16 * RT), threadIdx.x & 63, q8_slab);
    }
}

// ---- the launchers: the grid is what fits the machine (ww_conv_grid), at most one wave per item
template <class GEO, class EPI, int RT> int q8_tap_launch_stream(ww_ctx *ctx, const GEO &geo, const EPI &epi, const int8_t *w, hipStream_t st) {
    const long items = (geo.N + 16 * RT - 1) / (16 * RT) * (epi.Cout / 64);
    const int grid = ww_conv_grid(ctx, (const void *)k_q8_tap<GEO, EPI, RT>, Q8T_BLOCK, 0, (items + Q8T_WAVES - 1) / Q8T_WAVES, 1 << 20);
    hipLaunchKernelGGL((k_q8_tap<GEO, EPI, RT>), dim3(grid), dim3(Q8T_BLOCK), 0, st, geo, epi, w);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

// slab: the weight image of one channel tile, 64 nseg K bytes, at most Q8T_SLAB_FITS.  The launch asks for the next multiple of
// 16 KB, so the occupancy query sees few distinct sizes.
template <class GEO, class EPI, int RT>
int q8_tap_launch_lds(ww_ctx *ctx, const GEO &geo, const EPI &epi, const int8_t *w, size_t slab, hipStream_t st) {
    const int ctn = epi.Cout / 64;
    const long groups = (geo.N + 16 * RT - 1) / (16 * RT);
    const size_t smem = (slab + 16383) / 16384 * 16384;
    const void *fn = (const void *)k_q8_tap_lds<GEO, EPI, RT>;
    if (smem > 64 * 1024) WW_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Q8T_SLAB_FITS));
    int grid = ww_conv_grid(ctx, fn, Q8T_BLOCK, smem, (groups + Q8T_WAVES - 1) / Q8T_WAVES * ctn, 1 << 20);
    const int ctstep = grid >= ctn ? ctn : 1;
    grid -= grid % ctstep;
    hipLaunchKernelGGL((k_q8_tap_lds<GEO, EPI, RT>), dim3(grid), dim3(Q8T_BLOCK), smem, st, geo, epi, w, ctstep);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

template <class GEO, class EPI, int RT>
int q8_tap_launch(ww_ctx *ctx, const GEO &geo, const EPI &epi, const int8_t *w, bool lds, size_t slab, hipStream_t st) {
    return lds ? q8_tap_launch_lds<GEO, EPI, RT>(ctx, geo, epi, w, slab, st) : q8_tap_launch_stream<GEO, EPI, RT>(ctx, geo, epi, w, st);
}

}  // namespace

// The ResNet18Wakeword layers with bf16 / fp16 ACTIVATION STORAGE: every (B,H,W,C) tensor between the stem convolution and the global
// mean, and every gradient of one, is S = bf16 | fp16 in HBM (the `_st` entry points of wwhip.h; ww_conv2d.hip is the fp32-storage
// path).  The contract: arithmetic is fp32, a value is rounded (RNE, Act<S>::pack2) exactly where a tensor is stored and nowhere
// else, and BatchNorm statistics are taken from the STORED values (ww_act.h), finished in fp64 from fp32 partials.
//   * Conv2d: the 16-bit tap GEMM of ww_tap_gemm16.h (operands already of the matrix cores' type in HBM) with the image geometry of
//     ww_image.h, blocked summation, no epilogue and the statistics tail.  The weights are rounded once, by the per-tap packing pass.
//     The rows kernel stores S(acc) (S(acc + float(C)) when it accumulates); the dW kernel leaves fp32 partials for the existing sum
//     / ww_defer path.  With a partials pointer the forward rows kernel also leaves the per-column sums of its tile's STORED values
//     and their squares.
//   * BatchNorm(+activation): those partials (folded once when there are more than 1024 tiles), or a column-statistics pass over the
//     16-bit tensor where no producer left any (the stem) -> k_bn_finish (ww_nhwc.hip) -> one apply pass that can
//     add a residual, plain or with a scale|shift of its own: the block tail relu(bn2(c2) + (x | bn_d(cd))) is ONE pass with one
//     rounding.  Backward: the two passes of ww_bn_act_bwd on 16-bit x, da, dx; on small layers the apply pass finishes the sums.
//   * stem, max-pool (ww_image.h's kernels at T = S), the (B,HW,C) -> (B,C) mean and its gradient, the ReLU mask.
// Channel counts are multiples of 8: a 16-byte access is 8 elements.
#include "ww_image.h"
#include "ww_layers.h"
#include "ww_tap_gemm16.h"

namespace {

// ---- column statistics of a tall 16-bit (M, C) matrix: thread = (8 columns, row lane), one workgroup per row chunk, fp64
// accumulators that meet in LDS in a fixed order.  part[chunk][0:C | C:2C] (fp32) =
//   BWD == false: sum x, sum x^2                          (BatchNorm forward)
//   BWD == true : sum dz, sum dz xhat, dz = da act'(z)    (BatchNorm backward)
// grid = chunks, block 256, smem = 2 R C doubles (R = 256 / (C / 8) row lanes)
constexpr int ST_CHUNKS = 1024;
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void k_colstats16(const T *__restrict__ x, const T *__restrict__ da, const float *__restrict__ ss,
                                                    const float *__restrict__ mr, long M, int C, int act, long rows_per_chunk,
                                                    float *__restrict__ part) {
    extern __shared__ double red[];
    const int C8 = C >> 3, R = 256 / C8, cq = threadIdx.x % C8, r = threadIdx.x / C8;
    const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    double s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.0;
    float sc[8], sf[8], mu[8], rs[8];
    if constexpr (BWD) {
        ld8(ss + 8 * cq, sc); ld8(ss + C + 8 * cq, sf); ld8(mr + 8 * cq, mu); ld8(mr + C + 8 * cq, rs);
    }
    if (r < R)
        for (long rb = r0 + r; rb < r1; rb += 4L * R) {        // batches of four (clamped, unconditional) row loads
            float xv[4][8], dv[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long o = min(rb + (long)u * R, r1 - 1) * C + 8 * cq;
                ld8(x + o, xv[u]);
                if constexpr (BWD) ld8(da + o, dv[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (rb + (long)u * R < r1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if constexpr (BWD) {
                            const float dz = dv[u][e] * lin_act_grad(act, fmaf(xv[u][e], sc[e], sf[e]));
                            s[e] += dz;
                            q[e] += (double)dz * (double)((xv[u][e] - mu[e]) * rs[e]);
                        } else {
                            const double d = xv[u][e];
                            s[e] += d; q[e] += d * d;
                        }
                    }
                }
        }
    if (r < R) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { red[(2 * r) * C + 8 * cq + e] = s[e]; red[(2 * r + 1) * C + 8 * cq + e] = q[e]; }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * C; o += 256) {
        const int which = o >= C, c = o - which * C;
        double a = 0.0;
        for (int i = 0; i < R; ++i) a += red[(2 * i + which) * C + c];
        part[(long)blockIdx.x * 2 * C + o] = (float)a;
    }
}

// second level of the epilogue statistics: `rows` tile partials [rows][cols] -> out[ST_FOLD][cols], out row j = the sum of the rows
// [j per, (j + 1) per) in order (fp64, rounded once), so that one finish launch never walks more than ST_CHUNKS rows
constexpr int ST_FOLD = 256;
__global__ __launch_bounds__(256) void k_part_fold(const float *__restrict__ part, int rows, int cols, int per, float *__restrict__ out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < ST_FOLD * cols; i += gridDim.x * 256) {
        const int j = i / cols, c = i - j * cols;
        double a = 0.0;
        for (int r = j * per; r < min(rows, (j + 1) * per); ++r) a += (double)part[(long)r * cols + c];
        out[i] = (float)a;
    }
}

// y = S(act(fma(x, scale, shift) + idn)), idn = 0 | res | fma(res, rscale, rshift): n8 vectors of 8 elements
template <typename T>
__global__ __launch_bounds__(256) void k_bn_apply16(uint32_t n8, const T *__restrict__ x, const float *__restrict__ ss,
                                                    const T *__restrict__ res, const float *__restrict__ rss, int C, int act,
                                                    T *__restrict__ y) {
    const uint32_t C8 = (uint32_t)C >> 3;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const int c = (int)(i % C8) * 8;
        float v[8], sc[8], sf[8];
        ld8(x + (size_t)i * 8, v); ld8(ss + c, sc); ld8(ss + C + c, sf);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], sc[e], sf[e]);
        if (res) {
            float rv[8];
            ld8(res + (size_t)i * 8, rv);
            if (rss) {
                ld8(rss + c, sc); ld8(rss + C + c, sf);
#pragma unroll
                for (int e = 0; e < 8; ++e) rv[e] = fmaf(rv[e], sc[e], sf[e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += rv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = lin_act(act, v[e]);
        st8(y + (size_t)i * 8, v);
    }
}
// dx = S(bnact_bwd_one(x, da, ...)): the second pass of ww_bn_act_bwd
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_apply16(uint32_t n8, const T *__restrict__ x, const T *__restrict__ da,
                                                        const float *__restrict__ ss, const float *__restrict__ mr,
                                                        const float *__restrict__ sums, long M, int C, int act, int training,
                                                        T *__restrict__ dx) {
    const uint32_t C8 = (uint32_t)C >> 3;
    const float invM = 1.0f / (float)M;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const int c = (int)(i % C8) * 8;
        float xv[8], dv[8], sc[8], sf[8], mu[8], rs[8], s1[8] = {}, s2[8] = {}, o[8];
        ld8(x + (size_t)i * 8, xv); ld8(da + (size_t)i * 8, dv);
        ld8(ss + c, sc); ld8(ss + C + c, sf); ld8(mr + c, mu); ld8(mr + C + c, rs);
        if (training) { ld8(sums + c, s1); ld8(sums + C + c, s2); }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = bnact_bwd_one(xv[e], dv[e], sc[e], sf[e], mu[e], rs[e], s1[e], s2[e], invM, act, training);
        st8(dx + (size_t)i * 8, o);
    }
}
// the same pass finishing the statistics pass's chunk partials itself (the 16-bit twin of k_bnact_bwd_apply_fin, for the same small
// layers: 2 launches instead of 3).  A workgroup owns (row chunk, group of CG4 channel float4s = CG4 / 2 octets); every workgroup sums
// the group's partial columns in the same fixed order.  grid G_r * G_c, block 256: thread = (octet of the group's channels, row lane)
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_apply_fin16(const T *__restrict__ x, const T *__restrict__ da,
                                                            const float *__restrict__ part, int chunks, long M, int C, BnTile t,
                                                            const float *__restrict__ ss, const float *__restrict__ mr, int act,
                                                            T *__restrict__ dx, float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double redd[256 * 4];
    __shared__ double tot[128];
    __shared__ __align__(16) float sums[128];
    const int gc = blockIdx.x % t.G_c, c0 = gc * 4 * t.CG4, CG = 4 * t.CG4;
    const long rc = blockIdx.x / t.G_c;
    bn_group_totals(part, chunks, C, c0, t.CG4, tot, redd);
    if (threadIdx.x < CG) {
        const float s1 = (float)tot[threadIdx.x], s2 = (float)tot[CG + threadIdx.x];
        sums[threadIdx.x] = s1; sums[CG + threadIdx.x] = s2;
        if (rc == 0 && c0 + threadIdx.x < C) { dbeta[c0 + threadIdx.x] = s1; dgamma[c0 + threadIdx.x] = s2; }
    }
    __syncthreads();
    const int CG8 = t.CG4 >> 1, R = 256 / CG8, cq = threadIdx.x % CG8, rl = threadIdx.x / CG8;
    if (rl >= R || c0 + 8 * cq >= C) return;
    const size_t col = (size_t)c0 + 8 * cq;
    float sc[8], sf[8], mu[8], rs[8], s1[8], s2[8];
    ld8(ss + col, sc); ld8(ss + C + col, sf); ld8(mr + col, mu); ld8(mr + C + col, rs);
    ld8(sums + 8 * cq, s1); ld8(sums + CG + 8 * cq, s2);
    const float invM = 1.0f / (float)M;
    const long r0 = rc * t.rows_per_block, r1 = min(M, r0 + t.rows_per_block);
    for (long rb = r0 + rl; rb < r1; rb += 2L * R) {               // batches of two (clamped, unconditional) row loads
        float xv[2][8], dv[2][8], o[8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const size_t at = (size_t)min(rb + (long)u * R, r1 - 1) * C + col;
            ld8(x + at, xv[u]); ld8(da + at, dv[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (rb + (long)u * R < r1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = bnact_bwd_one(xv[u][e], dv[u][e], sc[e], sf[e], mu[e], rs[e], s1[e], s2[e], invM, act, 1);
                st8(dx + (size_t)(rb + (long)u * R) * C + col, o);
            }
    }
}
// dx = dy where y != 0, else 0 (16-bit words: a value is zero when its 15 low bits are)
__global__ __launch_bounds__(256) void k_relu_mask16(uint32_t n8, const uint4 *__restrict__ dy, const uint4 *__restrict__ y,
                                                     uint4 *__restrict__ dx) {
    auto keep = [](uint32_t d, uint32_t v) {
        return d & ((v & 0x7fffu ? 0xffffu : 0u) | (v & 0x7fff0000u ? 0xffff0000u : 0u));
    };
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const uint4 d = dy[i], v = y[i];
        dx[i] = make_uint4(keep(d.x, v.x), keep(d.y, v.y), keep(d.z, v.z), keep(d.w, v.w));
    }
}
// the mean over HW of (B, HW, C) -> (B, C) fp32: one workgroup per (image, 64 channels), 16 row lanes, fixed-order sum in LDS
template <typename T>
__global__ __launch_bounds__(1024) void k_mean16(const T *__restrict__ x, int B, int HW, int C, float *__restrict__ s) {
    __shared__ double sh[16][64];
    const int cl = threadIdx.x & 63, part = threadIdx.x >> 6, cg = (C + 63) / 64;
    const int b = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + cl;
    double a = 0.0;
    if (c < C) {
        const T *p = x + (size_t)b * HW * C + c;
#pragma unroll 8
        for (int h = part; h < HW; h += 16) a += (double)(float)p[(size_t)h * C];
    }
    sh[part][cl] = a;
    __syncthreads();
    if (part == 0 && c < C) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += sh[i][cl];
        s[(size_t)b * C + c] = (float)(t / HW);
    }
}
// its gradient: dx[b][hw][c] = S(dpool[b][c] / HW)
template <typename T>
__global__ __launch_bounds__(256) void k_mean_bwd16(uint32_t n8, const float *__restrict__ dpool, uint32_t HWC8, int HW, int C,
                                                    T *__restrict__ dx) {
    const uint32_t C8 = (uint32_t)C >> 3;
    const float hw = (float)HW;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const uint32_t b = i / HWC8, c = (i % C8) * 8;
        float v[8];
        ld8(dpool + (size_t)b * C + c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] / hw;
        st8(dx + (size_t)i * 8, v);
    }
}

// ---- host side
// f(T *) with T = the storage type of code st (WW_ACT_BF16 | WW_ACT_F16; the callers have refused everything else)
template <class F>
void with_storage(int st, F &&f) {
    if (st == WW_ACT_BF16) f((ww_bf16 *)nullptr);
    else f((ww_f16 *)nullptr);
}
// the image layer's instantiations of the 16-bit tap GEMM
template <typename H, bool DX> using ImageRows16 = Rows16<H, ImageRows<DX>, Epi16None, Tail16Stats>;

struct Layout16 { size_t wp_bytes, total_bytes; };      // [packed 16-bit weights | fp32 dW partials]
Layout16 layout16(long M, int Cin, int Cout, int k) {
    Layout16 l;
    l.wp_bytes = ((size_t)k * k * Cin * Cout * 2 + 15) / 16 * 16;
    l.total_bytes = l.wp_bytes + (size_t)dw_splits(M, Cin, Cout, k * k) * Cout * Cin * k * k * sizeof(float);
    return l;
}
bool shape16_ok(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    return B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= 0x7fffffffL && Cin >= 8 && Cout >= 8 && Cin % 8 == 0 && Cout % 8 == 0 &&
           k >= 1 && k <= 7 && (k & 1) && (stride == 1 || stride == 2);
}
int check_shape16(const char *who, int st, int B, int H, int W, int Cin, int Cout, int k, int stride) {
    ST_REQUIRE_STORAGE(who, st);
    WW_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= 0x7fffffffL, WW_E_INVALID, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    WW_REQUIRE(Cin >= 8 && Cout >= 8 && Cin % 8 == 0 && Cout % 8 == 0, WW_E_INVALID,
               "%s: channel counts must be positive multiples of 8, got Cin=%d Cout=%d", who, Cin, Cout);
    WW_REQUIRE(k >= 1 && k <= 7 && (k & 1), WW_E_INVALID, "%s: kernel_size=%d is not an odd number in 1..7", who, k);
    WW_REQUIRE(stride == 1 || stride == 2, WW_E_INVALID, "%s: stride=%d is not 1 or 2", who, stride);
    return WW_OK;
}
// the layers whose backward apply pass finishes the statistics itself: those of ww_bn_act_bwd (ww_nhwc.hip), by element count
constexpr long ST_FUSED_MAX = 4L << 20;
// row chunks of the column statistics: each row lane of a chunk gets at least four rows; at most 256 chunks (what one workgroup of
// the finishing apply pass re-reads) for the small layers, ST_CHUNKS for the tall ones
int st_chunks(long M, int C) {
    const int R = 256 / (C / 8);
    return (int)std::max<long>(1, std::min<long>(M * C <= ST_FUSED_MAX ? 256 : ST_CHUNKS, M / (4L * R)));
}
int check_bn16(const char *who, int st, long M, int C) {
    ST_REQUIRE_STORAGE(who, st);
    WW_REQUIRE(M >= 1 && C >= 8 && C % 8 == 0 && C <= 1024, WW_E_INVALID, "%s: bad shape (%ld,%d): C must be a multiple of 8 in 8..1024",
               who, M, C);
    WW_REQUIRE(ew8_ok(M * C), WW_E_INVALID, "%s: tensor too large for 32-bit vector indices", who);
    return WW_OK;
}

}  // namespace

extern "C" size_t ww_conv2d_st_scratch_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    if (!shape16_ok(B, H, W, Cin, Cout, k, stride)) return 0;
    return layout16((long)B * out_size(H, k, stride) * out_size(W, k, stride), Cin, Cout, k).total_bytes;
}

extern "C" int ww_conv2d_st_fwd(ww_ctx *ctx, int storage, const void *x, const float *w, int B, int H, int W, int Cin, int Cout, int k,
                                int stride, void *y, float *stat_part, void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && y && scratch, WW_E_INVALID, "ww_conv2d_st_fwd: null argument");
    int rc = check_shape16("ww_conv2d_st_fwd", storage, B, H, W, Cin, Cout, k, stride);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y) && al16(scratch), WW_E_INVALID, "ww_conv2d_st_fwd: tensors must be 16-byte aligned");
    const int Ho = out_size(H, k, stride), Wo = out_size(W, k, stride);
    const long M = (long)B * Ho * Wo;
    WW_REQUIRE(scratch_bytes >= layout16(M, Cin, Cout, k).total_bytes, WW_E_WORKSPACE, "ww_conv2d_st_fwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    const dim3 grid((Cout + 63) / 64, (unsigned)((M + 63) / 64));
    with_mode16(storage, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        typedef typename ModeH<MODE>::type Hh;
        hipLaunchKernelGGL(k_tap_pack16<Hh>, dim3(ew_grid((long)k * k * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, k * k, 0, (Hh *)scratch);
        const ImageRows16<Hh, false> a{(const Hh *)x, (const Hh *)scratch, (Hh *)y, {stat_part}, (int)M, Cin, Cout, k * k, 0,
                                       {Ho, Wo, H, W, k, stride, k / 2}, {}};
        hipLaunchKernelGGL((k_tap_rows16<MODE, ImageRows<false>, SumBlocked, Epi16None, Tail16Stats>), grid, dim3(256), 0, st, a);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_conv2d_st_bwd(ww_ctx *ctx, int storage, const void *x, const float *w, const void *dy, int B, int H, int W, int Cin,
                                int Cout, int k, int stride, void *dx, int accumulate_dx, float *dw, void *scratch,
                                size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && dy && dw && scratch, WW_E_INVALID, "ww_conv2d_st_bwd: null argument");
    int rc = check_shape16("ww_conv2d_st_bwd", storage, B, H, W, Cin, Cout, k, stride);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(dy) && al16(dx) && al16(scratch), WW_E_INVALID, "ww_conv2d_st_bwd: tensors must be 16-byte aligned");
    const int Ho = out_size(H, k, stride), Wo = out_size(W, k, stride), kk = k * k;
    const long M = (long)B * Ho * Wo;
    const Layout16 l = layout16(M, Cin, Cout, k);
    WW_REQUIRE(scratch_bytes >= l.total_bytes, WW_E_WORKSPACE, "ww_conv2d_st_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_LINEAR, st);
    float *part = (float *)((unsigned char *)scratch + l.wp_bytes);
    const DwRanges rg = dw_ranges16(M, Cin, Cout, kk);
    const long rps = rg.rps;
    const int nz = rg.nz;
    const long n = (long)Cout * Cin * kk;
    with_mode16(storage, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        typedef typename ModeH<MODE>::type Hh;
        if (dx) {
            hipLaunchKernelGGL(k_tap_pack16<Hh>, dim3(ew_grid((long)kk * Cin * Cout)), dim3(256), 0, st, w, Cout, Cin, kk, 1, (Hh *)scratch);
            const long Mx = (long)B * H * W;
            const ImageRows16<Hh, true> a{(const Hh *)dy, (const Hh *)scratch, (Hh *)dx, {nullptr}, (int)Mx, Cout, Cin, kk,
                                          accumulate_dx != 0, {H, W, Ho, Wo, k, stride, k / 2}, {}};
            hipLaunchKernelGGL((k_tap_rows16<MODE, ImageRows<true>, SumBlocked, Epi16None, Tail16Stats>),
                               dim3((Cin + 63) / 64, (unsigned)((Mx + 63) / 64)), dim3(256), 0, st, a);
        }
        const Dw16<Hh, ImageDw> d{(const Hh *)dy, (const Hh *)x, nz > 1 ? part : dw, (int)M, Cout, Cin, kk, (int)rps, nz,
                                  {Ho, Wo, H, W, k, stride, k / 2}};
        hipLaunchKernelGGL((k_tap_dw16<MODE, ImageDw, SumBlocked>), dim3((Cin + 63) / 64, (Cout + 63) / 64, kk * nz), dim3(256), 0, st, d);
    });
    WW_LAUNCH_CHECK();
    if (nz > 1 && !ww_defer(ctx, part, dw, n, nz, 0)) {
        hipLaunchKernelGGL(k_tap_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, nz, dw);
        WW_LAUNCH_CHECK();
    }
    return WW_OK;
}

extern "C" int ww_bn_act_st_fwd(ww_ctx *ctx, int storage, const void *x, long M, int C, const ww_bn_t *bn, int act, const void *res,
                                const float *res_ss, const float *stat_part, long stat_rows, void *y, float *ss, float *mr, void *scratch,
                                ww_stream_t stream) {
    WW_REQUIRE(ctx && x && bn && bn->gamma && bn->beta && ss && mr && scratch, WW_E_INVALID, "ww_bn_act_st_fwd: null argument");
    int rc = check_bn16("ww_bn_act_st_fwd", storage, M, C);
    if (rc) return rc;
    WW_REQUIRE(bn->training || (bn->running_mean && bn->running_var), WW_E_INVALID, "ww_bn_act_st_fwd: eval needs running statistics");
    WW_REQUIRE(act >= WW_LIN_NONE && act <= WW_LIN_HARDSIGMOID, WW_E_INVALID, "ww_bn_act_st_fwd: unknown activation %d", act);
    WW_REQUIRE(res || !res_ss, WW_E_INVALID, "ww_bn_act_st_fwd: res_ss without res");
    WW_REQUIRE(!stat_part || (stat_rows >= 1 && stat_rows <= 0x7fffffffL / (2 * C)), WW_E_INVALID, "ww_bn_act_st_fwd: bad stat_rows %ld", stat_rows);
    WW_REQUIRE(al16(x) && al16(y) && al16(res) && al16(ss) && al16(res_ss), WW_E_INVALID, "ww_bn_act_st_fwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    const float *part = (const float *)scratch;
    int chunks = st_chunks(M, C);
    const int R = 256 / (C / 8);
    const uint32_t n8 = (uint32_t)(M * C / 8);
    if (bn->training && stat_part) {
        // the producer's partials (ww_conv2d_st_fwd): as they are, or folded to ST_FOLD rows when there are more than one finish takes
        part = stat_part;
        chunks = (int)stat_rows;
        if (stat_rows > ST_CHUNKS) {
            const int per = (int)((stat_rows + ST_FOLD - 1) / ST_FOLD);
            hipLaunchKernelGGL(k_part_fold, dim3(ew_grid((long)ST_FOLD * 2 * C)), dim3(256), 0, st, stat_part, (int)stat_rows, 2 * C, per,
                               (float *)scratch);
            WW_LAUNCH_CHECK();
            part = (const float *)scratch;
            chunks = ST_FOLD;
        }
    } else if (bn->training) {
        with_storage(storage, [&](auto *tp) {
            typedef std::remove_pointer_t<decltype(tp)> T;
            hipLaunchKernelGGL((k_colstats16<T, false>), dim3(chunks), dim3(256), (size_t)2 * R * C * sizeof(double), st, (const T *)x,
                               (const T *)nullptr, (const float *)nullptr, (const float *)nullptr, M, C, 0, (M + chunks - 1) / chunks,
                               (float *)scratch);
        });
        WW_LAUNCH_CHECK();
    }
    // (eval: nothing was launched and `part` is never read -- k_bn_finish takes the running statistics)
    rc = ww_bn_finish_launch(part, chunks, M, C, bn, ss, mr, st);
    if (rc || !y) return rc;
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_bn_apply16<T>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, (const T *)x, (const float *)ss, (const T *)res, res_ss, C,
                           act, (T *)y);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_bn_act_st_bwd(ww_ctx *ctx, int storage, const void *x, const void *da, long M, int C, const float *ss, const float *mr,
                                int act, int training, void *dx, float *dgamma, float *dbeta, void *scratch, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && da && ss && mr && dx && dgamma && dbeta && scratch, WW_E_INVALID, "ww_bn_act_st_bwd: null argument");
    int rc = check_bn16("ww_bn_act_st_bwd", storage, M, C);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(da) && al16(dx) && al16(ss) && al16(mr) && al16(scratch), WW_E_INVALID,
               "ww_bn_act_st_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    float *part = (float *)scratch, *sums = part + (size_t)ST_CHUNKS * 2 * C;
    const int chunks = st_chunks(M, C), R = 256 / (C / 8);
    const uint32_t n8 = (uint32_t)(M * C / 8);
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL((k_colstats16<T, true>), dim3(chunks), dim3(256), (size_t)2 * R * C * sizeof(double), st, (const T *)x, (const T *)da,
                           ss, mr, M, C, act, (M + chunks - 1) / chunks, part);
    });
    WW_LAUNCH_CHECK();
    const BnTile t = training && M * C <= ST_FUSED_MAX && al16(part) ? bn_tile(M, C, chunks) : BnTile{0, 0, 0, 0};
    if (t.CG4 && t.CG4 % 2 == 0) {                 // (whole octets per channel group)
        const int blocks = (int)((M + t.rows_per_block - 1) / t.rows_per_block) * t.G_c;
        with_storage(storage, [&](auto *tp) {
            typedef std::remove_pointer_t<decltype(tp)> T;
            hipLaunchKernelGGL(k_bn_bwd_apply_fin16<T>, dim3(blocks), dim3(256), 0, st, (const T *)x, (const T *)da, (const float *)part, chunks,
                               M, C, t, ss, mr, act, (T *)dx, dgamma, dbeta);
        });
        WW_LAUNCH_CHECK();
        return WW_OK;
    }
    rc = ww_bnact_bwd_finish_launch(part, chunks, C, sums, dgamma, dbeta, st);
    if (rc) return rc;
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_bn_bwd_apply16<T>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, (const T *)x, (const T *)da, ss, mr, (const float *)sums,
                           M, C, act, training, (T *)dx);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_conv2d_stem_st_fwd(ww_ctx *ctx, int storage, const float *x, const float *w, int B, int H, int W, int C, int k,
                                     int stride, void *y, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && w && y, WW_E_INVALID, "ww_conv2d_stem_st_fwd: null argument");
    ST_REQUIRE_STORAGE("ww_conv2d_stem_st_fwd", storage);
    WW_REQUIRE(C % 8 == 0, WW_E_INVALID, "ww_conv2d_stem_st_fwd: channel count must be a multiple of 8, got C=%d", C);
    StemArgs g;
    int rc = check_stem("ww_conv2d_stem_st_fwd", B, H, W, C, k, stride, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(y), WW_E_INVALID, "ww_conv2d_stem_st_fwd: y must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_conv2d_stem_fwd<T>, dim3(stem_blocks(g, 2048)), dim3(256), 0, st, x, w, g, (T *)y);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_conv2d_stem_st_bwd_dw(ww_ctx *ctx, int storage, const float *x, const void *dy, int B, int H, int W, int C, int k,
                                        int stride, float *dw, void *scratch, size_t scratch_bytes, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && dy && dw && scratch, WW_E_INVALID, "ww_conv2d_stem_st_bwd_dw: null argument");
    ST_REQUIRE_STORAGE("ww_conv2d_stem_st_bwd_dw", storage);
    WW_REQUIRE(C % 8 == 0, WW_E_INVALID, "ww_conv2d_stem_st_bwd_dw: channel count must be a multiple of 8, got C=%d", C);
    StemArgs g;
    int rc = check_stem("ww_conv2d_stem_st_bwd_dw", B, H, W, C, k, stride, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(dy), WW_E_INVALID, "ww_conv2d_stem_st_bwd_dw: dy must be 16-byte aligned");
    WW_REQUIRE(scratch_bytes >= ww_conv2d_stem_scratch_bytes(C, k), WW_E_WORKSPACE, "ww_conv2d_stem_st_bwd_dw: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    const int blocks = stem_blocks(g, STEM_DW_BLOCKS);
    const long n = (long)C * k * k;
    float *part = (float *)scratch;
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_conv2d_stem_dw<T>, dim3(blocks, k), dim3(256), 0, st, x, (const T *)dy, g, blocks > 1 ? part : dw);
    });
    WW_LAUNCH_CHECK();
    if (blocks > 1 && !ww_defer(ctx, part, dw, n, blocks, 0)) {
        hipLaunchKernelGGL(k_tap_sum, dim3(ew_grid(n)), dim3(256), 0, st, part, n, blocks, dw);
        WW_LAUNCH_CHECK();
    }
    return WW_OK;
}

extern "C" int ww_maxpool3x3s2_st_fwd(ww_ctx *ctx, int storage, const void *x, int B, int H, int W, int C, void *y, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && y, WW_E_INVALID, "ww_maxpool3x3s2_st_fwd: null argument");
    ST_REQUIRE_STORAGE("ww_maxpool3x3s2_st_fwd", storage);
    WW_REQUIRE(C % 8 == 0, WW_E_INVALID, "ww_maxpool3x3s2_st_fwd: C must be a multiple of 8, got C=%d", C);
    PoolArgs g;
    int rc = check_pool("ww_maxpool3x3s2_st_fwd", B, H, W, C, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(y), WW_E_INVALID, "ww_maxpool3x3s2_st_fwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_maxpool_fwd<T>, dim3(ew_grid((long)B * g.Ho * g.Wo * (C / 4))), dim3(256), 0, st, (const T *)x, g, (T *)y);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_maxpool3x3s2_st_bwd(ww_ctx *ctx, int storage, const void *x, const void *dy, int B, int H, int W, int C, void *dx,
                                      ww_stream_t stream) {
    WW_REQUIRE(ctx && x && dy && dx, WW_E_INVALID, "ww_maxpool3x3s2_st_bwd: null argument");
    ST_REQUIRE_STORAGE("ww_maxpool3x3s2_st_bwd", storage);
    WW_REQUIRE(C % 8 == 0, WW_E_INVALID, "ww_maxpool3x3s2_st_bwd: C must be a multiple of 8, got C=%d", C);
    PoolArgs g;
    int rc = check_pool("ww_maxpool3x3s2_st_bwd", B, H, W, C, &g);
    if (rc) return rc;
    WW_REQUIRE(al16(x) && al16(dy) && al16(dx), WW_E_INVALID, "ww_maxpool3x3s2_st_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_maxpool_bwd<T>, dim3(ew_grid((long)B * H * W * (C / 4))), dim3(256), 0, st, (const T *)x, (const T *)dy, g, (T *)dx);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_mean_hw_st_fwd(ww_ctx *ctx, int storage, const void *x, int B, int HW, int C, float *mean, ww_stream_t stream) {
    WW_REQUIRE(ctx && x && mean, WW_E_INVALID, "ww_mean_hw_st_fwd: null argument");
    ST_REQUIRE_STORAGE("ww_mean_hw_st_fwd", storage);
    WW_REQUIRE(B >= 1 && HW >= 1 && C >= 8 && C % 8 == 0, WW_E_INVALID, "ww_mean_hw_st_fwd: bad shape (%d,%d,%d): C must be a multiple of 8",
               B, HW, C);
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_mean16<T>, dim3(B * ((C + 63) / 64)), dim3(1024), 0, st, (const T *)x, B, HW, C, mean);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_mean_hw_st_bwd(ww_ctx *ctx, int storage, const float *dmean, int B, int HW, int C, void *dx, ww_stream_t stream) {
    WW_REQUIRE(ctx && dmean && dx, WW_E_INVALID, "ww_mean_hw_st_bwd: null argument");
    ST_REQUIRE_STORAGE("ww_mean_hw_st_bwd", storage);
    WW_REQUIRE(B >= 1 && HW >= 1 && C >= 8 && C % 8 == 0 && ew8_ok((long)B * HW * C), WW_E_INVALID,
               "ww_mean_hw_st_bwd: bad shape (%d,%d,%d): C must be a multiple of 8", B, HW, C);
    WW_REQUIRE(al16(dmean) && al16(dx), WW_E_INVALID, "ww_mean_hw_st_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    const uint32_t n8 = (uint32_t)((long)B * HW * C / 8);
    with_storage(storage, [&](auto *tp) {
        typedef std::remove_pointer_t<decltype(tp)> T;
        hipLaunchKernelGGL(k_mean_bwd16<T>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, dmean, (uint32_t)((long)HW * C / 8), HW, C, (T *)dx);
    });
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_relu_mask_st_bwd(ww_ctx *ctx, int storage, const void *dy, const void *y, size_t n, void *dx, ww_stream_t stream) {
    WW_REQUIRE(ctx && dy && y && dx, WW_E_INVALID, "ww_relu_mask_st_bwd: null argument");
    ST_REQUIRE_STORAGE("ww_relu_mask_st_bwd", storage);
    WW_REQUIRE(ew8_ok((long)n), WW_E_INVALID, "ww_relu_mask_st_bwd: n=%zu must be a positive multiple of 8", n);
    WW_REQUIRE(al16(dy) && al16(y) && al16(dx), WW_E_INVALID, "ww_relu_mask_st_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ww_prof_scope ps_(ctx, WW_K_NHWC, st);
    const uint32_t n8 = (uint32_t)(n / 8);
    hipLaunchKernelGGL(k_relu_mask16, dim3(ew_grid(n8)), dim3(256), 0, st, n8, (const uint4 *)dy, (const uint4 *)y, (uint4 *)dx);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

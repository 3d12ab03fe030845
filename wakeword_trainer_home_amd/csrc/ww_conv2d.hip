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
// queued with ww_defer).  The geometry and the stem / pool kernels live in ww_image.h, which ww_conv2d16.hip (16-bit activation storage)
// shares.
#include "ww_image.h"

namespace {

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
    hipLaunchKernelGGL(k_conv2d_stem_fwd<float>, dim3(stem_blocks(g, 2048)), dim3(256), 0, st, x, w, g, y);
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
    hipLaunchKernelGGL(k_conv2d_stem_dw<float>, dim3(blocks, k), dim3(256), 0, st, x, dy, g, blocks > 1 ? part : dw);
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
    hipLaunchKernelGGL(k_maxpool_fwd<float>, dim3(ew_grid((long)B * g.Ho * g.Wo * (C / 4))), dim3(256), 0, st, x, g, y);
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
    hipLaunchKernelGGL(k_maxpool_bwd<float>, dim3(ew_grid((long)B * H * W * (C / 4))), dim3(256), 0, st, x, dy, g, dx);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

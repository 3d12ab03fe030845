// Operand staging shared by the 64 x 64-tile MFMA kernels of ww_tconv.hip and ww_conv2d.hip: the matrix mode of a kernel, the
// rounding store into an LDS tile and the transposing LDS read of a 16-bit fragment.
#pragma once
#include "ww_act.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef short short4v __attribute__((ext_vector_type(4)));
// matrix mode of a kernel: 0 = fp32 MFMA, 1 = bf16, 2 = fp16 operands (fp32 accumulation)
template <int MODE> struct ModeH { typedef ww_bf16 type; };
template <> struct ModeH<2> { typedef ww_f16 type; };

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

}  // namespace

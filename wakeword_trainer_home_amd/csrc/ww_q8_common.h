// What every int8 inference file (ww_q8*.hip) shares: the rounding law of DESIGN.md "Export", the clamps, the byte and int16
// packing of a lane's registers, the table look-up of the recurrences, and the host-side size and range helpers.
#pragma once
#include "ww_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

// R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh, arithmetic shift; |a| < 2^31, 2^30 <= m < 2^31, 1 <= sh <= 62: |a m| < 2^62
__device__ __forceinline__ long long q8_round(int a, int m, int sh) {
    return ((long long)a * (long long)m + (1ll << (sh - 1))) >> sh;
}

__device__ __forceinline__ int q8_clamp(long long r) {        // clamp(-128 + r, -128, 127): a tensor whose zero point is -128
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    return (int)r - 128;
}

__device__ __forceinline__ int q8_clamp_signed(long long r) { return (int)(r < -128 ? -128 : (r > 127 ? 127 : r)); }

template <int J> __device__ __forceinline__ int q8_byte(int d) { return (int)(signed char)((unsigned)d >> (8 * J)); }

__device__ __forceinline__ int q8_pack4(int a, int b, int c, int d) {
    return (int)((unsigned)(a & 255) | ((unsigned)(b & 255) << 8) | ((unsigned)(c & 255) << 16) | ((unsigned)(d & 255) << 24));
}

__device__ __forceinline__ void q8_unpack4(int d, int (&q)[4]) {
    q[0] = q8_byte<0>(d); q[1] = q8_byte<1>(d); q[2] = q8_byte<2>(d); q[3] = q8_byte<3>(d);
}

__device__ __forceinline__ int q8_pack16(int a, int b) { return (int)(((unsigned)a & 0xffffu) | ((unsigned)b << 16)); }
__device__ __forceinline__ int q8_lo16(int d) { return (int)(short)(d & 0xffff); }
__device__ __forceinline__ int q8_hi16(int d) { return d >> 16; }

// look(tab, a) = tab[clamp(a, -2048, 2047) + 2048]
__device__ __forceinline__ int q8_look(const int16_t *tab, long long a) {
    const int i = a < -2048 ? -2048 : (a > 2047 ? 2047 : (int)a);
    return (int)tab[i + 2048];
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline long q8_round256(long n) { return (n + 255) / 256 * 256; }
inline int q8_pad64(int c) { return (c + 63) / 64 * 64; }
inline bool q8_mult_ok(int m, int sh) { return m >= (1 << 30) && sh >= 1 && sh <= 62; }

}  // namespace

// f8.hpp — f32 <-> OCP E4M3 "fn" (VSG_SCALAR_F8) in plain bit arithmetic, host and device.
//
// E4M3: S.EEEE.MMM, bias 7; E = 0 is subnormal (M x 2^-9), S.1111.111 is NaN, there are no
// infinities and the largest finite value is S.1111.110 = 448.  The rounding contract of
// include/vsg.h: nearest, ties to even; NaN stays NaN; everything else at or beyond 448 in
// magnitude (464 would round to the NaN code) saturates to +-448.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSG_F8_HD __host__ __device__ __forceinline__
#else
#define VSG_F8_HD inline
#endif

namespace vsg {

VSG_F8_HD uint32_t f8_bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
VSG_F8_HD float f8_float_of(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}

VSG_F8_HD uint8_t f8_encode(float v) {
    const uint32_t u = f8_bits_of(v);
    const uint32_t sign = (u >> 24) & 0x80u;
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu);   // NaN
    if (a >= 0x43e00000u) return (uint8_t)(sign | 0x7eu);  // |v| >= 448 (inf too): saturate
    if (a < 0x3c800000u) {
        // |v| < 2^-6, the subnormal range of step 2^-9: adding 2^14 (ulp 2^-9 in f32) rounds
        // |v| to that step, ties to even, and leaves the count 0..8 in the low mantissa bits
        // (8 = 0.0001.000, the smallest normal)
        const float m = f8_float_of(a) + 16384.0f;
        return (uint8_t)(sign | (f8_bits_of(m) - 0x46800000u));
    }
    // normal range: re-bias the exponent (127 -> 7) and drop 20 mantissa bits; 0x7ffff plus
    // the lowest kept bit carries exactly when the dropped part is above, or at and odd
    // below, the midpoint, and the carry runs on into the exponent (at most up to 448)
    const uint32_t t = a - (120u << 23);
    return (uint8_t)(sign | ((t + 0x7ffffu + ((t >> 20) & 1u)) >> 20));
}

// exact widening
VSG_F8_HD float f8_decode(uint8_t b) {
    const uint32_t sign = (uint32_t)(b & 0x80u) << 24;
    const uint32_t mag = b & 0x7fu;
    if (mag == 0x7fu) return f8_float_of(sign | 0x7fc00000u);
    if (mag < 8u) return f8_float_of(sign | f8_bits_of((float)mag * 0.001953125f));  // M x 2^-9
    return f8_float_of(sign | ((mag << 20) + (120u << 23)));
}

}  // namespace vsg

// mfma_tile.hpp — what the matrix-core exact kernels (mfma_exact.hip, mfma_exact_f16.hip,
// mfma_exact_wide.hip) share: the swizzle of a 128-B LDS row, the LDS-DMA pointer types
// and the per-lane sorted top-KMAX list (the first two only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vsg_device.hpp"

namespace vsg {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// The K = 16 matrix instruction of a 2-byte storage type: one 16-B chunk is a lane's
// whole operand V, and both instructions take the same operand layout at the same
// rate, so a kernel written for one runs the other by swapping this trait alone.
template <typename T> struct Mfma16;
template <> struct Mfma16<_Float16> {
    typedef _Float16 V __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ floatx16 mma(V a, V b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma16<bf16_t> {
    typedef __bf16 V __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ floatx16 mma(V a, V b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

// 16-B slot of logical chunk c (0..7) in LDS row R: XOR swizzle so the sixteen
// lanes of a ds_read_b128 group (rows R..R+15, same chunk) hit distinct slots of
// the 64-bank row (conflict-free); applied to the glds SOURCE and to the read.
__device__ __forceinline__ int swz(int R, int c) { return c ^ ((R >> 1) & 7); }

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&ld)[KMAX], uint32_t (&li)[KMAX], float d, uint32_t id) {
    // ascending list, strict < : an equal distance from a later (larger) slot goes after
#pragma unroll
    for (int t = KMAX - 1; t >= 1; --t) {
        const bool shift = d < ld[t - 1];
        const bool here = !shift && d < ld[t];
        ld[t] = shift ? ld[t - 1] : (here ? d : ld[t]);
        li[t] = shift ? li[t - 1] : (here ? id : li[t]);
    }
    if (d < ld[0]) {
        ld[0] = d;
        li[0] = id;
    }
}

}  // namespace vsg

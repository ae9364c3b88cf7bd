// mfma_tile.hpp — what the matrix-core exact kernels (mfma_exact.hip, mfma_exact_f16.hip,
// mfma_exact_wide.hip) share: the swizzle of a 128-B LDS row, the LDS-DMA pointer types
// and the per-lane sorted top-KMAX list (the first two only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vsg {

typedef float floatx16 __attribute__((ext_vector_type(16)));

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

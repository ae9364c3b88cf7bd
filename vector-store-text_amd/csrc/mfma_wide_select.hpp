// mfma_wide_select.hpp — the selection of the wide-k matrix-core exact kernel
// (mfma_exact_wide.hip): a result list of up to 128 entries per query fits neither the
// registers (128 queries x 128 entries x 8 B = 128 KiB per block) nor the LDS a block has
// beside its two K stages, so a block keeps per query
//   LDS:     a threshold tau and a count;
//   memory:  a candidate pool of POOL packed (distance, slot) keys per (query, split).
// tau is an upper bound of the k-th smallest distance among the split's rows seen so far
// (+inf until k live rows were seen).  A distance survives when it is strictly below tau:
// rows arrive in increasing slot order, so an equal distance from a later slot loses, as
// topk_insert decides it.  Survivors are appended at a slot taken from the LDS count; a
// tile appends at most 128 per query, so a pool whose count passed POOL - 128 is
// compacted before the next tile: one wave sorts it by (distance, slot) in an LDS scratch
// (bitonic network), writes the first k back in order and sets tau to the k-th distance.
// Invariants: the pool always holds the k best rows seen, tau never falls below the true
// k-th distance, the count never passes POOL.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vsg {

// (distance, slot) -> one 64-bit key whose unsigned order is the (distance, slot) order:
// the float's bits made monotone (sign flipped; negative values inverted) above the slot.
// -0.0 is folded into +0.0 first, so that equal distances give equal high words.
__device__ __forceinline__ uint64_t wide_key(float d, uint32_t slot) {
    uint32_t u = __float_as_uint(d + 0.f);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((uint64_t)u << 32) | slot;
}
__device__ __forceinline__ float wide_key_dist(uint64_t key) {
    uint32_t u = (uint32_t)(key >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(u);
}
constexpr uint64_t WIDE_KEY_NONE = ~0ull;  // sorts behind every entry (its distance would be a NaN)

// orders one wave's LDS traffic across its lanes: the wave's ds operations execute in
// order, so only the compiler has to be kept from moving them
__device__ __forceinline__ void wide_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One wave: the `n` (wave-uniform, <= POOL) keys of `pool` sorted ascending in
// `scratch` (POOL keys of LDS, this wave's own); returns with scratch readable by
// every lane.  Sorts the next power of two >= max(n, 128), padded with WIDE_KEY_NONE.
template <int POOL>
__device__ __forceinline__ void wide_sort_pool(const uint64_t* pool, int n, uint64_t* scratch, int lane) {
    int N = 128;
    while (N < n) N <<= 1;  // <= POOL: n <= POOL, a power of two
    // the entries were stored by all four waves of the block: device-scope loads, so that
    // none is served from a line this compute unit cached at an earlier compaction
    for (int i = lane; i < N; i += 64)
        scratch[i] = i < n ? __hip_atomic_load(pool + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : WIDE_KEY_NONE;
    wide_wave_sync();
    for (int size = 2; size <= N; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < N / 2; t += 64) {
                const int i = 2 * t - (t & (stride - 1));  // t with a 0 inserted at the stride's bit
                const int j = i + stride;
                const uint64_t a = scratch[i], b = scratch[j];
                const bool up = (i & size) == 0;
                if ((a > b) == up) {
                    scratch[i] = b;
                    scratch[j] = a;
                }
            }
            wide_wave_sync();
        }
}

}  // namespace vsg

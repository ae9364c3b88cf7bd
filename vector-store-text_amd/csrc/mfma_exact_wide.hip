// mfma_exact_wide.hip — batched brute-force k-NN on the matrix cores (gfx950) for result
// lists of 17..128 entries, which the register top-16 of mfma_exact.hip and
// mfma_exact_f16.hip cannot hold.  Same answers as the VALU kernel, bit for bit on
// integer data.
//
// Distance part, as the siblings: block = 256 threads (2 x 2 waves), tile = 128 rows x
// 128 queries, wave (wr, wq) owns 64 x 64 = 2 x 2 MFMA tiles, A operand = base rows, B
// operand = queries, so C lane l holds query (l & 31) against 16 rows.  A K stage is one
// 128-B LDS row per base row and per query (32 floats or 64 halves) in two statically
// named buffers, XOR-swizzled, the next stage streamed in by LDS-DMA under the current
// stage's MFMAs.  Both storages are byte-addressed row-major rows (no K-tiled copy):
//   f32: `v_mfma_f32_32x32x2_f32`, half-wave h takes floats [16 h, 16 h + 16) of the stage;
//   f16: `v_mfma_f32_32x32x16_f16`, MFMA step t reads chunk 2 t + h; an odd number of
//        32-half groups leaves half a stage (mfma_exact_f16.hip);
//   bf16: the f16 code on `v_mfma_f32_32x32x16_bf16`.
// Stage 0 of the next row tile is issued right after the tile's last MFMAs and lands
// during the epilogue; flags and |x|^2 are fetched one row per lane at the top of the
// tile, so the epilogue's only memory traffic are the stores of its survivors.
//
// Selection part: mfma_wide_select.hpp.  The epilogue compares each distance with its
// query's threshold (one LDS word per query, read into two registers per lane) and
// appends the survivors to the (query, split) pool at a slot taken from the query's LDS
// count.  After the tile a barrier publishes counts and entries; wave w then compacts
// the flagged pools among queries w, w + 4, ... in lds_b, which no DMA targets between
// a tile's last stage and the next tile's first barrier.  After the last tile every
// pool is compacted once more and its first k entries, padded with +inf / VSG_EMPTY, are
// the split's partial list [q][split][k] for the merge.
//
// Control flow: the padding block returns before the first barrier; every other barrier
// is reached by all four waves (the compaction loops hold wave-level syncs only).
// Grid and XCD mapping: as mfma_exact.hip.
#include <hip/hip_runtime.h>

#include "mfma_tile.hpp"
#include "mfma_wide_select.hpp"
#include "vsg_device.hpp"
#include "vsg_dispatch.hpp"
#include "vsg_kernels.hpp"

namespace vsg {

constexpr int WROW = 128;             // bytes per LDS row = one K stage of a row
constexpr int WB = 128;               // rows and queries per tile
constexpr int WSTAGE = 2 * WB * WROW;  // one stage buffer: rows | queries
constexpr int WPOOL = MFMA_WIDE_POOL;
static_assert(WPOOL >= 2 * WB && (WPOOL & (WPOOL - 1)) == 0, "a tile's 128 appends fit behind a compacted pool");
static_assert(4 * WPOOL * 8 <= WSTAGE, "the four waves' sort scratch fits in one stage buffer");

// T: the stored element -- float, _Float16 or bf16_t (the f16 stage code on
// `v_mfma_f32_32x32x16_bf16`; "F16" below means a 2-byte element).
template <int MET, typename T>
__global__ __launch_bounds__(256, 2) void mfma_exact_wide_kernel(MfmaExactWideParams p) {
    constexpr bool F16 = sizeof(T) == 2;
    __shared__ __attribute__((aligned(16))) uint8_t lds_a[WSTAGE];
    __shared__ __attribute__((aligned(16))) uint8_t lds_b[WSTAGE];
    __shared__ float tau[WB];
    __shared__ int cnt[WB];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int wq = w & 1, wr = w >> 1;
    const int h = lane >> 5, r = lane & 31;

    // XCD-contiguous block -> (split, query tile)
    const int nb = gridDim.x;
    const int per = nb >> 3;
    const int L = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (L >= p.qtiles * p.splits) return;
    const int split = L / p.qtiles;
    const int qt = L % p.qtiles;
    const int q0 = qt * WB;
    const size_t ntiles = (p.nslots + WB - 1) / WB;
    const size_t t_beg = (size_t)split * p.tiles_per_split;
    const size_t t_end = min(t_beg + (size_t)p.tiles_per_split, ntiles);  // <= t_beg: a padding split
    const uint32_t row_bytes = (uint32_t)p.row_bytes;
    const int nch = p.row_bytes / 16;  // 16-B chunks per row, a multiple of 4 (f32: of 8)
    const int nst = (nch + 7) / 8;
    const bool half_tail = F16 && (nch & 4) != 0;  // the last stage holds chunks 0..3 only
    const int k = p.k;

    if (tid < WB) {
        tau[tid] = __builtin_inff();
        cnt[tid] = 0;
    }
    // pools of this block's queries: [q0 + query][split][WPOOL]
    uint64_t* const pools = p.pool + ((size_t)q0 * p.splits + split) * WPOOL;
    const size_t pool_stride = (size_t)p.splits * WPOOL;  // between two queries

    float qs2[2] = {0.f, 0.f};
    if constexpr (MET == MET_L2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int qi = q0 + wq * 64 + b * 32 + r;
            qs2[b] = qi < p.nq ? p.qsqnorm[qi] : 0.f;
        }
    }

    // LDS-DMA staging: the four waves fill the 1-KiB pieces (8 rows x 128 B) of the row
    // tile and the query tile.  Rows past nslots and queries past nq read the last valid
    // row of the tile (masked in the epilogue / never written out); chunks past a half
    // stage read that row's chunk & 3, so no load leaves [row, row + row_bytes).
    const int prow = lane >> 3, pslot = lane & 7;
    const int qlast = min(WB - 1, p.nq - 1 - q0);  // q0 < nq: qt < qtiles
    auto load_stage = [&](size_t tile, int s, uint8_t* xs) __attribute__((always_inline)) {
        const size_t r0 = tile * WB;  // tile < ntiles: r0 < nslots
        const int xlast = (int)min((size_t)(WB - 1), p.nslots - 1 - r0);
        const int cmask = (half_tail && s == nst - 1) ? 3 : 7;
        uint8_t* qs = xs + WB * WROW;
        const uint8_t* xb = p.vecs + r0 * row_bytes + (size_t)s * WROW;
        const uint8_t* qb = p.queries + (size_t)q0 * row_bytes + (size_t)s * WROW;
#pragma unroll
        for (int u = 0; u < WB / 8 / 4; ++u) {
            const int piece = w * (WB / 8 / 4) + u;
            const int R = piece * 8 + prow;
            const uint32_t xo = (uint32_t)min(R, xlast) * row_bytes + (uint32_t)(swz(R, pslot) & cmask) * 16;
            __builtin_amdgcn_global_load_lds((gptr_t)(xb + xo), (lptr_t)(xs + piece * 8 * WROW), 16, 0, 0);
            const uint32_t qo = (uint32_t)min(R, qlast) * row_bytes + (uint32_t)(swz(R, pslot) & cmask) * 16;
            __builtin_amdgcn_global_load_lds((gptr_t)(qb + qo), (lptr_t)(qs + piece * 8 * WROW), 16, 0, 0);
        }
    };

    // One wave, query `ql` of the tile (wave-uniform): sort its pool, keep the first k.
    // `out`: also write the partial list (after the last tile).
    uint64_t* const scratch = reinterpret_cast<uint64_t*>(lds_b) + w * WPOOL;
    auto compact = [&](int ql, bool out) __attribute__((always_inline)) {
        const int n = min(__builtin_amdgcn_readfirstlane(cnt[ql]), WPOOL);
        uint64_t* pool = pools + (size_t)ql * pool_stride;
        wide_sort_pool<WPOOL>(pool, n, scratch, lane);
        const int keep = min(n, k);
        if (!out) {
            for (int i = lane; i < keep; i += 64) pool[i] = scratch[i];
            if (lane == 0) {
                cnt[ql] = keep;
                tau[ql] = n >= k ? wide_key_dist(scratch[k - 1]) : __builtin_inff();
            }
        } else if (q0 + ql < p.nq) {
            const size_t o = ((size_t)(q0 + ql) * p.splits + split) * k;
            for (int i = lane; i < k; i += 64) {
                const uint64_t key = scratch[i];  // i < k <= 128 <= the sorted length
                p.part_d[o + i] = i < keep ? wide_key_dist(key) : __builtin_inff();
                p.part_i[o + i] = i < keep ? (uint32_t)key : VSG_EMPTY;
            }
        }
        wide_wave_sync();  // scratch is reused by the wave's next query
    };

    if (t_beg < t_end) load_stage(t_beg, 0, lds_a);
    for (size_t tile = t_beg; tile < t_end; ++tile) {
        const size_t r0 = tile * WB;
        floatx16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;
        // what the epilogue needs of the wave's 64 rows, one row per lane, issued here so
        // that it lands under the barrier below (32-bit slots: nslots <= MAX_SLOTS)
        const uint32_t last = (uint32_t)(p.nslots - 1);
        const uint32_t wrow = (uint32_t)r0 + wr * 64 + lane;
        const uint32_t removed = p.flags[min(wrow, last)] & 1u;
        float wsq = 0.f;
        if constexpr (MET == MET_L2) wsq = p.sqnorm[min(wrow, last)];

        // One K stage: the MFMAs of `cur` while the next stage of this tile streams into
        // `nxt`.  The caller places the barrier that ends the stage.
        auto stage = [&](int s, const uint8_t* cur, uint8_t* nxt) __attribute__((always_inline)) {
            if (s + 1 < nst) load_stage(tile, s + 1, nxt);  // nxt was last read before the previous barrier
            const uint8_t* xs = cur;
            const uint8_t* qs = cur + WB * WROW;
            const int ntq = (half_tail && s == nst - 1) ? 2 : 4;
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                if (!F16 || tq < ntq) {
                    // f32: floats [16 h + 4 tq, + 4); f16: chunk 2 tq + h = one K = 16 operand
                    const int c = F16 ? tq * 2 + h : h * 4 + tq;
                    uint4 xa[2], qb[2];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const int R = wr * 64 + a * 32 + r;
                        xa[a] = *reinterpret_cast<const uint4*>(xs + R * WROW + swz(R, c) * 16);
                    }
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int R = wq * 64 + b * 32 + r;
                        qb[b] = *reinterpret_cast<const uint4*>(qs + R * WROW + swz(R, c) * 16);
                    }
                    if constexpr (F16) {
                        using V8 = typename Mfma16<T>::V;
#pragma unroll
                        for (int a = 0; a < 2; ++a)
#pragma unroll
                            for (int b = 0; b < 2; ++b)
                                acc[a][b] = Mfma16<T>::mma(__builtin_bit_cast(V8, xa[a]), __builtin_bit_cast(V8, qb[b]),
                                                           acc[a][b]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int a = 0; a < 2; ++a)
#pragma unroll
                                for (int b = 0; b < 2; ++b) {
                                    const uint32_t av = e == 0 ? xa[a].x : e == 1 ? xa[a].y : e == 2 ? xa[a].z : xa[a].w;
                                    const uint32_t bv = e == 0 ? qb[b].x : e == 1 ? qb[b].y : e == 2 ? qb[b].z : qb[b].w;
                                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(av), __uint_as_float(bv),
                                                                                    acc[a][b], 0, 0, 0);
                                }
                    }
                }
            }
        };

        __syncthreads();  // drains the LDS-DMA (vmcnt(0)): this tile's stage 0 is published in
                          // lds_a; every wave is done with the previous tile's compaction
                          // (lds_b, tau, cnt) and, for the first tile, tau / cnt are set
        for (int s = 0; s < nst; s += 2) {
            stage(s, lds_a, lds_b);
            if (s + 1 < nst) {
                __syncthreads();
                stage(s + 1, lds_b, lds_a);
            }
            if (s + 2 < nst) __syncthreads();
        }
        // An even stage count ends on lds_b, and lds_a -- where the next tile's stage 0
        // goes -- was last read before a barrier.  An odd one ends on lds_a itself: one
        // more barrier before it is overwritten.  (lds_b, the sort scratch, is written
        // only behind the barrier that follows the epilogue.)
        if (nst & 1) __syncthreads();

        if (tile + 1 < t_end) load_stage(tile + 1, 0, lds_a);

        // epilogue: the dots become distances in place.  C register g of MFMA tile a = row
        // a * 32 + 8 (g / 4) + 4 h + g % 4 of the wave's 64.
        const uint64_t vmask = __ballot((wrow <= last) & !removed);
        const uint32_t vm[2] = {(uint32_t)vmask >> (4 * h), (uint32_t)(vmask >> 32) >> (4 * h)};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int j = 8 * (g >> 2) + (g & 3);
                const bool valid = (vm[a] >> j) & 1;
                float xs2 = 0.f;
                if constexpr (MET == MET_L2) {
                    const int x0 = __builtin_amdgcn_readlane(__float_as_int(wsq), a * 32 + j);
                    const int x1 = __builtin_amdgcn_readlane(__float_as_int(wsq), a * 32 + j + 4);
                    xs2 = __int_as_float(h ? x1 : x0);
                }
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float dot = acc[a][b][g];
                    const float d = (MET == MET_L2) ? (xs2 + qs2[b]) - 2.f * dot : 1.f - dot;
                    acc[a][b][g] = valid ? d : __builtin_inff();
                }
            }
        // the threshold filter: strictly below tau (an invalid row's +inf never is)
        const uint32_t rbase = (uint32_t)r0 + wr * 64 + 4 * h;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ql = wq * 64 + b * 32 + r;
            const float t = tau[ql];
            uint64_t* pool = pools + (size_t)ql * pool_stride;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float d = acc[a][b][g];
                    if (d < t) {
                        const uint32_t row = rbase + a * 32 + (g & 3) + 8 * (g >> 2);
                        const int pos = __hip_atomic_fetch_add(&cnt[ql], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (pos < WPOOL) pool[pos] = wide_key(d, row);  // always: <= WPOOL - 128 before the tile
                    }
                }
        }
        __syncthreads();  // counts and pool entries of all four waves are published
        for (int ql = w; ql < WB; ql += 4)
            if (__builtin_amdgcn_readfirstlane(cnt[ql]) > WPOOL - WB) compact(ql, false);
    }
    __syncthreads();  // a split without tiles: tau / cnt are set; else the waves are done with lds_b
    for (int ql = w; ql < WB; ql += 4) compact(ql, true);
}

hipError_t launch_mfma_exact_wide(Storage st, MetricKind mk, const MfmaExactWideParams& p, hipStream_t s) {
    if (p.k <= 16 || p.k > MFMA_WIDE_MAX_K) return hipErrorNotSupported;
    if (p.row_bytes <= 0 || p.row_bytes % (st == ST_F32 ? 128 : 64) || p.nslots == 0 || p.nq <= 0 || p.splits <= 0 ||
        p.tiles_per_split <= 0 || p.qtiles != (p.nq + WB - 1) / WB || !p.pool)
        return hipErrorInvalidValue;
    const int total = p.qtiles * p.splits;
    const int nb = (total + 7) / 8 * 8;
    auto pick = [&](auto tt) {
        using T = typename decltype(tt)::T;
        return mk == MK_L2 ? mfma_exact_wide_kernel<MET_L2, T> : mfma_exact_wide_kernel<MET_DOT, T>;
    };
    auto kern = st == ST_F16 ? pick(TypeTag<_Float16>{}) : st == ST_BF16 ? pick(TypeTag<bf16_t>{}) : pick(TypeTag<float>{});
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace vsg

// mfma_exact_f16.hip — batched brute-force k-NN of an f16 index on the f16 matrix
// cores (gfx950): D = X . Q^T over the stored f16 rows and the f16 prepared queries
// with `v_mfma_f32_32x32x16_f16` (f16 x f16 products exact in f32, f32 accumulation),
// fused with the per-lane register top-KMAX of mfma_exact.hip.  A bf16 index runs the
// same kernel on `v_mfma_f32_32x32x16_bf16` (the element type is a template parameter;
// "half" below reads "2-byte element").
//
//   block = 256 threads (4 waves), tile = 128 rows x 128 queries (2 x 2 waves), or
//   256 rows x 64 queries (4 x 1) for batches <= 64; wave (wr, wq) owns 64 x 64 =
//   2 x 2 MFMA tiles.  A operand = base rows, B operand = queries: C lane l holds
//   query (l & 31) against 16 rows, as in the f32 kernel.
//   K stage = 64 halves = one 128-B LDS row of eight 16-B chunks (the f32 kernel's
//   swizzle and 1-KiB LDS-DMA pieces).  One chunk is one lane's whole operand of a
//   K = 16 MFMA -- a dot product does not care which 8 elements a lane takes as long
//   as the row lane and the query lane take the same -- so MFMA step t of a stage
//   reads chunk 2 t + (lane >> 5) of its row with one ds_read_b128: 8 reads feed
//   16 MFMAs per stage and wave.
//   Rows are whole 32-half groups: an odd number of groups leaves half a stage, run
//   with 4 chunks (2 MFMA steps); its DMA lanes of chunks 4..7 re-read chunks 0..3,
//   so no load leaves [row, row + row_bytes).
//
// Rows are short (C4: 256 B = two stages), so a row tile does not start with an
// exposed load: stage 0 of the next row tile is issued right after the tile's last
// MFMAs and lands during the epilogue; the barrier that publishes it is the next
// tile's first.  The epilogue issues no load of its own (vmcnt counts in order: it
// would wait for that DMA): each lane loads the flag and |x|^2 of one of the wave's 64
// rows at the top of the tile, and the epilogue reads its 2 x 16 rows' values from the
// owning lanes (ballot / readlane).  Every tile starts in lds_a; an odd stage count
// ends there too and pays one more barrier before the prefetch overwrites it.
//
// Grid, partial lists [q][part][KMAX] and ties: as mfma_exact.hip.
#include <hip/hip_runtime.h>

#include "mfma_tile.hpp"
#include "vsg_device.hpp"
#include "vsg_kernels.hpp"

namespace vsg {

constexpr int HROW = 128;  // bytes per LDS row = one K stage of a row (64 halves)

// T: the stored element, _Float16 or bf16_t (bf16 rows and bf16-rounded queries on
// `v_mfma_f32_32x32x16_bf16`: bf16 x bf16 products are exact in f32 as well).  Two-byte
// elements either way, so stages, swizzle, DMA pieces and epilogue are the same code.
template <typename T, int KMAX, int MET, int WQ, int WR>
__global__ __launch_bounds__(64 * WQ * WR, 2) void mfma_exact_f16_kernel(MfmaExactF16Params p) {
    using V8 = typename Mfma16<T>::V;
    constexpr int BQ = 64 * WQ, BR = 64 * WR, NW = WQ * WR, STAGE = (BR + BQ) * HROW;
    __shared__ __attribute__((aligned(16))) uint8_t lds_a[STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t lds_b[STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int wq = w % WQ, wr = w / WQ;
    const int h = lane >> 5, r = lane & 31;

    // XCD-contiguous block -> (split, query tile)
    const int nb = gridDim.x;
    const int per = nb >> 3;
    const int L = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (L >= p.qtiles * p.splits) return;
    const int split = L / p.qtiles;
    const int qt = L % p.qtiles;
    const int q0 = qt * BQ;
    const size_t ntiles = (p.nslots + BR - 1) / BR;
    const size_t t_beg = (size_t)split * p.tiles_per_split;
    const size_t t_end = min(t_beg + (size_t)p.tiles_per_split, ntiles);  // <= t_beg: a padding split
    const uint32_t row_bytes = (uint32_t)p.row_bytes;
    const int nch = p.row_bytes / 16;  // 16-B chunks per row, a multiple of 4
    const int nst = (nch + 7) / 8;
    const bool half_tail = (nch & 4) != 0;  // the last stage holds chunks 0..3 only

    float ld[2][KMAX];
    uint32_t li[2][KMAX];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < KMAX; ++t) {
            ld[b][t] = __builtin_inff();
            li[b][t] = VSG_EMPTY;
        }

    float qs2[2] = {0.f, 0.f};
    if constexpr (MET == MET_L2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int qi = q0 + wq * 64 + b * 32 + r;
            qs2[b] = qi < p.nq ? p.qsqnorm[qi] : 0.f;
        }
    }

    // LDS-DMA staging: the NW waves fill the 1-KiB pieces (8 rows x 128 B) of the row
    // tile and the query tile round-robin.  Lane -> (row of the piece, LDS slot); the
    // source is a wave-uniform stage base + a 32-bit offset.  Rows past nslots and
    // queries past nq read the last valid row of the tile (masked in the epilogue /
    // never written out); chunks past a half stage read that row's chunk & 3.
    const int prow = lane >> 3, pslot = lane & 7;
    const int qlast = min(BQ - 1, p.nq - 1 - q0);  // q0 < nq: qt < qtiles
    auto load_stage = [&](size_t tile, int s, uint8_t* xs) __attribute__((always_inline)) {
        const size_t r0 = tile * BR;  // tile < ntiles: r0 < nslots
        const int xlast = (int)min((size_t)(BR - 1), p.nslots - 1 - r0);
        const int cmask = (half_tail && s == nst - 1) ? 3 : 7;
        uint8_t* qs = xs + BR * HROW;
        const uint8_t* xb = p.vecs + r0 * row_bytes + (size_t)s * HROW;
        const uint8_t* qb = p.queries + (size_t)q0 * row_bytes + (size_t)s * HROW;
#pragma unroll
        for (int u = 0; u < BR / 8 / NW; ++u) {
            const int piece = w * (BR / 8 / NW) + u;
            const int R = piece * 8 + prow;
            const uint32_t off = (uint32_t)min(R, xlast) * row_bytes + (uint32_t)(swz(R, pslot) & cmask) * 16;
            __builtin_amdgcn_global_load_lds((gptr_t)(xb + off), (lptr_t)(xs + piece * 8 * HROW), 16, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < BQ / 8 / NW; ++u) {
            const int piece = w * (BQ / 8 / NW) + u;
            const int R = piece * 8 + prow;
            const uint32_t off = (uint32_t)min(R, qlast) * row_bytes + (uint32_t)(swz(R, pslot) & cmask) * 16;
            __builtin_amdgcn_global_load_lds((gptr_t)(qb + off), (lptr_t)(qs + piece * 8 * HROW), 16, 0, 0);
        }
    };

    if (t_beg < t_end) load_stage(t_beg, 0, lds_a);
    for (size_t tile = t_beg; tile < t_end; ++tile) {
        const size_t r0 = tile * BR;
        floatx16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;
        // What the epilogue needs of the wave's 64 rows, one row per lane: validity and
        // |x|^2 (32-bit slots: nslots <= MAX_SLOTS).  Two loads per lane and tile, issued
        // here so that they land under the barrier below; the epilogue fetches its rows'
        // values from the owning lanes (ballot / readlane), so it issues no load that
        // would queue behind the next tile's DMA (vmcnt counts in order).
        const uint32_t last = (uint32_t)(p.nslots - 1);
        const uint32_t wrow = (uint32_t)r0 + wr * 64 + lane;
        const uint32_t removed = p.flags[min(wrow, last)] & 1u;
        float wsq = 0.f;
        if constexpr (MET == MET_L2) wsq = p.sqnorm[min(wrow, last)];

        // One K stage: the MFMAs of `cur` while the next stage (of this tile or of the
        // next one) streams into `nxt`.  cur / nxt are two distinct __shared__ arrays
        // named statically, so the compiler can tell the DMA target from the ds_read
        // source (mfma_exact.hip).  The caller places the barrier that ends the stage.
        auto stage = [&](int s, const uint8_t* cur, uint8_t* nxt) __attribute__((always_inline)) {
            if (s + 1 < nst) load_stage(tile, s + 1, nxt);  // nxt was last read before the previous barrier
            const uint8_t* xs = cur;
            const uint8_t* qs = cur + BR * HROW;
            const int ntq = (half_tail && s == nst - 1) ? 2 : 4;
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                if (tq < ntq) {
                    V8 xa[2], qb[2];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const int R = wr * 64 + a * 32 + r;
                        xa[a] = *reinterpret_cast<const V8*>(xs + R * HROW + swz(R, tq * 2 + h) * 16);
                    }
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int R = wq * 64 + b * 32 + r;
                        qb[b] = *reinterpret_cast<const V8*>(qs + R * HROW + swz(R, tq * 2 + h) * 16);
                    }
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            acc[a][b] = Mfma16<T>::mma(xa[a], qb[b], acc[a][b]);
                }
            }
        };

        __syncthreads();  // drains the LDS-DMA (vmcnt(0)): this tile's stage 0 is published in
                          // lds_a, and every wave is done with the previous tile's buffers
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
        // more barrier before it is overwritten.
        if (nst & 1) __syncthreads();

        if (tile + 1 < t_end) load_stage(tile + 1, 0, lds_a);

        // epilogue: the dots become distances in place, then the register top-KMAX (rows
        // arrive in increasing slot order).  C register g of MFMA tile a = row a * 32 +
        // 8 (g / 4) + 4 h + g % 4 of the wave's 64.
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
        const uint32_t rbase = (uint32_t)r0 + wr * 64 + 4 * h;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const uint32_t row = rbase + a * 32 + (g & 3) + 8 * (g >> 2);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float d = acc[a][b][g];
                    if (d < ld[b][KMAX - 1]) topk_insert<KMAX>(ld[b], li[b], d, row);
                }
            }
        }
    }

    const int nparts = p.splits * WR * 2;
    const int part = (split * WR + wr) * 2 + h;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int qi = q0 + wq * 64 + b * 32 + r;
        if (qi >= p.nq) continue;
        const size_t o = ((size_t)qi * nparts + part) * KMAX;
#pragma unroll
        for (int t = 0; t < KMAX; ++t) {
            p.part_d[o + t] = ld[b][t];
            p.part_i[o + t] = ld[b][t] < __builtin_inff() ? li[b][t] : VSG_EMPTY;
        }
    }
}

template <typename T>
static hipError_t launch_mfma_exact_2byte(MetricKind mk, const MfmaExactF16Params& p, hipStream_t s) {
    // (bq, br) = (128, 128) or (64, 256), both 256-thread blocks; rows of whole 32-element groups
    if (p.kmax != 16 || !((p.bq == 128 && p.br == 128) || (p.bq == 64 && p.br == 256))) return hipErrorNotSupported;
    if (p.row_bytes <= 0 || p.row_bytes % 64 || p.nslots == 0 || p.nq <= 0) return hipErrorInvalidValue;
    const int total = p.qtiles * p.splits;
    const int nb = (total + 7) / 8 * 8;
    if (p.bq == 128) {
        auto kern = mk == MK_L2 ? mfma_exact_f16_kernel<T, 16, MET_L2, 2, 2> : mfma_exact_f16_kernel<T, 16, MET_DOT, 2, 2>;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, p);
    } else {
        auto kern = mk == MK_L2 ? mfma_exact_f16_kernel<T, 16, MET_L2, 1, 4> : mfma_exact_f16_kernel<T, 16, MET_DOT, 1, 4>;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, p);
    }
    return hipGetLastError();
}

hipError_t launch_mfma_exact_f16(Storage st, MetricKind mk, const MfmaExactF16Params& p, hipStream_t s) {
    if (st == ST_F16) return launch_mfma_exact_2byte<_Float16>(mk, p, s);
    if (st == ST_BF16) return launch_mfma_exact_2byte<bf16_t>(mk, p, s);
    return hipErrorInvalidValue;
}

}  // namespace vsg

// mfma_exact_f8.hip — batched brute-force k-NN of an FP8 (E4M3) index on the FP8 matrix
// cores (gfx950): D = X . Q^T over the stored 1-byte rows and the FP8-rounded queries with
// `v_mfma_f32_32x32x64_f8f6f4`, both operand formats E4M3 and no block scales (E4M3 x E4M3
// products are exact in f32, f32 accumulation), fused with the per-lane register top-KMAX
// of mfma_exact.hip.
//
//   block, wave tiles, XCD mapping, per-tile flag / |x|^2 fetch, epilogue and partial
//   lists: mfma_exact_f16.hip, so the same plan and merge serve this kernel.
//   K stage = 128 elements = one 128-B LDS row of eight 16-B chunks (the siblings' swizzle
//   and 1-KiB LDS-DMA pieces): a 1536-d row is 12 stages where f16 has 24, with half the
//   barriers per tile.  A lane's operand of the K = 64 MFMA is 32 B = two chunks -- a dot
//   product does not care which 32 elements a lane takes as long as the row lane and the
//   query lane take the same -- so MFMA step t (0, 1) of a stage gives lane half h chunks
//   4 t + 2 h and 4 t + 2 h + 1.  The swizzle XORs a chunk number with a per-row constant,
//   so the pair stays one aligned 32-B block of the LDS row (in either order): two
//   ds_read_b128 per operand and step, 8 reads feed 8 MFMAs of K = 64 per stage and wave
//   (the f16 kernel: 8 reads for 16 MFMAs of K = 16, a quarter of the elements).
//   Rows are whole 64-element groups: an odd number of groups leaves half a stage, run
//   with chunks 0..3 (one MFMA step); its DMA lanes of chunks 4..7 re-read chunks 0..3,
//   so no load leaves [row, row + row_bytes).
//
// Prefetch of the next tile's stage 0 under the epilogue, the barriers and the
// statically named double buffer: as mfma_exact_f16.hip.
#include <hip/hip_runtime.h>

#include "mfma_tile.hpp"
#include "vsg_device.hpp"
#include "vsg_kernels.hpp"

namespace vsg {

constexpr int F8ROW = 128;  // bytes per LDS row = one K stage of a row (128 elements)

typedef int intx8 __attribute__((ext_vector_type(8)));

// a lane's 32-B operand: the 16-B chunks c and c + 1 (c even) of LDS row R at `base`
__device__ __forceinline__ intx8 f8_operand(const uint8_t* base, int R, int c) {
    const uint4 lo = *reinterpret_cast<const uint4*>(base + R * F8ROW + swz(R, c) * 16);
    const uint4 hi = *reinterpret_cast<const uint4*>(base + R * F8ROW + swz(R, c + 1) * 16);
    intx8 v;
    v[0] = (int)lo.x, v[1] = (int)lo.y, v[2] = (int)lo.z, v[3] = (int)lo.w;
    v[4] = (int)hi.x, v[5] = (int)hi.y, v[6] = (int)hi.z, v[7] = (int)hi.w;
    return v;
}

template <int KMAX, int MET, int WQ, int WR>
__global__ __launch_bounds__(64 * WQ * WR, 2) void mfma_exact_f8_kernel(MfmaExactF16Params p) {
    constexpr int BQ = 64 * WQ, BR = 64 * WR, NW = WQ * WR, STAGE = (BR + BQ) * F8ROW;
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
        uint8_t* qs = xs + BR * F8ROW;
        const uint8_t* xb = p.vecs + r0 * row_bytes + (size_t)s * F8ROW;
        const uint8_t* qb = p.queries + (size_t)q0 * row_bytes + (size_t)s * F8ROW;
#pragma unroll
        for (int u = 0; u < BR / 8 / NW; ++u) {
            const int piece = w * (BR / 8 / NW) + u;
            const int R = piece * 8 + prow;
            const uint32_t off = (uint32_t)min(R, xlast) * row_bytes + (uint32_t)(swz(R, pslot) & cmask) * 16;
            __builtin_amdgcn_global_load_lds((gptr_t)(xb + off), (lptr_t)(xs + piece * 8 * F8ROW), 16, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < BQ / 8 / NW; ++u) {
            const int piece = w * (BQ / 8 / NW) + u;
            const int R = piece * 8 + prow;
            const uint32_t off = (uint32_t)min(R, qlast) * row_bytes + (uint32_t)(swz(R, pslot) & cmask) * 16;
            __builtin_amdgcn_global_load_lds((gptr_t)(qb + off), (lptr_t)(qs + piece * 8 * F8ROW), 16, 0, 0);
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
        // validity and |x|^2 of the wave's 64 rows, one row per lane, loaded here so that
        // the epilogue issues no load behind the next tile's DMA (mfma_exact_f16.hip)
        const uint32_t last = (uint32_t)(p.nslots - 1);
        const uint32_t wrow = (uint32_t)r0 + wr * 64 + lane;
        const uint32_t removed = p.flags[min(wrow, last)] & 1u;
        float wsq = 0.f;
        if constexpr (MET == MET_L2) wsq = p.sqnorm[min(wrow, last)];

        // One K stage: the MFMAs of `cur` while the next stage (of this tile or of the
        // next one) streams into `nxt`; two distinct, statically named __shared__ arrays.
        // The caller places the barrier that ends the stage.
        auto stage = [&](int s, const uint8_t* cur, uint8_t* nxt) __attribute__((always_inline)) {
            if (s + 1 < nst) load_stage(tile, s + 1, nxt);  // nxt was last read before the previous barrier
            const uint8_t* xs = cur;
            const uint8_t* qs = cur + BR * F8ROW;
            const int nt = (half_tail && s == nst - 1) ? 1 : 2;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < nt) {
                    intx8 xa[2], qb[2];
#pragma unroll
                    for (int a = 0; a < 2; ++a) xa[a] = f8_operand(xs, wr * 64 + a * 32 + r, 4 * t + 2 * h);
#pragma unroll
                    for (int b = 0; b < 2; ++b) qb[b] = f8_operand(qs, wq * 64 + b * 32 + r, 4 * t + 2 * h);
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            // formats (cbsz, blgp) 0 = E4M3 for both operands; scale operands 0:
                            // the compiler selects the instruction without block scales
                            acc[a][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xa[a], qb[b], acc[a][b], 0, 0, 0,
                                                                                       0, 0, 0);
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
        // An odd stage count ends on lds_a itself, where the next tile's stage 0 goes: one
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

hipError_t launch_mfma_exact_f8(MetricKind mk, const MfmaExactF16Params& p, hipStream_t s) {
    // (bq, br) = (128, 128) or (64, 256), both 256-thread blocks; rows of whole 64-element groups
    if (p.kmax != 16 || !((p.bq == 128 && p.br == 128) || (p.bq == 64 && p.br == 256))) return hipErrorNotSupported;
    if (p.row_bytes <= 0 || p.row_bytes % 64 || p.nslots == 0 || p.nq <= 0) return hipErrorInvalidValue;
    const int total = p.qtiles * p.splits;
    const int nb = (total + 7) / 8 * 8;
    if (p.bq == 128) {
        auto kern = mk == MK_L2 ? mfma_exact_f8_kernel<16, MET_L2, 2, 2> : mfma_exact_f8_kernel<16, MET_DOT, 2, 2>;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, p);
    } else {
        auto kern = mk == MK_L2 ? mfma_exact_f8_kernel<16, MET_L2, 1, 4> : mfma_exact_f8_kernel<16, MET_DOT, 1, 4>;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace vsg

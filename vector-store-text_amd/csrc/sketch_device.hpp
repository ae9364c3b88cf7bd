// sketch_device.hpp — the device side of the int8 sketch prefilter of the register
// search (sketch.hpp: format and bound; hnsw_regset.hpp beam_reg: where it runs;
// DESIGN.md §3.1).  Included by hnsw_search_reg.hip only.
#pragma once
#include "hnsw_common.hpp"
#include "hnsw_regset.hpp"
#include "sketch.hpp"

namespace vsg {

// Sketch prefilter of the register search (sketch.hpp): a sketch
// row is dim bytes u = rint(x / scale) + 128 in 16-B chunks, split over GS lanes
// with VMS chunks each (64 / GS rows per pass, US passes in flight).
//
// Sketch shape of a row shape (G, VM) of f32 rows: G * VM / 4 sketch chunks.
// U: the f32 passes in flight of the kernel the sketch pass is compiled into.
template <int G, int VM, int U> struct SketchShape {
    static constexpr int SC = G * VM / 4;
    static constexpr int GS = SC <= 48 ? 16 : SC <= 128 ? 32 : 64;
    static constexpr int VMS = (SC + GS - 1) / GS;
    // passes in flight: the raw sketch words (4 VMS US registers) and the query's two int8
    // planes (8 VMS) stay within what the f32 pass holds in row words (4 VM U, dead
    // meanwhile), so the sketch pass does not set the kernel's register peak: at 3 chunks per
    // lane 4 passes beside U = 4, 2 beside U = 2 (3 there: 175 VGPRs at 768-d, a wave per SIMD
    // less than with 2)
    static constexpr int US = VMS <= 1 ? 8 : VMS <= 3 ? (U >= 4 ? 4 : 2) : 2;
    static constexpr int LDS_BYTES = VMS * 2 * GS * 16;  // the query image (SketchQ)
};

// The f32 passes in flight (U) of the prefilter instance of a search row shape: the search
// shape's own.  VSG_PREFILTER_U2=1 (probes) gives the 768- / 1536-d instances of the 2-row
// class U = 2 and with it 3 waves per SIMD instead of 2 (159 VGPRs against 203): measured 1 %
// faster than U = 4 at 10k queries, 8 % slower at 2,048 and 4,096 and 11 % slower at 512
// (DESIGN.md §3.1), so not the default.  Same sums in the same order whatever U.
#ifndef VSG_PREFILTER_U2
#define VSG_PREFILTER_U2 0
#endif
template <int G, int VM, int U> constexpr int prefilter_u() { return VSG_PREFILTER_U2 && VM == 6 && U > 2 ? 2 : U; }

// Sum of `a` over each G-lane group, valid in the group's first lane (group_sum0's moves;
// integer adds are exact in any order).
template <int G> __device__ __forceinline__ int group_isum0(int a) {
    if constexpr (G >= 64) a += __shfl_xor(a, 32);
    if constexpr (G >= 32) a += __builtin_amdgcn_ds_swizzle(a, 0x401F);
    if constexpr (G >= 16) a += __builtin_amdgcn_mov_dpp(a, 0x108, 0xF, 0xF, true);
    if constexpr (G >= 8) a += __builtin_amdgcn_mov_dpp(a, 0x104, 0xF, 0xF, true);
    if constexpr (G >= 4) a += __builtin_amdgcn_mov_dpp(a, 0x4E, 0xF, 0xF, true);
    if constexpr (G >= 2) a += __builtin_amdgcn_mov_dpp(a, 0xB1, 0xF, 0xF, true);
    return a;
}

// The query in the sketch layout, kept in LDS (VGPRs would cost the kernel a wave per
// SIMD): its 16-bit quantisation q16 = 256 h + l (sketch.hpp) as two int8 planes.  Lane sl
// of a group reads the 16 h bytes and the 16 l bytes of its sketch chunks v * GS + sl, unit
// (v * 2 + plane) * GS + sl, so a wave's reads of one unit are consecutive (no bank
// conflicts; the 64 / GS row groups read the same words).  k: scale, error share and norm
// bound of the query; k.sq = 0: the query has no usable scale and runs unfiltered.
template <int GS, int VMS> struct SketchQ {
    static constexpr int CHUNKS = VMS * GS;  // sketch chunks (16 elements) of the image
    const uint4* img;                        // LDS, 2 * CHUNKS units
    SketchQuery k;

    // the 16 query elements of sketch chunk c (zero past the row)
    static __device__ __forceinline__ void elems(const uint8_t* __restrict__ qrow, int nchunks, int c, float (&e)[16]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int fc = c * 4 + j;
            uint4 raw = make_uint4(0u, 0u, 0u, 0u);
            if (fc < nchunks) raw = *reinterpret_cast<const uint4*>(qrow + (size_t)fc * 16);
            e[j * 4 + 0] = __uint_as_float(raw.x);
            e[j * 4 + 1] = __uint_as_float(raw.y);
            e[j * 4 + 2] = __uint_as_float(raw.z);
            e[j * 4 + 3] = __uint_as_float(raw.w);
        }
    }

    // qrow: the prepared f32 query (nchunks 16-B chunks, zero past dim); lds: 2 * CHUNKS * 16 bytes
    __device__ __forceinline__ void stage(const uint8_t* __restrict__ qrow, int nchunks, int dim, uint8_t* lds) {
        uint4* dst = reinterpret_cast<uint4*>(lds);
        img = dst;
        float mx = 0.f, s2 = 0.f;
        for (int c = lane_id(); c < CHUNKS; c += 64) {
            float e[16];
            elems(qrow, nchunks, c, e);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float a = __builtin_fabsf(e[i]);
                if (!(a <= 3.4028234e38f)) mx = __builtin_inff();  // NaN or inf
                mx = a > mx ? a : mx;
                s2 = __builtin_fmaf(e[i], e[i], s2);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(mx, o);
            mx = m2 > mx ? m2 : mx;
            s2 += __shfl_xor(s2, o);
        }
        const float sq = sketch_qscale(mx);  // wave-uniform
        float r2 = 0.f;
        if (sq > 0.f) {
            for (int c = lane_id(); c < CHUNKS; c += 64) {
                float e[16];
                elems(qrow, nchunks, c, e);
                uint32_t hw[4], lw[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    hw[j] = 0u;
                    lw[j] = 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int q16 = sketch_q16(e[j * 4 + i], sq);
                        r2 += sketch_qres2(e[j * 4 + i], sq, q16);
                        hw[j] |= ((uint32_t)sketch_q16_hi(q16) & 0xFFu) << (8 * i);
                        lw[j] |= ((uint32_t)sketch_q16_lo(q16) & 0xFFu) << (8 * i);
                    }
                }
                const int v = c / GS, sl = c % GS;
                dst[(v * 2 + 0) * GS + sl] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
                dst[(v * 2 + 1) * GS + sl] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) r2 += __shfl_xor(r2, o);
        }
        k = sketch_query(mx, r2, s2, dim);
        wave_sync();
    }
};

// out[r] = an upper bound of q . x_r, from the sketch rows of ids[0..count): sketch_upper
// (sketch.hpp) of the integer sums H = sum x'_i h_i, L = sum x'_i l_i, x' = u ^ 0x80 the
// row's signed bytes, four products per v_dot4.  +inf / NaN for a row without a usable
// sketch (err = +inf, or not converted yet: its meta words are all ones).  meta: (scale,
// err) pairs.  schunks: 16-B chunks of a sketch row (its stride).  Wave-uniform count.
template <int GS, int VMS, int US>
__device__ __forceinline__ void rows_sketch(const uint8_t* __restrict__ sk, size_t stride, int schunks,
                                            const float2* __restrict__ meta, const uint32_t* ids, int count,
                                            const SketchQ<GS, VMS>& q, float* out) {
    constexpr int RS = 64 / GS;
    const int lane = lane_id();
    const int sub = lane / GS;
    const int sl = lane % GS;
    for (int base = 0; base < count; base += RS * US) {
        uint4 raw[US][VMS];
        float2 mt[US];
#pragma unroll
        for (int u = 0; u < US; ++u) {
            const int r = base + u * RS + sub;
            const uint32_t id = ids[r < count ? r : count - 1];
            const uint8_t* row = sk + (size_t)id * stride;
            mt[u] = meta[id];
#pragma unroll
            for (int v = 0; v < VMS; ++v) {
                const int c = v * GS + sl;
                raw[u][v] = *reinterpret_cast<const uint4*>(row + (size_t)(c < schunks ? c : schunks - 1) * 16);
            }
        }
        // the query's planes, from LDS under the row loads
        uint4 qh[VMS], ql[VMS];
#pragma unroll
        for (int v = 0; v < VMS; ++v) {
            qh[v] = q.img[(v * 2 + 0) * GS + sl];
            ql[v] = q.img[(v * 2 + 1) * GS + sl];
        }
#pragma unroll
        for (int u = 0; u < US; ++u) {
            if (base + u * RS >= count) break;
            int ah = 0, al = 0;
#pragma unroll
            for (int v = 0; v < VMS; ++v) {
                const uint32_t w[4] = {raw[u][v].x, raw[u][v].y, raw[u][v].z, raw[u][v].w};
                const uint32_t h[4] = {qh[v].x, qh[v].y, qh[v].z, qh[v].w};
                const uint32_t l[4] = {ql[v].x, ql[v].y, ql[v].z, ql[v].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = (int)(w[j] ^ 0x80808080u);
                    ah = __builtin_amdgcn_sdot4(x, (int)h[j], ah, false);
                    al = __builtin_amdgcn_sdot4(x, (int)l[j], al, false);
                }
            }
            ah = group_isum0<GS>(ah);
            al = group_isum0<GS>(al);
            const int r = base + u * RS + sub;
            if (sl == 0 && r < count) out[r] = sketch_upper(q.k, SketchMeta{mt[u].x, mt[u].y}, ah, al);
        }
    }
}

// beam_reg's PRE of the prefiltered search: the sketch rows, the query's sketch image and
// the counters of one query.
template <int GS, int VMS, int US> struct SketchPre {
    const uint8_t* sk;
    const float2* meta;
    size_t stride;
    int schunks;
    SketchQ<GS, VMS> q;
    uint32_t nsketch = 0, nexact = 0;  // sketch rows / f32 rows read (one query)

    // Drop from w.todo[0..cnt) every id whose lower bound 1 - (q . x~ + |q| err) is not
    // below tkey (cand_key of the bound with slot 0: at or below the candidate's own
    // key); survivors keep their order.  Returns their count.  Uses w.tdist.
    __device__ __forceinline__ int filter(WaveLds& w, int cnt, uint64_t tkey) {
        if (!(q.k.sq > 0.f)) return cnt;  // no usable query scale: nothing is rejected
        const int lane = lane_id();
        rows_sketch<GS, VMS, US>(sk, stride, schunks, meta, w.todo, cnt, q, w.tdist);
        wave_sync();
        nsketch += (uint32_t)cnt;
        const float ub = lane < cnt ? w.tdist[lane] : 0.f;  // >= q . x (inf / NaN: no sketch)
        const uint32_t cid = lane < cnt ? w.todo[lane] : 0u;
        const bool finite = __builtin_fabsf(ub) < __builtin_inff();
        const bool keep = lane < cnt && !(finite && cand_key(1.f - ub, 0u) >= tkey);
        const uint64_t km = __ballot(keep);
        wave_sync();
        if (keep) w.todo[lanes_below(km)] = cid;
        wave_sync();
        return popc64(km);
    }
};

}  // namespace vsg

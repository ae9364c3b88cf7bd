// sketch_device.hpp — the device side of the int8 sketch prefilter of the register
// search (sketch.hpp: format and bound; hnsw_regset.hpp beam_reg: where it runs;
// DESIGN.md §3.1).  Included by hnsw_search_reg.hip only.
#pragma once
#include "hnsw_common.hpp"
#include "hnsw_regset.hpp"

namespace vsg {

// Sketch prefilter of the register search (sketch.hpp): a sketch
// row is dim bytes u = rint(x / scale) + 128 in 16-B chunks, split over GS lanes
// with VMS chunks each (64 / GS rows per pass, US passes in flight).
//
// Sketch shape of a row shape (G, VM) of f32 rows: G * VM / 4 sketch chunks.
template <int G, int VM> struct SketchShape {
    static constexpr int SC = G * VM / 4;
    static constexpr int GS = SC <= 48 ? 16 : SC <= 128 ? 32 : 64;
    static constexpr int VMS = (SC + GS - 1) / GS;
    // passes in flight: the raw sketch words and the query image together stay within
    // the f32 pass's row words (dead meanwhile), so the variant keeps the plain kernel's
    // waves per SIMD
    static constexpr int US = VMS <= 1 ? 8 : VMS <= 3 ? 4 : 2;
    static constexpr int LDS_BYTES = VMS * 4 * GS * 16;  // the query image (SketchQ)
};

// f32 image of the query in the sketch layout, kept in LDS (VGPRs would cost the
// kernel a wave per SIMD): lane sl of a group reads the 16 elements of its sketch
// chunks v * GS + sl as four 16-B units, unit (v * 4 + j) * GS + sl = f32 chunk
// (v * GS + sl) * 4 + j of the query, so a wave's reads of one unit are consecutive
// (no bank conflicts; the 64 / GS row groups read the same words).  The registers that
// hold it during a sketch pass are those of the f32 pass's row words, dead meanwhile.
// sumq = sum q_i (the +128 bias of the bytes), qn = an upper bound of |q|.
template <int GS, int VMS> struct SketchQ {
    static constexpr int UNITS = VMS * 4 * GS;  // 16-B units of the image
    const uint4* img;                           // LDS
    float sumq, qn;

    // qrow: the prepared f32 query (nchunks 16-B chunks, zero past dim); lds: UNITS * 16 bytes
    __device__ __forceinline__ void stage(const uint8_t* __restrict__ qrow, int nchunks, int dim, uint8_t* lds) {
        uint4* dst = reinterpret_cast<uint4*>(lds);
        float s = 0.f, s2 = 0.f;
        for (int t = lane_id(); t < UNITS; t += 64) {
            const int v = t / (4 * GS), j = (t / GS) % 4, sl = t % GS;
            const int fc = (v * GS + sl) * 4 + j;
            uint4 raw = make_uint4(0u, 0u, 0u, 0u);
            if (fc < nchunks) raw = *reinterpret_cast<const uint4*>(qrow + (size_t)fc * 16);
            dst[t] = raw;
            const float e[4] = {__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z),
                                __uint_as_float(raw.w)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s += e[i];
                s2 = __builtin_fmaf(e[i], e[i], s2);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o);
            s2 += __shfl_xor(s2, o);
        }
        img = dst;
        sumq = s;
        qn = __builtin_sqrtf(s2) * (1.f + (float)(dim + 8) * 1.1920929e-7f);  // sketch_qnorm_up
        wave_sync();
    }
};

// out[r] = an upper bound of q . x_r, from the sketch rows of ids[0..count): scale *
// (sum q_i u_i - 128 sum q) + |q| err.  +inf / NaN for a row without a usable sketch
// (err = +inf, or not converted yet: its meta words are all ones).  meta: (scale, err)
// pairs.  schunks: 16-B chunks of a sketch row (its stride).  Wave-uniform count.
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
        // the query image, from LDS under the row loads
        uint4 qx[VMS][4];
#pragma unroll
        for (int v = 0; v < VMS; ++v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) qx[v][j] = q.img[(v * 4 + j) * GS + sl];
        }
#pragma unroll
        for (int u = 0; u < US; ++u) {
            if (base + u * RS >= count) break;
            float acc = 0.f;
#pragma unroll
            for (int v = 0; v < VMS; ++v) {
                const uint32_t w[4] = {raw[u][v].x, raw[u][v].y, raw[u][v].z, raw[u][v].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc = __builtin_fmaf((float)(w[j] & 0xFFu), __uint_as_float(qx[v][j].x), acc);
                    acc = __builtin_fmaf((float)((w[j] >> 8) & 0xFFu), __uint_as_float(qx[v][j].y), acc);
                    acc = __builtin_fmaf((float)((w[j] >> 16) & 0xFFu), __uint_as_float(qx[v][j].z), acc);
                    acc = __builtin_fmaf((float)(w[j] >> 24), __uint_as_float(qx[v][j].w), acc);
                }
            }
            acc = group_sum0<GS>(acc);
            const int r = base + u * RS + sub;
            if (sl == 0 && r < count) {
                const float t = acc - 128.f * q.sumq;
                out[r] = __builtin_fmaf(q.qn, mt[u].y, mt[u].x * t);
            }
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

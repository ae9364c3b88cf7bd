// sketch_device.hpp — the device side of the int8 sketch in the register search: the
// prefilter (sketch.hpp: format and bound; hnsw_regset.hpp beam_reg: where it runs;
// DESIGN.md §3.1) and the int8 traversal (the row policy SketchI8 below).
// Included by hnsw_search_reg.hip only.
#pragma once
#include "hnsw_common.hpp"
#include "hnsw_regset.hpp"
#include "sketch.hpp"
#include "vsg_dispatch.hpp"

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
    float sum2;  // the f32 sum of squares of the query's elements (|q|^2 of the int8 walk's l2sq)

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
        sum2 = s2;
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

// ------------------------------------------------------------- int8 traversal --
// VSG_FLAG_I8_TRAVERSAL: the register search walks the sketch rows.  SketchI8
// is the storage tag of that walk: QReg<G, VM, SketchI8> is not a register image of the query
// but the row-access policy -- the query's two int8 planes in LDS (SketchQ), the sketch rows,
// their meta pairs and |x|^2 -- and rows_dist hands every call to its rows(), so dist_one,
// greedy_level, beam_reg, the visited table, the admission, the persistent grid and the
// extraction are the register search's own code instantiated on this tag.
struct SketchI8 {};
template <> struct RowPolicy<SketchI8> {
    static constexpr bool own = true;
};

// Row shape (lanes per row, 16-B chunks per lane, passes in flight) from the sketch row's
// chunk count (its 128-B-aligned stride: a multiple of 8 chunks).  Every shape keeps 8-12
// 16-B loads per lane in flight (32-48 VGPRs of raw words; the query costs none, it is in
// LDS) and 16 to 64 rows per round trip: an expansion's ~20-30 fresh rows are one or two
// round trips.  768-d (48 chunks): 16 lanes x 3 chunks x 4 passes, the prefilter's sketch
// shape at that size: 148 VGPRs, 3 waves per SIMD; 8 x 6 x 2 took 177 and 2 and ran the C2
// batch of 10k queries 11 % slower, 512 queries 4 % faster.  Dimensions
// above 2048 (128 chunks) have no instance.
constexpr int I8_MAX_CHUNKS = 128;
#ifndef VSG_I8_SHAPE48
#define VSG_I8_SHAPE48 16, 3, 4  // probe builds: another shape for 33..48 chunks
#endif
template <typename F> inline void dispatch_shape_i8(int sc, F&& f) {
    if (sc <= 8) f(Shape<8, 1, 8>{});
    else if (sc <= 16) f(Shape<16, 1, 8>{});
    else if (sc <= 32) f(Shape<16, 2, 4>{});
    else if (sc <= 48) f(Shape<VSG_I8_SHAPE48>{});
    else if (sc <= 96) f(Shape<32, 3, 4>{});
    else f(Shape<32, 4, 2>{});
}

template <int G, int VM> struct QReg<G, VM, SketchI8> {
    static constexpr int LDS_BYTES = VM * 2 * G * 16;  // the query image (SketchQ)
    SketchQ<G, VM> sq;
    const uint8_t* sk;
    const float2* meta;
    const float* sqnorm;  // |x|^2 of the f32 rows (l2sq)
    size_t stride;
    int schunks;
    // the f32 side, for rows and queries without a usable sketch: the rows, the prepared
    // query, and the f32 search's row shape (its sums in its order)
    const uint8_t* fvecs;
    const uint8_t* fq;
    size_t frow_bytes;
    int fnchunks, gf, vmf;

    // lds: LDS_BYTES, after the visited table and the staging
    __device__ __forceinline__ void setup(const SearchParams& p, int qi, uint8_t* lds) {
        sk = p.sk;
        meta = reinterpret_cast<const float2*>(p.sk_meta);
        sqnorm = p.sqnorm;
        stride = p.sk_stride;
        schunks = (int)(p.sk_stride / 16);
        fvecs = p.g.vecs;
        frow_bytes = p.g.row_bytes;
        fnchunks = p.g.nchunks;
        fq = p.queries + (size_t)qi * p.g.row_bytes;
        gf = p.i8_gf;
        vmf = p.i8_vmf;
        sq.stage(fq, fnchunks, p.sk_dim, lds);
    }
    // the query has a usable quantisation (else every row is scored in f32: the f32 walk)
    __device__ __forceinline__ bool usable() const { return sq.k.sq > 0.f; }

    // The f32 distance of the listed rows whose out[] is NaN (all of them: every row), as
    // the plain kernel's rows_dist computes it with the f32 row shape (GF lanes, vmf chunks
    // per lane in order, group_sum0) -- row and query chunks straight from memory, 64 / GF
    // rows at a time.  Rare by construction (all-zero or non-finite rows and queries, rows a
    // concurrent build has not converted yet), so it is written for few registers, not speed.
    template <int GF, int MET>
    __device__ __forceinline__ void rows_f32(const uint32_t* ids, int count, float* out, bool all) const {
        constexpr int RF = 64 / GF;
        const int lane = lane_id();
        const int sub = lane / GF;
        const int sl = lane % GF;
#pragma unroll 1
        for (int base = 0; base < count; base += RF) {
            const int r = base + sub;
            const int rr = r < count ? r : count - 1;
            const float cur = out[rr];
            const bool need = r < count && (all || cur != cur);
            if (!__ballot(need)) continue;
            const uint8_t* row = fvecs + (size_t)ids[rr] * frow_bytes;
            float acc = 0.f;
#pragma unroll 1
            for (int v = 0; v < vmf; ++v) {
                const int c = v * GF + sl;
                if (c < fnchunks) {  // past the row both images are zero: nothing is added
                    float x[4], y[4];
                    load_chunk<float>(row, c, x);
                    load_chunk<float>(fq, c, y);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = metric_fma<MET>(x[e], y[e], acc);
                }
            }
            acc = group_sum0<GF>(acc);
            if (sl == 0 && need) out[r] = (MET == MET_L2) ? acc : 1.f - acc;
        }
    }

    // rows_dist of the int8 walk: out[r] = the metric distance of the sketch estimate
    // (sketch_estimate, sketch.hpp) of row ids[r].  All U x VM 16-B loads of a pass and its
    // (scale, err) pairs (and |x|^2 for l2sq) are issued before any arithmetic; a word's bias
    // flips with one xor, v_dot4_i32_i8 forms the two integer sums four products at a time,
    // group_isum0 reduces them.  A row without a usable sketch is marked NaN (no usable pair
    // gives one: p and S are finite) and scored from its f32 row afterwards.
    template <int U, int MET>
    __device__ __forceinline__ void rows(const uint32_t* ids, int count, float* out) const {
        constexpr int RS = 64 / G;
        const int lane = lane_id();
        const int sub = lane / G;
        const int sl = lane % G;
        if (usable()) {
            bool bad = false;
            for (int base = 0; base < count; base += RS * U) {
                uint4 raw[U][VM];
                float2 mt[U];
                [[maybe_unused]] float xn[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int r = base + u * RS + sub;
                    const uint32_t id = ids[r < count ? r : count - 1];
                    const uint8_t* row = sk + (size_t)id * stride;
                    mt[u] = meta[id];
                    if constexpr (MET == MET_L2) xn[u] = sqnorm[id];
#pragma unroll
                    for (int v = 0; v < VM; ++v) {
                        const int c = v * G + sl;
                        raw[u][v] = *reinterpret_cast<const uint4*>(row + (size_t)(c < schunks ? c : schunks - 1) * 16);
                    }
                }
                // the query's planes, from LDS under the row loads
                uint4 qh[VM], ql[VM];
#pragma unroll
                for (int v = 0; v < VM; ++v) {
                    qh[v] = sq.img[(v * 2 + 0) * G + sl];
                    ql[v] = sq.img[(v * 2 + 1) * G + sl];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (base + u * RS >= count) break;
                    int ah = 0, al = 0;
#pragma unroll
                    for (int v = 0; v < VM; ++v) {
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
                    ah = group_isum0<G>(ah);
                    al = group_isum0<G>(al);
                    const int r = base + u * RS + sub;
                    if (sl == 0 && r < count) {
                        const SketchMeta m{mt[u].x, mt[u].y};
                        const float est = sketch_estimate(sq.k, m, ah, al);
                        float d;
                        if constexpr (MET == MET_L2) d = sketch_dist_l2(est, xn[u], sq.sum2);
                        else d = sketch_dist_dot(est);
                        const bool ok = sketch_usable(m);
                        out[r] = ok ? d : __builtin_nanf("");
                        bad = bad || !ok;
                    }
                }
            }
            if (!__ballot(bad)) return;
            wave_sync();
        }
        const bool all = !usable();
        switch (gf) {
            case 4: rows_f32<4, MET>(ids, count, out, all); break;
            case 8: rows_f32<8, MET>(ids, count, out, all); break;
            case 16: rows_f32<16, MET>(ids, count, out, all); break;
            case 32: rows_f32<32, MET>(ids, count, out, all); break;
            default: rows_f32<64, MET>(ids, count, out, all); break;
        }
    }
};

}  // namespace vsg

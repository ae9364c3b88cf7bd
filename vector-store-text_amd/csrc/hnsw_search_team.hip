// hnsw_search_team.hip — the register search (hnsw_search_reg.hip) with a team of 2 or 4
// waves per query, for batches so small that one wave per query leaves most of the chip
// idle.
//
// One workgroup = one query.  Wave 0, the leader, runs the register search as it is:
// dist_one, greedy_level, beam_reg, the same RegSet / Visited / admit / compact, the same
// LDS carve.  It walks the graph alone; only the distance evaluations of each call of
// rows_dist -- the one dependent step that is parallel across rows -- are shared.  The
// storage tag TeamRows<T> is a row policy (vsg_device.hpp RowPolicy): rows_dist hands the
// call to QReg<G, VM, TeamRows<T>>::rows(), which publishes the row count in a team word
// in LDS; every wave of the team then scores a contiguous slice of the listed rows
// (team_slice, hnsw_search_team.hpp) with rows_dist_plain on its own register image of the
// query, straight into the leader's w.tdist.  A row's distance is summed by G lanes x VM
// chunks in the same order wherever the row stands in a list, so every distance, and with
// it the walk and the result, is the one-wave kernel's bit for bit.
//
// Barriers (block barriers of 2 or 4 waves; a mismatch hangs the workgroup):
//   * leader, per rows() call:  write count; barrier A; score; barrier B.
//   * helper, forever:          barrier A; read count; DONE -> leave; score; barrier B.
//   * leader, once, after the walk: write DONE; barrier A (QReg::done()).
//   So the leader executes A B A B ... A and each helper the same sequence.  What keeps
//   this true:
//   - rows() is reached only under wave-uniform control flow (every branch of dist_one,
//     greedy_level and beam_reg around rows_dist tests ballots or scalars), and only by
//     the leader; the helpers never run the walk;
//   - the kernel has no early return: the leader's body is straight-line code with
//     exactly one done() between the walk and the extraction, reached on every path --
//     an empty index (p.entry == VSG_EMPTY) skips the walk, not done(); short result
//     rows are padded after it;
//   - the team word is written only by the leader, before A, and read by the helpers
//     between A and B (or before leaving), so no write overtakes a read;
//   - ids / out are the leader's w.todo / w.tdist: the same LDS for all waves (carve());
//     the leader's writes to w.todo precede A, the team's writes to w.tdist precede B.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "hnsw_common.hpp"
#include "hnsw_regset.hpp"
#include "hnsw_search_team.hpp"
#include "vsg_dispatch.hpp"

namespace vsg {

template <typename T> struct TeamRows {};
template <typename T> struct RowPolicy<TeamRows<T>> {
    static constexpr bool own = true;
};

// The row policy of a team wave: the wave's own register image of the query, the rows, the
// wave's place in the team and the team word.
template <int G, int VM, typename T> struct QReg<G, VM, TeamRows<T>> {
    QReg<G, VM, T> img;
    const uint8_t* vecs;
    size_t row_bytes;
    int nchunks;
    int wave, waves;
    volatile uint32_t* word;  // LDS, 16 B: [0] = rows of the current call, or TEAM_DONE

    __device__ __forceinline__ void setup(const SearchParams& p, int qi, int wave_, int waves_, uint8_t* word_lds) {
        vecs = p.g.vecs;
        row_bytes = p.g.row_bytes;
        nchunks = p.g.nchunks;
        wave = wave_;
        waves = waves_;
        word = reinterpret_cast<volatile uint32_t*>(word_lds);
        img.load(p.queries + (size_t)qi * p.g.row_bytes, p.g.nchunks);
    }

    // this wave's slice of the listed rows
    template <int U, int MET>
    __device__ __forceinline__ void score(const uint32_t* ids, int count, float* out) const {
        const TeamSlice s = team_slice(count, waves, wave, 64 / G);
        if (s.count > 0)
            rows_dist_plain<G, VM, U, T, MET>(vecs, row_bytes, nchunks, ids + s.begin, s.count, img, out + s.begin);
    }

    // rows_dist of the leader (wave-uniform count)
    template <int U, int MET>
    __device__ __forceinline__ void rows(const uint32_t* ids, int count, float* out) const {
        if (lane_id() == 0) word[0] = (uint32_t)count;
        __syncthreads();  // A
        score<U, MET>(ids, count, out);
        __syncthreads();  // B
    }

    // leader: the walk is over
    __device__ __forceinline__ void done() const {
        if (lane_id() == 0) word[0] = TEAM_DONE;
        __syncthreads();  // A
    }

    // helper: score slices of the leader's lists until the walk is over
    template <int U, int MET> __device__ __forceinline__ void help(const uint32_t* ids, float* out) const {
        for (;;) {
            __syncthreads();  // A
            const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)word[0]);
            if (c == TEAM_DONE) break;
            score<U, MET>(ids, (int)c, out);
            __syncthreads();  // B
        }
    }
};

template <int G, int VM, int U, typename T, int MET, int R>
__global__ __launch_bounds__(256) void hnsw_search_team_kernel(SearchParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using TT = TeamRows<T>;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int qi = blockIdx.x;
    const GraphDev g = to_dev(p.g);
    WaveLds w = carve(smem, 0, p.hash_size, 0);
    QReg<G, VM, TT> q;
    q.setup(p, qi, wave, (int)(blockDim.x >> 6), smem + wave_lds_bytes(p.hash_size, 0, 0));
    if (wave != 0) {
        q.template help<U, MET>(w.todo, w.tdist);
    } else {
        uint64_t ndist = 0, nadj = 0;
        BeamProf pf;
        int count = 0;
        uint64_t* ok = p.out_keys + (size_t)qi * p.k;
        float* od = p.out_dist + (size_t)qi * p.k;
        const bool walk = p.entry != VSG_EMPTY;
        RegSet<R> B;
        if (walk) {
            uint32_t cur = p.entry;
            float dcur = dist_one<G, VM, U, TT, MET>(g, q, cur, w);
            ++ndist;
            for (int l = p.max_level; l >= 1; --l) greedy_level<G, VM, U, TT, MET>(g, q, l, cur, dcur, w, ndist, nadj);
            beam_reg<G, VM, U, TT, MET, R>(g, q, 0, cur, dcur, p.ef, w, B, ndist, nadj, pf);
        }
        q.done();  // the one place the helpers are released, on every path
        if (walk) {
            // the extraction of search_reg_one (hnsw_search_reg.hip): tombstones skipped in
            // the output; ascending top-ef keys, slots of the alive ones staged in the
            // (finished) visited table, keys gathered after
            uint32_t alive = 0;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (B.k[r] != VSG_KEY_EMPTY && !(p.flags[(uint32_t)B.k[r] & VSG_ID_MASK] & 1)) alive |= 1u << r;
            uint32_t* sel = w.vis.tab;
            const int lim = min(p.ef, B.size);
            for (int x = 0; x < lim && count < p.k; ++x) {
                uint64_t b = VSG_KEY_EMPTY;
#pragma unroll
                for (int r = 0; r < R; ++r) b = B.k[r] < b ? B.k[r] : b;
                b = wave_min64(b);
                if (b == VSG_KEY_EMPTY) break;
                bool live = false;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (B.k[r] == b) {
                        live = (alive >> r) & 1u;
                        B.k[r] = VSG_KEY_EMPTY;
                    }
                if (__ballot(live)) {
                    if (lane == 0) {
                        od[count] = key_dist(b);
                        sel[count] = (uint32_t)b & VSG_ID_MASK;
                    }
                    ++count;
                }
            }
            wave_sync();
            for (int j = lane; j < count; j += 64) ok[j] = p.keys ? p.keys[sel[j]] : (uint64_t)sel[j];
        }
        for (int j = count + lane; j < p.k; j += 64) {
            ok[j] = ~0ull;
            od[j] = __builtin_inff();
        }
        if (lane == 0) {
            if (p.out_counts) p.out_counts[qi] = (uint32_t)count;
            if (p.stats) {
                atomicAdd(&p.stats[0], (unsigned long long)ndist);
                atomicAdd(&p.stats[1], (unsigned long long)nadj);
                atomicAdd(&p.stats[2], 1ull);
            }
        }
    }
}

size_t search_team_lds_bytes(int hash) { return wave_lds_bytes(hash, 0, 0) + 16; }

// f(kernel) for the instance of (storage, metric, row shape, register rows): the row shapes
// and register-row classes of launch_search_reg, so the sums are the one-wave kernel's
template <typename F> static void team_instance(Storage st, MetricKind mk, int nchunks, int ef, F&& f) {
    auto with_rows = [&](auto rtag) {
        constexpr int R = decltype(rtag)::value;
        auto body = [&](auto sh, auto tt, auto mt) {
            constexpr int G = decltype(sh)::G, VM = decltype(sh)::VM, U = decltype(sh)::U;
            using T = typename decltype(tt)::T;
            constexpr int MET = decltype(mt)::MET;
            f(hnsw_search_team_kernel<G, VM, U, T, MET, R>);
        };
        if constexpr (R == 2) dispatch_all<SHAPE_SEARCH_SMALL_EF>(st, mk, nchunks, body);
        else dispatch_all<SHAPE_SEARCH>(st, mk, nchunks, body);
    };
    if (ef <= 64) with_rows(std::integral_constant<int, 2>{});
    else with_rows(std::integral_constant<int, 4>{});
}

static bool team_args_ok(int nchunks, int ef, int hash_size, int waves) {
    return (waves == 2 || waves == 4) && ef >= 1 && ef <= TEAM_MAX_EF && hash_size >= 8 && shape_supported(nchunks);
}

// Teams of `waves` waves resident on the whole device at once (occupancy of the instance at
// 64 * waves threads and its LDS size, times the CUs), cached per (device, kernel, LDS, waves).
int search_team_capacity(Storage st, MetricKind mk, int nchunks, int ef, int hash_size, int waves) {
    if (!team_args_ok(nchunks, ef, hash_size, waves)) return 0;
    static std::mutex mu;
    static std::map<std::tuple<int, const void*, size_t, int>, int> cache;
    const size_t lds = search_team_lds_bytes(hash_size);
    int dev = 0, res = 0;
    (void)hipGetDevice(&dev);
    team_instance(st, mk, nchunks, ef, [&](auto kern) {
        std::lock_guard<std::mutex> lk(mu);
        const auto key = std::make_tuple(dev, (const void*)kern, lds, waves);
        auto it = cache.find(key);
        if (it != cache.end()) {
            res = it->second;
            return;
        }
        int cus = 0, per_cu = 0;
        if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * waves, lds) != hipSuccess) {
            (void)hipGetLastError();
            per_cu = 0;
        }
        res = std::max(0, per_cu * cus);
        cache[key] = res;
    });
    return res;
}

// One workgroup of `waves` waves per query; the caller sends only batches within
// search_team_capacity (vsg_index.cpp run_graph), unfiltered, greedy descent, f32 / f16 rows.
hipError_t launch_search_team(Storage st, MetricKind mk, const SearchParams& p, int waves, hipStream_t s) {
    if (p.nq <= 0) return hipSuccess;
    if (!team_args_ok(p.g.nchunks, p.ef, p.hash_size, waves) || p.k > p.ef || p.hash_size < p.k || p.filt || p.i8 ||
        p.upper_ef > 1 || p.nq > (1 << 22))  // 256 work-items each: the AQL grid size is 32-bit
        return hipErrorInvalidValue;
    const size_t lds = search_team_lds_bytes(p.hash_size);
    hipError_t err = hipSuccess;
    team_instance(st, mk, p.g.nchunks, p.ef, [&](auto kern) {
        if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3((unsigned)p.nq), dim3(64 * waves), lds, s, p);
        err = hipGetLastError();
    });
    return err;
}

}  // namespace vsg

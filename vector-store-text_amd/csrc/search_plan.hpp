// search_plan.hpp — the arithmetic of one device search, host only (no HIP include):
// the partial-list shape of the two exact kernels, the visited-table size of the graph
// search and the carve-up of the search workspace.  Pure functions of their arguments,
// structs by value: vsg_index.cpp's search_device_locked calls them on every search,
// tests/cpp/test_search_plan.cpp sweeps them on the CPU (a mistake here drops rows
// from an exact search without any error).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace vsg {

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the 128 x 128 MFMA tile (vsg_kernels.hpp MFMA_BQ / MFMA_BR; equality is asserted in
// vsg_index.cpp) and the most partial lists one merge wave walks
constexpr int PLAN_MFMA_BQ = 128, PLAN_MFMA_BR = 128;
constexpr int PLAN_MERGE_LISTS = 64;
constexpr size_t PLAN_MAX_BLOCKS = 32768;

// Partial-list shape of an exact search: each (query, list) holds `kmax` (MFMA) or k
// (VALU) entries; more than 64 lists per query are whole 64-list groups, merged in two
// stages (stage 1 writes ngroups k-lists per query behind the np_lists partial entries).
struct ExactPlan {
    // MFMA: (query tile, row split) blocks
    int bq = 0, br = 0, qtiles = 0, kmax = 0, nparts = 0;
    size_t splits = 0, tiles_per_split = 0;
    // VALU: grid.y row blocks
    int nblocks = 1, rows_per_block = 1;
    // both
    int ngroups = 0;              // 0: one merge over all lists
    size_t np_lists = 0, np = 0;  // entries: partial lists, and those + the group results
    int lists() const { return nparts ? nparts : nblocks; }  // partial lists per query
};

// f32 matrix-core brute force: k <= 16, nq >= 1, slots >= 1
static inline ExactPlan plan_exact_mfma(size_t nq, size_t slots, size_t k) {
    ExactPlan p;
    p.bq = nq <= 64 ? 64 : PLAN_MFMA_BQ;        // the 64-query tile for small batches
    p.br = p.bq == 64 ? 256 : PLAN_MFMA_BR;     // ... 256 rows deep
    p.qtiles = (int)((nq + p.bq - 1) / p.bq);
    const size_t ntiles = (slots + p.br - 1) / p.br;
    // (query tile, row split) blocks in whole rounds of resident blocks (2 per CU:
    // 64 / 80 KiB of LDS): 1,024 = two rounds of the 128 x 128 tile, 512 = one of
    // the 256 x 64 tile (round 2: 1,024 blocks of a 128 x 64 tile, 1.33 rounds)
    const size_t target = p.bq == 64 ? 512 : 1024;
    size_t splits = std::min<size_t>(ntiles, std::max<size_t>(1, (target + p.qtiles - 1) / p.qtiles));
    const size_t tps = (ntiles + splits - 1) / splits;
    splits = (ntiles + tps - 1) / tps;
    p.kmax = 16;
    // more than 64 partial lists per query: whole 64-list groups (padding splits
    // hold no rows and write empty lists), merged in two stages
    const size_t lists = (size_t)(p.br / 64) * 2;  // per split: row waves x half-waves
    if (splits * lists > PLAN_MERGE_LISTS) {
        splits = (splits * lists + 63) / 64 * 64 / lists;
        p.ngroups = (int)(splits * lists / 64);
    }
    p.splits = splits;
    p.tiles_per_split = tps;
    p.nparts = (int)(splits * lists);
    p.np_lists = nq * (size_t)p.nparts * p.kmax;
    p.np = p.np_lists + (p.ngroups ? nq * (size_t)p.ngroups * k : 0);
    return p;
}

// VALU brute force (any storage, k <= MAX_EXACT_K): min_waves is VSG_EXACT_MIN_WAVES
static inline ExactPlan plan_exact_valu(size_t nq, size_t slots, size_t k, size_t min_waves) {
    ExactPlan p;
    // grid.y = row blocks (<= 65535 per dimension).  4,096-row blocks fill the
    // chip from ~32 queries on; a smaller batch gets more, shorter blocks so
    // the launch still holds >= VSG_EXACT_MIN_WAVES waves (at one query the
    // 245 waves of 4,096-row blocks read C5's 6 GB at 0.11 of HBM,
    // profiles/r03_bench_c5_batches.jsonl), down to 64 rows per block
    const size_t nb = std::max<size_t>((slots + 4095) / 4096, std::min((min_waves + nq - 1) / nq, (slots + 63) / 64));
    int nblocks = (int)std::min<size_t>(PLAN_MAX_BLOCKS, std::max<size_t>(1, nb));
    // large k: bound the partial lists (nq x nblocks x k x 8 B) to ~1 GiB
    const size_t cap_blocks = std::max<size_t>(1, ((size_t)1 << 30) / (8 * nq * k));
    nblocks = (int)std::min<size_t>((size_t)nblocks, cap_blocks);
    // more than 64 lists per query: merged in two stages (64-list groups in
    // parallel, then the group results), not by one wave walking all of them
    if (nblocks > PLAN_MERGE_LISTS && slots > 0) {
        nblocks = (nblocks + 63) / 64 * 64;  // padding blocks hold no rows (empty lists)
        p.ngroups = nblocks / 64;
    }
    p.rows_per_block = (int)((slots + nblocks - 1) / nblocks);
    if (slots == 0) nblocks = 1;
    p.nblocks = nblocks;
    p.np_lists = nq * (size_t)nblocks * k;
    p.np = p.np_lists + (p.ngroups ? nq * (size_t)p.ngroups * k : 0);
    return p;
}

// Visited table of the graph search (entries, a multiple of 64, <= 16,384): LDS is the
// occupancy limit at large ef, and a forgotten node costs one more row read -- cheap
// for short rows.  factor_env / min_env: the values of VSG_SEARCH_HASH_FACTOR and
// VSG_SEARCH_HASH_MIN (probes; null or empty: the defaults).
static inline int search_hash_size(int ef, size_t row_bytes, bool reg, const char* factor_env, const char* min_env) {
    const auto env = [](const char* v, double dflt) { return v && *v ? atof(v) : dflt; };
    const bool wide = row_bytes >= 1024;
    // register kernel: sweep in profiles/r01_search_hash_reg.jsonl
    const int factor = (int)env(factor_env, wide ? (reg ? 8 : 12) : (reg ? 4 : 6));
    // VSG_SEARCH_HASH_MIN: smallest table (entries, multiple of 64)
    const int hmin = std::max(64, (int)env(min_env, wide ? 2048 : 1024)) & ~63;
    const int raw = std::min(16384, (int)(((long)factor * ef + 63) & ~63L));
    return std::max(raw, hmin);
}

// One search's scratch block: byte offsets of its regions, in this order, each
// rounded up to 256 B (a region of 0 bytes takes none and shares the next one's offset).
struct SearchLayout {
    struct Sizes {
        size_t queries = 0;      // prepared queries (nq x row_bytes)
        size_t qnorms = 0;       // |q|^2 (MFMA exact)
        size_t part = 0;         // partial distances, and again for the partial ids
        size_t q16 = 0;          // f16 traversal: f16 queries,
        size_t cand_keys = 0;    //   candidate slots (the beam handed to the re-rank),
        size_t cand_dist = 0;    //   candidate distances,
        size_t cand_counts = 0;  //   candidate counts
        size_t overflow = 0;     // filtered search: per-query overflow flags,
        size_t rerun = 0;        //   the re-run lists in device memory
    };
    size_t queries = 0, qnorms = 0, part_d = 0, part_i = 0, q16 = 0, cand_keys = 0, cand_dist = 0, cand_counts = 0,
           overflow = 0, rerun = 0, counter = 0, total = 0;
    SearchLayout() = default;
    explicit SearchLayout(const Sizes& b) {
        size_t at = 0;
        const auto take = [&at](size_t bytes) {
            const size_t o = at;
            at += align256(bytes);
            return o;
        };
        queries = take(b.queries);
        qnorms = take(b.qnorms);
        part_d = take(b.part);
        part_i = take(b.part);
        q16 = take(b.q16);
        cand_keys = take(b.cand_keys);
        cand_dist = take(b.cand_dist);
        cand_counts = take(b.cand_counts);
        overflow = take(b.overflow);
        rerun = take(b.rerun);
        counter = take(256);  // persistent-grid counter (one word)
        total = at;
    }
};

}  // namespace vsg

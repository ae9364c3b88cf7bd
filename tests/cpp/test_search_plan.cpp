// CPU check of csrc/search_plan.hpp (no GPU, no HIP): the partial-list plans of the two
// exact kernels, the visited-table rule and the workspace layout.
//   1. invariants swept over batch sizes, row counts and k: every row is in exactly one
//      block / split, every partial list in exactly one merge group, the layout's
//      regions are aligned, ordered and disjoint and sum to the closed form that
//      search_device_locked used before the layout existed;
//   2. fixed cases, computed from the expressions the plans were moved out of.
// Built with -fsanitize=address,undefined by tests/test_search_plan.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../vector-store-text_amd/csrc/search_plan.hpp"

using namespace vsg;

static int g_failed = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_failed <= 20) {                        \
                std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

static const size_t NQS[] = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 10000};
static const size_t SLOTS[] = {0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 5000, 1000000, (size_t)1 << 29};
static const size_t KS[] = {1, 10, 16, 17, 8192};

// the rules the two plans share: lists per query vs merge groups, entries
static void check_groups(const ExactPlan& p, size_t nq, size_t k, const char* what, size_t slots) {
    const int lists = p.lists();
    if (p.ngroups == 0)
        CHECK(lists <= 64, "%s nq %zu slots %zu k %zu: %d lists in one merge", what, nq, slots, k, lists);
    else
        CHECK(p.ngroups > 0 && lists == 64 * p.ngroups, "%s nq %zu slots %zu k %zu: %d lists, %d groups", what, nq,
              slots, k, lists, p.ngroups);
    CHECK(p.np == p.np_lists + nq * (size_t)p.ngroups * k, "%s nq %zu slots %zu k %zu: np %zu np_lists %zu", what, nq,
          slots, k, p.np, p.np_lists);
}

static void sweep_mfma() {
    for (size_t nq : NQS)
        for (size_t slots : SLOTS)
            for (size_t k : KS) {
                // the MFMA search takes k <= 16 and an index with rows (an empty one goes to the VALU plan)
                if (k > 16 || slots == 0) continue;
                const ExactPlan p = plan_exact_mfma(nq, slots, k);
                CHECK((p.bq == 64 && p.br == 256) || (p.bq == 128 && p.br == 128), "tile %d x %d", p.bq, p.br);
                CHECK((p.bq == 64) == (nq <= 64), "nq %zu bq %d", nq, p.bq);
                CHECK((size_t)p.qtiles * p.bq >= nq && (size_t)(p.qtiles - 1) * p.bq < nq, "nq %zu qtiles %d", nq,
                      p.qtiles);
                CHECK(p.kmax == 16, "kmax %d", p.kmax);
                const size_t ntiles = (slots + p.br - 1) / p.br;
                CHECK(p.tiles_per_split >= 1 && p.splits >= 1, "nq %zu slots %zu", nq, slots);
                // every row tile is in a split
                CHECK(p.splits * p.tiles_per_split * p.br >= slots, "nq %zu slots %zu: %zu x %zu x %d", nq, slots,
                      p.splits, p.tiles_per_split, p.br);
                // the first ceil(ntiles / tps) splits hold at least one tile each; the rest are padding
                const size_t used = (ntiles + p.tiles_per_split - 1) / p.tiles_per_split;
                CHECK(used <= p.splits && (used - 1) * p.tiles_per_split < ntiles, "nq %zu slots %zu: used %zu of %zu",
                      nq, slots, used, p.splits);
                CHECK(p.nparts == (int)(p.splits * (size_t)(p.br / 64) * 2), "nparts %d splits %zu", p.nparts, p.splits);
                // the splits that fit the kernel's int fields and a grid dimension
                CHECK(p.splits <= 65535 && p.tiles_per_split <= 0x7FFFFFFF, "splits %zu tps %zu", p.splits,
                      p.tiles_per_split);
                check_groups(p, nq, k, "mfma", slots);
                CHECK(p.np_lists == nq * (size_t)p.nparts * 16, "np_lists %zu", p.np_lists);
            }
}

static void sweep_valu() {
    for (size_t nq : NQS)
        for (size_t slots : SLOTS)
            for (size_t k : KS)
                for (size_t min_waves : {(size_t)8192, (size_t)1, (size_t)100000}) {
                    const ExactPlan p = plan_exact_valu(nq, slots, k, min_waves);
                    const size_t nb = (size_t)p.nblocks, rpb = (size_t)p.rows_per_block;
                    CHECK(p.nblocks >= 1 && p.nblocks <= 32768, "nq %zu slots %zu k %zu: nblocks %d", nq, slots, k,
                          p.nblocks);
                    CHECK(p.rows_per_block >= 0, "rpb %d", p.rows_per_block);
                    // every row is in a block
                    CHECK(nb * rpb >= slots, "nq %zu slots %zu k %zu: %zu x %zu", nq, slots, k, nb, rpb);
                    // no block but the padding of the 64-list rounding is without rows
                    const size_t used = rpb ? (slots + rpb - 1) / rpb : 0;
                    CHECK((nb - 1) * rpb < slots || (p.ngroups > 0 && nb - used < 64) || slots == 0,
                          "nq %zu slots %zu k %zu: %zu blocks of %zu rows, %zu used", nq, slots, k, nb, rpb, used);
                    if (slots == 0) CHECK(p.nblocks == 1 && p.ngroups == 0, "empty index: nblocks %d", p.nblocks);
                    check_groups(p, nq, k, "valu", slots);
                    CHECK(p.np_lists == nq * nb * k, "np_lists %zu", p.np_lists);
                    // the partial lists (distances + ids) stay near 1 GiB
                    if (p.nblocks > 1) CHECK(p.np_lists * 8 <= ((size_t)1 << 30) + 64 * nq * k * 8, "np_lists %zu", p.np_lists);
                }
}

// the closed form of the workspace size before SearchLayout
static size_t old_total(const SearchLayout::Sizes& b) {
    const size_t qp_b = align256(b.queries), qsq_b = align256(b.qnorms), part_b = align256(b.part);
    const size_t rr_b = align256(b.q16) + align256(b.cand_keys) + align256(b.cand_dist) + align256(b.cand_counts);
    const size_t filt_b = align256(b.overflow) + align256(b.rerun);
    return qp_b + qsq_b + 2 * part_b + rr_b + filt_b + 256;
}

static void check_layout(const SearchLayout::Sizes& b) {
    const SearchLayout l(b);
    const size_t off[] = {l.queries,   l.qnorms,      l.part_d,   l.part_i, l.q16,    l.cand_keys,
                          l.cand_dist, l.cand_counts, l.overflow, l.rerun,  l.counter};
    const size_t len[] = {b.queries,   b.qnorms,      b.part,     b.part,  b.q16, b.cand_keys,
                          b.cand_dist, b.cand_counts, b.overflow, b.rerun, 256};
    size_t end = 0;  // of the regions before: ordered and disjoint
    for (int i = 0; i < 11; ++i) {
        CHECK(off[i] % 256 == 0, "region %d at %zu", i, off[i]);
        CHECK(off[i] >= end, "region %d at %zu overlaps the one before (ends %zu)", i, off[i], end);
        CHECK(off[i] - end < 256, "region %d at %zu leaves a hole after %zu", i, off[i], end);
        end = off[i] + len[i];
        CHECK(end <= l.total, "region %d ends at %zu > total %zu", i, end, l.total);
    }
    CHECK(l.queries == 0, "queries at %zu", l.queries);
    CHECK(l.total == old_total(b), "total %zu != closed form %zu", l.total, old_total(b));
    // the offsets search_device_locked summed by hand
    const size_t qp_b = align256(b.queries), qsq_b = align256(b.qnorms), part_b = align256(b.part);
    CHECK(l.part_d == qp_b + qsq_b && l.part_i == qp_b + qsq_b + part_b && l.q16 == qp_b + qsq_b + 2 * part_b,
          "partial lists at %zu / %zu, f16 queries at %zu", l.part_d, l.part_i, l.q16);
    CHECK(l.counter + 256 == l.total, "counter at %zu of %zu", l.counter, l.total);
}

static void sweep_layout() {
    for (size_t nq : NQS)
        for (size_t row_bytes : {(size_t)16, (size_t)264 * 4, (size_t)3072})
            for (size_t np : {(size_t)0, (size_t)70, (size_t)124080})
                for (int mode = 0; mode < 8; ++mode) {
                    SearchLayout::Sizes b;
                    b.queries = nq * row_bytes;
                    if (mode & 1) b.qnorms = nq * 4;
                    b.part = np * 4;
                    if (mode & 2) {
                        const size_t ef = 36;
                        b.q16 = nq * row_bytes / 2;
                        b.cand_keys = nq * ef * 8;
                        b.cand_dist = b.cand_counts = nq * ef * 4;
                    }
                    if (mode & 4) {
                        b.overflow = nq;
                        check_layout(b);  // the fallback without the re-run lists
                        b.rerun = 1234567 + nq;
                    }
                    check_layout(b);
                }
}

struct Fixed {
    const char* plan;
    size_t nq, slots, k;
    // -1: not pinned
    long bq, br, qtiles, splits, tps, nparts, nblocks, rpb, ngroups, np_lists, np;
};

// from the parent's expressions (search_device_locked before the plans were moved out)
static const Fixed FIXED[] = {
    {"mfma", 40, 5000, 10, 64, 256, 1, 24, 1, 192, -1, -1, 3, 122880, 124080},
    {"mfma", 160, 5000, 10, 128, 128, 2, 48, 1, 192, -1, -1, 3, 491520, 496320},
    {"mfma", 40, 1200, 10, -1, -1, -1, 5, -1, 40, -1, -1, 0, -1, 25600},
    {"mfma", 100, 3000, 10, -1, -1, -1, 32, -1, 128, -1, -1, 2, 204800, 206800},
    {"mfma", 256, 1000000, 11, -1, -1, -1, 496, 16, 1984, -1, -1, 31, 8126464, 8213760},
    {"valu", 1, 1000000, 10, -1, -1, -1, -1, -1, -1, 8192, 123, 128, -1, 83200},
    {"valu", 40, 5000, 10, -1, -1, -1, -1, -1, -1, 128, 40, 2, -1, 52000},
    {"valu", 160, 5000, 10, -1, -1, -1, -1, -1, -1, 52, 97, 0, -1, 83200},
    {"valu", 7, 0, 10, -1, -1, -1, -1, -1, -1, 1, 0, 0, -1, 70},
    {"valu", 64, 1000000, 8192, -1, -1, -1, -1, -1, -1, 256, 3907, 4, -1, 136314880},
    {"valu", 1, 100, 10, -1, -1, -1, -1, -1, -1, 2, 50, 0, -1, 20},
};

static void fixed_cases() {
    for (const Fixed& f : FIXED) {
        const bool mfma = f.plan[0] == 'm';
        const ExactPlan p = mfma ? plan_exact_mfma(f.nq, f.slots, f.k) : plan_exact_valu(f.nq, f.slots, f.k, 8192);
        const auto same = [&](const char* name, long want, long got) {
            CHECK(want < 0 || want == got, "%s nq %zu slots %zu k %zu: %s %ld, expected %ld", f.plan, f.nq, f.slots,
                  f.k, name, got, want);
        };
        if (mfma) {
            same("bq", f.bq, p.bq);
            same("br", f.br, p.br);
            same("qtiles", f.qtiles, p.qtiles);
            same("splits", f.splits, (long)p.splits);
            same("tiles_per_split", f.tps, (long)p.tiles_per_split);
            same("nparts", f.nparts, p.nparts);
        } else {
            same("nblocks", f.nblocks, p.nblocks);
            same("rows_per_block", f.rpb, p.rows_per_block);
        }
        same("ngroups", f.ngroups, p.ngroups);
        same("np_lists", f.np_lists, (long)p.np_lists);
        same("np", f.np, (long)p.np);
    }
    CHECK(search_hash_size(36, 3072, true, nullptr, nullptr) == 2048, "%d", search_hash_size(36, 3072, true, nullptr, nullptr));
    CHECK(search_hash_size(192, 256, true, nullptr, nullptr) == 1024, "%d", search_hash_size(192, 256, true, nullptr, nullptr));
    CHECK(search_hash_size(4096, 3072, false, nullptr, nullptr) == 16384, "%d",
          search_hash_size(4096, 3072, false, nullptr, nullptr));
    // unset and empty variables are the defaults; set ones override them (probes)
    CHECK(search_hash_size(36, 3072, true, "", "") == 2048, "empty variables");
    CHECK(search_hash_size(448, 3072, true, nullptr, nullptr) == 3584, "8 x 448");
    CHECK(search_hash_size(448, 3072, true, "4", "100") == 1792, "factor 4, min 64");
    CHECK(search_hash_size(10, 256, true, "4", "100") == 64, "min rounds down to a multiple of 64");
    CHECK(search_hash_size(10, 256, true, "4", "1") == 64, "min is at least 64");
    for (int ef = 1; ef <= 4096; ++ef)
        for (int reg = 0; reg < 2; ++reg)
            for (size_t rb : {(size_t)256, (size_t)1024}) {
                const int hs = search_hash_size(ef, rb, reg != 0, nullptr, nullptr);
                CHECK(hs % 64 == 0 && hs >= (rb >= 1024 ? 2048 : 1024) && hs <= 16384, "ef %d: %d", ef, hs);
            }
}

int main() {
    sweep_mfma();
    sweep_valu();
    sweep_layout();
    fixed_cases();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

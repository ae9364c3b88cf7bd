// CPU check of plan_exact_mfma_wide (csrc/search_plan.hpp; no GPU, no HIP), swept over
// batch sizes, row counts, k in 17..128 and split caps.  Built with
// -fsanitize=address,undefined by tests/test_exact_wide_plan.py.
#include <cstdio>

#include "../../vector-store-text_amd/csrc/search_plan.hpp"

using namespace vsg;

static int g_failed = 0;

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond) && ++g_failed <= 20) {                                  \
            std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond);     \
            std::printf(__VA_ARGS__);                                       \
            std::printf("\n");                                              \
        }                                                                   \
    } while (0)

int main() {
    const size_t NQS[] = {32, 33, 64, 65, 128, 129, 257, 1000, 10000, 70000, 1000000};
    const size_t SLOTS[] = {4096, 4097, 4099, 5000, 8192, 65537, 1000000, 12500000, (size_t)1 << 29};
    const size_t KS[] = {17, 40, 100, 127, 128};
    const size_t CAPS[] = {0, 1, 2, 3, 64, 65, 100000};
    for (size_t nq : NQS)
        for (size_t slots : SLOTS)
            for (size_t k : KS)
                for (size_t cap : CAPS) {
                    const ExactWidePlan p = plan_exact_mfma_wide(nq, slots, k, cap);
                    const size_t ntiles = (slots + 127) / 128;
                    CHECK(p.bq == 128 && p.br == 128 && p.kmax == (int)k && p.qpad >= nq && p.qpad < nq + 128 &&
                              p.qpad == (size_t)p.qtiles * 128, "tile %d x %d kmax %d nq %zu qpad %zu", p.bq, p.br, p.kmax, nq, p.qpad);
                    // split s holds tiles [s tps, min((s + 1) tps, ntiles)): disjoint by construction;
                    // together they reach the last tile, and only the 64-list rounding is empty
                    const size_t tps = p.tiles_per_split;
                    CHECK(tps >= 1 && p.splits >= 1 && p.splits * tps >= ntiles, "nq %zu slots %zu: %zu x %zu", nq, slots, p.splits, tps);
                    const size_t used = (ntiles + tps - 1) / tps;
                    CHECK(used <= p.splits && (p.splits == used || (p.ngroups > 0 && p.splits - used < 64)),
                          "nq %zu slots %zu cap %zu: %zu of %zu splits used", nq, slots, cap, used, p.splits);
                    if (cap) CHECK(used <= cap, "cap %zu: %zu splits used", cap, used);
                    CHECK(p.splits <= 65535 && tps <= 0x7FFFFFFF && (size_t)p.qtiles * p.splits <= 0x7FFFFFFF, "grid");
                    // one k-list per (query, split); above 64 lists whole 64-list groups
                    CHECK(p.nparts == (int)p.splits && p.lists() == p.nparts, "nparts %d splits %zu", p.nparts, p.splits);
                    CHECK(p.nparts > 64 ? p.nparts % 64 == 0 && p.ngroups == p.nparts / 64 : p.ngroups == 0, "%d lists, %d groups",
                          p.nparts, p.ngroups);
                    CHECK(p.np_lists == nq * p.splits * k && p.np == p.np_lists + nq * (size_t)p.ngroups * k, "np %zu", p.np);
                    CHECK(p.pool == p.qpad * p.splits * PLAN_WIDE_POOL, "pool %zu", p.pool);
                    // the workspace: lists (distances, ids) and pools are disjoint regions of their size
                    SearchLayout::Sizes sz;
                    sz.queries = nq * 256;
                    sz.qnorms = nq * 4;
                    sz.part = p.np * 4;
                    sz.pool = p.pool * 8;
                    const SearchLayout at(sz);
                    CHECK(at.part_d + sz.part <= at.part_i && at.part_i + sz.part <= at.pool &&
                              at.pool + sz.pool <= at.counter && at.counter + 256 == at.total && at.pool % 256 == 0,
                          "regions %zu %zu %zu %zu of %zu", at.part_d, at.part_i, at.pool, at.counter, at.total);
                    // bound: 512 MiB of pools + 4 KiB per padded query, and the lists below the pools
                    CHECK(sz.pool <= ((size_t)512 << 20) + p.qpad * 4096, "nq %zu slots %zu cap %zu: pools %zu B", nq, slots, cap, sz.pool);
                    CHECK(2 * sz.part <= sz.pool, "lists %zu B above the pools %zu B", 2 * sz.part, sz.pool);
                }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

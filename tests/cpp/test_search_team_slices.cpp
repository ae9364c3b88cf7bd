// CPU check of team_slice (csrc/hnsw_search_team.hpp; no HIP): a team's slices are in order, disjoint,
// whole lane groups except the last, and cover [0, count).  Built by tests/test_search_team_slices.py.
#include <cstdio>
#include <initializer_list>

#include "../../vector-store-text_amd/csrc/hnsw_search_team.hpp"

using namespace vsg;
int main() {
    int failed = 0;
    for (int waves : {2, 4})
        for (int group : {1, 2, 4, 8, 16})
            for (int count = 0; count <= 64; ++count) {
                int next = 0;
                bool ok = true;
                for (int w = 0; w < waves; ++w) {
                    const TeamSlice s = team_slice(count, waves, w, group);
                    ok = ok && s.begin == next && s.count >= 0 && (s.count % group == 0 || s.begin + s.count == count);
                    ok = ok && s.count <= ((count + waves - 1) / waves + group - 1) / group * group;
                    next = s.begin + s.count;
                }
                ok = ok && next == count;
                if (!ok && ++failed <= 20) std::printf("FAIL count %d waves %d group %d\n", count, waves, group);
            }
    if (failed) {
        std::printf("%d cases failed\n", failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

// hnsw_search_team.hpp — how the rows of one expansion are split over the waves of a
// search team (hnsw_search_team.hip).  Plain C++ apart from the function attributes, so
// the CPU test (tests/cpp/test_search_team_slices.cpp) includes it without HIP.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "vsg_kernels.hpp"
#define VSG_TEAM_HD __host__ __device__
#else
#define VSG_TEAM_HD
#endif

namespace vsg {

#ifdef __HIPCC__
// One workgroup of `waves` (2 or 4) waves per query: wave 0 walks as launch_search_reg's
// kernel does and all waves score each expansion's rows.  Same results, bit for bit.
// Unfiltered searches with the greedy descent and ef <= TEAM_MAX_EF on the stored rows only
// (hipErrorInvalidValue otherwise); meant for batches of at most search_team_capacity()
// queries -- the teams resident on the device at once.
hipError_t launch_search_team(Storage st, MetricKind mk, const SearchParams& p, int waves, hipStream_t s);
int search_team_capacity(Storage st, MetricKind mk, int nchunks, int ef, int hash_size, int waves);
#endif

// team word value: the search is over, the helpers leave
constexpr uint32_t TEAM_DONE = 0xFFFFFFFFu;
// largest max(ef, k) with a team instance (the 2- and 4-row register classes)
constexpr int TEAM_MAX_EF = 192;

struct TeamSlice {
    int begin, count;
};

// Wave `wave` of `waves` scores rows [begin, begin + count) of the `count` listed ones:
// contiguous slices of ceil(count / waves) rows rounded up to whole lane groups
// (group_rows = 64 / G rows per pass), in wave order; the last ones may be short or empty.
static inline VSG_TEAM_HD TeamSlice team_slice(int count, int waves, int wave, int group_rows) {
    int per = (count + waves - 1) / waves;
    per = (per + group_rows - 1) / group_rows * group_rows;
    const int b = wave * per < count ? wave * per : count;
    const int e = b + per < count ? b + per : count;
    return TeamSlice{b, e - b};
}

}  // namespace vsg

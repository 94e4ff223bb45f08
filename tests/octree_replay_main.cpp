// octree_replay_main.cpp — a stand-alone program over the host side of
// OctreeGridDataPointsFilter (csrc/common/pmx_octree_replay.h): the replay of
// the reference's swapCols / mapidx sequence on column numbers and the random
// sampler's draws, for a host build with -fsanitize=address,undefined
// (tests/test_octree_chain.py builds and runs it and compares what it prints
// with the numpy restatement of tests/octree_cases.py).
//   replay N p0 p1 ...   the input column each kept column holds
//   rand L               the L factors as float bit patterns, then the next rand()
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common/pmx_octree_replay.h"

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "replay")) {
        const long long n = std::atoll(argv[2]);
        std::vector<int32_t> picks;
        for (int i = 3; i < argc; ++i) picks.push_back((int32_t)std::atoll(argv[i]));
        for (int32_t p : picks)
            if (p < 0 || p >= n) return 2;
        const std::vector<int32_t> col = pmx::octree_replay_columns(picks.data(), (int64_t)picks.size(), n);
        for (int32_t c : col) std::printf("%d ", (int)c);
        std::printf("\n");
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "rand")) {
        const long long L = std::atoll(argv[2]);
        std::srand(987);
        std::vector<float> fac((size_t)L);
        pmx::octree_rand_factors(L, fac.data());
        for (float f : fac) {
            unsigned u;
            std::memcpy(&u, &f, sizeof(u));
            std::printf("%u ", u);
        }
        std::printf("%d\n", std::rand());
        return 0;
    }
    return 2;
}

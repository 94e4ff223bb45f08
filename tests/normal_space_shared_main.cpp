// normal_space_shared_main.cpp — a stand-alone program over the host side of
// NormalSpaceDataPointsFilter that the library compiles in
// (csrc/common/pmx_nss.h, csrc/common/pmx_octree_replay.h): the bucket of a
// normal, the shuffle, the picks over grouped points and the column replay.
// The grouping, a device sort in the library, is a std::stable_sort here.
// tests/test_normal_space_reference.py builds it under AddressSanitizer and
// UndefinedBehaviorSanitizer and compares what it prints with the literal
// program (normal_space_main.cpp): two routes to one answer.
//
//   normal_space_shared filter|time <f|d> <file> <n> <nbSample> <seed> <srand> <epsilon bits>
//       the arguments and the output of normal_space_main.cpp's filter (no
//       stale count: the second line is 0) and time
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common/pmx_nss.h"
#include "common/pmx_octree_replay.h"

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <typename T>
static int run(bool timed, const char* path, int64_t n, int64_t nb_sample, uint64_t seed, unsigned srand_seed,
               double epsilon) {
    std::vector<T> normals((size_t)n * 3);
    std::FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(normals.data(), sizeof(T), normals.size(), f) != normals.size()) {
        std::fprintf(stderr, "cannot read %ld normals from %s\n", (long)n, path);
        return 2;
    }
    std::fclose(f);
    const T eps = (T)epsilon;
    std::srand(srand_seed);
    std::vector<int32_t> col((size_t)n);
    for (int64_t i = 0; i < n; ++i) col[(size_t)i] = (int32_t)i;
    double t_shuffle = 0, t_pick = 0, t_replay = 0;
    const auto t_all = std::chrono::steady_clock::now();
    if (nb_sample < n) {
        double cols = 0, rows = 0;
        size_t nb_bucket = 0;
        pmx::nss_bucket_counts<T>(eps, cols, rows, nb_bucket);
        std::vector<uint32_t> key((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const T* p = &normals[(size_t)i * 3];
            const size_t b = pmx::nss_normal_defined<T>(p[0], p[1], p[2]) ? pmx::nss_bucket_of<T>(p[0], p[1], p[2], eps)
                                                                          : nb_bucket;
            if (b >= nb_bucket) {
                std::printf("undefined %ld\n", (long)i);
                return 3;
            }
            key[(size_t)i] = (uint32_t)b;
        }
        auto t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> ids((size_t)n);
        pmx::nss_shuffle(n, ids.data());
        t_shuffle = ms_since(t0);
        std::stable_sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
        std::vector<uint32_t> begin;
        for (int64_t j = 0; j < n; ++j)
            if (j == 0 || key[(size_t)ids[(size_t)j]] != key[(size_t)ids[(size_t)j - 1]]) begin.push_back((uint32_t)j);
        t0 = std::chrono::steady_clock::now();
        const std::vector<int32_t> picks = pmx::nss_picks(ids.data(), begin.data(), (int64_t)begin.size(), n, nb_sample,
                                                          seed);
        t_pick = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        col = pmx::octree_replay_columns(picks.data(), nb_sample, n);
        t_replay = ms_since(t0);
    }
    const double total = ms_since(t_all);
    if (timed) {
        std::printf("total_ms %.3f shuffle_ms %.3f pick_ms %.3f replay_ms %.3f\n", total, t_shuffle, t_pick, t_replay);
        return 0;
    }
    for (int32_t c : col) std::printf("%d ", c);
    std::printf("\n0\n%d\n", std::rand());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9 && (!std::strcmp(argv[1], "filter") || !std::strcmp(argv[1], "time"))) {
        const bool timed = argv[1][0] == 't';
        const int64_t n = std::atoll(argv[4]), nb = std::atoll(argv[5]);
        const uint64_t seed = std::strtoull(argv[6], nullptr, 10);
        const unsigned sr = (unsigned)std::strtoul(argv[7], nullptr, 10);
        const uint64_t bits = std::strtoull(argv[8], nullptr, 10);
        double eps;
        std::memcpy(&eps, &bits, sizeof(eps));
        return argv[2][0] == 'd' ? run<double>(timed, argv[3], n, nb, seed, sr, eps)
                                 : run<float>(timed, argv[3], n, nb, seed, sr, eps);
    }
    std::fprintf(stderr, "usage: normal_space_shared filter|time T file n nbSample seed srand epsbits\n");
    return 2;
}

// normal_space_main.cpp — a stand-alone, literal restatement of
// NormalSpaceDataPointsFilter (DataPointsFilters/NormalSpace.cpp:47-181) for
// tests/test_normal_space_reference.py, test_gpu_normal_space.py and
// test_normal_space_chain.py.  It shares no code with the library: buckets are
// a vector of vectors filled point by point in shuffled order with the host
// library's acos / atan2 / fmod, the picks come from std::mt19937 and
// std::uniform_int_distribution with the bucket erased once empty, and the
// columns move by swaps and an unordered_map lookup table.  The cloud is a row of
// column numbers, so what it prints is, per output column, the input column it
// holds.
//
//   normal_space mt
//       the 10 000th output of a default-seeded std::mt19937
//   normal_space keys <f|d> <file> <n> <epsilon bits>
//       the bucket index of every point, in point order
//   normal_space filter <f|d> <file> <n> <nbSample> <seed> <srand> <epsilon bits>
//       line 1: the kept columns; line 2: the stale table lookups; line 3: the
//       next rand() of the process.  "undefined <i>" and exit status 3 for a
//       normal with a NaN or |nz| > 1 or a bucket index >= bucket_count.
//   normal_space time <f|d> <file> <n> <nbSample> <seed> <srand> <epsilon bits>
//       as filter, printing the milliseconds of the whole and of its phases
// <file>: n x 3 values of T, point-major.  <epsilon bits>: the parameter as the
// 64 bits of a double, in decimal; it is cast to T as the reference's
// parameter is.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <unordered_map>
#include <utility>
#include <vector>

template <typename T>
struct Filter {
    std::size_t nbSample, seed;
    T epsilon;
    std::size_t bucket_count;
    Filter(std::size_t nb, std::size_t sd, T eps)
        : nbSample(nb), seed(sd), epsilon(eps),
          bucket_count(std::size_t(std::ceil(2.0 * M_PI / epsilon) * std::ceil(M_PI / epsilon))) {}

    std::size_t bucket_index(T theta, T phi) const {
        if (theta == static_cast<T>(M_PI)) theta = 0.0;
        if (phi == 2 * static_cast<T>(M_PI)) phi = 0.0;
        return static_cast<std::size_t>(std::floor(theta / epsilon) * std::ceil(2.0 * M_PI / epsilon) +
                                        std::floor(phi / epsilon));
    }
    // false for a normal or a bucket the reference leaves undefined
    bool bucket_of(const T* nrm, std::size_t& out) const {
        if (nrm[0] != nrm[0] || nrm[1] != nrm[1] || !(nrm[2] <= 1.0 && nrm[2] >= -1.0)) return false;
        const T theta = std::acos(nrm[2]);
        const T phi = std::fmod(std::atan2(nrm[1], nrm[0]) + 2. * M_PI, 2. * M_PI);
        out = bucket_index(theta, phi);
        return out < bucket_count;
    }
};

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <typename T>
static int run(const char* mode, const char* path, long n, std::size_t nbSample, std::size_t seed, unsigned srand_seed,
               double eps) {
    std::vector<T> normals((std::size_t)n * 3);
    std::FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(normals.data(), sizeof(T), normals.size(), f) != normals.size()) {
        std::fprintf(stderr, "cannot read %ld normals from %s\n", n, path);
        return 2;
    }
    std::fclose(f);
    const Filter<T> flt(nbSample, seed, (T)eps);
    if (!std::strcmp(mode, "keys")) {
        for (long i = 0; i < n; ++i) {
            std::size_t b = 0;
            if (!flt.bucket_of(&normals[(std::size_t)i * 3], b)) {
                std::printf("undefined %ld\n", i);
                return 3;
            }
            std::printf("%zu ", b);
        }
        std::printf("\n");
        return 0;
    }
    const bool timed = !std::strcmp(mode, "time");
    std::srand(srand_seed);
    std::vector<int> cloud((std::size_t)n);  // column j holds input column cloud[j]
    for (long i = 0; i < n; ++i) cloud[(std::size_t)i] = (int)i;
    long stale = 0;
    double t_shuffle = 0, t_fill = 0, t_pick = 0, t_swap = 0;
    const auto t_all = std::chrono::steady_clock::now();
    if (nbSample < std::size_t(n)) {
        std::mt19937 gen(seed);
        std::vector<std::vector<int> > buckets;
        buckets.resize(flt.bucket_count);
        std::vector<std::size_t> picks;
        picks.reserve(nbSample);

        auto t0 = std::chrono::steady_clock::now();
        std::vector<std::size_t> order((std::size_t)n);
        for (long i = 0; i < n; ++i) order[(std::size_t)i] = (std::size_t)i;
        // std::random_shuffle(first, last) of libstdc++ (removed in C++17)
        for (long i = 1; i < n; ++i) {
            const long j = std::rand() % (i + 1);
            if (i != j) std::swap(order[(std::size_t)i], order[(std::size_t)j]);
        }
        t_shuffle = ms_since(t0);

        t0 = std::chrono::steady_clock::now();
        for (auto p : order) {
            std::size_t b = 0;
            if (!flt.bucket_of(&normals[p * 3], b)) {
                // (the reference meets the points in shuffled order; name the first in point order)
                for (long i = 0; i < n; ++i)
                    if (!flt.bucket_of(&normals[(std::size_t)i * 3], b)) {
                        std::printf("undefined %ld\n", i);
                        return 3;
                    }
            }
            buckets[b].push_back((int)p);
        }
        std::vector<std::vector<int> > kept;
        for (auto& bucket : buckets)
            if (!bucket.empty()) kept.push_back(std::move(bucket));
        buckets.swap(kept);
        t_fill = ms_since(t0);

        t0 = std::chrono::steady_clock::now();
        for (std::size_t i = 0; i < nbSample; i++) {
            std::uniform_int_distribution<std::size_t> draw(0, buckets.size() - 1);
            const std::size_t which = draw(gen);
            std::vector<int>& members = buckets[which];
            const int last = members[members.size() - 1];
            members.pop_back();
            picks.push_back(static_cast<std::size_t>(last));
            if (members.empty()) buckets.erase(buckets.begin() + (std::ptrdiff_t)which);
        }
        t_pick = ms_since(t0);

        t0 = std::chrono::steady_clock::now();
        std::unordered_map<std::size_t, std::size_t> table;
        std::size_t idx = 0;
        for (std::size_t id : picks) {
            if (id < idx) {
                id = table[id];
                if ((std::size_t)cloud[id] != picks[idx]) ++stale;  // the table no longer knows where it went
            }
            std::swap(cloud[idx], cloud[id]);
            table[idx] = id;
            ++idx;
        }
        cloud.resize(nbSample);
        t_swap = ms_since(t0);
    }
    const double total = ms_since(t_all);
    if (timed) {
        std::printf("total_ms %.3f shuffle_ms %.3f fill_ms %.3f pick_ms %.3f swap_ms %.3f\n", total, t_shuffle, t_fill,
                    t_pick, t_swap);
        return 0;
    }
    for (int c : cloud) std::printf("%d ", c);
    std::printf("\n%ld\n%d\n", stale, std::rand());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "mt")) {
        std::mt19937 gen;
        gen.discard(9999);
        std::printf("%lu\n", (unsigned long)gen());
        return 0;
    }
    if (argc >= 6) {
        const bool keys = !std::strcmp(argv[1], "keys");
        const bool is_double = argv[2][0] == 'd';
        const long n = std::atol(argv[4]);
        const std::size_t nbSample = keys ? 1 : (std::size_t)std::strtoull(argv[5], nullptr, 10);
        const std::size_t seed = keys || argc < 9 ? 1 : (std::size_t)std::strtoull(argv[6], nullptr, 10);
        const unsigned sr = keys || argc < 9 ? 1u : (unsigned)std::strtoul(argv[7], nullptr, 10);
        const uint64_t bits = std::strtoull(argv[keys ? 5 : 8], nullptr, 10);
        double eps;
        std::memcpy(&eps, &bits, sizeof(eps));
        if ((keys && argc == 6) || (!keys && argc == 9))
            return is_double ? run<double>(argv[1], argv[3], n, nbSample, seed, sr, eps)
                             : run<float>(argv[1], argv[3], n, nbSample, seed, sr, eps);
    }
    std::fprintf(stderr, "usage: normal_space mt | keys T file n epsbits | filter|time T file n nbSample seed srand "
                         "epsbits\n");
    return 2;
}

// keep_rand_main.cpp — a stand-alone restatement of the two rand()-driven keep
// filters on a handful of points, for tests/test_keep_filters_chain.py: it
// runs the same libc srand / rand sequence as the numpy references of
// tests/keep_cases.py and prints what the loops leave, so the aliasing of
// MaxPointCount's "switch" and MaxDensity's integer division are pinned by
// plain C++ semantics and not by the library under test.
//
//   keep_rand maxpointcount <n> <maxCount> <seed>
//       column i holds the value i; prints the values of the kept columns, or
//       "unchanged" (MaxPointCount.cpp:67-102)
//   keep_rand maxdensity <seed> <maxDensity> <d0> <d1> ...
//       prints one 0 / 1 per point (MaxDensity.cpp:59-105), T = float
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// A column of a column-major matrix the way an Eigen block expression is one:
// copying the object copies the reference to the storage, assigning to it
// copies the coefficients.
struct ColView {
    float* p;
    int rows;
    ColView(float* p_, int rows_) : p(p_), rows(rows_) {}
    ColView(const ColView&) = default;
    const ColView& operator=(const ColView& o) const {
        for (int r = 0; r < rows; ++r) p[r] = o.p[r];
        return *this;
    }
};
struct Matrix {
    int rows, cols;
    std::vector<float> a;
    Matrix(int r, int c) : rows(r), cols(c), a((size_t)r * c) {}
    ColView col(size_t j) { return ColView(&a[j * rows], rows); }
};

static int max_point_count(int n, size_t maxCount, size_t seed) {
    Matrix features(2, n);
    for (int i = 0; i < n; ++i) features.a[(size_t)i * 2] = features.a[(size_t)i * 2 + 1] = (float)i;
    const size_t last = (size_t)(features.cols - 1);
    if (maxCount <= last) {
        std::srand((unsigned)seed);
        for (size_t j = 0; j < maxCount; ++j) {
            const float u = (float)(std::rand() / (float)RAND_MAX);
            const size_t pick = j + (size_t)((last - j) * u);  // size_t * float: a float product
            const auto held = features.col(j);  // a view of column j, not a copy of it
            features.col(j) = features.col(pick);
            features.col(pick) = held;
        }
        for (size_t j = 0; j < maxCount; ++j) std::printf("%d ", (int)features.a[j * 2]);
        std::printf("\n");
    } else {
        std::printf("unchanged\n");
    }
    return 0;
}

static int max_density(unsigned seed, float maxDensity, const std::vector<float>& densities) {
    std::srand(seed);
    const int total = (int)densities.size();
    float top = densities[0];
    for (float d : densities) top = d > top ? d : top;
    int saturated = 0;
    for (float d : densities) saturated += d == top ? 1 : 0;
    for (int i = 0; i < total; ++i) {
        const float d = densities[i];
        int kept = 1;
        if (d > maxDensity) {
            const float u = (float)std::rand() / (float)RAND_MAX;
            float accept = maxDensity / d;
            if (d == top) accept = accept * (1 - saturated / total);  // int / int
            kept = u < accept ? 1 : 0;
        }
        std::printf("%d ", kept);
    }
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 5 && !std::strcmp(argv[1], "maxpointcount"))
        return max_point_count(std::atoi(argv[2]), (size_t)std::atoll(argv[3]), (size_t)std::atoll(argv[4]));
    if (argc >= 5 && !std::strcmp(argv[1], "maxdensity")) {
        std::vector<float> d;
        for (int i = 4; i < argc; ++i) d.push_back(std::strtof(argv[i], nullptr));
        return max_density((unsigned)std::atoi(argv[2]), std::strtof(argv[3], nullptr), d);
    }
    std::fprintf(stderr, "usage: keep_rand maxpointcount n maxCount seed | maxdensity seed maxDensity d...\n");
    return 2;
}

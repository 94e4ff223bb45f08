// covariance_sampling_shared_main.cpp — the host side the library compiles in
// (csrc/common/pmx_covs.h, pmx_octree_replay.h) as a stand-alone program, for
// tests/test_covariance_sampling_reference.py: the same input file and the same
// first two output lines as tests/covariance_sampling_main.cpp.  Where the
// library sorts on the device, this program sorts index arrays on the host by
// falling |m_k| with ties by rising index, and hands covs_picks only the first
// min(n, nbSample) entries of each, as the library does.
//
//   covariance_sampling_shared filter <f|d> <file> <n> <nbSample>
//       line 1: the kept columns; line 2: the deepest 1-based list position read
//   covariance_sampling_shared eigen <file of 36 doubles>
//       covs_sym_eigen of that covariance in double: line 1 the eigenvalues,
//       line 2 the basis (row-major, column k the vector of eigenvalue k)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common/pmx_covs.h"
#include "common/pmx_octree_replay.h"

template <typename T>
static int run(const char* path, long n, int64_t nb_sample) {
    std::vector<T> data((std::size_t)n * 6 + 40);
    std::FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(data.data(), sizeof(T), data.size(), f) != data.size()) {
        std::fprintf(stderr, "cannot read %ld points, normals and 40 values from %s\n", n, path);
        return 2;
    }
    std::fclose(f);
    const T* pts = data.data();
    const T* nrm = pts + (std::size_t)n * 3;
    const T* c = nrm + (std::size_t)n * 3;
    const T inv = (T)(1.0 / (double)c[3]);
    const T* X = c + 4;
    std::vector<int32_t> col((std::size_t)n);
    for (long i = 0; i < n; ++i) col[(std::size_t)i] = (int32_t)i;
    int64_t depth = 0;
    if (nb_sample < n) {
        auto proj = [&](int64_t i, T (&m)[6]) {
            T v[6];
            pmx::covs_v<T>(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2], c[0],
                           c[1], c[2], inv, v);
            for (int k = 0; k < 6; ++k) m[k] = pmx::covs_dot<T>(v, X, k);
        };
        std::vector<T> mag((std::size_t)n * 6);
        for (long i = 0; i < n; ++i) {
            T m[6];
            proj(i, m);
            for (int k = 0; k < 6; ++k) mag[(std::size_t)k * n + i] = std::fabs(m[k]);
        }
        const int64_t H = std::min<int64_t>(n, nb_sample);
        std::vector<int32_t> heads((std::size_t)(6 * H)), order((std::size_t)n);
        for (int k = 0; k < 6; ++k) {
            for (long i = 0; i < n; ++i) order[(std::size_t)i] = (int32_t)i;
            const T* mk = &mag[(std::size_t)k * n];
            std::stable_sort(order.begin(), order.end(), [mk](int32_t a, int32_t b) { return mk[a] > mk[b]; });
            std::copy(order.begin(), order.begin() + H, heads.begin() + k * H);
        }
        std::vector<int32_t> picks;
        if (!pmx::covs_picks<T>(heads.data(), H, n, nb_sample, proj, picks, &depth)) {
            std::fprintf(stderr, "a list ran out before nbSample picks\n");
            return 4;
        }
        col = pmx::octree_replay_columns(picks.data(), nb_sample, n);
    }
    for (int32_t x : col) std::printf("%d ", x);
    std::printf("\n%lld\n", (long long)depth);
    return 0;
}

// the library's basis of a covariance, before any rounding to T: 6 eigenvalues,
// then the 36 entries of the basis (row-major, column k the vector), %.17g
static int eigen(const char* path) {
    double cov[36], w[6], V[36];
    std::FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(cov, sizeof(double), 36, f) != 36) {
        std::fprintf(stderr, "cannot read 36 doubles from %s\n", path);
        return 2;
    }
    std::fclose(f);
    pmx::covs_sym_eigen(cov, w, V);
    for (double x : w) std::printf("%.17g ", x);
    std::printf("\n");
    for (double x : V) std::printf("%.17g ", x);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "eigen")) return eigen(argv[2]);
    if (argc == 6 && !std::strcmp(argv[1], "filter")) {
        const long n = std::atol(argv[4]);
        const int64_t nb = (int64_t)std::strtoll(argv[5], nullptr, 10);
        return argv[2][0] == 'd' ? run<double>(argv[3], n, nb) : run<float>(argv[3], n, nb);
    }
    std::fprintf(stderr, "usage: covariance_sampling_shared filter T file n nbSample | eigen file\n");
    return 2;
}

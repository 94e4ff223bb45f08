// covariance_sampling_main.cpp — a stand-alone, literal restatement of
// CovarianceSamplingDataPointsFilter's selection
// (DataPointsFilters/CovarianceSampling.cpp:136-249) for
// tests/test_covariance_sampling_reference.py and
// test_gpu_covariance_sampling.py, without Eigen.  It shares no code with the
// library: v is a vector of 6-vectors, the six lists are
// std::list<std::pair<int, T>> sorted by list::sort with the reference's
// comparator, the picks pop fronts guarded by the sampledPoints flags, and the
// columns move by swaps and an unordered_map lookup table.  The cloud is a row
// of column numbers, so what it prints is, per output column, the input column
// it holds.  The centre, L and the basis are inputs: those three are what the
// library defines and the reference leaves to Eigen and to its summation order.
//
//   covariance_sampling filter <f|d> <file> <n> <nbSample>
//       line 1: the kept columns; line 2: the deepest 1-based list position
//       read; line 3: the stale table lookups
//   covariance_sampling time <f|d> <file> <n> <nbSample>
//       as filter, printing the milliseconds of the whole and of its phases
// <file>: values of T — n x 3 points, n x 3 normals (both point-major), the
// centre (3), L (1), the basis (36, row-major 6 x 6, column k the vector X_k).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <unordered_map>
#include <utility>
#include <vector>

template <typename T>
struct Vector6 {
    T a[6];
    T dot(const T* basis, std::size_t k) const {  // sequential, as the library defines the projection
        T s = a[0] * basis[k];
        for (std::size_t r = 1; r < 6; ++r) s = s + a[r] * basis[r * 6 + k];
        return s;
    }
};

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <typename T>
static int run(bool timed, const char* path, long n, std::size_t nbSample) {
    const std::size_t nbPoints = (std::size_t)n;
    std::vector<T> data(nbPoints * 6 + 40);
    std::FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(data.data(), sizeof(T), data.size(), f) != data.size()) {
        std::fprintf(stderr, "cannot read %ld points, normals and 40 values from %s\n", n, path);
        return 2;
    }
    std::fclose(f);
    const T* features = data.data();
    const T* normals = features + nbPoints * 3;
    const T* center = normals + nbPoints * 3;
    const T Lnorm = center[3];
    const T* eigenVe = center + 4;

    std::vector<int> cloud(nbPoints);  // column j holds input column cloud[j]
    for (std::size_t i = 0; i < nbPoints; ++i) cloud[i] = (int)i;
    long stale = 0;
    std::size_t depth = 0;
    double t_v = 0, t_sort = 0, t_pick = 0, t_swap = 0;
    const auto t_all = std::chrono::steady_clock::now();
    if (nbSample < nbPoints) {
        std::vector<std::size_t> keepIndexes;
        keepIndexes.resize(nbSample);

        // B.1 - the v-6 of each candidate
        auto t0 = std::chrono::steady_clock::now();
        std::vector<Vector6<T> > v;
        v.resize(nbPoints);
        const T invL = (T)(1. / Lnorm);
        for (std::size_t i = 0; i < nbPoints; ++i) {
            const T p[3] = {features[i * 3] - center[0], features[i * 3 + 1] - center[1],
                            features[i * 3 + 2] - center[2]};
            const T* ni = normals + i * 3;
            v[i].a[0] = invL * (p[1] * ni[2] - p[2] * ni[1]);
            v[i].a[1] = invL * (p[2] * ni[0] - p[0] * ni[2]);
            v[i].a[2] = invL * (p[0] * ni[1] - p[1] * ni[0]);
            v[i].a[3] = ni[0];
            v[i].a[4] = ni[1];
            v[i].a[5] = ni[2];
        }
        t_v = ms_since(t0);

        // B.2 - the 6 sorted lists
        t0 = std::chrono::steady_clock::now();
        std::vector<std::list<std::pair<int, T> > > L;
        L.resize(6);
        auto comp = [](const std::pair<int, T>& p1, const std::pair<int, T>& p2) -> bool {
            return p1.second > p2.second;
        };
        for (std::size_t k = 0; k < 6; ++k) {
            for (std::size_t i = 0; i < nbPoints; ++i)
                L[k].push_back(std::make_pair((int)i, std::fabs(v[i].dot(eigenVe, k))));
            L[k].sort(comp);
        }
        t_sort = ms_since(t0);

        t0 = std::chrono::steady_clock::now();
        std::vector<T> t(6, T(0.));
        std::vector<bool> sampledPoints(nbPoints, false);
        std::size_t popped[6] = {0, 0, 0, 0, 0, 0};
        for (std::size_t i = 0; i < nbSample; ++i) {
            // B.3 - the least constrained vector
            std::size_t k = 0;
            for (std::size_t j = 0; j < 6; ++j) {
                if (t[k] > t[j]) k = j;
            }
            while (sampledPoints[L[k].front().first]) {
                L[k].pop_front();
                ++popped[k];
            }
            const std::size_t idToKeep = static_cast<std::size_t>(L[k].front().first);
            L[k].pop_front();
            ++popped[k];
            if (popped[k] > depth) depth = popped[k];
            sampledPoints[idToKeep] = true;
            // B.4 - the running totals
            for (std::size_t j = 0; j < 6; ++j) {
                const T magnitude = v[idToKeep].dot(eigenVe, j);
                t[j] += (magnitude * magnitude);
            }
            keepIndexes[i] = idToKeep;
        }
        t_pick = ms_since(t0);

        // (4) the columns
        t0 = std::chrono::steady_clock::now();
        std::unordered_map<std::size_t, std::size_t> mapidx;
        std::size_t idx = 0;
        for (std::size_t id : keepIndexes) {
            if (id < idx) {
                id = mapidx[id];
                if ((std::size_t)cloud[id] != keepIndexes[idx]) ++stale;  // the table no longer knows where it went
            }
            std::swap(cloud[idx], cloud[id]);
            mapidx[idx] = id;
            ++idx;
        }
        cloud.resize(nbSample);
        t_swap = ms_since(t0);
    }
    const double total = ms_since(t_all);
    if (timed) {
        std::printf("total_ms %.3f v_ms %.3f sort_ms %.3f pick_ms %.3f swap_ms %.3f\n", total, t_v, t_sort, t_pick,
                    t_swap);
        return 0;
    }
    for (int c : cloud) std::printf("%d ", c);
    std::printf("\n%zu\n%ld\n", depth, stale);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && (!std::strcmp(argv[1], "filter") || !std::strcmp(argv[1], "time"))) {
        const bool timed = !std::strcmp(argv[1], "time");
        const long n = std::atol(argv[4]);
        const std::size_t nbSample = (std::size_t)std::strtoull(argv[5], nullptr, 10);
        return argv[2][0] == 'd' ? run<double>(timed, argv[3], n, nbSample) : run<float>(timed, argv[3], n, nbSample);
    }
    std::fprintf(stderr, "usage: covariance_sampling filter|time T file n nbSample\n");
    return 2;
}

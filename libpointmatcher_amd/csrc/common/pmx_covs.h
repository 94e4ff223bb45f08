// pmx_covs.h — what the host and the device share of
// CovarianceSamplingDataPointsFilter (DataPointsFilters/CovarianceSampling.cpp:
// 74-250; Gelfand et al. 2003, stability sampling): plain C++, no kernels, so a
// stand-alone program can include it.
//   covs_v          v_i = [inv * ((p - c) x n) ; n] of one point (:142-148, :169-173)
//   covs_dot        the projection of v_i on one basis column (:189, :224)
//   covs_dist       a point's distance from the centre, the term of Lavg (:123)
//   covs_sym_eigen  the basis the library defines: cyclic Jacobi on the
//                   symmetric 6 x 6 covariance in double (the rotation of
//                   sym_eigen in pmx_normals.hip), ascending, signed
//   covs_picks      the pick loop over the six sorted lists (:195-229)
// Every expression is +, -, x in T with each operation rounded on its own
// (the including file sets fp contract off), so the host and the device
// evaluate it to the same bits.  The column order of the output is the
// swapCols / mapidx sequence of OctreeGrid (:233-249): octree_replay_columns of
// pmx_octree_replay.h.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PMX_COVS_HD __host__ __device__
#else
#define PMX_COVS_HD
#endif

namespace pmx {

// v = [inv * ((p - c) x n) ; n]: each difference, each cross-product component
// a * b - c * d and each product by inv rounded in T
template <typename T>
PMX_COVS_HD inline void covs_v(T px, T py, T pz, T nx, T ny, T nz, T cx, T cy, T cz, T inv, T (&v)[6]) {
    const T dx = px - cx, dy = py - cy, dz = pz - cz;
    v[0] = inv * (dy * nz - dz * ny);
    v[1] = inv * (dz * nx - dx * nz);
    v[2] = inv * (dx * ny - dy * nx);
    v[3] = nx;
    v[4] = ny;
    v[5] = nz;
}

// m_k = ((((v0 x0 + v1 x1) + v2 x2) + v3 x3) + v4 x4) + v5 x5, X row-major 6 x 6
// with column k the basis vector X_k
template <typename T>
PMX_COVS_HD inline T covs_dot(const T (&v)[6], const T* X, int k) {
    return ((((v[0] * X[k] + v[1] * X[6 + k]) + v[2] * X[12 + k]) + v[3] * X[18 + k]) + v[4] * X[24 + k]) +
           v[5] * X[30 + k];
}

// the distance of a point from the centre (Lavg, :123): sqrt((dx dx + dy dy) + dz dz) in T
template <typename T>
PMX_COVS_HD inline T covs_dist(T px, T py, T pz, T cx, T cy, T cz) {
    const T dx = px - cx, dy = py - cy, dz = pz - cz;
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

template <typename T>
PMX_COVS_HD inline bool covs_finite(T x) {
    return x - x == (T)0;  // (false for an infinity and for a NaN)
}

// cyclic Jacobi eigen-decomposition of a symmetric 6 x 6 matrix in double, the
// rotation, the stopping rule, the ascending order and the sign convention of
// sym_eigen (pmx_normals.hip): w ascending, V row-major with column k the
// vector of w[k], its largest-magnitude component positive (the first on ties)
inline void covs_sym_eigen(const double* cov, double* w, double* V) {
    constexpr int D = 6;
    double a[D][D];
    double fro = 0.0;
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            a[r][c] = cov[r * D + c];
            fro += a[r][c] * a[r][c];
            V[r * D + c] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 50; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < D; ++p)
            for (int q = p + 1; q < D; ++q) off += a[p][q] * a[p][q];
        if (!(off > 1e-36 * fro)) break;
        for (int p = 0; p < D; ++p)
            for (int q = p + 1; q < D; ++q) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < D; ++r) {
                    const double arp = a[r][p], arq = a[r][q];
                    a[r][p] = c * arp - s * arq;
                    a[r][q] = s * arp + c * arq;
                }
                for (int r = 0; r < D; ++r) {
                    const double apr = a[p][r], aqr = a[q][r];
                    a[p][r] = c * apr - s * aqr;
                    a[q][r] = s * apr + c * aqr;
                }
                for (int r = 0; r < D; ++r) {
                    const double vrp = V[r * D + p], vrq = V[r * D + q];
                    V[r * D + p] = c * vrp - s * vrq;
                    V[r * D + q] = s * vrp + c * vrq;
                }
            }
    }
    for (int i = 0; i < D; ++i) w[i] = a[i][i];
    for (int i = 0; i < D; ++i)
        for (int j = i + 1; j < D; ++j)
            if (w[j] < w[i]) {
                const double wi = w[i];
                w[i] = w[j];
                w[j] = wi;
                for (int r = 0; r < D; ++r) {
                    const double vi = V[r * D + i];
                    V[r * D + i] = V[r * D + j];
                    V[r * D + j] = vi;
                }
            }
    for (int j = 0; j < D; ++j) {
        double big = V[j];
        for (int r = 1; r < D; ++r)
            if (std::fabs(V[r * D + j]) > std::fabs(big)) big = V[r * D + j];
        if (big < 0.0)
            for (int r = 0; r < D; ++r) V[r * D + j] = -V[r * D + j];
    }
}

// The pick loop (CovarianceSampling.cpp:195-229).  heads: six arrays of H
// point indices each (list k at heads + k * H), list k by falling |m_k| with
// ties by rising index — the first H entries of the reference's sorted
// std::list.  proj(i, m) gives the six signed projections of point i in T.
// t[6] is held in T; k is the first index of the smallest t; fronts already
// sampled are skipped; the front is picked; t[j] += m_j * m_j.  Every entry
// read from a list is a distinct point that ends up sampled, so no list is
// read past position nb_sample: H = min(n, nb_sample) is enough.  *depth: the
// deepest 1-based list position read.  False (picks incomplete) if a list
// would be read past H, which that argument excludes.
template <typename T, typename Proj>
inline bool covs_picks(const int32_t* heads, int64_t H, int64_t n, int64_t nb_sample, Proj proj,
                       std::vector<int32_t>& picks, int64_t* depth) {
    T t[6] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    int64_t pos[6] = {0, 0, 0, 0, 0, 0};
    std::vector<bool> sampled((std::size_t)n, false);
    picks.clear();
    picks.reserve((std::size_t)nb_sample);
    *depth = 0;
    for (int64_t i = 0; i < nb_sample; ++i) {
        int k = 0;
        for (int j = 0; j < 6; ++j)
            if (t[k] > t[j]) k = j;
        const int32_t* list = heads + (int64_t)k * H;
        while (pos[k] < H && sampled[(std::size_t)list[pos[k]]]) ++pos[k];
        if (pos[k] >= H) return false;
        const int32_t id = list[pos[k]++];
        if (pos[k] > *depth) *depth = pos[k];
        sampled[(std::size_t)id] = true;
        T m[6];
        proj((int64_t)id, m);
        for (int j = 0; j < 6; ++j) t[j] = t[j] + m[j] * m[j];
        picks.push_back(id);
    }
    return true;
}

}  // namespace pmx

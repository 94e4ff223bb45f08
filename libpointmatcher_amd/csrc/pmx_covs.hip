// pmx_covs.hip — CovarianceSamplingDataPointsFilter on the device
// (DataPointsFilters/CovarianceSampling.cpp:74-250; Gelfand et al. 2003,
// stability sampling).
//
// The reference builds v_i = [(1 / L) (p_i - c) x n_i ; n_i] for every point,
// the 6 x 6 covariance of the v_i and its eigenvectors X_k, sorts the points
// six times by falling |v_i . X_k|, and nbSample times takes the first point
// not yet sampled of the list whose running sum of squared projections is the
// smallest; the picks are then moved to the front by the swapCols / mapidx
// sequence of OctreeGrid.  Here:
//   covs_moment_kernel  a fixed grid: pass 0 the three coordinate sums in fp64,
//                       the count of non-finite points and the extents' min /
//                       max; pass 1 (torqueNorm 1) the sum of the T distances
//                       from the centre.  Per-block partials, summed by the
//                       host in block order.
//   covs_cov_kernel     a fixed grid: v_i once per point, the 21 upper-triangle
//                       products in T accumulated in fp64, per-block partials
//   the basis           on the host: Jacobi in double (common/pmx_covs.h),
//                       rounded to T; or the caller's
//   covs_key_kernel     one point per lane: v_i again, six projections in
//                       registers, six key arrays (the inverted bits of |m|)
//   pmx_sort_pairs      six stable sorts of (key, index); the first nbSample
//                       indices of each list go to the host
//   the picks           on the host (covs_picks, sequential by nature), then the
//                       replay on column numbers
//   gather_columns_kernel   whole feature and descriptor columns
// No atomics; deterministic.  The per-point expressions are those of
// common/pmx_covs.h on both sides: +, -, x and sqrt in T, each rounded on its
// own, so the device's keys order the points as the host's values would.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "common/pmx_covs.h"
#include "common/pmx_octree_replay.h"
#include "pmx_columns.h"
#include "pmx_internal.h"
#include "pmx_p2plane.h"
#include "pmx_sort.h"

#include "../../include/pmx.h"

namespace pmx {

constexpr int kCovsBlocks = kRedBlocks;  // the fixed reduction grid (deterministic sums)
constexpr int kCovsMomentNV = 4;         // sum x, sum y, sum z | sum dist; non-finite points
constexpr int kCovsCovNV = 21;           // the upper triangle, row by row

template <typename T>
__device__ __forceinline__ T covs_wave_min(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T covs_wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// Fixed grid of kCovsBlocks x 256, point i on thread i mod (grid x 256).
// f: the features (4 x n point-major), d: the descriptors with the normal at
// rows nrow .. nrow + 2.  pass 0: partials = {sum x, sum y, sum z, non-finite
// points} per block (value-major, block_store), minmax[block * 6 ..] = min x, y,
// z, max x, y, z of the block's points (+inf / -inf for a block without any).
// pass 1: partials[0] = the sum of covs_dist from (cx, cy, cz).
template <typename T>
__global__ __launch_bounds__(256) void covs_moment_kernel(const P4<T>* __restrict__ f, const T* __restrict__ d,
                                                          int desc_dim, int nrow, int64_t n, int pass, T cx, T cy,
                                                          T cz, double* __restrict__ partials,
                                                          T* __restrict__ minmax) {
    double acc[kCovsMomentNV] = {0.0, 0.0, 0.0, 0.0};
    const T inf = std::numeric_limits<T>::infinity();
    T lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const P4<T> p = f[i];
        if (pass == 0) {
            const T* q = d + i * desc_dim + nrow;
            acc[0] += (double)p.x;
            acc[1] += (double)p.y;
            acc[2] += (double)p.z;
            const bool ok = covs_finite(p.x) && covs_finite(p.y) && covs_finite(p.z) && covs_finite(q[0]) &&
                            covs_finite(q[1]) && covs_finite(q[2]);
            if (!ok) acc[3] += 1.0;
            lo[0] = p.x < lo[0] ? p.x : lo[0];
            lo[1] = p.y < lo[1] ? p.y : lo[1];
            lo[2] = p.z < lo[2] ? p.z : lo[2];
            hi[0] = p.x > hi[0] ? p.x : hi[0];
            hi[1] = p.y > hi[1] ? p.y : hi[1];
            hi[2] = p.z > hi[2] ? p.z : hi[2];
        } else {
            acc[0] += (double)covs_dist<T>(p.x, p.y, p.z, cx, cy, cz);
        }
    }
    block_store<kCovsMomentNV>(acc, partials);
    if (pass != 0) return;
    __shared__ T mm[4][6];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const T l = covs_wave_min(lo[a]), h = covs_wave_max(hi[a]);
        if ((threadIdx.x & 63) == 0) {
            mm[wave][a] = l;
            mm[wave][3 + a] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        T r = mm[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) {
            const T o = mm[w][threadIdx.x];
            r = threadIdx.x < 3 ? (o < r ? o : r) : (o > r ? o : r);
        }
        minmax[(int64_t)blockIdx.x * 6 + threadIdx.x] = r;
    }
}

// Fixed grid as above: v_i once per point, the 21 products v_r * v_c (r <= c)
// in T, each accumulated in fp64; per-block partials (value-major).
template <typename T>
__global__ __launch_bounds__(256) void covs_cov_kernel(const P4<T>* __restrict__ f, const T* __restrict__ d,
                                                       int desc_dim, int nrow, int64_t n, T cx, T cy, T cz, T inv,
                                                       double* __restrict__ partials) {
    double acc[kCovsCovNV];
#pragma unroll
    for (int a = 0; a < kCovsCovNV; ++a) acc[a] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const P4<T> p = f[i];
        const T* q = d + i * desc_dim + nrow;
        T v[6];
        covs_v<T>(p.x, p.y, p.z, q[0], q[1], q[2], cx, cy, cz, inv, v);
        int a = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) acc[a++] += (double)(v[r] * v[c]);
    }
    block_store<kCovsCovNV>(acc, partials);
}

// the basis X (36 values of T, row-major, column k the vector X_k), by value
template <typename T>
struct CovsBasis {
    T x[36];
};

template <typename T>
struct CovsKey;
template <>
struct CovsKey<float> {
    typedef uint32_t type;
    static __device__ __forceinline__ uint32_t of(float m) { return ~__float_as_uint(fabsf(m)); }
};
template <>
struct CovsKey<double> {
    typedef uint64_t type;
    static __device__ __forceinline__ uint64_t of(double m) { return ~(uint64_t)__double_as_longlong(fabs(m)); }
};

// One point per lane: key[k * n + i] = the inverted bit pattern of |m_k(i)|, so
// that a rising stable sort lists the points by falling magnitude with ties by
// rising index (the bit patterns of non-negative values order as the values).
template <typename T>
__global__ __launch_bounds__(256) void covs_key_kernel(const P4<T>* __restrict__ f, const T* __restrict__ d,
                                                       int desc_dim, int nrow, int64_t n, T cx, T cy, T cz, T inv,
                                                       CovsBasis<T> X, typename CovsKey<T>::type* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const P4<T> p = f[i];
    const T* q = d + i * desc_dim + nrow;
    T v[6];
    covs_v<T>(p.x, p.y, p.z, q[0], q[1], q[2], cx, cy, cz, inv, v);
#pragma unroll
    for (int k = 0; k < 6; ++k) key[(int64_t)k * n + i] = CovsKey<T>::of(covs_dot<T>(v, X.x, k));
}

// the host's sum of one value's per-block partials, in block order
static double covs_block_sum(const double* partials, int v) {
    double s = 0.0;
    for (int b = 0; b < kCovsBlocks; ++b) s += partials[(size_t)v * kCovsBlocks + b];
    return s;
}

// h_f / h_desc: the host's copy of the cloud (the picked points' projections
// and the first non-finite point are taken from it); d_f / d_desc: the cloud on
// the device, 4 x n and desc_dim x n point-major.  Outputs (device, capacity
// nb_sample): d_of, d_od.  The caller has taken the reference's early exits and
// checked 1 <= nb_sample < n < 2^31, torque_norm in 0..2, nrow + 3 <= desc_dim
// and a finite basis.
template <typename T>
int covs_run(const T* h_f, const T* h_desc, const T* d_f, int64_t n, const T* d_desc, int desc_dim, int nrow,
             int64_t nb_sample, int torque_norm, const double* basis, T* d_of, T* d_od, int64_t* n_out,
             pmx_covs_report& rep, hipStream_t st, std::string& err) {
    typedef typename CovsKey<T>::type K;
    *n_out = 0;
    rep = pmx_covs_report{};
    const int64_t H = nb_sample;  // (< n) the head of each list the picks can reach

    size_t tsort = 0;
    {
        K* k0 = nullptr;
        uint32_t* v0 = nullptr;
        (void)pmx_sort_pairs(nullptr, tsort, k0, k0, v0, v0, (int)n, 0, (int)(8 * sizeof(K)), st);
    }
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_part = take(sizeof(double) * kCovsCovNV * kCovsBlocks), o_mm = take(sizeof(T) * 6 * kCovsBlocks),
                 o_key = take(sizeof(K) * 6 * (size_t)n), o_skey = take(sizeof(K) * (size_t)n),
                 o_iota = take(sizeof(uint32_t) * (size_t)n), o_order = take(sizeof(uint32_t) * (size_t)n),
                 o_heads = take(sizeof(int32_t) * 6 * (size_t)H), o_temp = take(tsort);
    char* buf = nullptr;
    if (hipMalloc(&buf, total) != hipSuccess) {
        err = "CovarianceSamplingDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    double* part = (double*)(buf + o_part);
    T* mm = (T*)(buf + o_mm);
    K* key = (K*)(buf + o_key);
    K* skey = (K*)(buf + o_skey);
    uint32_t* iota = (uint32_t*)(buf + o_iota);
    uint32_t* order = (uint32_t*)(buf + o_order);
    int32_t* heads = (int32_t*)(buf + o_heads);
    void* temp = buf + o_temp;
    const P4<T>* pf = (const P4<T>*)d_f;
    const dim3 fixed(kCovsBlocks), grid(column_blocks(n)), block(256);
    std::vector<double> hp((size_t)kCovsCovNV * kCovsBlocks);
    auto read_partials = [&](int nv) {
        return hipGetLastError() == hipSuccess &&
               hipMemcpyAsync(hp.data(), part, sizeof(double) * (size_t)nv * kCovsBlocks, hipMemcpyDeviceToHost,
                              st) == hipSuccess &&
               hipStreamSynchronize(st) == hipSuccess;
    };

    // ---- 1. the centre (:103-110), the extents, the non-finite points ----
    hipLaunchKernelGGL(covs_moment_kernel<T>, fixed, block, 0, st, pf, d_desc, desc_dim, nrow, n, 0, (T)0, (T)0, (T)0,
                       part, mm);
    if (!read_partials(kCovsMomentNV)) return PMX_E_HIP;
    if (covs_block_sum(hp.data(), 3) != 0.0) {
        for (int64_t i = 0; i < n; ++i) {
            const T* p = h_f + i * 4;
            const T* q = h_desc + i * desc_dim + nrow;
            if (!(covs_finite(p[0]) && covs_finite(p[1]) && covs_finite(p[2]) && covs_finite(q[0]) &&
                  covs_finite(q[1]) && covs_finite(q[2]))) {
                err = "CovarianceSamplingDataPointsFilter: point " + std::to_string(i) +
                      " has a non-finite coordinate or normal";
                return PMX_E_BAD_PARAM;
            }
        }
        err = "CovarianceSamplingDataPointsFilter: inconsistent non-finite count";
        return PMX_E_STATE;
    }
    T c[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = (T)(covs_block_sum(hp.data(), a) / (double)n);
        rep.center[a] = (double)c[a];
    }

    // ---- 2. L (:113-133) ----
    T L = (T)1;
    if (torque_norm == 1) {
        hipLaunchKernelGGL(covs_moment_kernel<T>, fixed, block, 0, st, pf, d_desc, desc_dim, nrow, n, 1, c[0], c[1],
                           c[2], part, mm);
        if (!read_partials(1)) return PMX_E_HIP;
        L = (T)(covs_block_sum(hp.data(), 0) / (double)n);
    } else if (torque_norm == 2) {
        std::vector<T> hm((size_t)6 * kCovsBlocks);
        if (hipMemcpyAsync(hm.data(), mm, sizeof(T) * hm.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PMX_E_HIP;
        T ext = (T)0;
        for (int a = 0; a < 3; ++a) {
            T lo = hm[(size_t)a], hi = hm[(size_t)3 + a];
            for (int b = 1; b < kCovsBlocks; ++b) {
                lo = std::min(lo, hm[(size_t)b * 6 + a]);
                hi = std::max(hi, hm[(size_t)b * 6 + 3 + a]);
            }
            const T e = hi - lo;
            if (a == 0 || e > ext) ext = e;
        }
        L = ext / (T)2;
    }
    if (torque_norm != 0 && !(L > (T)0)) {
        err = "CovarianceSamplingDataPointsFilter: torqueNorm " + std::to_string(torque_norm) +
              " gives L = 0 (every point at the centroid)";
        return PMX_E_BAD_PARAM;
    }
    rep.lnorm = (double)L;
    const T inv = (T)(1.0 / (double)L);

    // ---- 3. the covariance (:136-156) ----
    hipLaunchKernelGGL(covs_cov_kernel<T>, fixed, block, 0, st, pf, d_desc, desc_dim, nrow, n, c[0], c[1], c[2], inv,
                       part);
    if (!read_partials(kCovsCovNV)) return PMX_E_HIP;
    {
        int a = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) {
                const double s = covs_block_sum(hp.data(), a++);
                rep.cov[r * 6 + cc] = s;
                rep.cov[cc * 6 + r] = s;
            }
    }

    // ---- 4. the basis ----
    double Xd[36];
    covs_sym_eigen(rep.cov, rep.eigval, Xd);
    if (basis) std::copy(basis, basis + 36, Xd);
    CovsBasis<T> X;
    for (int a = 0; a < 36; ++a) {
        X.x[a] = (T)Xd[a];
        rep.eigvec[a] = (double)X.x[a];
    }

    // ---- 5. six lists by falling |m_k|, ties by rising index (:177-193) ----
    hipLaunchKernelGGL(covs_key_kernel<T>, grid, block, 0, st, pf, d_desc, desc_dim, nrow, n, c[0], c[1], c[2], inv, X,
                       key);
    hipLaunchKernelGGL(iota_kernel<uint32_t>, grid, block, 0, st, iota, n);
    for (int k = 0; k < 6; ++k) {
        size_t t = tsort;
        if (pmx_sort_pairs(temp, t, key + (size_t)k * (size_t)n, skey, iota, order, (int)n, 0, (int)(8 * sizeof(K)),
                           st) != hipSuccess)
            return PMX_E_HIP;
        if (hipMemcpyAsync(heads + (size_t)k * (size_t)H, order, sizeof(int32_t) * (size_t)H,
                           hipMemcpyDeviceToDevice, st) != hipSuccess)
            return PMX_E_HIP;
    }
    std::vector<int32_t> hh((size_t)6 * (size_t)H);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(hh.data(), heads, sizeof(int32_t) * hh.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    for (int32_t id : hh)
        if (id < 0 || (int64_t)id >= n) {
            err = "CovarianceSamplingDataPointsFilter: inconsistent sorted list";
            return PMX_E_STATE;
        }

    // ---- 6. the picks (:195-229), 7. the columns (:233-249) ----
    std::vector<int32_t> picks;
    auto proj = [&](int64_t i, T (&m)[6]) {
        const T* p = h_f + i * 4;
        const T* q = h_desc + i * desc_dim + nrow;
        T v[6];
        covs_v<T>(p[0], p[1], p[2], q[0], q[1], q[2], c[0], c[1], c[2], inv, v);
        for (int k = 0; k < 6; ++k) m[k] = covs_dot<T>(v, X.x, k);
    };
    if (!covs_picks<T>(hh.data(), H, n, nb_sample, proj, picks, &rep.depth)) {
        err = "CovarianceSamplingDataPointsFilter: a sorted list ran out before nbSample picks";
        return PMX_E_STATE;
    }
    const std::vector<int32_t> col = octree_replay_columns(picks.data(), nb_sample, n);
    int32_t* d_col = (int32_t*)iota;  // (free since the last sort; nb_sample < n entries)
    if (hipMemcpyAsync(d_col, col.data(), sizeof(int32_t) * (size_t)nb_sample, hipMemcpyHostToDevice, st) !=
        hipSuccess)
        return PMX_E_HIP;
    hipLaunchKernelGGL(gather_columns_kernel<T>, dim3(column_blocks(nb_sample)), block, 0, st, d_f, d_desc, 4,
                       desc_dim, d_col, nb_sample, d_of, d_od);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = nb_sample;
    return PMX_OK;
}

template int covs_run<float>(const float*, const float*, const float*, int64_t, const float*, int, int, int64_t, int,
                             const double*, float*, float*, int64_t*, pmx_covs_report&, hipStream_t, std::string&);
template int covs_run<double>(const double*, const double*, const double*, int64_t, const double*, int, int, int64_t,
                              int, const double*, double*, double*, int64_t*, pmx_covs_report&, hipStream_t,
                              std::string&);

}  // namespace pmx

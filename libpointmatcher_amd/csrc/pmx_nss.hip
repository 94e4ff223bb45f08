// pmx_nss.hip — NormalSpaceDataPointsFilter on the device
// (DataPointsFilters/NormalSpace.cpp:47-181; Rusinkiewicz & Levoy's
// normal-space sampling).
//
// The reference shuffles the point indices with std::random_shuffle, drops
// them in that order into a grid of buckets over (theta, phi) of the normal,
// removes the empty buckets, and nbSample times draws a bucket from a mt19937,
// takes its last member and erases the bucket once empty; the picks are then
// moved to the front by the swapCols / mapidx sequence of OctreeGrid.  Here:
//   nss_key_kernel   one point per lane: theta and phi in fp64, both quotients
//                    by eps, and a certificate that the reference's T
//                    evaluation falls in the same bucket (kNssMargin below);
//                    an uncertified point is flagged
//   the flagged points (DeviceSelect::Flagged, in index order) are evaluated
//                    on the host with the literal T expression and the host
//                    library (common/pmx_nss.h) and their keys patched
//   the shuffle      on the host: n - 1 rand() draws, the permutation uploaded;
//                    every HIP call of the filter runs with the caller's rand()
//                    state set aside (NssRandState, common/pmx_nss.h)
//   nss_perm_kernel  (key[perm[i]], perm[i])
//   pmx_sort_pairs   stable, two 8-bit passes (nbBucket <= 128 * 64 + a few
//                    rows): buckets in index order, members in shuffled order
//   nss_head_kernel + DeviceSelect::Flagged   where each non-empty bucket starts
//   the picks        on the host over the read-back order (nbSample steps,
//                    sequential by nature), then the replay on column numbers
//   gather_columns_kernel   whole feature and descriptor columns
// No atomics; deterministic.  Bit-identical to the reference, column order
// included, where the host library's acos / atan2 / fmod are the reference
// build's.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "common/pmx_nss.h"
#include "common/pmx_octree_replay.h"
#include "pmx_columns.h"
#include "pmx_internal.h"
#include "pmx_sort.h"

#include "../../include/pmx.h"

namespace pmx {

// ---- the certificate's margin ----
// A point is certified when the bucket the reference computes in T cannot
// differ from the one computed here in fp64.  Both are floor(angle / eps), so
// it is enough that the fp64 quotient is farther from every integer (and the
// angle from its wrap points) than the two evaluations can be apart.  With
// u_T the unit roundoff of T (2^-24, 2^-53), u = 2^-53, an H-ulp host function
// and a V-ulp device function (an ulp of x is at most 2 u |x|), the distance
// between the quotients, in units of A / eps for an angle bounded by A:
//   theta (A = pi):    host acos 2 H u_T, the T division u_T; device acos
//                      2 V u, the fp64 division u:
//                      (2 H + 1) u_T + (2 V + 1) u
//   phi   (A = 2 pi):  host atan2 (|.| <= pi) H u_T, the fp64 add of 2 pi
//                      (a sum <= 3 pi) 1.5 u, fmod exact, the rounding to T
//                      u_T, the T division u_T; device atan2 V u, the add
//                      1.5 u, the division u:
//                      (H + 2) u_T + (V + 4) u
// H = 2: the largest error glibc documents for acosf / atan2f / acos / atan2
// on x86-64.  V = 6: the OpenCL full-profile bound for atan2 (acos: 4), which
// the device library is built to.  The sums are doubled for the second-order
// terms and for measuring against the computed quotient instead of the exact
// one.  It is a property of T and of the two libraries' bounds, not a tuned
// number: float flags about 2 * (1.9e-5 + 3.1e-5) of uniformly spread normals
// at eps = pi / 64, double about 1e-12.
constexpr double kNssHostUlp = 2.0, kNssDevUlp = 6.0, kNssU64 = 1.1102230246251565e-16;
template <typename T>
constexpr double nss_unit_roundoff() {
    return sizeof(T) == 4 ? 5.9604644775390625e-08 : kNssU64;
}
template <typename T>
constexpr double nss_margin_theta() {  // in units of pi / eps
    return 2.0 * ((2.0 * kNssHostUlp + 1.0) * nss_unit_roundoff<T>() + (2.0 * kNssDevUlp + 1.0) * kNssU64);
}
template <typename T>
constexpr double nss_margin_phi() {  // in units of 2 pi / eps
    return 2.0 * ((kNssHostUlp + 2.0) * nss_unit_roundoff<T>() + (kNssDevUlp + 4.0) * kNssU64);
}

// One point per lane.  nrm: the descriptors (desc_dim x n point-major), the
// normal at rows nrow .. nrow + 2.  eps: the T value of epsilon, widened;
// cols = ceil(2 pi / eps); mt / mp: the margins as quotient distances.  A
// certified point gets its bucket and flag 0, any other (a NaN or |nz| > 1
// included: the host names it) key 0 and flag 1.
template <typename T>
__global__ __launch_bounds__(256) void nss_key_kernel(const T* __restrict__ nrm, int desc_dim, int nrow, int64_t n,
                                                      double eps, double cols, double mt, double mp,
                                                      uint32_t* __restrict__ key, uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T* p = nrm + i * desc_dim + nrow;
    const double nx = (double)p[0], ny = (double)p[1], nz = (double)p[2];
    uint32_t k = 0, f = 1;
    if (nx == nx && ny == ny && nz >= -1.0 && nz <= 1.0) {
        const double two_pi = 2. * M_PI;
        const double theta = acos(nz);
        const double phi = fmod(atan2(ny, nx) + two_pi, two_pi);
        const double qt = theta / eps, qp = phi / eps;
        const double ft = floor(qt), fp = floor(qp);
        const bool ok = qt - ft > mt && (ft + 1.0) - qt > mt && qp - fp > mp && (fp + 1.0) - qp > mp &&
                        theta < M_PI - mt * eps && phi > mp * eps && phi < two_pi - mp * eps;
        if (ok) {
            k = (uint32_t)(ft * cols + fp);  // (< nbBucket: theta < pi and phi < 2 pi by more than the margin)
            f = 0;
        }
    }
    key[i] = k;
    flag[i] = f;
}

// the rechecked keys: key[idx[j]] = val[j]
__global__ __launch_bounds__(256) void nss_patch_kernel(const uint32_t* __restrict__ idx,
                                                        const uint32_t* __restrict__ val, int64_t m,
                                                        uint32_t* __restrict__ key) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) key[idx[j]] = val[j];  // (idx < n: the select's output over 0 .. n-1)
}

// the sort's input in shuffled order: (key[perm[i]], perm[i])
__global__ __launch_bounds__(256) void nss_perm_kernel(const uint32_t* __restrict__ key,
                                                       const uint32_t* __restrict__ perm, int64_t n,
                                                       uint32_t* __restrict__ skey) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) skey[i] = key[perm[i]];  // (perm: a permutation of 0 .. n-1 built by the host)
}

// head[j] = 1 where a bucket starts in the sorted keys
__global__ __launch_bounds__(256) void nss_head_kernel(const uint32_t* __restrict__ skey, int64_t n,
                                                       uint32_t* __restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) head[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1u : 0u;
}

// h_desc: the host's copy of the descriptors (the flagged points' normals are
// read from it); d_f / d_desc: the cloud on the device, rows x n and
// desc_dim x n point-major.  Outputs (device, capacity nb_sample): d_of, d_od.
// The caller has taken the reference's early exits (rows 3, nb_sample >= n) and
// set the process's rand() state aside in rs before its first HIP call.
template <typename T>
int nss_run(const T* h_desc, const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int nrow,
            int64_t nb_sample, uint64_t seed, T eps, T* d_of, T* d_od, int64_t* n_out, int64_t* n_recheck,
            NssRandState& rs, hipStream_t st, std::string& err) {
    *n_out = 0;
    *n_recheck = 0;
    double cols = 0, brows = 0;
    size_t nb_bucket = 0;
    nss_bucket_counts<T>(eps, cols, brows, nb_bucket);
    int kbits = 1;
    while (((size_t)1 << kbits) < nb_bucket) ++kbits;

    uint32_t *key, *flag, *iota, *sel, *perm, *skey, *skey2, *order;
    int64_t* nsel;
    void* temp;
    size_t tsort = 0, tsel = 0;
    {
        uint32_t* v0 = nullptr;
        int64_t* c0 = nullptr;
        (void)pmx_sort_pairs(nullptr, tsort, v0, v0, v0, v0, (int)n, 0, kbits, st);
        (void)hipcub::DeviceSelect::Flagged(nullptr, tsel, v0, v0, v0, c0, (int)n, st);
    }
    const size_t tb = std::max(tsort, tsel);
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t w = sizeof(uint32_t) * (size_t)n;
    const size_t o_key = take(w), o_flag = take(w), o_iota = take(w), o_sel = take(w), o_perm = take(w),
                 o_skey = take(w), o_skey2 = take(w), o_order = take(w), o_nsel = take(sizeof(int64_t)),
                 o_temp = take(tb);
    char* buf = nullptr;
    if (hipMalloc(&buf, total) != hipSuccess) {
        err = "NormalSpaceDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    key = (uint32_t*)(buf + o_key);
    flag = (uint32_t*)(buf + o_flag);
    iota = (uint32_t*)(buf + o_iota);
    sel = (uint32_t*)(buf + o_sel);
    perm = (uint32_t*)(buf + o_perm);
    skey = (uint32_t*)(buf + o_skey);
    skey2 = (uint32_t*)(buf + o_skey2);
    order = (uint32_t*)(buf + o_order);
    nsel = (int64_t*)(buf + o_nsel);
    temp = buf + o_temp;
    const dim3 grid(column_blocks(n)), block(256);

    // ---- 1. bucket keys, the flagged points rechecked on the host ----
    const double de = (double)eps;
    hipLaunchKernelGGL(nss_key_kernel<T>, grid, block, 0, st, d_desc, desc_dim, nrow, n, de, cols,
                       nss_margin_theta<T>() * (M_PI / de), nss_margin_phi<T>() * (2. * M_PI / de), key, flag);
    hipLaunchKernelGGL(iota_kernel<uint32_t>, grid, block, 0, st, iota, n);
    size_t t = tb;
    if (hipcub::DeviceSelect::Flagged(temp, t, iota, flag, sel, nsel, (int)n, st) != hipSuccess) return PMX_E_HIP;
    int64_t m = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&m, nsel, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    if (m < 0 || m > n) {
        err = "NormalSpaceDataPointsFilter: inconsistent recheck count";
        return PMX_E_STATE;
    }
    if (m > 0) {
        std::vector<uint32_t> idx((size_t)m), val((size_t)m);
        if (hipMemcpyAsync(idx.data(), sel, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PMX_E_HIP;
        for (int64_t j = 0; j < m; ++j) {
            const int64_t i = idx[(size_t)j];
            const T* p = h_desc + i * desc_dim + nrow;
            if (!nss_normal_defined<T>(p[0], p[1], p[2])) {
                err = "NormalSpaceDataPointsFilter: the normal of point " + std::to_string(i) +
                      " has a NaN or |nz| > 1 (the reference leaves it undefined)";
                return PMX_E_BAD_PARAM;
            }
            const size_t b = nss_bucket_of<T>(p[0], p[1], p[2], eps);
            if (b >= nb_bucket) {
                err = "NormalSpaceDataPointsFilter: the normal of point " + std::to_string(i) + " falls in bucket " +
                      std::to_string(b) + " of " + std::to_string(nb_bucket) +
                      " (the reference writes out of range)";
                return PMX_E_BAD_PARAM;
            }
            val[(size_t)j] = (uint32_t)b;
        }
        // (sel is read by the patch kernel; val goes through iota, free since the select)
        if (hipMemcpyAsync(iota, val.data(), sizeof(uint32_t) * (size_t)m, hipMemcpyHostToDevice, st) != hipSuccess)
            return PMX_E_HIP;
        hipLaunchKernelGGL(nss_patch_kernel, dim3(column_blocks(m)), block, 0, st, sel, iota, m, key);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;  // (val: a local)
    }

    // ---- 2. the shuffle ----
    std::vector<int32_t> hperm((size_t)n);
    rs.draw([&] { nss_shuffle(n, hperm.data()); });
    if (hipMemcpyAsync(perm, hperm.data(), w, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;

    // ---- 3. stable grouping, the buckets' starts ----
    hipLaunchKernelGGL(nss_perm_kernel, grid, block, 0, st, key, perm, n, skey);
    t = tb;
    if (pmx_sort_pairs(temp, t, skey, skey2, perm, order, (int)n, 0, kbits, st) != hipSuccess) return PMX_E_HIP;
    hipLaunchKernelGGL(nss_head_kernel, grid, block, 0, st, skey2, n, flag);
    hipLaunchKernelGGL(iota_kernel<uint32_t>, grid, block, 0, st, iota, n);
    t = tb;
    if (hipcub::DeviceSelect::Flagged(temp, t, iota, flag, sel, nsel, (int)n, st) != hipSuccess) return PMX_E_HIP;
    int64_t nb = 0;
    std::vector<int32_t> ids((size_t)n);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&nb, nsel, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(ids.data(), order, w, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    if (nb <= 0 || nb > n || (size_t)nb > nb_bucket) {
        err = "NormalSpaceDataPointsFilter: inconsistent bucket count";
        return PMX_E_STATE;
    }
    std::vector<uint32_t> begin((size_t)nb);
    if (hipMemcpyAsync(begin.data(), sel, sizeof(uint32_t) * (size_t)nb, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;

    // ---- 4. the picks, 5. the columns ----
    const std::vector<int32_t> picks = nss_picks(ids.data(), begin.data(), nb, n, nb_sample, seed);
    const std::vector<int32_t> col = octree_replay_columns(picks.data(), nb_sample, n);
    int32_t* d_col = (int32_t*)iota;
    if (hipMemcpyAsync(d_col, col.data(), sizeof(int32_t) * (size_t)nb_sample, hipMemcpyHostToDevice, st) !=
        hipSuccess)
        return PMX_E_HIP;
    hipLaunchKernelGGL(gather_columns_kernel<T>, dim3(column_blocks(nb_sample)), block, 0, st, d_f, d_desc, rows,
                       desc_dim, d_col, nb_sample, d_of, d_od);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = nb_sample;
    *n_recheck = m;
    return PMX_OK;
}

template int nss_run<float>(const float*, const float*, int, int64_t, const float*, int, int, int64_t, uint64_t, float,
                            float*, float*, int64_t*, int64_t*, NssRandState&, hipStream_t, std::string&);
template int nss_run<double>(const double*, const double*, int, int64_t, const double*, int, int, int64_t, uint64_t,
                             double, double*, double*, int64_t*, int64_t*, NssRandState&, hipStream_t,
                             std::string&);

}  // namespace pmx

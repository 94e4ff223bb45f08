// pmx_filters_capi.hip — the stand-alone data filters of include/pmx.h:
// SurfaceNormal, SamplingSurfaceNormal, VoxelGrid, OctreeGrid, the keep-filters and the
// sensor-bias family (IncidenceAngle, Sphericality, RemoveSensorBias) on the
// device, each on a temporary context or stream (the self-match of the normals
// uses the grid match); and pmx_transform_cloud, the Transformation modules'
// compute, which is stand-alone in the same way.
#include "pmx_ctx.h"
#include "common/pmx_covs.h"
#include "common/pmx_nss.h"

namespace pmxc {

// SurfaceNormalDataPointsFilter (DataPointsFilters/SurfaceNormal.cpp:80-290):
// self-match on a temporary context, the statistics kernel, and the
// smoothNormals pass on the host (the reference smooths in place, point by
// point: later points see the already smoothed normals of earlier ones,
// :256-283 — a sequential dependency kept as is).
template <typename T>
int surface_normals_impl(int device, const T* feat, int rows, int64_t n, int knn, double maxDist, unsigned flags,
                         T* o_nrm, T* o_dens, T* o_eval, T* o_evec, T* o_ids, T* o_mdist, int64_t* degenerate) {
    if (rows != 3 && rows != 4) {
        g_err = "SurfaceNormalDataPointsFilter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (knn < 1) {  // (SurfaceNormal.h:68: min 1; k > 16 on the wave-per-query search)
        g_err = "SurfaceNormalDataPointsFilter: knn must be >= 1";
        return PMX_E_BAD_PARAM;
    }
    if (degenerate) *degenerate = 0;
    if (n <= 0) return PMX_OK;
    pmx_ctx* c = nullptr;
    int rc = pmx_ctx_create(device, sizeof(T) == 8 ? PMX_F64 : PMX_F32, &c);
    if (rc) {
        g_err = "SurfaceNormalDataPointsFilter: no HIP device";
        return rc;
    }
    struct Guard {
        pmx_ctx* c;
        ~Guard() { pmx_ctx_destroy(c); }
    } guard{c};
    auto err = [&](int r) {
        g_err = c->err;
        return r;
    };
    c->reuse_on = false;
    c->search_type = 1;
    if (c->grid_mode == 0) c->grid_mode = 1;
    const int D = rows - 1;
    std::vector<T> I((size_t)rows * rows, (T)0);
    for (int i = 0; i < rows; ++i) I[(size_t)i * rows + i] = 1;
    if ((rc = set_reference_impl<T>(c, feat, rows, n, nullptr))) return err(rc);
    if ((rc = set_reading_impl<T>(c, feat, rows, n, I.data()))) return err(rc);
    if ((rc = match_impl<T>(c, I.data(), knn, maxDist, nullptr))) return err(rc);
    const int64_t per = D + 1 + D + D * D + 1;  // normals, density, eigen values, eigen vectors, mean distance
    T* d_out = nullptr;
    unsigned long long* d_deg = nullptr;
    HIPCHK(c, hipMalloc((void**)&d_out, sizeof(T) * (size_t)(n * per)));
    std::unique_ptr<void, void (*)(void*)> free_out(d_out, [](void* p) { (void)hipFree(p); });
    HIPCHK(c, hipMalloc((void**)&d_deg, sizeof(unsigned long long)));
    std::unique_ptr<void, void (*)(void*)> free_deg(d_deg, [](void* p) { (void)hipFree(p); });
    HIPCHK(c, hipMemsetAsync(d_deg, 0, sizeof(unsigned long long), c->stream));
    T* d_nrm = d_out;
    T* d_dens = d_nrm + n * D;
    T* d_eval = d_dens + n;
    T* d_evec = d_eval + n * D;
    T* d_md = d_evec + n * D * D;
    const GridLevel& L = c->lv(c->ids_level);
    launch_surface_normals<T>((const P4<T>*)c->d_rd, (const P4<T>*)L.gpts, c->d_ids, (const T*)c->d_dists, n, knn, D,
                              d_nrm, d_dens, d_eval, d_evec, d_md, d_deg, c->stream);
    HIPCHK(c, hipGetLastError());
    std::vector<T> h((size_t)(n * per));
    unsigned long long deg = 0;
    HIPCHK(c, hipMemcpyAsync(h.data(), d_out, sizeof(T) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&deg, d_deg, sizeof(deg), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // slot order -> point order
    auto take = [&](int64_t off, int span, T* dst) {
        if (!dst) return;
        std::vector<T> src(h.begin() + off, h.begin() + off + n * span);
        (void)unpermute<T>(c, src, dst, span);  // (host_order below has run)
    };
    const bool smooth = (flags & PMX_SN_SMOOTH) && o_nrm;
    if ((rc = host_order(c))) return err(rc);
    take(0, D, o_nrm);
    take(n * D, 1, o_dens);
    take(n * (D + 1), D, o_eval);
    take(n * (2 * D + 1), D * D, o_evec);
    take(n * (2 * D + 1 + D * D), 1, o_mdist);
    if (o_ids || smooth) {
        std::vector<T> dd((size_t)(n * knn));
        std::vector<int32_t> ii((size_t)(n * knn));
        if ((rc = get_matches_impl<T>(c, dd.data(), ii.data()))) return err(rc);
        if (o_ids)  // matches.ids.cast<T>() (SurfaceNormal.cpp:250-253)
            for (size_t e = 0; e < ii.size(); ++e) o_ids[e] = (T)ii[e];
        if (smooth) {  // SurfaceNormal.cpp:256-283, in place, point order
            const T inf = std::numeric_limits<T>::infinity();
            for (int64_t i = 0; i < n; ++i) {
                T cur[3] = {0, 0, 0}, mean[3] = {0, 0, 0};
                for (int r = 0; r < D; ++r) cur[r] = o_nrm[i * D + r];
                int cnt = 0;
                for (int j = 0; j < knn; ++j) {
                    if (dd[(size_t)(i * knn + j)] == inf) continue;
                    const int64_t ref = ii[(size_t)(i * knn + j)];
                    const T* nb = o_nrm + ref * D;
                    T dot = 0;
                    for (int r = 0; r < D; ++r) dot = dot + cur[r] * nb[r];
                    for (int r = 0; r < D; ++r) mean[r] = dot > (T)0 ? mean[r] + nb[r] : mean[r] - nb[r];
                    ++cnt;
                }
                for (int r = 0; r < D; ++r) o_nrm[i * D + r] = mean[r] / (T)cnt;
            }
        }
    }
    if (degenerate) *degenerate = (int64_t)deg;
    return PMX_OK;
}

// SamplingSurfaceNormalDataPointsFilter::inPlaceFilter
// (DataPointsFilters/SamplingSurfaceNormal.cpp:80-342): the split and the leaf
// statistics on the device (pmx_ssn.hip), the sampling and the output cloud
// here — fuseRange's draws in leaf order (:285-309), the output in index
// order (:145-164).
template <typename T>
int voxel_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, const double* vsize,
               bool centroid, bool avg, T* feat_out, T* desc_out, int64_t* n_out) {
    if (rows != 3 && rows != 4) {
        g_err = "VoxelGridDataPointsFilter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    *n_out = 0;
    if (n <= 0) return PMX_OK;
    if (hipSetDevice(device) != hipSuccess) {
        g_err = "VoxelGridDataPointsFilter: no HIP device";
        return PMX_E_HIP;
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return PMX_E_HIP;
    std::unique_ptr<std::remove_pointer<hipStream_t>::type, void (*)(hipStream_t)> free_st(
        st, [](hipStream_t s) { (void)hipStreamDestroy(s); });
    const size_t fb = sizeof(T) * (size_t)rows * n, db = sizeof(T) * (size_t)desc_dim * n;
    char* buf = nullptr;
    if (hipMalloc(&buf, 2 * (fb + db) + 512) != hipSuccess) {
        g_err = "VoxelGridDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    T* d_f = (T*)buf;
    T* d_d = (T*)(buf + ((fb + 255) & ~(size_t)255));
    T* d_of = (T*)((char*)d_d + ((db + 255) & ~(size_t)255));
    T* d_od = d_of + (size_t)rows * n;
    if (hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    if (db && hipMemcpyAsync(d_d, desc, db, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    std::string err;
    int64_t m = 0;
    const int rc = voxel_run<T>(d_f, rows, n, db ? d_d : nullptr, desc_dim, vsize, centroid, avg, d_of, d_od, &m, st,
                                err);
    if (rc) {
        g_err = err.empty() ? std::string("VoxelGridDataPointsFilter: HIP failure") : err;
        return rc;
    }
    if (hipMemcpyAsync(feat_out, d_of, sizeof(T) * (size_t)rows * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (db && desc_out &&
        hipMemcpyAsync(desc_out, d_od, sizeof(T) * (size_t)desc_dim * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = m;
    return PMX_OK;
}

// The keep-filters (pmx_keep.hip): upload, predicate + compaction, download of
// the kept columns
template <typename T>
int keep_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, int pred, int index,
              int flag, double value, T* feat_out, T* desc_out, int64_t* n_out) {
    *n_out = 0;
    std::string err;
    int64_t m = 0;
    if (n <= 0) {  // (the parameter checks of keep_run still apply to an empty cloud)
        const int rc = keep_run<T>(nullptr, rows, 0, nullptr, desc_dim, pred, index, flag, value, nullptr, nullptr, &m,
                                   nullptr, err);
        if (rc) g_err = err;
        return rc;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_err = "keep filter: no HIP device";
        return PMX_E_HIP;
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return PMX_E_HIP;
    std::unique_ptr<std::remove_pointer<hipStream_t>::type, void (*)(hipStream_t)> free_st(
        st, [](hipStream_t s) { (void)hipStreamDestroy(s); });
    const size_t fb = sizeof(T) * (size_t)rows * n, db = sizeof(T) * (size_t)desc_dim * n;
    const size_t fa = (fb + 255) & ~(size_t)255, da = (db + 255) & ~(size_t)255;
    char* buf = nullptr;
    if (hipMalloc(&buf, 2 * (fa + da)) != hipSuccess) {
        g_err = "keep filter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    T* d_f = (T*)buf;
    T* d_d = (T*)(buf + fa);
    T* d_of = (T*)(buf + fa + da);
    T* d_od = (T*)(buf + 2 * fa + da);
    if (hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    if (db && hipMemcpyAsync(d_d, desc, db, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    const int rc = keep_run<T>(d_f, rows, n, db ? d_d : nullptr, desc_dim, pred, index, flag, value, d_of, d_od, &m, st,
                               err);
    if (rc) {
        g_err = err.empty() ? std::string("keep filter: HIP failure") : err;
        return rc;
    }
    if (m > 0 && hipMemcpyAsync(feat_out, d_of, sizeof(T) * (size_t)rows * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (m > 0 && db && desc_out &&
        hipMemcpyAsync(desc_out, d_od, sizeof(T) * (size_t)desc_dim * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = m;
    return PMX_OK;
}

// OctreeGridDataPointsFilter (pmx_octree.hip): upload, the tree walk and the
// sampler, download of the kept columns
template <typename T>
int octree_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, int64_t max_pts,
                double max_size, int method, T* feat_out, T* desc_out, int64_t* n_out) {
    *n_out = 0;
    std::string err;
    int64_t m = 0;
    if (n <= 0) {  // (the parameter checks of octree_run still apply to an empty cloud)
        const int rc = octree_run<T>(nullptr, rows, 0, nullptr, desc_dim, max_pts, max_size, method, nullptr, nullptr,
                                     &m, nullptr, err);
        if (rc) g_err = err;
        return rc;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_err = "OctreeGridDataPointsFilter: no HIP device";
        return PMX_E_HIP;
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return PMX_E_HIP;
    std::unique_ptr<std::remove_pointer<hipStream_t>::type, void (*)(hipStream_t)> free_st(
        st, [](hipStream_t s) { (void)hipStreamDestroy(s); });
    const size_t fb = sizeof(T) * (size_t)rows * n, db = sizeof(T) * (size_t)desc_dim * n;
    const size_t fa = (fb + 255) & ~(size_t)255, da = (db + 255) & ~(size_t)255;
    char* buf = nullptr;
    if (hipMalloc(&buf, 2 * (fa + da)) != hipSuccess) {
        g_err = "OctreeGridDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    T* d_f = (T*)buf;
    T* d_d = (T*)(buf + fa);
    T* d_of = (T*)(buf + fa + da);
    T* d_od = (T*)(buf + 2 * fa + da);
    if (hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    if (db && hipMemcpyAsync(d_d, desc, db, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    const int rc = octree_run<T>(d_f, rows, n, db ? d_d : nullptr, desc_dim, max_pts, max_size, method, d_of, d_od, &m,
                                 st, err);
    if (rc) {
        g_err = err.empty() ? std::string("OctreeGridDataPointsFilter: HIP failure") : err;
        return rc;
    }
    if (m > 0 && hipMemcpyAsync(feat_out, d_of, sizeof(T) * (size_t)rows * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (m > 0 && db && desc_out &&
        hipMemcpyAsync(desc_out, d_od, sizeof(T) * (size_t)desc_dim * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = m;
    return PMX_OK;
}

// NormalSpaceDataPointsFilter (pmx_nss.hip): the parameter checks and the
// reference's early exits here, then upload, the sampling and the download of
// the nb_sample kept columns
template <typename T>
int nss_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, int normals_row,
             int64_t nb_sample, uint64_t seed, double epsilon, T* feat_out, T* desc_out, int64_t* n_out,
             int64_t* n_recheck) {
    *n_out = 0;
    if (n_recheck) *n_recheck = 0;
    if (rows != 3 && rows != 4) {
        g_err = "NormalSpaceDataPointsFilter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (nb_sample < 1 || desc_dim < 0 || n < 0) {
        g_err = "NormalSpaceDataPointsFilter: nbSample must be >= 1, the point count and the descriptor dimension >= 0";
        return PMX_E_BAD_PARAM;
    }
    const T eps = (T)epsilon;  // (NormalSpace.h:68: the bounds as T values, Comp<T>)
    if (!(eps >= (T)0.04908738521 && eps <= (T)3.14159265359)) {
        g_err = "NormalSpaceDataPointsFilter: epsilon must be in [0.04908738521, 3.14159265359]";
        return PMX_E_BAD_PARAM;
    }
    if (n > (int64_t)0x7fffffff) {
        g_err = "NormalSpaceDataPointsFilter: more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    if (rows == 3 || nb_sample >= n) {  // NormalSpace.cpp:73-82 (n = 0 included): the cloud as it is, nothing drawn
        if (n > 0) std::memcpy(feat_out, feat, sizeof(T) * (size_t)rows * n);
        if (n > 0 && desc_dim > 0 && desc_out) std::memcpy(desc_out, desc, sizeof(T) * (size_t)desc_dim * n);
        *n_out = n;
        return PMX_OK;
    }
    if (normals_row < 0 || normals_row + 3 > desc_dim) {
        g_err = "NormalSpaceDataPointsFilter: the normals (3 rows from normals_row) are not rows of the descriptors";
        return PMX_E_BAD_PARAM;
    }
    NssRandState rs;  // (the GPU runtime does not leave the process's generator alone: common/pmx_nss.h)
    if (hipSetDevice(device) != hipSuccess) {
        g_err = "NormalSpaceDataPointsFilter: no HIP device";
        return PMX_E_HIP;
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return PMX_E_HIP;
    std::unique_ptr<std::remove_pointer<hipStream_t>::type, void (*)(hipStream_t)> free_st(
        st, [](hipStream_t s) { (void)hipStreamDestroy(s); });
    const size_t fb = sizeof(T) * (size_t)rows * n, db = sizeof(T) * (size_t)desc_dim * n;
    const size_t fa = (fb + 255) & ~(size_t)255, da = (db + 255) & ~(size_t)255;
    const size_t ofb = sizeof(T) * (size_t)rows * nb_sample, odb = sizeof(T) * (size_t)desc_dim * nb_sample;
    const size_t ofa = (ofb + 255) & ~(size_t)255;
    char* buf = nullptr;
    if (hipMalloc(&buf, fa + da + ofa + odb) != hipSuccess) {
        g_err = "NormalSpaceDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    T* d_f = (T*)buf;
    T* d_d = (T*)(buf + fa);
    T* d_of = (T*)(buf + fa + da);
    T* d_od = (T*)(buf + fa + da + ofa);
    if (hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    if (hipMemcpyAsync(d_d, desc, db, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    std::string err;
    int64_t m = 0, rechecked = 0;
    const int rc = nss_run<T>(desc, d_f, rows, n, d_d, desc_dim, normals_row, nb_sample, seed, eps, d_of, d_od, &m,
                              &rechecked, rs, st, err);
    if (rc) {
        g_err = err.empty() ? std::string("NormalSpaceDataPointsFilter: HIP failure") : err;
        return rc;
    }
    if (hipMemcpyAsync(feat_out, d_of, sizeof(T) * (size_t)rows * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (desc_out &&
        hipMemcpyAsync(desc_out, d_od, sizeof(T) * (size_t)desc_dim * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = m;
    if (n_recheck) *n_recheck = rechecked;
    return PMX_OK;
}

// CovarianceSamplingDataPointsFilter (pmx_covs.hip): the checks in the
// reference's order (CovarianceSampling.cpp:77-86) with the early exit before
// any look at the normals, then upload, the sampling and the download of the
// nb_sample kept columns
template <typename T>
int covs_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, int normals_row,
              int64_t nb_sample, int torque_norm, const double* basis, T* feat_out, T* desc_out, int64_t* n_out,
              pmx_covs_report* report) {
    const char* who = "CovarianceSamplingDataPointsFilter: ";
    *n_out = 0;
    if (report) *report = pmx_covs_report{};
    if (rows != 4) {  // (:77 only asserts; a release build would read the homogeneous row as z)
        g_err = std::string(who) + "3-D clouds only (4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (nb_sample < 1 || desc_dim < 0 || n < 0) {
        g_err = std::string(who) + "nbSample must be >= 1, the point count and the descriptor dimension >= 0";
        return PMX_E_BAD_PARAM;
    }
    if (torque_norm < 0 || torque_norm > 2) {
        g_err = std::string(who) + "torqueNorm must be 0 (L = 1), 1 (L = Lavg) or 2 (L = Lmax)";
        return PMX_E_BAD_PARAM;
    }
    if (n > (int64_t)0x7fffffff) {
        g_err = std::string(who) + "more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    if (nb_sample >= n) {  // :81 (n = 0 included): the cloud as it is
        if (n > 0) std::memcpy(feat_out, feat, sizeof(T) * (size_t)rows * n);
        if (n > 0 && desc_dim > 0 && desc_out) std::memcpy(desc_out, desc, sizeof(T) * (size_t)desc_dim * n);
        *n_out = n;
        return PMX_OK;
    }
    if (normals_row < 0 || normals_row + 3 > desc_dim) {  // :85
        g_err = std::string(who) + "the normals (3 rows from normals_row) are not rows of the descriptors";
        return PMX_E_BAD_PARAM;
    }
    if (basis)
        for (int a = 0; a < 36; ++a)
            if (!covs_finite((T)basis[a])) {
                g_err = std::string(who) + "the supplied basis has a non-finite entry";
                return PMX_E_BAD_PARAM;
            }
    NssRandState rs;  // (the filter draws nothing; the GPU runtime does not leave the process's generator alone)
    if (hipSetDevice(device) != hipSuccess) {
        g_err = std::string(who) + "no HIP device";
        return PMX_E_HIP;
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return PMX_E_HIP;
    std::unique_ptr<std::remove_pointer<hipStream_t>::type, void (*)(hipStream_t)> free_st(
        st, [](hipStream_t s) { (void)hipStreamDestroy(s); });
    const size_t fb = sizeof(T) * (size_t)rows * n, db = sizeof(T) * (size_t)desc_dim * n;
    const size_t fa = (fb + 255) & ~(size_t)255, da = (db + 255) & ~(size_t)255;
    const size_t ofb = sizeof(T) * (size_t)rows * nb_sample, odb = sizeof(T) * (size_t)desc_dim * nb_sample;
    const size_t ofa = (ofb + 255) & ~(size_t)255;
    char* buf = nullptr;
    if (hipMalloc(&buf, fa + da + ofa + odb) != hipSuccess) {
        g_err = std::string(who) + "device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    T* d_f = (T*)buf;
    T* d_d = (T*)(buf + fa);
    T* d_of = (T*)(buf + fa + da);
    T* d_od = (T*)(buf + fa + da + ofa);
    if (hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    if (hipMemcpyAsync(d_d, desc, db, hipMemcpyHostToDevice, st) != hipSuccess) return PMX_E_HIP;
    std::string err;
    int64_t m = 0;
    pmx_covs_report rep;
    const int rc = covs_run<T>(feat, desc, d_f, n, d_d, desc_dim, normals_row, nb_sample, torque_norm, basis, d_of,
                               d_od, &m, rep, st, err);
    if (rc) {
        g_err = err.empty() ? std::string(who) + "HIP failure" : err;
        return rc;
    }
    if (hipMemcpyAsync(feat_out, d_of, sizeof(T) * (size_t)rows * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (desc_out &&
        hipMemcpyAsync(desc_out, d_od, sizeof(T) * (size_t)desc_dim * m, hipMemcpyDeviceToHost, st) != hipSuccess)
        return PMX_E_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = m;
    if (report) *report = rep;
    return PMX_OK;
}

// A stream and one device allocation for a stand-alone elementwise filter
struct FilterDevice {
    hipStream_t st = nullptr;
    char* buf = nullptr;
    ~FilterDevice() {
        if (buf) (void)hipFree(buf);
        if (st) (void)hipStreamDestroy(st);
    }
    int open(int device, size_t bytes, const char* who) {
        if (hipSetDevice(device) != hipSuccess) {
            g_err = std::string(who) + ": no HIP device";
            return PMX_E_HIP;
        }
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess ||
            hipMalloc(&buf, bytes) != hipSuccess) {
            g_err = std::string(who) + ": device allocation failed";
            return PMX_E_HIP;
        }
        return PMX_OK;
    }
};
static size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// IncidenceAngle, Sphericality (pmx_sensor.hip): upload, one kernel, download
template <typename T>
int incidence_impl(int device, const T* nrm, const T* obs, int span, int64_t n, T* out) {
    const char* who = "IncidenceAngleDataPointsFilter";
    if (span != 2 && span != 3) {
        g_err = std::string(who) + ": normals and observationDirections must have 2 or 3 rows";
        return PMX_E_BAD_PARAM;
    }
    if (n <= 0) return PMX_OK;
    if (n > (int64_t)0x7fffffff) {
        g_err = std::string(who) + ": more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    const size_t vb = sizeof(T) * (size_t)span * n, va = pad256(vb), ob = sizeof(T) * (size_t)n;
    FilterDevice dev;
    int rc = dev.open(device, 2 * va + ob, who);
    if (rc) return rc;
    T* d_n = (T*)dev.buf;
    T* d_o = (T*)(dev.buf + va);
    T* d_a = (T*)(dev.buf + 2 * va);
    bool ok = hipMemcpyAsync(d_n, nrm, vb, hipMemcpyHostToDevice, dev.st) == hipSuccess &&
              hipMemcpyAsync(d_o, obs, vb, hipMemcpyHostToDevice, dev.st) == hipSuccess;
    if (ok) launch_incidence_angles<T>(d_n, d_o, span, n, d_a, dev.st);
    ok = ok && hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(out, d_a, ob, hipMemcpyDeviceToHost, dev.st) == hipSuccess &&
         hipStreamSynchronize(dev.st) == hipSuccess;
    if (!ok) {
        g_err = std::string(who) + ": HIP failure";
        return PMX_E_HIP;
    }
    return PMX_OK;
}

template <typename T>
int sphericality_impl(int device, const T* eig, int64_t n, T* o_sph, T* o_un, T* o_st) {
    const char* who = "SphericalityDataPointsFilter";
    if (n <= 0) return PMX_OK;
    if (n > (int64_t)0x7fffffff) {
        g_err = std::string(who) + ": more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    const size_t eb = sizeof(T) * 3 * (size_t)n, ea = pad256(eb), ob = sizeof(T) * (size_t)n, oa = pad256(ob);
    FilterDevice dev;
    int rc = dev.open(device, ea + 3 * oa, who);
    if (rc) return rc;
    T* d_e = (T*)dev.buf;
    T* d_s = (T*)(dev.buf + ea);
    T* d_u = o_un ? (T*)(dev.buf + ea + oa) : nullptr;
    T* d_t = o_st ? (T*)(dev.buf + ea + 2 * oa) : nullptr;
    bool ok = hipMemcpyAsync(d_e, eig, eb, hipMemcpyHostToDevice, dev.st) == hipSuccess;
    if (ok) launch_sphericality<T>(d_e, n, d_s, d_u, d_t, dev.st);
    ok = ok && hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(o_sph, d_s, ob, hipMemcpyDeviceToHost, dev.st) == hipSuccess &&
         (!o_un || hipMemcpyAsync(o_un, d_u, ob, hipMemcpyDeviceToHost, dev.st) == hipSuccess) &&
         (!o_st || hipMemcpyAsync(o_st, d_t, ob, hipMemcpyDeviceToHost, dev.st) == hipSuccess) &&
         hipStreamSynchronize(dev.st) == hipSuccess;
    if (!ok) {
        g_err = std::string(who) + ": HIP failure";
        return PMX_E_HIP;
    }
    return PMX_OK;
}

// RemoveSensorBias (pmx_sensor.hip): upload, correction + compaction, download
// of the kept columns
template <typename T>
int sensor_bias_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, int inc_row,
                     int obs_row, int sensor_type, double angle_threshold, T* feat_out, T* desc_out, int64_t* n_out) {
    const char* who = "RemoveSensorBiasDataPointsFilter";
    *n_out = 0;
    std::string err;
    int64_t m = 0;
    // before the device is touched, and for an empty cloud too
    int rc = sensor_bias_check(rows, n, desc_dim, inc_row, obs_row, sensor_type, err);
    if (rc) g_err = err;
    if (rc || n <= 0) return rc;
    const size_t fb = sizeof(T) * (size_t)rows * n, db = sizeof(T) * (size_t)desc_dim * n;
    const size_t fa = pad256(fb), da = pad256(db);
    FilterDevice dev;
    if ((rc = dev.open(device, 3 * fa + 2 * da, who))) return rc;
    T* d_f = (T*)dev.buf;
    T* d_cf = (T*)(dev.buf + fa);
    T* d_of = (T*)(dev.buf + 2 * fa);
    T* d_d = (T*)(dev.buf + 3 * fa);
    T* d_od = (T*)(dev.buf + 3 * fa + da);
    if (hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, dev.st) != hipSuccess ||
        (db && hipMemcpyAsync(d_d, desc, db, hipMemcpyHostToDevice, dev.st) != hipSuccess)) {
        g_err = std::string(who) + ": HIP failure";
        return PMX_E_HIP;
    }
    rc = sensor_bias_run<T>(d_f, rows, n, db ? d_d : nullptr, desc_dim, inc_row, obs_row, sensor_type, angle_threshold,
                            d_cf, d_of, d_od, &m, dev.st, err);
    if (rc) {
        g_err = err.empty() ? std::string(who) + ": HIP failure" : err;
        return rc;
    }
    if (m > 0 && (hipMemcpyAsync(feat_out, d_of, sizeof(T) * (size_t)rows * m, hipMemcpyDeviceToHost, dev.st) !=
                      hipSuccess ||
                  hipMemcpyAsync(desc_out, d_od, sizeof(T) * (size_t)desc_dim * m, hipMemcpyDeviceToHost, dev.st) !=
                      hipSuccess)) {
        g_err = std::string(who) + ": HIP failure";
        return PMX_E_HIP;
    }
    if (hipStreamSynchronize(dev.st) != hipSuccess) {
        g_err = std::string(who) + ": HIP failure";
        return PMX_E_HIP;
    }
    *n_out = m;
    return PMX_OK;
}

// Transformation::compute (pmx_transform.hip): the checks before the device is
// touched (they hold for an empty cloud too), then upload, one kernel in place
// on the device, download.  Only the listed spans cross the bus: when other
// descriptor rows exist the spans are packed on the host into records of
// n_spans * D rows, rotated there and scattered back; the other rows are a host
// copy.  Spans that tile the whole descriptor are uploaded as they are.
template <typename T>
int transform_impl(int device, const T* feat, int rows, int64_t n, const T* params, const T* desc, int desc_dim,
                   const int* spans, int n_spans, T* feat_out, T* desc_out, double* kernel_ms) {
    const char* who = "Transformation";
    if (kernel_ms) *kernel_ms = 0;
    if (rows != 3 && rows != 4) {
        g_err = std::string(who) + ": clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (n < 0 || desc_dim < 0 || n_spans < 0) {
        g_err = std::string(who) + ": the point count, the descriptor dimension and the span count must be >= 0";
        return PMX_E_BAD_PARAM;
    }
    if (n_spans > kXformMaxSpans) {
        g_err = std::string(who) + ": more than " + std::to_string(kXformMaxSpans) + " spans to rotate";
        return PMX_E_BAD_PARAM;
    }
    if (n_spans > 0 && (desc_dim == 0 || !spans || (!desc && n > 0))) {
        g_err = std::string(who) + ": spans to rotate were given without descriptors";
        return PMX_E_BAD_PARAM;
    }
    const int D = rows - 1;
    for (int k = 0; k < n_spans; ++k) {
        if (spans[k] < 0 || spans[k] > desc_dim - D) {
            g_err = std::string(who) + ": span " + std::to_string(k) + " (rows " + std::to_string(spans[k]) + " .. " +
                    std::to_string((int64_t)spans[k] + D - 1) + ") leaves the " + std::to_string(desc_dim) +
                    " descriptor rows";
            return PMX_E_BAD_PARAM;
        }
        for (int j = 0; j < k; ++j)
            if (spans[j] < spans[k] + D && spans[k] < spans[j] + D) {
                g_err = std::string(who) + ": spans " + std::to_string(j) + " and " + std::to_string(k) + " overlap";
                return PMX_E_BAD_PARAM;
            }
    }
    if ((n + 255) / 256 > (int64_t)0x7fffffff) {
        g_err = std::string(who) + ": more than 2^39 points";
        return PMX_E_BAD_PARAM;
    }
    if (n == 0) return PMX_OK;
    XformArgs<T> a{};
    for (int e = 0; e < rows * rows; ++e) a.p[e] = params[e];
    a.nspan = n_spans;
    const int S = n_spans * D;           // span rows per point
    const bool packed = S < desc_dim;    // (no overlap: S == desc_dim means the spans tile the descriptor)
    for (int k = 0; k < n_spans; ++k) a.off[k] = packed ? k * D : spans[k];
    std::vector<T> pk;
    if (packed && S > 0) {
        pk.resize((size_t)S * (size_t)n);
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < n_spans; ++k)
                for (int r = 0; r < D; ++r) pk[(size_t)(i * S + k * D + r)] = desc[i * desc_dim + spans[k] + r];
    }
    const T* h_sp = packed ? pk.data() : desc;  // what is uploaded when S > 0
    const size_t fb = sizeof(T) * (size_t)rows * n, sb = sizeof(T) * (size_t)S * n, fa = pad256(fb);
    FilterDevice dev;
    int rc = dev.open(device, fa + sb, who);
    if (rc) return rc;
    T* d_f = (T*)dev.buf;
    T* d_s = sb ? (T*)(dev.buf + fa) : nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct Events {
        hipEvent_t &a, &b;
        ~Events() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } events{ev0, ev1};
    bool ok = hipMemcpyAsync(d_f, feat, fb, hipMemcpyHostToDevice, dev.st) == hipSuccess &&
              (!sb || hipMemcpyAsync(d_s, h_sp, sb, hipMemcpyHostToDevice, dev.st) == hipSuccess);
    if (ok && kernel_ms)
        ok = hipEventCreate(&ev0) == hipSuccess && hipEventCreate(&ev1) == hipSuccess &&
             hipEventRecord(ev0, dev.st) == hipSuccess;
    if (ok) launch_transform_cloud<T>(d_f, rows, n, a, d_s, S, d_f, d_s, dev.st);
    ok = ok && hipGetLastError() == hipSuccess;
    if (ok && kernel_ms) ok = hipEventRecord(ev1, dev.st) == hipSuccess;
    // the rows the transformation leaves alone (with the rotated spans' old
    // values, overwritten below): a host copy while the device works
    if (ok && packed && desc_out != desc) std::memcpy(desc_out, desc, sizeof(T) * (size_t)desc_dim * n);
    T* h_so = packed ? pk.data() : desc_out;
    ok = ok && hipMemcpyAsync(feat_out, d_f, fb, hipMemcpyDeviceToHost, dev.st) == hipSuccess &&
         (!sb || hipMemcpyAsync(h_so, d_s, sb, hipMemcpyDeviceToHost, dev.st) == hipSuccess) &&
         hipStreamSynchronize(dev.st) == hipSuccess;
    if (!ok) {
        g_err = std::string(who) + ": HIP failure";
        return PMX_E_HIP;
    }
    if (kernel_ms) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) *kernel_ms = ms;
    }
    if (packed && S > 0)
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < n_spans; ++k)
                for (int r = 0; r < D; ++r) desc_out[i * desc_dim + spans[k] + r] = pk[(size_t)(i * S + k * D + r)];
    return PMX_OK;
}

template <typename T>
int ssn_impl(int device, const T* feat, int rows, int64_t n, const T* desc, int desc_dim, int knn, int method,
             double ratio_d, double max_box_d, unsigned flags, T* feat_out, T* desc_out, T* o_nrm, T* o_dens,
             T* o_eval, T* o_evec, int64_t* n_out, int64_t* unfit_out) {
    if (rows != 3 && rows != 4) {
        g_err = "SamplingSurfaceNormalDataPointsFilter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (knn < 3) {
        g_err = "SamplingSurfaceNormalDataPointsFilter: knn must be >= 3";
        return PMX_E_BAD_PARAM;
    }
    if (method != 0 && method != 1) {
        g_err = "SamplingSurfaceNormalDataPointsFilter: samplingMethod must be 0 or 1";
        return PMX_E_BAD_PARAM;
    }
    if (n > (int64_t)0x7fffffff) {
        g_err = "SamplingSurfaceNormalDataPointsFilter: more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    if (n_out) *n_out = 0;
    if (unfit_out) *unfit_out = 0;
    if (n <= 0) return PMX_OK;
    pmx_ctx* c = nullptr;
    int rc = pmx_ctx_create(device, sizeof(T) == 8 ? PMX_F64 : PMX_F32, &c);
    if (rc) {
        g_err = "SamplingSurfaceNormalDataPointsFilter: no HIP device";
        return rc;
    }
    struct Guard {
        pmx_ctx* c;
        ~Guard() { pmx_ctx_destroy(c); }
    } guard{c};
    const int D = rows - 1;
    void* d_pts = nullptr;
    if (hipMalloc(&d_pts, sizeof(P4<T>) * n) != hipSuccess) {
        g_err = "SamplingSurfaceNormalDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_pts(d_pts, [](void* p) { (void)hipFree(p); });
    if ((rc = upload_raw(c, feat, sizeof(T) * (size_t)rows * n))) {
        g_err = c->err;
        return rc;
    }
    launch_pack_p4<T>((const T*)c->d_raw, rows, n, n, (P4<T>*)d_pts, c->stream);
    const T ratio = (T)ratio_d, max_box = (T)max_box_d;
    const bool want_eig = (flags & (PMX_SSN_NORMALS | PMX_SSN_EIGVALUES | PMX_SSN_EIGVECTORS)) != 0;
    std::vector<int32_t> perm, lf, lc, fit;
    std::vector<T> rec;
    std::string err;
    if ((rc = ssn_run<T>((const P4<T>*)d_pts, D, n, knn, max_box, want_eig, c->stream, perm, lf, lc, fit, rec, err))) {
        g_err = err;
        return rc;
    }
    const int RS = D + D + 1 + D + D * D;
    // fuseRange's sampling, leaf by leaf in the recursion's order
    std::vector<int32_t> keep_leaf((size_t)n, -1);  // by point index: the leaf whose record it takes
    int64_t unfit = 0, kept = 0;
    for (size_t l = 0; l < lf.size(); ++l) {
        const int32_t f = lf[l], cnt = lc[l];
        if (!fit[l]) {
            unfit += cnt;
            continue;
        }
        if (method == 0) {
            for (int32_t i = 0; i < cnt; ++i) {
                const float r = (float)std::rand() / (float)RAND_MAX;
                if (r < ratio) {
                    keep_leaf[(size_t)perm[(size_t)(f + i)]] = (int32_t)l;
                    ++kept;
                }
            }
        } else {  // the smallest index of the leaf carries its mean
            keep_leaf[(size_t)perm[(size_t)f]] = (int32_t)l;
            ++kept;
        }
    }
    int64_t o = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t l = keep_leaf[(size_t)k];
        if (l < 0) continue;
        const T* R = rec.data() + (size_t)l * RS;
        if (feat_out) {
            if (method == 0) {
                for (int r = 0; r < rows; ++r) feat_out[o * rows + r] = feat[k * rows + r];
            } else {
                for (int r = 0; r < D; ++r) feat_out[o * rows + r] = R[r];
                feat_out[o * rows + D] = 1;
            }
        }
        if (desc_out && desc && desc_dim > 0) {
            if (method == 1 && (flags & PMX_SSN_AVERAGE)) {  // mergedDesc (:320-328)
                const int32_t f = lf[(size_t)l], cnt = lc[(size_t)l];
                for (int cc = 0; cc < desc_dim; ++cc) {
                    T s = 0;
                    for (int32_t i = 0; i < cnt; ++i) s = s + desc[(int64_t)perm[(size_t)(f + i)] * desc_dim + cc];
                    desc_out[o * desc_dim + cc] = s / (T)cnt;
                }
            } else {
                for (int cc = 0; cc < desc_dim; ++cc) desc_out[o * desc_dim + cc] = desc[k * desc_dim + cc];
            }
        }
        if (o_nrm)
            for (int r = 0; r < D; ++r) o_nrm[o * D + r] = R[D + r];
        if (o_dens) o_dens[o] = R[2 * D];
        if (o_eval)
            for (int r = 0; r < D; ++r) o_eval[o * D + r] = R[2 * D + 1 + r];
        if (o_evec)
            for (int e = 0; e < D * D; ++e) o_evec[o * D * D + e] = R[3 * D + 1 + e];
        ++o;
    }
    (void)kept;
    if (n_out) *n_out = o;
    if (unfit_out) *unfit_out = unfit;
    return PMX_OK;
}

}  // namespace pmxc

using namespace pmxc;

extern "C" {

int pmx_sampling_surface_normals(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc,
                                 int desc_dim, int knn, int sampling_method, double ratio, double max_box_dim,
                                 unsigned flags, void* feat_out, void* desc_out, void* normals, void* densities,
                                 void* eig_values, void* eig_vectors, int64_t* n_out, int64_t* unfit) {
    if ((!feat && n > 0) || (desc_dim > 0 && !desc && n > 0)) {
        g_err = "null cloud";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return ssn_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, knn, sampling_method,
                               ratio, max_box_dim, flags, (float*)feat_out, (float*)desc_out, (float*)normals,
                               (float*)densities, (float*)eig_values, (float*)eig_vectors, n_out, unfit);
    if (dtype == PMX_F64)
        return ssn_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim, knn,
                                sampling_method, ratio, max_box_dim, flags, (double*)feat_out, (double*)desc_out,
                                (double*)normals, (double*)densities, (double*)eig_values, (double*)eig_vectors,
                                n_out, unfit);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_voxel_grid(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                   const double* vsize, int use_centroid, int average_desc, void* feat_out, void* desc_out,
                   int64_t* n_out) {
    if ((!feat && n > 0) || (desc_dim > 0 && !desc && n > 0) || !vsize || !n_out || (!feat_out && n > 0) ||
        desc_dim < 0) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return voxel_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, vsize,
                                 use_centroid != 0, average_desc != 0, (float*)feat_out, (float*)desc_out, n_out);
    if (dtype == PMX_F64)
        return voxel_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim, vsize,
                                  use_centroid != 0, average_desc != 0, (double*)feat_out, (double*)desc_out, n_out);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_keep_filter(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                    int predicate, int index, int flag, double value, void* feat_out, void* desc_out,
                    int64_t* n_out) {
    if ((!feat && n > 0) || (desc_dim > 0 && !desc && n > 0) || !n_out || (!feat_out && n > 0) ||
        (desc_dim > 0 && !desc_out && n > 0)) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return keep_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, predicate, index,
                                flag, value, (float*)feat_out, (float*)desc_out, n_out);
    if (dtype == PMX_F64)
        return keep_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim, predicate, index,
                                 flag, value, (double*)feat_out, (double*)desc_out, n_out);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_octree_grid(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                    int64_t max_point_by_node, double max_size_by_node, int sampling_method, void* feat_out,
                    void* desc_out, int64_t* n_out) {
    if ((!feat && n > 0) || (desc_dim > 0 && !desc && n > 0) || !n_out || (!feat_out && n > 0) ||
        (desc_dim > 0 && !desc_out && n > 0)) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return octree_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, max_point_by_node,
                                  max_size_by_node, sampling_method, (float*)feat_out, (float*)desc_out, n_out);
    if (dtype == PMX_F64)
        return octree_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim,
                                   max_point_by_node, max_size_by_node, sampling_method, (double*)feat_out,
                                   (double*)desc_out, n_out);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_normal_space(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                     int normals_row, int64_t nb_sample, uint64_t seed, double epsilon, void* feat_out,
                     void* desc_out, int64_t* n_out, int64_t* n_recheck) {
    // (n beyond the contract is refused by the checks before anything is read)
    const bool sized = n > 0 && n <= (int64_t)0x7fffffff;
    if (!n_out || (sized && (!feat || !feat_out || (desc_dim > 0 && (!desc || !desc_out))))) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return nss_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, normals_row,
                               nb_sample, seed, epsilon, (float*)feat_out, (float*)desc_out, n_out, n_recheck);
    if (dtype == PMX_F64)
        return nss_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim, normals_row,
                                nb_sample, seed, epsilon, (double*)feat_out, (double*)desc_out, n_out, n_recheck);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_covariance_sampling(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc,
                            int desc_dim, int normals_row, int64_t nb_sample, int torque_norm, const double* basis,
                            void* feat_out, void* desc_out, int64_t* n_out, pmx_covs_report* report) {
    // (n beyond the contract is refused by the checks before anything is read)
    const bool sized = n > 0 && n <= (int64_t)0x7fffffff;
    if (!n_out || (sized && (!feat || !feat_out || (desc_dim > 0 && (!desc || !desc_out))))) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return covs_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, normals_row,
                                nb_sample, torque_norm, basis, (float*)feat_out, (float*)desc_out, n_out, report);
    if (dtype == PMX_F64)
        return covs_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim, normals_row,
                                 nb_sample, torque_norm, basis, (double*)feat_out, (double*)desc_out, n_out, report);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_incidence_angles(int device, int dtype, const void* normals, const void* obs, int span, int64_t n,
                         void* angles_out) {
    if (n > 0 && (!normals || !obs || !angles_out)) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return incidence_impl<float>(device, (const float*)normals, (const float*)obs, span, n, (float*)angles_out);
    if (dtype == PMX_F64)
        return incidence_impl<double>(device, (const double*)normals, (const double*)obs, span, n,
                                      (double*)angles_out);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_sphericality(int device, int dtype, const void* eig_values, int64_t n, unsigned flags, void* sph_out,
                     void* unstruct_out, void* struct_out) {
    const bool un = (flags & PMX_SPH_UNSTRUCTURENESS) != 0, st = (flags & PMX_SPH_STRUCTURENESS) != 0;
    if (n > 0 && (!eig_values || !sph_out || (un && !unstruct_out) || (st && !struct_out))) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return sphericality_impl<float>(device, (const float*)eig_values, n, (float*)sph_out,
                                        un ? (float*)unstruct_out : nullptr, st ? (float*)struct_out : nullptr);
    if (dtype == PMX_F64)
        return sphericality_impl<double>(device, (const double*)eig_values, n, (double*)sph_out,
                                         un ? (double*)unstruct_out : nullptr, st ? (double*)struct_out : nullptr);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_remove_sensor_bias(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc,
                           int desc_dim, int inc_row, int obs_row, int sensor_type, double angle_threshold,
                           void* feat_out, void* desc_out, int64_t* n_out) {
    if (!n_out || (n > 0 && (!feat || !feat_out || (desc_dim > 0 && (!desc || !desc_out))))) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return sensor_bias_impl<float>(device, (const float*)feat, rows, n, (const float*)desc, desc_dim, inc_row,
                                       obs_row, sensor_type, angle_threshold, (float*)feat_out, (float*)desc_out,
                                       n_out);
    if (dtype == PMX_F64)
        return sensor_bias_impl<double>(device, (const double*)feat, rows, n, (const double*)desc, desc_dim, inc_row,
                                        obs_row, sensor_type, angle_threshold, (double*)feat_out, (double*)desc_out,
                                        n_out);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_transform_cloud(int device, int dtype, const void* feat, int rows, int64_t n, const void* params,
                        const void* desc, int desc_dim, const int* span_rows, int n_spans, void* feat_out,
                        void* desc_out, double* kernel_ms) {
    if (!params || (n > 0 && (!feat || !feat_out || (desc_dim > 0 && (!desc || !desc_out))))) {
        g_err = "null argument";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return transform_impl<float>(device, (const float*)feat, rows, n, (const float*)params, (const float*)desc,
                                     desc_dim, span_rows, n_spans, (float*)feat_out, (float*)desc_out, kernel_ms);
    if (dtype == PMX_F64)
        return transform_impl<double>(device, (const double*)feat, rows, n, (const double*)params, (const double*)desc,
                                      desc_dim, span_rows, n_spans, (double*)feat_out, (double*)desc_out, kernel_ms);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

int pmx_surface_normals(int device, int dtype, const void* feat, int rows, int64_t n, int knn, double maxDist,
                        unsigned flags, void* normals, void* densities, void* eig_values, void* eig_vectors,
                        void* matched_ids, void* mean_dists, int64_t* degenerate) {
    if (!feat && n > 0) {
        g_err = "null cloud";
        return PMX_E_BAD_PARAM;
    }
    if (dtype == PMX_F32)
        return surface_normals_impl<float>(device, (const float*)feat, rows, n, knn, maxDist, flags, (float*)normals,
                                           (float*)densities, (float*)eig_values, (float*)eig_vectors,
                                           (float*)matched_ids, (float*)mean_dists, degenerate);
    if (dtype == PMX_F64)
        return surface_normals_impl<double>(device, (const double*)feat, rows, n, knn, maxDist, flags,
                                            (double*)normals, (double*)densities, (double*)eig_values,
                                            (double*)eig_vectors, (double*)matched_ids, (double*)mean_dists,
                                            degenerate);
    g_err = "dtype must be PMX_F32 or PMX_F64";
    return PMX_E_BAD_PARAM;
}

}  // extern "C"

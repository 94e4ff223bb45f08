// pmx_internal.h — shared device types and launcher declarations for libpmx.
//
// HBM layout:
//   reference  P4<T>[M_pad]  (x, y, z, h) — AoS, 16 B (f32) / 32 B (f64) per
//              point, padded with +inf points to a multiple of kTile so every
//              LDS tile load is full and branch-free;
//   normals    P4<T>[M]      (nx, ny, nz, 0);
//   grid       the reference (and its normals) sorted by cell, + cell starts;
//   reading    P4<T>[N]      already transformed by T_refMean_dataIn, in SLOT
//              order (Morton order of the initial cell; slot -> query index
//              kept on the host for the mirrors);
//   dists / weights T[N * k], ids int32[N * k], slot-major (the memory order
//              of the reference's column-major k x N Eigen matrices, up to the
//              slot permutation).  ids are reference indices after a brute-
//              force match and grid positions after a grid match.
// 2-D clouds (rows = 3) are embedded as (x, y, 0, h) with the 3x3 transform
// embedded in a 4x4; adding the +0 z-term is exact, so distances equal the
// 2-D sums bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "pmx_match_plan.h"
#include "pmx_sums.h"

struct pmx_covs_report;  // include/pmx.h (what pmx_covariance_sampling reports)

namespace pmx {

template <typename T>
struct alignas(4 * sizeof(T)) P4 {
    T x, y, z, w;
};

// Loads through explicitly global pointers.  Pointers read from device
// tables (the grid-level table of the device loop) are generic, and generic
// loads compile to flat_load (which also waits on lgkmcnt, serialising with
// LDS / scalar traffic); these helpers make every gather a global_load.
template <typename T>
struct Vec4Of;
template <>
struct Vec4Of<float> {
    typedef float V __attribute__((ext_vector_type(4)));
};
template <>
struct Vec4Of<double> {
    typedef double V __attribute__((ext_vector_type(4)));
};
// Workgroup index remapped so that consecutive indices share an XCD: blocks
// are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md, "Workgroup
// dispatch, XCD placement"), so without it the neighbouring tiles of the slot
// order, which gather the same reference lines, sit in eight different L2s.
// A bijection on [0, gridDim.x) for any grid size; performance only.
__device__ __forceinline__ uint32_t xcd_block() {
    const uint32_t nb = gridDim.x, b = blockIdx.x;
    const uint32_t q = nb >> 3, r = nb & 7u, x = b & 7u, i = b >> 3;
    return x < r ? x * (q + 1u) + i : r * (q + 1u) + (x - r) * q + i;
}

template <typename T>
__device__ __forceinline__ P4<T> gld(const P4<T>* p, int64_t i) {
    typedef typename Vec4Of<T>::V V;
    const V v = ((const __attribute__((address_space(1))) V*)p)[i];
    return P4<T>{v.x, v.y, v.z, v.w};
}
// 32-bit element index: the byte offset stays 32-bit, so the load is
// `global_load v, v_off, s[base]` (no 64-bit address arithmetic per lane).
// Callers guarantee count * sizeof(element) < 4 GiB (pmx_set_reference
// checks the reference; the grid arrays are sized from it).
template <typename T>
__device__ __forceinline__ P4<T> gld32(const P4<T>* p, uint32_t i) {
    typedef typename Vec4Of<T>::V V;
    const uint32_t off = i * (uint32_t)sizeof(P4<T>);
    const V v = *(const __attribute__((address_space(1))) V*)((const __attribute__((address_space(1))) char*)p + off);
    return P4<T>{v.x, v.y, v.z, v.w};
}
template <typename E>
__device__ __forceinline__ E gld32(const E* p, uint32_t i) {
    const uint32_t off = i * (uint32_t)sizeof(E);
    return *(const __attribute__((address_space(1))) E*)((const __attribute__((address_space(1))) char*)p + off);
}
__device__ __forceinline__ uint32_t gld(const uint32_t* p, int64_t i) {
    return ((const __attribute__((address_space(1))) uint32_t*)p)[i];
}
__device__ __forceinline__ int32_t gld(const int32_t* p, int64_t i) {
    return ((const __attribute__((address_space(1))) int32_t*)p)[i];
}

// Stores of per-query outputs the NEXT kernel reads (match distances, ids,
// safe radii): plain stores (write-through agent-scope stores measured the
// same)
template <typename V>
__device__ __forceinline__ void st_out(V* p, V v) {
    *p = v;
}

template <typename T>
struct Mat4 {
    T m[16];  // row-major
};

constexpr int kBlock = 256;   // threads per block (4 waves of 64)
constexpr int kTile = 1024;   // reference points per LDS tile
constexpr int kSub = 32;      // sub-block of the min-then-rescan k=1 scheme

// device-side select state for quantile filters (one per context)
struct SelectState {
    unsigned long long prefix;   // key bits resolved so far
    unsigned long long rank;     // rank still to find inside the current prefix
    unsigned long long count;    // number of finite keys (global)
    double limit;                // resolved threshold (T value)
    double ratio;                // quantile ratio (T value)
    int err;                     // PMX_E_EMPTY_QUANTILE etc.
    int pad;
};

// ---- match (pmx_match.hip) ----
template <typename T>
void launch_match(const P4<T>* ref, int64_t M_pad, const P4<T>* rd, int64_t N, const Mat4<T>& Tm,
                  int knn, T maxR2, T* dists, int32_t* ids, T* part_d, int32_t* part_i,
                  int64_t part_cap, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int cu_count);
template <typename T>
int64_t match_part_elems(int64_t N, int64_t M_pad, int knn, int cu_count);
// KDTreeVarDistMatcher after the brute-force match: entries beyond their
// query's radius become (inf, -1) (the k nearest within a radius are the
// prefix of the k nearest)
template <typename T>
void launch_apply_radii(T* dists, int32_t* ids, const T* radii, int64_t N, int k, hipStream_t s);
// dst[s] = src[order[s]] (order == null: a copy)
template <typename T>
void launch_gather_scalar(const T* src, const int32_t* order, int64_t n, T* dst, hipStream_t s);

template <typename T>
void launch_transform(const P4<T>* in, P4<T>* out, int64_t N, const Mat4<T>& Tm, hipStream_t s);

// quantile window fused into the grid match (pmx_spec.h); null = off
struct SpecSel;

// ---- grid levels and the device-resident loop ----
struct GridGeom {
    double lo[3];
    double h, inv_h;
    int g[3];
};
// one grid level as the kernels see it (device table, indexed by LoopCtl::level)
template <typename T>
struct GridDesc {
    const P4<T>* gpts;
    const P4<T>* gpn;  // point, normal interleaved (2 P4 per position; null without normals)
    const int32_t* gidx;
    const uint32_t* start;
    GridGeom G;
    const T* gw;  // the reference's weight descriptor in position order (GenericDescriptorOutlierFilter; null: none)
};
// Per-context control word of the device-resident ICP loop (pmx_loop.hip):
// every kernel of an enqueued iteration reads it first.  done != 0 makes the
// kernels of the iterations enqueued past convergence return at once; T is
// the step transform (embedded 4x4, T values) and level the grid level of
// this iteration's match, both written by the previous iteration's step.
// A sharded loop that enqueues iterations without reading the window verdict
// back (pmx_loop_capi.hip) marks a window miss done = kCtlStalled: the rest of
// the enqueued iterations return at once (every kernel tests done != 0), and
// the host replays the stalled iteration's radix passes at its batch check.
constexpr int kCtlStalled = 2;
struct LoopCtl {
    int done;
    int level;
    int prev_level;  // level of the match the output buffers hold (-1: none; temporal reuse, pmx_grid.hip)
    int use_tile;    // the next match runs the tile kernel's warm form (tile dispatch, pmx_step.h)
    double T[16];
    double Tprev[16];  // the step transform of that previous match
};
// The two sides of a grid match as match_grid (pmx_chain.hip) hands them to
// launch_grid_match; the kernels take the fields written out.
template <typename T>
struct MatchQuery {
    const P4<T>* rd;
    int64_t N;
    Mat4<T> Tm;
    int k;
    T maxR2;
    const T* radii;         // per-query radii (KDTreeVarDistMatcher; null: maxR2 for all)
    const uint32_t* waves;  // the tile kernel: the table form's wave table,
    int64_t n_waves;
    uint32_t max_pts;  // and the largest box scanned from LDS
    // temporal reuse: a block whose misses are at most coop_max searches each
    // with a whole wave (pmx_grid.hip coop_search), more take the per-lane
    // search; Tprev is the transform of the previous match (reuse mode 2)
    int coop_max = 0;
    Mat4<T> Tprev{};
};
template <typename T>
struct MatchOut {
    T* dists;
    int32_t* ids;  // positions in the level's gpts (launch_pos_to_index maps them back)
    unsigned long long *vpart, *vout;  // the spread pair / fallback counters (null: none), and their sum
    int* iter_err;
    unsigned long long* xseg = nullptr;  // several ranks: this rank's window segment, packed by the counter sum
    T* safe = nullptr;                   // safe radii (reuse mode != 0)
    // k = 1: each query's neighbour record (the grid point, its position in
    // w), written by every search that leaves a safe radius, so that the
    // certificate reads it with the query instead of gathering it by id
    // (null: off).  With the level's interleaved point / normal records
    // (GridDesc::gpn) the normals follow at nbr + N, for the point-to-plane reduction.
    P4<T>* nbr = nullptr;
};
template <typename T>
__device__ __forceinline__ void ctl_transform(const LoopCtl* ctl, Mat4<T>& Tm) {
#pragma unroll
    for (int i = 0; i < 16; ++i) Tm.m[i] = (T)ctl->T[i];
}

// k-NN for k > kLaneMaxK (pmx_knn_wide.hip): one wave per query, the k-list
// spread over the wave.  start == null: brute force over pts[0, M) (ids are
// indices); otherwise a grid level (ids are positions), G its geometry.
template <typename T>
void launch_knn_wide(const P4<T>* pts, const int32_t* gidx, const uint32_t* start, const GridGeom* G, int64_t M,
                     const P4<T>* rd, int64_t N, const Mat4<T>& Tm, int k, T maxR2, const T* radii, T* out_d,
                     int32_t* out_i, unsigned long long* visited, const LoopCtl* ctl, const GridDesc<T>* gd,
                     SpecSel* spec, hipStream_t s);


// ---- grid match (pmx_grid.hip) ----
// Launches what the plan says (pmx_match_plan.h).  D is the level the host
// chose; ids written are positions in its gpts.  ctl / gd (device loop, every
// form but the table's): the kernels take the transform, the level
// (gd[ctl->level]) and the reuse mode from the device, and under tile
// dispatch ctl->use_tile lets one of the two enqueued kernels run.
void set_tile_prof(unsigned long long* buf);
template <typename T>
void launch_grid_match(const GridMatchPlan& plan, const GridDesc<T>& D, const MatchQuery<T>& Q, const MatchOut<T>& O,
                       const LoopCtl* ctl, const GridDesc<T>* gd, SpecSel* spec, SelectState* spec_st,
                       hipEvent_t ev_start, hipEvent_t ev_end, hipStream_t s);
// several ranks: the quantile window's pick over the all-gathered segments
// (pmx_spec.h); MatchOut::xseg is this rank's segment, packed by the counter sum.
// stall: a miss sets ctl->done = kCtlStalled (the host did not read the
// verdict; it replays the iteration).  force_miss: treat the window as
// missed (test hook, option force_miss).
template <typename T>
void launch_spec_pick(const unsigned long long* segs, int nseg, SpecSel* spec, SelectState* st, LoopCtl* ctl,
                      int stall, int force_miss, hipStream_t s);
// ---- once-per-compute setup on the device (pmx_setup.hip) ----
// a uniform grid shape as the host sizes it (cells = g0 * g1 * g2)
struct SetupShape {
    double lo[3];
    double h;
    int g[3];
    int64_t cells;
};
// scratch of the setup sorts (keys32 / keys32_out alias keys64 / keys64_out)
struct SetupScratch {
    unsigned long long* keys64 = nullptr;
    unsigned long long* keys64_out = nullptr;
    uint32_t* keys32 = nullptr;
    uint32_t* keys32_out = nullptr;
    int32_t* idx = nullptr;
    int32_t* idx_out = nullptr;
    uint32_t* counts = nullptr;  // cells + 1
    void* temp = nullptr;        // hipcub temporary storage
    size_t temp_bytes = 0;
};
template <typename T>
struct Off3 {
    T v[3];
    int on;
};
// offset (may be null): rows - 1 values subtracted per axis in T (centring)
template <typename T>
void launch_pack_p4(const T* raw, int rows, int64_t n, int64_t n_pad, P4<T>* out, hipStream_t s,
                    const T* offset = nullptr);
template <typename T>
void launch_pack_nrm(const T* raw, int D, int64_t n, P4<T>* out, hipStream_t s);
template <typename T>
void launch_bbox(const P4<T>* p, int64_t n, double* scratch, double* out, hipStream_t s);
size_t bbox_scratch_bytes();
template <typename T>
void launch_occupancy(const P4<T>* p, int64_t n, const SetupShape& s, void* scratch, hipStream_t st);
size_t occupancy_bytes(int64_t cells);  // the scratch of launch_occupancy (count first)
// the largest trial grid launch_occupancy takes: build_grid's trial sizes are
// maxe/64 and maxe/128, i.e. at most 129 cells per axis
constexpr int64_t kOccMaxCells = (int64_t)129 * 129 * 129;
template <typename T>
int build_level_device(const P4<T>* pts, int64_t M, const P4<T>* nrm, const SetupShape& s, int64_t valid,
                       const SetupScratch& sc, P4<T>* gp, P4<T>* gpn, int32_t* gi, uint32_t* gstart, hipStream_t st);
template <typename T>
int reading_order_device(const P4<T>* raw, int64_t n, const Mat4<T>& M0, const SetupShape& s, bool morton,
                         const SetupScratch& sc, P4<T>* sorted, hipStream_t st);
size_t setup_temp_bytes(int64_t n, int64_t max_cells);
void launch_unpermute(const void* src, const int32_t* order, int64_t n, int span, size_t esz, void* dst,
                      hipStream_t s);
// SamplingSurfaceNormalDataPointsFilter's recursive median split and
// per-leaf statistics (pmx_ssn.hip).  Returns the point order (leaves
// contiguous, index order inside), the leaves (first, count), their fit flag
// and records (mean D, normal D, density, eigen values D, eigen vectors D*D);
// 0 or a PMX_E_* code with err set.
template <typename T>
int ssn_run(const P4<T>* d_pts, int D, int64_t n, int knn, T max_box, bool want_eig, hipStream_t st,
            std::vector<int32_t>& perm, std::vector<int32_t>& leaf_first, std::vector<int32_t>& leaf_cnt,
            std::vector<int32_t>& fit, std::vector<T>& rec, std::string& err);
// VoxelGridDataPointsFilter (pmx_voxel.hip): device in / out, capacity n
template <typename T>
int voxel_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, const double vsize[3], bool centroid,
              bool avg, T* d_of, T* d_od, int64_t* n_out, hipStream_t st, std::string& err);
// The keep-filters (pmx_keep.hip; pred / index / flag / value: pmx_keep_filter
// of include/pmx.h): device in / out, capacity n
template <typename T>
int keep_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int pred, int index, int flag,
             double value, T* d_of, T* d_od, int64_t* n_out, hipStream_t st, std::string& err);
// The stable compaction under them (pmx_keep.hip), for any kernel that decides
// one point per thread in blocks of kKeepBlock: the kernel ends in
// keep_block_ballot, keep_compact scans the block counts and copies the kept
// columns of d_f / d_desc to d_of / d_od (capacity n) in point order.
constexpr int kKeepBlock = 256;  // points per block: one per thread, four waves
constexpr int kKeepWaves = kKeepBlock / 64;
struct KeepScratch {
    unsigned long long* masks = nullptr;  // one ballot per wave
    uint32_t* cnt = nullptr;              // kept points per block
    uint32_t* off = nullptr;              // their exclusive scan, off[nb] = the kept count
    int64_t nb = 0;
    KeepScratch() = default;
    KeepScratch(const KeepScratch&) = delete;
    KeepScratch& operator=(const KeepScratch&) = delete;
    ~KeepScratch() {
        if (masks) (void)hipFree(masks);
    }
    int alloc(int64_t n);  // PMX_OK or PMX_E_HIP
};
// k: the calling thread's point is kept (false past n).  Every thread of the
// block calls it; the wave's 64-bit ballot and the block's kept count are stored.
__device__ __forceinline__ void keep_block_ballot(bool k, unsigned long long* __restrict__ masks,
                                                  uint32_t* __restrict__ block_cnt) {
    __shared__ uint32_t wc[kKeepWaves];
    const unsigned long long m = __ballot(k);  // 64 lanes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        masks[(int64_t)blockIdx.x * kKeepWaves + wave] = m;
        wc[wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int w = 0; w < kKeepWaves; ++w) c += wc[w];
        block_cnt[blockIdx.x] = c;
    }
}
// the exclusive scan of s.cnt into s.off (s.off[s.nb] = the kept count), for a
// caller that scatters by itself (pmx_elements.hip)
void launch_keep_scan(const KeepScratch& s, hipStream_t st);
template <typename T>
int keep_compact(const T* d_f, int rows, const T* d_desc, int desc_dim, const KeepScratch& s, T* d_of,
                 T* d_od, int64_t* n_out, hipStream_t st);
// OctreeGridDataPointsFilter (pmx_octree.hip; the parameters: pmx_octree_grid of
// include/pmx.h): device in / out, capacity n.  The random sampler draws from
// the process's rand() state on the calling thread.
template <typename T>
int octree_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int64_t max_pts, double max_size,
               int method, T* d_of, T* d_od, int64_t* n_out, hipStream_t st, std::string& err);
// NormalSpaceDataPointsFilter (pmx_nss.hip; the parameters: pmx_normal_space of
// include/pmx.h) past the reference's early exits (rows 4, 1 <= nb_sample < n <
// 2^31, nrow + 3 <= desc_dim, eps in range).  h_desc: the host's descriptors
// (the rechecked points are evaluated from them); the rest device in / out,
// capacity nb_sample.  Draws n - 1 times from the process's rand() state on the
// calling thread, after the keys are known (an error return draws nothing); rs
// holds that state aside during every HIP call (common/pmx_nss.h).
class NssRandState;
template <typename T>
int nss_run(const T* h_desc, const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int nrow,
            int64_t nb_sample, uint64_t seed, T eps, T* d_of, T* d_od, int64_t* n_out, int64_t* n_recheck,
            NssRandState& rs, hipStream_t st, std::string& err);
// CovarianceSamplingDataPointsFilter (pmx_covs.hip; the parameters:
// pmx_covariance_sampling of include/pmx.h) past the reference's early exits
// (rows 4, 1 <= nb_sample < n < 2^31, torque_norm in 0..2, nrow + 3 <= desc_dim,
// basis null or finite).  h_f / h_desc: the host's cloud (the picked points'
// projections are evaluated from it); the rest device in / out, capacity
// nb_sample.  rep: what the call reports, zeroed first.
template <typename T>
int covs_run(const T* h_f, const T* h_desc, const T* d_f, int64_t n, const T* d_desc, int desc_dim, int nrow,
             int64_t nb_sample, int torque_norm, const double* basis, T* d_of, T* d_od, int64_t* n_out,
             ::pmx_covs_report& rep, hipStream_t st, std::string& err);
// IncidenceAngle, Sphericality and RemoveSensorBias (pmx_sensor.hip); device
// pointers, point-major.  sensor_bias_run: d_cf is scratch of rows x n for the
// corrected features; outputs of capacity n.  sensor_bias_check: its parameter
// checks (they hold for an empty cloud too), PMX_OK or PMX_E_BAD_PARAM with err set
int sensor_bias_check(int rows, int64_t n, int desc_dim, int inc_row, int obs_row, int sensor_type, std::string& err);
template <typename T>
void launch_incidence_angles(const T* nrm, const T* obs, int span, int64_t n, T* angles, hipStream_t st);
template <typename T>
void launch_sphericality(const T* eig, int64_t n, T* sph, T* unstruct, T* structure, hipStream_t st);
template <typename T>
int sensor_bias_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int inc_row, int obs_row,
                    int sensor_type, double angle_threshold, T* d_cf, T* d_of, T* d_od, int64_t* n_out,
                    hipStream_t st, std::string& err);
// Transformation::compute on a whole cloud (pmx_transform.hip; the parameters:
// pmx_transform_cloud of include/pmx.h); device pointers, point-major.  a.p: the
// rows x rows row-major parameters; a.off[0 .. a.nspan): row offsets, in a
// descriptor record of `stride` rows, of the D-row spans the rotation block
// multiplies.  An output may be its own input.
constexpr int kXformMaxSpans = 8;  // (PMX_TRANSFORM_MAX_SPANS)
template <typename T>
struct XformArgs {
    T p[16];
    int nspan;
    int off[kXformMaxSpans];
};
template <typename T>
void launch_transform_cloud(const T* feat, int rows, int64_t n, const XformArgs<T>& a, const T* desc, int stride,
                            T* feat_out, T* desc_out, hipStream_t st);
// The same on a context's resident reading (pmx_transform_reading): rd / nrm
// the records in slot order, order the slot -> index table (null: identity);
// the outputs point-major in index order (rows and rows - 1 values per point).
// Tdev (device; null: a.p) the rows x rows matrix read on the device; with
// a.add_mean, mean[r] is added to coordinate r after the expression.
template <typename T>
struct XformReadingArgs {
    T p[16];
    T mean[3];
    int add_mean;
};
template <typename T>
void launch_transform_reading(const P4<T>* rd, const P4<T>* nrm, const int32_t* order, int rows, int64_t n,
                              const XformReadingArgs<T>& a, const T* Tdev, T* feat_out, T* nrm_out, hipStream_t st);
void preload_transform();
// code-object preloads (one per translation unit, called by pmx_ctx_create)
void preload_setup();
void preload_ssn();
void preload_match();
void preload_grid();
void preload_select();
void preload_reduce();
void preload_loop();
void preload_normals();
// SurfaceNormalDataPointsFilter statistics over a self-match (pmx_normals.hip)
template <typename T>
void launch_surface_normals(const P4<T>* pts, const P4<T>* gpts, const int32_t* ids, const T* dists, int64_t N,
                            int k, int D, T* o_nrm, T* o_dens, T* o_eval, T* o_evec, T* o_mdist,
                            unsigned long long* degenerate, hipStream_t s);
// spread pair / fallback counters of the grid kernels (bytes; zero-initialised once)
size_t grid_counter_bytes();
void launch_pos_to_index(const int32_t* pos, const int32_t* gidx, int32_t* out, int64_t n, hipStream_t s);

}  // namespace pmx

// ---- the outlier chain and the weight of one match entry ----
#include "pmx_weight.h"

namespace pmx {

// ---- SurfaceNormalOutlierFilter (pmx_snormal.hip) ----
// the reading's normals (raw: D x n point-major) as resident records in slot
// order (order == null: identity), rotated by the rotation block of M0
template <typename T>
void launch_reading_normals(const T* raw, int D, const int32_t* order, int64_t n, const Mat4<T>& M0, P4<T>* out,
                            hipStream_t s);

// ---- robust scale estimators (pmx_robust.hip) ----
// the exact median index count / 2 (Matches::getMedianAbsDeviation's
// nth_element, Matches.cpp:110-120) instead of the quantile rule
// (size_t)((T)count * ratio): passed as the select's ratio
constexpr double kRatioMedianIndex = 2.0;
// a given 0-based rank r among the finite keys (MaxQuantileOnAxis, pmx_keep.hip):
// passed as kRatioRankBase + r, exact below 2^52; the per-pass select
// (launch_select_pick) only
constexpr double kRatioRankBase = 4.0;
enum RobustScaleMode { kRSNone = 0, kRSMad = 1, kRSStd = 2, kRSBergFirst = 3, kRSBergNext = 4, kRSKeep = 5 };
// dev[i] = |d[i] - median| for finite d (median: st->limit), +inf otherwise
template <typename T>
void launch_abs_dev(const T* d, int64_t n, const SelectState* st, T* dev, const LoopCtl* ctl, hipStream_t s);
// sum of d (pass 0) / of (d - mean)^2 with mean = (T)(sum / n) (pass 1) into
// partials (kRedBlocks x 1), summed by launch_finalize
template <typename T>
void launch_moment(const T* d, int64_t n, int pass, const double* sum, double* partials, int64_t n_total,
                   const LoopCtl* ctl, hipStream_t s);
// the scale (a T value stored as double) of the iteration, from the mode
template <typename T>
void launch_robust_scale(int mode, const SelectState* st, const double* sums, int64_t n, double target,
                         double* scale, const LoopCtl* ctl, hipStream_t s);

// ---- quantile / weights (pmx_select.hip) ----
// one radix-select pass: histogram of digit `pass` among keys matching the
// resolved prefix.  hist must be zero on entry (select zeroes it on exit).
template <typename T>
void launch_select_hist(const T* d, int64_t n, uint32_t* hist, const SelectState* st, int pass,
                        const LoopCtl* ctl, const SpecSel* spec, hipStream_t s);
// resolve the digit of `pass`; pass 0 also computes count and the target
// rank from ratio (host value, or *ratio_dev when non-null).
// spec (may be null): skipped when the window resolved the quantile; the
// last pass re-centres the window
template <typename T>
void launch_select_pick(uint32_t* hist, SelectState* st, int pass, double ratio,
                        const double* ratio_dev, int* iter_err, const LoopCtl* ctl, SpecSel* spec, hipStream_t s);
template <typename T>
int select_passes();
// every pass in one launch (single rank; pmx_select.hip select_all_kernel):
// selx = selx_bytes() of zeroed device memory per context, re-zeroed whenever
// the launch's block count changes (select_all_blocks)
size_t selx_bytes();
int64_t select_all_blocks(int64_t n);
constexpr int kSelTimeout = -30;  // iteration error: a select_all wait timed out
// vpart / vout (may be null): the match's counter phase merged into this
// launch (pmx_selectall.h counter_merged); the spread counters are then
// zeroed by the next point-to-plane launch (launch_p2plane_partial's vzero)
template <typename T>
void launch_select_all(const T* d, int64_t n, void* selx, SelectState* st, double ratio, const double* ratio_dev,
                       int* iter_err, const LoopCtl* ctl, SpecSel* spec, const unsigned long long* vpart,
                       unsigned long long* vout, hipStream_t s);
int select_bins(int pass, int key_bits);

// VarTrimmed pieces
// development trace of the VarTrimmed walk (PMX_VT_TRACE=1): printed by
// pmx_vartrim_partial_sums
extern int g_vt_trace;
template <typename T>
size_t vartrim_trace_offset(int64_t n);
int vartrim_trace_max();
template <typename T>
void launch_vartrim(const T* d, int64_t n, int points_nbr, T minRatio, T maxRatio, const T* deno,
                    void* scratch, size_t scratch_bytes, double* ratio_dev, int* err_dev, SelectState* st,
                    const LoopCtl* ctl, hipStream_t s);
template <typename T>
size_t vartrim_scratch_bytes(int64_t n);
size_t vartrim_scratch_head();  // leading bytes of that scratch that must be zero at allocation
int vartrim_hdr_copy();     // int offset of the last call's counters in that scratch (pmx_vartrim_partial_sums)

// ---- the resident match (host side) ----
// What every reduction reads of the last match, built in one place
// (match_view, pmx_chain.hip).  The struct stops at the launchers: they unpack
// it, and the hot kernels keep written-out parameters (a struct passed to a
// kernel by value cost a VGPR and 2 % on the device loop: DESIGN.md, "The
// grid match's plan").
template <typename T>
struct MatchView {
    const P4<T>* rd;   // the reading, slot order
    const P4<T>* ref;  // the points the ids index (point-to-point gather)
    // the point-to-plane gather: point and normal records with index stride
    // rs (2: a grid level's interleaved records, nrm = pn + 1; 1: the
    // reference and its normals)
    const P4<T>* pn;
    const P4<T>* nrm;
    int rs;
    const T* d;
    const int32_t* ids;
    int k;
    int64_t N;
    // k = 1 after a grid match that left its neighbour records with the
    // normals (points, then normals at nbr + N, slot order), or null.  Each
    // launcher decides whether its kernel reads them in place of the gather.
    const P4<T>* nbr;
    const int32_t* gidx;  // ids -> original reference ids (null: they are)
    const T* gw;          // the reference's weight descriptor in the order of the ids (null: none uploaded)
};

// ---- reductions (pmx_reduce.hip) ----
constexpr int kRedBlocks = 512;  // fixed reduction grid (deterministic sums; 256 / 1024 measured slower)
// (the layout of every reduction's values: pmx_sums.h)
// m: the resident match; Tm: the step transform
// ctl / gd (device loop, may be null): early exit, step transform and the
// grid level whose positions the ids are (the records then come from gd)
// vzero (may be null): the match's spread counters, zeroed by block 0 (a
// counter phase merged into the select launch read them)
template <typename T>
void launch_p2plane_partial(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, int dim,
                            double* partials, const LoopCtl* ctl, const GridDesc<T>* gd, unsigned long long* vzero,
                            hipStream_t s);
void launch_finalize(const double* partials, int nblocks, int nv, double* out, const LoopCtl* ctl, hipStream_t s);
template <typename T>
void launch_p2point_pass1(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, double* partials,
                          const LoopCtl* ctl, const GridDesc<T>* gd, hipStream_t s);
template <typename T>
void launch_p2point_means(const double* sums, T* means_dev, int dim, const LoopCtl* ctl, hipStream_t s);
// both passes' sums in one (device loop; the step centres the moments,
// pmx_step.h): P2PointSums::kMomentsNV values
template <typename T>
void launch_p2point_moments(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, double* partials,
                            const LoopCtl* ctl, const GridDesc<T>* gd, hipStream_t s);
// similarity (PointToPointSimilarity): a tenth sum, sigma (pmx_reduce.hip)
template <typename T>
void launch_p2point_pass2(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, const T* means_dev,
                          bool similarity, double* partials, const LoopCtl* ctl, const GridDesc<T>* gd,
                          hipStream_t s);
// the chain's weights of every entry, w[N * k] (entry_weight, the
// SurfaceNormal factor included): the host mirror and what reads it
template <typename T>
void launch_weights_chain(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, T* w, hipStream_t s);

// ---- GenericDescriptorOutlierFilter (pmx_generic.hip) ----
// a grid level's copy of the reference's weight descriptor: out[pos] = desc[gidx[pos]]
template <typename T>
void launch_gd_permute(const T* desc, const int32_t* gidx, int64_t n, T* out, hipStream_t s);
// soft mode's m = max over the match's entries of (id valid ? desc[id] : 0),
// a T value stored as double at *out.  partials: kGDMaxBlocks doubles;
// ticket: one zeroed word (left zero).  ctl / gd (device loop): early exit, and
// the descriptor copy of the level whose positions the ids are.
constexpr int kGDMaxBlocks = 256;
template <typename T>
void launch_gd_max(const int32_t* ids, int64_t n, const T* desc, double* partials, unsigned int* ticket, double* out,
                   const LoopCtl* ctl, const GridDesc<T>* gd, hipStream_t s);

}  // namespace pmx

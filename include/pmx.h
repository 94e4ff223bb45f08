/*
 * pmx.h — C ABI of the MI355X-native ICP inner loop (the drop-in boundary).
 *
 * One pmx_ctx per ICP object (and per GPU rank).  It owns a HIP stream, the
 * device-resident reference / reading clouds, the k x N match and weight
 * arrays, and (optionally) an RCCL communicator.  Not thread-safe — exactly
 * like the reference's ICP object (pointmatcher/PointMatcher.h:652-764 keeps
 * mutable per-object state).  Plain pointers and sizes only: no torch/HIP
 * types cross this boundary.
 *
 * Each entry point replaces one reference interface (paths relative to the
 * libpointmatcher repository root):
 *
 *   pmx_set_reference   Matcher::init(filteredReference)
 *                         pointmatcher/PointMatcher.h:481, MatchersImpl.cpp:77-83
 *                         (+ the centred reference of ICP.cpp:291-302)
 *   pmx_set_reading     the once-per-compute reading copy + transformations.apply
 *                         (ICP.cpp:337-347)
 *   pmx_match           transformations.apply(stepReading, T_iter) fused with
 *                         Matcher::findClosests (ICP.cpp:381-387,
 *                         PointMatcher.h:484, MatchersImpl.cpp:85-101)
 *   pmx_outlier_*       OutlierFilter::compute and the chain product
 *                         (PointMatcher.h:504-512, OutlierFilter.cpp:63-103,
 *                          OutlierFiltersImpl.cpp:51-223)
 *   pmx_set_reading_normals / pmx_outlier_surface_normal
 *                       SurfaceNormalOutlierFilter::compute on the step reading's
 *                         rotated "normals" (OutlierFiltersImpl.cpp:225-285,
 *                          ICP.cpp:381-390)
 *   pmx_set_reference_weight_descriptor / pmx_outlier_generic_descriptor
 *                       GenericDescriptorOutlierFilter::compute on a one-row
 *                         descriptor of the filtered reference
 *                         (OutlierFiltersImpl.cpp:290-374)
 *   pmx_p2plane_system  ErrorElements + PointToPlane normal equations
 *                         (ErrorMinimizer.cpp:58-193, PointToPlane.cpp:171-243)
 *   pmx_p2point_system  ErrorElements + PointToPoint weighted moments
 *                         (PointToPoint.cpp:61-81)
 *   pmx_p2point_similarity_system
 *                       the same, and sigma = sum ||pc||^2 w of
 *                         PointToPointSimilarityErrorMinimizer::compute
 *                         (ErrorMinimizers/PointToPointSimilarity.cpp:43-98)
 *   pmx_p2plane_covariance / pmx_loop_covariance
 *                       the sums of PointToPlaneWithCovErrorMinimizer::
 *                         estimateCovariance (ErrorMinimizers/
 *                         PointToPlaneWithCov.cpp:72-162), read through
 *                         ErrorMinimizer::getCovariance (PointMatcher.h:553)
 *   pmx_match_quality / pmx_loop_quality
 *                       the sums of ErrorMinimizer::getResidualError and
 *                         getOverlap (PointMatcher.h:552-554; PointToPlane.cpp:
 *                         316-465, PointToPoint.cpp:104-164), with
 *                         pmx_set_reading_noise / pmx_set_reference_descriptors
 *   pmx_error_elements_prepare / pmx_error_elements /
 *   pmx_loop_error_elements_prepare
 *                       ErrorMinimizer::getErrorElements (PointMatcher.h:549-551,
 *                         ErrorMinimizer.cpp:58-193): the kept pairs themselves
 *   pmx_transform_cloud Transformation::compute on a cloud the caller keeps
 *                         (TransformationsImpl.cpp:49-231), stand-alone
 *   pmx_transform_reading / pmx_transform_reading_offset
 *                       the same on the context's resident reading: no upload,
 *                         T_iter of a finished device loop read on the device
 *   pmx_get_matches /   lazy host mirrors of Matches / OutlierWeights for
 *   pmx_get_weights       CPU modules and inspectors (PointMatcher.h:371-391)
 *
 * The 6x6 / 3x3 solves, the transform update and the convergence checks stay
 * on the host (PointToPlane.cpp:108-161, ICP.cpp:411-427).
 *
 * Errors: every call returns 0 or a negative PMX_E_* code; pmx_last_error()
 * gives the message.  The host shim maps codes to the reference exception
 * types (PointMatcher.h:83-100):
 *   PMX_E_NO_POINTS       -> ConvergenceError("ErrorMnimizer: no point to minimize")
 *   PMX_E_EMPTY_QUANTILE  -> ConvergenceError("no outlier to filter")
 *   PMX_E_BAD_PARAM       -> InvalidParameter
 *   PMX_E_TRANSFORMATION  -> TransformationError (device loop; not with the
 *                            similarity minimiser, whose transformation
 *                            checks nothing, TransformationsImpl.cpp:197-203)
 *   PMX_E_CONVERGENCE     -> ConvergenceError (device loop checkers)
 *   PMX_E_HIP / PMX_E_RCCL / PMX_E_STATE -> std::runtime_error
 */
#ifndef PMX_H
#define PMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmx_ctx pmx_ctx;

enum { PMX_F32 = 0, PMX_F64 = 1 };

enum {
    PMX_OK = 0,
    PMX_E_NO_POINTS = -1,
    PMX_E_EMPTY_QUANTILE = -2,
    PMX_E_BAD_PARAM = -3,
    PMX_E_TRANSFORMATION = -4, /* device loop: T_iter not rigid (|1 - det R| > 1e-3).  It cannot occur in a
                                  loop begun with minimizer 3 (PointToPointSimilarity): that chain holds a
                                  SimilarityTransformation and the determinant is not checked */
    PMX_E_CONVERGENCE = -5,    /* device loop: a checker raised ConvergenceError */
    PMX_E_HIP = -10,
    PMX_E_RCCL = -11,
    PMX_E_STATE = -12,
    PMX_E_NO_DEVICE = -13
};

/* per-iteration statistics (ErrorElements, ErrorMinimizer.cpp:133-192;
 * ICP.cpp:432-436).  Counts are global over all ranks. */
typedef struct pmx_stats {
    int64_t kept;               /* ErrorElements columns P: dist != inf && w != 0 */
    int64_t nonzero_weights;    /* (w != 0).count()                 ErrorMinimizer.cpp:75 */
    int64_t rejected_matches;   /* nbRejectedMatches                ErrorMinimizer.cpp:191 */
    int64_t rejected_points;    /* nbRejectedPoints                 ErrorMinimizer.cpp:192 */
    double sum_w;               /* sum of kept weights (weightedPointUsedRatio * k * N) */
    double limit;               /* last quantile threshold (diagnostic, T value) */
    int64_t n_total;            /* k * N over all ranks */
    int64_t visited;            /* pair evaluations of the iteration's match (PointCountTouched) */
    int64_t fallback_queries;   /* grid tile search: queries re-run by the per-lane shell search
                                   (diagnostic; local to this rank) */
} pmx_stats;

/* ------------------------------------------------------------ context --- */
/* device: HIP device ordinal; dtype: PMX_F32 | PMX_F64. */
int pmx_ctx_create(int device, int dtype, pmx_ctx** out);
int pmx_ctx_destroy(pmx_ctx* ctx);
/* One developer option of the context (README "Options": switches between
 * measured alternatives and test hooks; the defaults are the tuned path).
 * Also read at pmx_ctx_create from PMX_OPTS="name=value,...".  No reference
 * counterpart: the reference's tuning is its YAML parameters, which the host
 * chain (include/pmx_icp.h) maps as they are.  PMX_E_BAD_PARAM for an
 * unknown name or a malformed value. */
int pmx_ctx_set_option(pmx_ctx* ctx, const char* name, const char* value);
const char* pmx_last_error(const pmx_ctx* ctx);
/* number of visible HIP devices (0 when no GPU / driver) */
int pmx_device_count(void);
/* library build string, e.g. "pmx 0.1 gfx950" */
const char* pmx_version(void);

/* ---------------------------------------------------------- multi-GPU --- */
/* RCCL unique id (128 bytes) generated on rank 0 and broadcast by the
 * launcher; every rank then calls pmx_comm_init.  With a communicator set,
 * pmx_set_reading takes the rank's shard of the reading cloud and every
 * exchange step (quantile histograms or window segments, VarTrimmed's
 * distances, the normal equations) is a collective on the context stream
 * over RCCL/xGMI — issued whenever a communicator exists, also at nranks 1.
 * (The reference is single-process: these have no reference counterpart;
 * the sharded results equal the single-process ones) */
int pmx_comm_unique_id(void* out128);
int pmx_comm_init(pmx_ctx* ctx, const void* uid128, int nranks, int rank);
/* Host-staged collectives: the caller's transport (MPI, gloo, a test
 * harness) instead of RCCL.  The library copies the device buffer to pinned
 * host memory, synchronises its stream, calls the callback and copies the
 * result back.  allreduce: in place over `count` elements of `type`
 * (PMX_COLL_*) with `op`; allgather: `bytes` from every rank into recv, in
 * rank order.  A callback returns 0 on success.  Exclusive with
 * pmx_comm_init; call before pmx_set_reading. */
enum { PMX_COLL_F64 = 0, PMX_COLL_U32 = 1, PMX_COLL_U64 = 2 };
enum { PMX_COLL_SUM = 0, PMX_COLL_MAX = 1 };
typedef int (*pmx_allreduce_fn)(void* user, void* buf, int64_t count, int type, int op);
typedef int (*pmx_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes);
int pmx_comm_init_host(pmx_ctx* ctx, int nranks, int rank, pmx_allreduce_fn allreduce, pmx_allgather_fn allgather,
                       void* user);
/* kind: 0 none, 1 RCCL, 2 host callbacks */
int pmx_comm_size(const pmx_ctx* ctx, int* nranks, int* rank, int* kind);
/* Collectives this context has issued since creation (all-reduces,
 * all-gathers; 0 without a communicator).  A sharded iteration whose
 * quantile was resolved inside the exchanged key window issues two: the
 * window segments' all-gather and the normal equations' all-reduce. */
int pmx_comm_stats(const pmx_ctx* ctx, uint64_t* allreduces, uint64_t* allgathers);
/* How a sharded device loop synchronised (no reference counterpart: the
 * reference has one process, ICP.cpp:371-430).  verdict_syncs: iterations
 * whose window verdict the host read back (one stream synchronisation each;
 * only while the window is settling: after a miss, until two hits in a row);
 * async_iterations: iterations enqueued without reading it (zero host
 * synchronisations: a miss stalls the device loop); stalls: those misses,
 * each replayed at the next batch check (its radix passes and histogram
 * all-reduces, then the rest of the iteration). */
int pmx_comm_loop_stats(const pmx_ctx* ctx, uint64_t* verdict_syncs, uint64_t* async_iterations, uint64_t* stalls);

/* ------------------------------------------------------------ clouds --- */
/* feat: rows x M column-major (point-major) T array, rows = D + 1 with the
 * homogeneous row last (D = 2 or 3).  The caller passes the CENTRED
 * reference (ICP.cpp:299).  normals: D x M (point-major) or NULL.  Copied
 * to HBM once and kept resident across iterations and ICP calls. */
int pmx_set_reference(pmx_ctx* ctx, const void* feat, int rows, int64_t M, const void* normals);
/* The same with the centring done on the device: offset = the D reference
 * means (T values, ICP.cpp:291-292), subtracted from every point in T as
 * ICP.cpp:299 does (features.topRows(dim - 1) -= mean).  The caller then
 * needs no centred host copy of the reference. */
int pmx_set_reference_centred(pmx_ctx* ctx, const void* feat, int rows, int64_t M, const void* normals,
                              const void* offset);
/* pmx_set_reference_centred by the cloud's own mean: the mean in T, each
 * coordinate summed sequentially in point order and divided by M
 * (ICP.cpp:291-292), is computed on a host thread while the cloud and its
 * normals upload, written to mean_out (rows - 1 T values) and subtracted on
 * the device.  Replaces ICP::compute's host mean + centring (ICP.cpp:291-299)
 * followed by Matcher::init (:302). */
int pmx_set_reference_mean_centred(pmx_ctx* ctx, const void* feat, int rows, int64_t M, const void* normals,
                                   void* mean_out);
/* reading shard: rows x N.  T0 (rows x rows, row-major T) is applied once on
 * the device (T_refMean_dataIn, ICP.cpp:345-347). */
int pmx_set_reading(pmx_ctx* ctx, const void* feat, int rows, int64_t N, const void* T0);
/* KDTreeVarDistMatcher (MatchersImpl.cpp:106-150): a maximum search radius
 * per reading point (its maxDistField descriptor, N T values in the order of
 * pmx_set_reading's points; NULL clears).  While set, pmx_match uses these
 * radii (squared in T, as libnabo does) instead of its maxDist.  Cleared by
 * the next pmx_set_reading. */
int pmx_set_reading_radii(pmx_ctx* ctx, const void* radii);
/* SurfaceNormalOutlierFilter: the reading's "normals" descriptor (D x N
 * point-major T, in the order of pmx_set_reading's points; a sharded context
 * takes its shard's; NULL clears).  The rotation block of pmx_set_reading's T0
 * is applied once on the device (the reference transforms the descriptors
 * with the points, ICP.cpp:345-347), each component (m0 n0 + m1 n1) + m2 n2
 * in T, and the records follow the reading's slot order.  Cleared by the next
 * pmx_set_reading. */
int pmx_set_reading_normals(pmx_ctx* ctx, const void* normals);
/* ErrorMinimizer::getOverlap's descriptors (pmx_match_quality).  The reading's
 * "simpleSensorNoise": N T values in the order of pmx_set_reading's points (a
 * sharded context takes its shard's), kept in the reading's slot order; NULL
 * clears, and so does the next pmx_set_reading. */
int pmx_set_reading_noise(pmx_ctx* ctx, const void* noise);
/* The reference's "simpleSensorNoise" and "densities": M T values each, in the
 * order of pmx_set_reference's points; either may be NULL (absent).  Every call
 * replaces both; the next pmx_set_reference clears them.  The densities must
 * not be NaN: the median is taken from their sorted order, where a NaN would
 * rank by its bit pattern. */
int pmx_set_reference_descriptors(pmx_ctx* ctx, const void* noise, const void* densities);
/* GenericDescriptorOutlierFilter: the one-row descriptor of the reference that
 * the filter reads, M T values in the order of pmx_set_reference's points.
 * NULL clears it, and so does the next pmx_set_reference.  Every built grid
 * level keeps a copy in its own point order, so a pair gathers its value by
 * the match id alone.  The values must not be NaN: the soft form's maximum is
 * taken with comparisons, which a NaN would drop or keep depending on where
 * it stands. */
int pmx_set_reference_weight_descriptor(pmx_ctx* ctx, const void* desc);

/* ------------------------------------------------------------- match --- */
/* search structure, mirroring KDTreeMatcher's searchType
 * (MatchersImpl.h:85; libnabo: 0 brute force, 1/2 kd-tree): 0 = brute force
 * over all N*M pairs (LDS-tiled), 1 or 2 = uniform grid with exact shell
 * search (default).  Both return identical results (same arithmetic, same
 * lowest-index tie rule).  Takes effect at the next pmx_match. */
int pmx_set_search(pmx_ctx* ctx, int search_type);

/* T_iter: rows x rows row-major T.  knn >= 1 (KDTreeMatcher's bound,
 * MatchersImpl.h:83; k > 16 on the wave-per-query search, lists past 1024
 * entries in chunks of 1024; N * knn entries must fit in device memory),
 * maxDist: radius (inclusive, squared in T; +inf = none), epsilon: the
 * search is exact, so any epsilon >= 0 is satisfied.  visited (may be NULL)
 * receives the pair evaluations of this call when they are known at launch
 * (brute force: N*M; grid: 0 — the exact count is returned in
 * pmx_stats.visited by the next system call).  Results stay on the device. */
int pmx_match(pmx_ctx* ctx, const void* T_iter, int knn, double maxDist, double epsilon,
              uint64_t* visited);

/* ----------------------------------------------------- outlier filters --- */
/* chain_pos 0 writes the weights, chain_pos > 0 multiplies into them
 * (OutlierFilter.cpp:90-99).  pmx_outlier_default = empty chain
 * (w = dist != inf, OutlierFilter.cpp:70-85). */
int pmx_outlier_default(pmx_ctx* ctx);
int pmx_outlier_null(pmx_ctx* ctx, int chain_pos);
int pmx_outlier_maxdist(pmx_ctx* ctx, int chain_pos, double maxDist);
int pmx_outlier_mindist(pmx_ctx* ctx, int chain_pos, double minDist);
int pmx_outlier_mediandist(pmx_ctx* ctx, int chain_pos, double factor);
int pmx_outlier_trimmed(pmx_ctx* ctx, int chain_pos, double ratio);
int pmx_outlier_vartrimmed(pmx_ctx* ctx, int chain_pos, double minRatio, double maxRatio,
                           double lambda);
/* SurfaceNormalOutlierFilter::compute (OutlierFiltersImpl.cpp:225-285) for
 * the last pmx_match and its T_iter: eps = cos(maxAngle), computed by the
 * caller in T.  w = 0 for an entry without neighbour, else 0 when
 * |n^_reading . n^_reference| < eps with the reading normal rotated by T_iter
 * and both normalised in T (a zero normal gives NaN and is kept), else 1.
 * Without reading normals (pmx_set_reading_normals) or reference normals the
 * filter is all ones, entries without neighbour included.  It reads no
 * distance, so the quantile filters of the same chain are unaffected. */
int pmx_outlier_surface_normal(pmx_ctx* ctx, int chain_pos, double eps);
/* GenericDescriptorOutlierFilter::compute (OutlierFiltersImpl.cpp:312-374) for
 * the last pmx_match, on the descriptor of pmx_set_reference_weight_descriptor
 * (PMX_E_STATE without one); at most one per chain (PMX_E_BAD_PARAM).  With id
 * the matched reference point: w = 0 for an entry without neighbour; hard
 * (soft == 0): w = desc[id] > threshold (larger_than != 0) or desc[id] <
 * threshold, both strict and in T, 1 or 0; soft: w = desc[id] / m, a division
 * in T, m the maximum of the undivided weights over all k x N entries of every
 * rank, the zeros of the entries without neighbour included (m <= 0 is not
 * guarded: IEEE gives the infinities and NaNs the reference gives).  The soft
 * form's weights are real-valued: the systems are the weighted ones, as with
 * the RobustOutlierFilter; a pair of weight 0 is not kept, one of negative
 * weight is.  It reads no distance, so the quantile filters of the same
 * chain are unaffected. */
int pmx_outlier_generic_descriptor(pmx_ctx* ctx, int chain_pos, int soft, int larger_than, double threshold);
/* RobustOutlierFilter::robustFiltering (OutlierFiltersImpl.cpp:494-598):
 * real-valued weights w = robust(e^2), e^2 = dist / scale^2; at most one per
 * chain.  robust_fct: PMX_RF_*; tuning: k (after the berg substitution,
 * :419-433); approximation: the unsquared threshold (+inf = none); the
 * scale of this call (the filter's iteration state stays with the caller,
 * :500-531): PMX_RS_NONE (1), _MAD sqrt(median |d - median d|), _STD
 * sqrt(std), _BERG_FIRST 1.9 sqrt(quantile(0.5)), _BERG_NEXT 0.85 (s -
 * berg_target) + berg_target, _KEEP the previous call's scale at this chain
 * position; point2plane: distanceType point2plane (needs reference normals).
 * The scale stays on the device; pmx_robust_scale reads it back. */
enum { PMX_RF_CAUCHY = 0, PMX_RF_WELSCH = 1, PMX_RF_SC = 2, PMX_RF_GM = 3, PMX_RF_TUKEY = 4, PMX_RF_HUBER = 5,
       PMX_RF_L1 = 6, PMX_RF_STUDENT = 7 };
enum { PMX_RS_NONE = 0, PMX_RS_MAD = 1, PMX_RS_STD = 2, PMX_RS_BERG_FIRST = 3, PMX_RS_BERG_NEXT = 4,
       PMX_RS_KEEP = 5 };
int pmx_outlier_robust(pmx_ctx* ctx, int chain_pos, int robust_fct, double tuning, double approximation,
                       int scale_mode, double berg_target, int point2plane);
int pmx_robust_scale(pmx_ctx* ctx, int chain_pos, double* scale);

/* ---------------------------------------------------------- minimizers --- */
/* Point-to-plane normal equations for the step transform of the last
 * pmx_match: A (n x n row-major, n = 6 in 3D / 3 in 2D, full matrix, not
 * symmetrised: A = sum w F F^T) and b = -sum w F (d . n), accumulated in
 * double from T-precision products.  Synchronises the stream.  Returns
 * PMX_E_EMPTY_QUANTILE if a quantile filter of this iteration had no finite
 * distance, PMX_E_NO_POINTS if no weight is non-zero. */
int pmx_p2plane_system(pmx_ctx* ctx, double* A, double* b, pmx_stats* st);
/* PointToPlaneErrorMinimizer's force2D / force4DOF (PointToPlane.cpp:177-312)
 * for the same match: the normal equations of the forced minimisation, A
 * n x n row-major and b as above.
 *   PMX_FORCE_NONE  pmx_p2plane_system.
 *   PMX_FORCE_2D    n = 3, x = (angle, t_x, t_y): the 2-D form over the x, y
 *                   rows of the transformed reading point, the matched point
 *                   and its normal, F = [p_x n_y - p_y n_x; n_x; n_y] and
 *                   dot = (p_x - q_x) n_x + (p_y - q_y) n_y, without a z term:
 *                   sums of their own, not a block of the 6-DOF ones.  On a 2-D
 *                   context it is pmx_p2plane_system.
 *   PMX_FORCE_4DOF  n = 4, x = (yaw, t_x, t_y, t_z): F = [p_x n_y - p_y n_x; n]
 *                   with the full 3-D dot, which is rows and columns 2..5 of
 *                   the 6-DOF system, bit for bit.  PMX_E_BAD_PARAM on a 2-D
 *                   context (a dimension mismatch in the reference).
 * The outlier chain, its weights and the statistics are the unforced ones.
 * The step is solvePossiblyUnderdeterminedLinearSystem on (A, b), then
 * AngleAxis(yaw, unitZ) + t (4-DOF) or the identity with Rotation2D and
 * (t_x, t_y) in its top rows (2-D); common/pmx_dense.h holds both.  Several
 * ranks: one all-reduce of the packed sums, as the unforced call. */
enum { PMX_FORCE_NONE = 0, PMX_FORCE_2D = 1, PMX_FORCE_4DOF = 2 };
int pmx_p2plane_system_forced(pmx_ctx* ctx, int force, double* A, double* b, pmx_stats* st);
/* Point-to-point: mean_p, mean_q (D each, T values), m = sum (qc w) pc^T
 * (D x D row-major, double sums of T products). */
int pmx_p2point_system(pmx_ctx* ctx, double* mean_p, double* mean_q, double* m, pmx_stats* st);
/* PointToPointSimilarityErrorMinimizer::compute's sums
 * (ErrorMinimizers/PointToPointSimilarity.cpp:55-73): mean_p, mean_q and m as
 * pmx_p2point_system, and *sigma = sum over the kept pairs of ||p - mean_p||^2 w
 * (:69): each pair's squared norm of the centred step reading point in T,
 * (x x + y y) + z z, times its weight, summed in double.  The caller forms
 * scale = (sum of m's singular values, the last negated with a reflection)
 * / sigma, 1 when sigma < 0.0001 (:82-90).  Several ranks: sigma is reduced in
 * the moments' exchange, no collective of its own. */
int pmx_p2point_similarity_system(pmx_ctx* ctx, double* mean_p, double* mean_q, double* m, double* sigma,
                                  pmx_stats* st);
/* PointToPlaneWithCovErrorMinimizer::estimateCovariance
 * (ErrorMinimizers/PointToPlaneWithCov.cpp:72-162) for the last pmx_match, its
 * recorded filter chain and its T_iter; callable after pmx_p2plane_system.
 * T_step (rows x rows row-major T) is the increment the caller solved from
 * that system; alpha, beta, gamma, t_x, t_y, t_z are derived from it in T as
 * :94-99.  Over the ErrorElements columns (dist != inf && w != 0; a robust
 * weight's value is not used, :106-150) it returns
 *   H = sum a a^T                (J_hessian, :136-138)
 *   Q = sum (u u^T + v v^T)      (d2J_dZdX d2J_dZdX^T, :140-158)
 * as 6 x 6 row-major full symmetric matrices, fp64 sums of T-precision
 * products, and the number of columns in *pairs (may be NULL); global over
 * all ranks (one all-reduce).  The covariance is sensorStdDev^2 H^-1 Q H^-1
 * (:156-161), left to the caller.  The point ranges in a, u, v are norms in
 * the centred reference frame, as the reference computes them (:116-119), not
 * sensor ranges; a zero range gives NaN.  Synchronises the stream.
 * PMX_E_BAD_PARAM for a 2-D context or a reference without normals (the
 * reference returns max * I there, :91-92); PMX_E_STATE without a match. */
int pmx_p2plane_covariance(pmx_ctx* ctx, const void* T_step, double* H, double* Q, int64_t* pairs);
/* ErrorMinimizer::getResidualError and getOverlap (PointMatcher.h:552-554) for
 * the last pmx_match and its recorded filter chain, as reductions over the
 * resident match.  minimizer: 0 PointToPlane, 1 PointToPoint, 2
 * PointToPlaneWithCov, 3 PointToPointSimilarity (pmx_loop_cfg's numbers).
 * T_step (rows x rows row-major T; NULL: the match's own T_iter) transforms the
 * reading for the point-to-plane residual.  Over the ErrorElements columns
 * (the kept links: dist != inf && w != 0, w the chain's weight as
 * pmx_get_weights returns it), every term in T in the reference's order, the
 * sums in double:
 *   residual   point-to-plane: sum w ((d . n)^2), d = T_step p - q
 *              (PointToPlane.cpp:338-350); point-to-point and similarity: sum
 *              sqrt(dist), the match's own squared distance (PointToPoint.cpp:
 *              155-164)
 *   links      the number of columns;  dist_sum: sum sqrt(dist)
 *   overlap    num / den by the branch the descriptors present select
 *              (pmx_set_reading_noise, pmx_set_reference_descriptors):
 *     point-to-plane (PointToPlane.cpp:387-464): a link's uncertainty u in T is
 *       branch 1  (medianRadius + noise_rd[i]) + noise_ref[id]  (both noises
 *                 and densities; medianRadius = 1 / pow(medianDensity, 1/3.) in
 *                 double, medianDensity the element (size_t)(links * 0.5) of
 *                 the kept links' reference densities in ascending order)
 *       branch 2  noise_rd[i] + noise_ref[id];  3  noise_rd[i];  4  noise_ref[id]
 *       num = reading points with a kept link of sqrt(dist) < u, den = reading
 *       points with a kept link + nbRejectedPoints.
 *     point-to-point (PointToPoint.cpp:139-151), branch 3 (reading noise):
 *       mean = (T)(dist_sum / links); num = links with sqrt(dist) < mean +
 *       noise_rd[i], den = links.
 *     branch 0: no noise present, num = den = 0 and the caller falls back to
 *       the weighted used ratio (getWeightedPointUsedRatio).
 * The reference identifies a reading point by comparing the coordinates of
 * consecutive ErrorElements columns (PointToPlane.cpp:435-459), so two reading
 * points with identical transformed coordinates that are adjacent among the
 * kept links count as one there; here every reading point counts for itself.
 * The two agree whenever no two reading points coincide.
 * Without a kept link num = den = 0 and no second pass runs.
 * Global over all ranks: one all-reduce per pass (two with an overlap branch).
 * Branch 1 over more than one rank returns PMX_E_BAD_PARAM (the median of the
 * ranks' densities is not implemented).  Synchronises the stream; PMX_E_STATE
 * without a match. */
typedef struct pmx_quality {
    double residual;
    int64_t overlap_num, overlap_den;
    int64_t links;
    double dist_sum;
    double median_density; /* branch 1 only, a T value */
    int branch;
} pmx_quality;
int pmx_match_quality(pmx_ctx* ctx, const void* T_step, int minimizer, pmx_quality* out);
/* ErrorMinimizer::getErrorElements (PointMatcher.h:549-551, ErrorMinimizer.cpp:
 * 58-193) for the last pmx_match and its recorded filter chain: the kept pairs
 * as columns, compacted on the device.  A column is an entry (i, s) with
 * dist != inf && w != 0, i the reading index (this rank's shard) rising and s
 * the link rank 0..k-1 rising within i (ErrorMinimizer.cpp:98-135); w is the
 * chain's weight as pmx_get_weights returns it, so a negative weight is a
 * column and a zero one is not.
 * pmx_error_elements_prepare flags, scans and compacts into buffers the
 * context owns and returns the counts of this rank's shard: columns,
 * rejected_matches (entries with dist != inf and w == 0) and rejected_points
 * (reading points without a kept entry).  T_step (rows x rows row-major T;
 * NULL: the match's own T_iter) transforms the reading.  PMX_E_STATE without a
 * match; PMX_E_NO_POINTS when no column exists (the counts are still returned;
 * the reference throws "no point to minimize", :76-77); PMX_E_EMPTY_QUANTILE
 * as the system calls return it; PMX_E_BAD_PARAM beyond 2^31 - 1 entries.
 * pmx_error_elements copies the prepared columns out (P = columns, point-major;
 * every pointer may be NULL):
 *   reading        rows x P T: the step reading point, each row ((m0 x + m1 y) +
 *                  m2 z) + m3 h separately rounded, the homogeneous row the
 *                  resident point's own; a 2-D context has rows = 3 (x, y, h)
 *   reference      rows x P T: the matched reference point as the context holds
 *                  it (the centred frame of pmx_set_reference_centred)
 *   ref_normals    (rows - 1) x P T: its normal; PMX_E_BAD_PARAM on a reference
 *                  without normals
 *   dists, weights P T: the entry's squared distance and chain weight
 *   ids            P int32: the original reference index
 *   reading_index, link_rank
 *                  P int32: i (shard-local) and s
 * PMX_E_STATE without a prepare, or once a new match, filter call, reading,
 * reading normals or radii, or reference (descriptor) has made the prepared
 * columns stale.  The buffers are reused by the next prepare and freed with the
 * context.  No collective: every rank returns its shard's columns, and the
 * ranks' columns in rank order are the single-process columns.  Both calls
 * synchronise the stream; neither belongs inside an iteration. */
typedef struct pmx_elements_info {
    int64_t columns, rejected_matches, rejected_points;
} pmx_elements_info;
/* The step transform of the last match (rows x rows row-major T): pmx_match's
 * T_iter, or after a finished device loop the transform its last match ran at.
 * PMX_E_STATE without a match. */
int pmx_get_step_transform(pmx_ctx* ctx, void* T_step);
int pmx_error_elements_prepare(pmx_ctx* ctx, const void* T_step, pmx_elements_info* info);
int pmx_error_elements(pmx_ctx* ctx, void* reading, void* reference, void* ref_normals, void* dists, int32_t* ids,
                       void* weights, int32_t* reading_index, int32_t* link_rank);

/* ---------------------------------------------------------- host mirrors --- */
/* dists: k x N T (point-major), ids: k x N int32 (this rank's shard) */
int pmx_get_matches(pmx_ctx* ctx, void* dists, int32_t* ids);
int pmx_get_weights(pmx_ctx* ctx, void* w);
/* The last VarTrimmedDist filter's partial sums (OutlierFiltersImpl.cpp:
 * 196-198: std::partial_sum in T over the sorted finite positive distances):
 * *count of them, copied into out when out != NULL and capacity suffices.
 * Diagnostic (the sequential rounding the device reproduces in parallel). */
int pmx_vartrim_partial_sums(pmx_ctx* ctx, void* out, int64_t capacity, int64_t* count);
/* shape of the current match arrays */
int pmx_get_shape(const pmx_ctx* ctx, int64_t* n_local, int* knn);
/* Grid level `level` of the reference (the spatial index Matcher::init
 * builds, MatchersImpl.cpp:77-83), once its build on any stream is complete
 * (built on demand if it was not): *count records; ids (count int32) the
 * original reference index of each record, points (count x 4 T) and normals
 * (count x 4 T, only with normals on the reference) the records the matcher
 * and the point-to-plane reduction read.  Any of the three may be NULL.
 * Diagnostic (tests check the records against the input clouds). */
int pmx_grid_level_records(pmx_ctx* ctx, int level, int64_t* count, int32_t* ids, void* points, void* normals);

/* ------------------------------------------------------------- timing --- */
/* HIP-event timing of the dominant kernel (the match kernel) on the context
 * stream: enable, then read the accumulated device time and launch count. */
int pmx_timing_enable(pmx_ctx* ctx, int on);
int pmx_timing_read(pmx_ctx* ctx, double* match_ms, int64_t* match_launches, double* other_ms);
int pmx_sync(pmx_ctx* ctx);

/* ------------------------------------------------- device-resident loop --- */
/* The ICP loop body (ICP.cpp:371-430) with the step solve, the T_iter update
 * (ICP.cpp:419) and the transformation checkers (TransformationChecker.cpp,
 * TransformationCheckersImpl.cpp:45-225) on the device: iterations are
 * enqueued back to back and the host synchronises once per pmx_loop_run.
 * Requirements: a grid matcher (pmx_set_search 1/2, per-lane kernel), filters
 * among default / Null / MaxDist / MinDist / MedianDist / TrimmedDist /
 * VarTrimmedDist / Robust (at most one; with PointToPoint only its
 * point2point distance) / SurfaceNormal (at most one; filter_p[i][0] = eps
 * = cos(maxAngle) in T) / GenericDescriptor (at most one; filter_p[i] = {soft,
 * larger_than, threshold}; needs pmx_set_reference_weight_descriptor, else
 * PMX_E_STATE; any minimiser of the loop), PointToPlane (with force2D or force4DOF: cfg.force;
 * 4-DOF on 3-D clouds only) or PointToPlane with the covariance (no force), or
 * PointToPoint / PointToPointSimilarity (no force), checkers among Counter /
 * Differential (smoothLength < 64) / Bound.  Otherwise pmx_loop_begin returns PMX_E_BAD_PARAM and the caller
 * keeps the per-module calls. */
enum { PMX_CHECK_COUNTER = 0, PMX_CHECK_DIFFERENTIAL = 1, PMX_CHECK_BOUND = 2 };
enum { PMX_FILTER_DEFAULT = 0, PMX_FILTER_NULL = 1, PMX_FILTER_MAXDIST = 2, PMX_FILTER_MINDIST = 3,
       PMX_FILTER_MEDIANDIST = 4, PMX_FILTER_TRIMMED = 5, PMX_FILTER_VARTRIMMED = 6, PMX_FILTER_ROBUST = 7,
       PMX_FILTER_SURFACENORMAL = 8, PMX_FILTER_GENERICDESCRIPTOR = 9 };
/* RobustOutlierFilter's scale estimator in a loop configuration */
enum { PMX_RSE_NONE = 0, PMX_RSE_MAD = 1, PMX_RSE_STD = 2, PMX_RSE_BERG = 3 };
typedef struct pmx_loop_cfg {
    int knn;
    double max_dist;
    int n_filters;              /* 0: the empty chain's default (dist != inf) */
    int filter_kind[8];         /* PMX_FILTER_* */
    double filter_p[8][3];      /* maxDist / minDist / factor / ratio / (minRatio, maxRatio, lambda) / eps */
    int minimizer;              /* 0 PointToPlane, 1 PointToPoint, 2 PointToPlane with covariance
                                   (PointToPlane's iterations; pmx_loop_covariance afterwards),
                                   3 PointToPointSimilarity (PointToPointSimilarity.cpp:43-98: the step
                                   scales; T0 and T_iter need not be rigid, ICP.cpp:145-148) */
    int n_checkers;
    int checker_kind[8];        /* PMX_CHECK_* */
    double checker_p[8][3];     /* Counter: max; Differential: rot, trans, smoothLength; Bound: rot, trans */
    int keep_trace;             /* record T_iter of every iteration (pmx_loop_trace) */
    /* PMX_FILTER_ROBUST (OutlierFiltersImpl.cpp:380-598): the filter's
     * parameters and its call counter at the loop's start.  The scale of
     * iteration i is recomputed while robust_first_call + i <=
     * robust_nb_iter_for_scale (or always when that is 0), berg's first
     * computation at call 1 — robustFiltering's schedule (:500-531). */
    int robust_fct;             /* PMX_RF_* */
    int robust_estimator;       /* PMX_RSE_* */
    int robust_p2pl;            /* distanceType point2plane */
    int robust_nb_iter_for_scale;
    int robust_first_call;      /* the filter's iteration counter before the loop (1: never called) */
    double robust_tuning;       /* after berg's tuning substitution (:419-433) */
    double robust_approx;       /* approximation (inf: none) */
    double robust_berg_target;  /* berg: the target scale */
    int force;                  /* PMX_FORCE_* of PointToPlane (minimizer 0 only); 0: none */
} pmx_loop_cfg;
typedef struct pmx_loop_status {
    int iterations;             /* iterations completed (IterationsCount) */
    int done;                   /* the loop has stopped */
    int reason;                 /* 1 Counter (MaxNumIterationsReached), 2 Differential, 3 error */
    int error;                  /* 0 or a PMX_E_* code; pmx_last_error has the reference's message */
    int64_t point_count_touched;/* sum of the iterations' pair evaluations */
    pmx_stats last;             /* statistics of the last iteration that reached the minimiser */
    double T_iter[16];          /* rows x rows */
    double cond[8][2];          /* checkers' condition variables */
} pmx_loop_status;
/* reset the loop: configuration, initial T_iter (rows x rows, T values;
 * normally the identity) — the checkers' init (ICP.cpp:368-369) */
int pmx_loop_begin(pmx_ctx* ctx, const pmx_loop_cfg* cfg, const void* T_iter0);
/* run up to n more iterations (fewer if a checker stops the loop or an error
 * is raised) and fill *st.  Iterations are enqueued in small batches with one
 * batch in flight ahead of the host's check of the stop flag.  Returns 0, or
 * the error the ICP raised (st->error, message in pmx_last_error), or a
 * HIP / RCCL / state error. */
int pmx_loop_run(pmx_ctx* ctx, int n, pmx_loop_status* st);
/* pmx_p2plane_covariance for a finished loop begun with minimizer 2
 * (PointToPlaneWithCovErrorMinimizer::compute keeps the estimate of every
 * iteration and getCovariance returns the last, PointToPlaneWithCov.cpp:61-69,
 * 165-169: only that one is computed): H, Q and *pairs of the last iteration
 * that reached the minimiser, at the transform its match ran at and the
 * increment its step solved, both still on the device.  PMX_E_STATE while the
 * loop is not done, after a loop that stopped on an error, or one begun with
 * another minimizer; PMX_E_BAD_PARAM for a 2-D context. */
int pmx_loop_covariance(pmx_ctx* ctx, double* H, double* Q, int64_t* pairs);
/* pmx_match_quality for a finished loop, whatever its minimizer: the last
 * executed iteration's match, limits and step transform are still on the
 * device.  PMX_E_STATE before a loop has finished or after one that stopped on
 * an error. */
int pmx_loop_quality(pmx_ctx* ctx, int minimizer, pmx_quality* out);
/* pmx_error_elements_prepare for a finished loop: its last match and step
 * transform, as pmx_loop_quality; pmx_error_elements then copies the columns. */
int pmx_loop_error_elements_prepare(pmx_ctx* ctx, pmx_elements_info* info);
/* transformation->compute(reading, T) on the context's resident reading:
 * feat_out rows x N point-major T in the caller's index order; normals_out
 * D x N or NULL (PMX_E_STATE when asked for and no reading normals are set).
 * T_params rows x rows row-major T; NULL: the finished loop's T_iter, read on
 * the device (PMX_E_STATE without a finished loop, or after one that stopped
 * on an error).  Synchronises the stream.
 * The points are the reading as the context holds it, T0 * reading
 * (pmx_set_reading) and the normals R0 * normals (pmx_set_reading_normals);
 * nothing is uploaded, one kernel (pmx_transform.hip) and one download per
 * output.  Every row is pmx_transform_cloud's separately rounded expression,
 * the homogeneous one included; the normals get the rotation block only.
 * "Finished loop" means a pmx_loop_begin after the last pmx_set_reading whose
 * pmx_loop_run reported done.  PMX_E_STATE when no reading is set; N = 0 is a
 * result.  Several ranks: each transforms its own shard, no collective. */
int pmx_transform_reading(pmx_ctx* ctx, const void* T_params, void* feat_out, void* normals_out);
/* The same with a translation added to each coordinate r < D after the
 * expression, (...) + offset[r], one more rounding in T (offset: D values, T;
 * NULL: none): the un-centring of a reading held in the frame of
 * pmx_set_reference_centred, in the same kernel.  The homogeneous row and the
 * normals are not offset. */
int pmx_transform_reading_offset(pmx_ctx* ctx, const void* T_params, const void* offset, void* feat_out,
                                 void* normals_out);
/* T_iter after each completed iteration (keep_trace): count x rows x rows T */
int pmx_loop_trace(pmx_ctx* ctx, int first, int count, void* out);
/* Quantile window statistics of the device loop (no reference counterpart;
 * diagnostics): iterations whose TrimmedDist / MedianDist quantile (chain
 * position 0) was resolved inside the match's key window, and iterations
 * that ran the radix passes instead.  Both results are exact; counts
 * accumulate over the loops of this context since the last pmx_loop_begin. */
int pmx_loop_select_stats(pmx_ctx* ctx, uint64_t* window_hits, uint64_t* window_misses);
/* Per-iteration diagnostics of the device loop (no reference counterpart):
 * for iterations [first, first + count) of the current loop (at most the
 * last 1024), 4 int64 each: the grid level the match ran on, the quantile
 * window verdict (1 resolved in the window, 0 radix passes, -1 no window),
 * the pairs the match evaluated (MatchersImpl.cpp:98's visit count) and the
 * queries that needed a full search (the rest were certified by temporal
 * reuse).  Synchronises the context stream. */
int pmx_loop_diag(pmx_ctx* ctx, int first, int count, int64_t* out);

/* ------------------------------------------------------ data filters --- */
/* SurfaceNormalDataPointsFilter::inPlaceFilter
 * (DataPointsFilters/SurfaceNormal.cpp:80-290) on the GPU: the self k-NN of
 * the cloud on the exact grid matcher (the filter's KDTreeMatcher with
 * ALLOW_SELF_MATCH, :158-162), then one kernel for the per-point statistics.
 * Standalone (a temporary context on `device`); pmx_last_error(NULL) has the
 * message of a failed call.
 *   feat: rows x n point-major T (dtype PMX_F32 / PMX_F64), rows = D + 1
 *   knn >= 1 (SurfaceNormal.h:68), maxDist: neighbour radius (+inf = none)
 *   outputs (point-major T, each may be NULL): normals D x n, densities n,
 *   eig_values D x n (ascending), eig_vectors D*D x n (serializeEigVec,
 *   row-major; column j = eigenvector of eig_values[j], largest component
 *   positive), matched_ids knn x n (reference indices as T, -1 = none),
 *   mean_dists n; degenerate (may be NULL): points whose C failed the rank test.
 *   flags: PMX_SN_SMOOTH = smoothNormals (sequential in point order, as the
 *   reference; needs normals). */
enum { PMX_SN_SMOOTH = 1 };
int pmx_surface_normals(int device, int dtype, const void* feat, int rows, int64_t n, int knn, double maxDist,
                        unsigned flags, void* normals, void* densities, void* eig_values, void* eig_vectors,
                        void* matched_ids, void* mean_dists, int64_t* degenerate);

/* SamplingSurfaceNormalDataPointsFilter::inPlaceFilter
 * (DataPointsFilters/SamplingSurfaceNormal.cpp:80-342) on the GPU: the
 * recursive median split (buildNew) level by level over all boxes, the leaf
 * statistics (fuseRange) one thread per leaf; the sampling (samplingMethod 0:
 * rand() < ratio per point of every fitted leaf, the process's rand() state;
 * 1: the leaf's mean) and the output assembly on the host.  Standalone (a
 * temporary context on `device`); pmx_last_error(NULL) on failure.
 * Deterministic where the reference is implementation-defined: ties of the
 * median split broken by point index, a leaf's points in index order.
 *   feat: rows x n point-major T; desc: desc_dim x n point-major T (may be
 *   NULL when desc_dim = 0) — averaged per leaf with PMX_SSN_AVERAGE and
 *   samplingMethod 1, else the kept point's own
 *   outputs (point-major, sized for n points, each may be NULL): feat_out
 *   rows x n_out, desc_out desc_dim x n_out, normals D x n_out, densities
 *   n_out, eig_values D x n_out (ascending), eig_vectors D*D x n_out
 *   (serializeEigVec, row-major); unfit: points of dropped leaves. */
enum { PMX_SSN_NORMALS = 1, PMX_SSN_DENSITIES = 2, PMX_SSN_EIGVALUES = 4, PMX_SSN_EIGVECTORS = 8,
       PMX_SSN_AVERAGE = 16 };
int pmx_sampling_surface_normals(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc,
                                 int desc_dim, int knn, int sampling_method, double ratio, double max_box_dim,
                                 unsigned flags, void* feat_out, void* desc_out, void* normals, void* densities,
                                 void* eig_values, void* eig_vectors, int64_t* n_out, int64_t* unfit);

/* VoxelGridDataPointsFilter (DataPointsFilters/VoxelGrid.cpp:60-343): one
 * point per occupied voxel (vsize: vSizeX, vSizeY, vSizeZ), the voxel's
 * first point, with useCentroid its features replaced by the voxel mean, else
 * feature rows 1..3 set to the voxel centre as the reference does; descriptors
 * (desc_dim x n, may be NULL) averaged when average_desc.  Kept points in
 * index order; feat_out / desc_out hold n points.  Bit-identical to the
 * reference (sequential T sums in point order). */
int pmx_voxel_grid(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                   const double* vsize, int use_centroid, int average_desc, void* feat_out, void* desc_out,
                   int64_t* n_out);

/* The keep-filters: a per-point predicate, then a stable compaction of whole
 * feature and descriptor columns — the loops of
 *   PMX_KEEP_SHADOW          ShadowDataPointsFilter (DataPointsFilters/Shadow.cpp:62-94):
 *                            keep |normalized(n) . normalized(p)| > value, value =
 *                            sin(eps) computed by the caller in T; index = the row
 *                            offset of "normals" (span D) in desc; normalized()
 *                            leaves a zero vector as it is (Eigen 3.3)
 *   PMX_KEEP_MAX_QUANTILE    MaxQuantileOnAxisDataPointsFilter
 *                            (DataPointsFilters/MaxQuantileOnAxis.cpp:65-98): keep
 *                            feat[index] < limit, limit the element of rank
 *                            size_t(n * value) of that row (value = ratio, the
 *                            product in T), found by an exact radix select; strict,
 *                            so the points tied with the limit are dropped
 *   PMX_KEEP_REMOVE_NAN      RemoveNaNDataPointsFilter (DataPointsFilters/RemoveNaN.cpp:
 *                            47-66): keep the points without a NaN in any feature
 *                            row, the homogeneous one included
 *   PMX_KEEP_CUT_DESCRIPTOR  CutAtDescriptorThresholdDataPointsFilter
 *                            (DataPointsFilters/CutAtDescriptorThreshold.cpp:61-102):
 *                            v = desc[index]; keep v <= value when flag
 *                            (useLargerThan: the larger ones are cut), else v >= value
 * Every predicate is evaluated in T in the reference's operation order,
 * multiplies and adds rounded separately.  The kept points come out in their
 * input order (two passes and a scan, no atomics: deterministic);
 * feat_out / desc_out hold n points.  n = 0 and a kept count of 0 are results,
 * not errors.  PMX_E_BAD_PARAM for rows other than 3 or 4, an unknown
 * predicate, an index that is not a row of the features (MAX_QUANTILE) or of
 * desc (SHADOW: index + D rows; CUT_DESCRIPTOR).  Standalone like
 * pmx_voxel_grid; pmx_last_error(NULL) on failure. */
enum { PMX_KEEP_SHADOW = 0, PMX_KEEP_MAX_QUANTILE = 1, PMX_KEEP_REMOVE_NAN = 2, PMX_KEEP_CUT_DESCRIPTOR = 3 };
int pmx_keep_filter(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                    int predicate, int index, int flag, double value, void* feat_out, void* desc_out,
                    int64_t* n_out);

/* OctreeGridDataPointsFilter (DataPointsFilters/OctreeGrid.cpp:48-366, the tree
 * utils/octree.hpp:229-385): one point per non-empty leaf of an octree (rows =
 * 4) or quadtree (rows = 3).  Root box octree.hpp:238-251 in T; a node is a
 * leaf when double(radius) * 2 <= max_size_by_node or it holds <=
 * max_point_by_node points (:312), else each point goes to child
 * sum_i (p_i > center_i) << i (:181-189) of radius radius * 0.5 and centre
 * center +- 0.5 * radius, rounded in T (:335-341).  Leaves come in the
 * reference's visit order (:373-385: depth first, children 0 .. 2^dim - 1,
 * empty ones skipped), their members by rising input index; the leaves are the
 * literal recursion's whatever its depth (duplicates with max_size_by_node 0
 * end only when the radius underflows to 0).  sampling_method:
 *   0 first     the first member of each leaf (OctreeGrid.cpp:48-71)
 *   1 random    member size_t((n - 1) * float(rand() / float(RAND_MAX))), the
 *               product in float; srand(1), one rand() per leaf in visit
 *               order, srand(1) again (:85-137): the call draws from the
 *               process's rand() state on the calling thread and leaves it as
 *               srand(1) does
 *   2 centroid  feature rows but the homogeneous one, and every descriptor row:
 *               the sequential sum in T over the members in order, divided by
 *               T(n); the homogeneous row of the first member (:147-210)
 *   3 medoid    the first member strictly nearest the leaf's mean (sequential
 *               sums from 0; dist = sqrt((dx*dx + dy*dy) + dz*dz) in T)
 *               (:219-282)
 * Methods 0 and 1 are bit-identical to the reference, output column order
 * included: the reference moves pick k to column k by swapCols and a lookup
 * table (:55-67) that is one level deep and goes stale, so its kept columns
 * are not always the picks; that sequence is replayed on column numbers on the
 * host and whole columns are gathered.  Methods 2 and 3 DIVERGE from the
 * reference where it misbehaves: the reference reads and accumulates columns
 * through the same stale table, so its output depends on wrongly addressed
 * columns step by step; here column k is the centroid or medoid of leaf k
 * computed from the input cloud's own columns.  The two agree whenever no
 * lookup is stale, e.g. for a cloud already in visit order.
 * desc: desc_dim x n (may be NULL with desc_dim 0); feat_out / desc_out hold n
 * points.  n = 0 returns 0 points.  Non-finite coordinates are outside the
 * contract (a non-finite bounding box is PMX_E_BAD_PARAM); n < 2^31.
 * PMX_E_BAD_PARAM for rows other than 3 or 4, a sampling_method outside 0..3,
 * max_point_by_node < 1 or max_size_by_node < 0.  Deterministic (no atomics).
 * Standalone like pmx_voxel_grid; pmx_last_error(NULL) on failure. */
int pmx_octree_grid(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                    int64_t max_point_by_node, double max_size_by_node, int sampling_method, void* feat_out,
                    void* desc_out, int64_t* n_out);

/* NormalSpaceDataPointsFilter (DataPointsFilters/NormalSpace.cpp:47-181,
 * parameters NormalSpace.h:63-70): normal-space sampling of a 3-D cloud with
 * normals (desc rows normals_row .. normals_row + 2).  In the reference's call
 * order: rows = 3 (a 2-D cloud, :73-77), nb_sample >= n (:81) and n = 0 copy
 * the input to the outputs and draw nothing.  Otherwise the point indices are
 * shuffled by std::random_shuffle as libstdc++ runs it — for i = 1 .. n-1, j =
 * rand() % (i + 1), swap when i != j — i.e. n - 1 draws from the process's
 * rand() state on the calling thread, which is left where they leave it (seed
 * does not touch it; :100-102).  In that order each point goes to bucket
 * size_t(floor(theta / eps) * cols + floor(phi / eps)) with theta = acos(nz)
 * and phi = T(fmod(double(atan2(ny, nx)) + 2 pi, 2 pi)), theta == T(pi) and
 * phi == 2 T(pi) wrapped to 0 (so nz = -1 lands in row 0), the divisions and
 * floors in T, the product and sum in double; cols = ceil(2.0 * M_PI / eps),
 * rows = ceil(M_PI / eps), nbBucket = size_t(cols * rows), eps = T(epsilon)
 * (:53, :114-116, :169-181).  Empty buckets are removed; nb_sample times a
 * bucket is drawn from std::mt19937(seed) with
 * std::uniform_int_distribution<size_t>(0, buckets left - 1), its last member
 * is taken and popped, and the bucket is erased once empty (:129-145).  The
 * picks move to the front by the swapCols / mapidx sequence of
 * pmx_octree_grid's methods 0 and 1, stale lookups included (:149-165).
 * The certificate: the device evaluates theta, phi and both quotients in fp64
 * and keeps its bucket only where both quotients are farther from an integer,
 * theta from pi and phi from 0 and 2 pi, than the host function's error in T,
 * the device function's in fp64 and the rounding of the T division can
 * separate the two evaluations (pmx_nss.hip, kNss*; the device acos / atan2 are
 * within a few ulp of the host library's, not bit-equal).  Every other point
 * is evaluated on the host with the literal T expression; *n_recheck (may be
 * NULL) is their count.  The grouping is a stable sort, no atomics, so the
 * result is deterministic and bit-identical to the reference, output column
 * order included, on a host whose acos / atan2 / fmod agree with the reference
 * build's.
 * Inputs the reference leaves undefined are refused with PMX_E_BAD_PARAM and a
 * message naming the first offending point: a normal with a NaN or |nz| > 1
 * (its asserts :108-111), and a bucket index >= nbBucket (the T division can
 * round theta / eps up to rows; a release build writes out of range).  Also
 * PMX_E_BAD_PARAM: rows other than 3 or 4, nb_sample < 1, epsilon outside
 * [0.04908738521, 3.14159265359] compared in T, n >= 2^31, and — when the
 * sampling runs — normals_row < 0 or normals_row + 3 > desc_dim.  An error
 * return draws nothing, and the GPU runtime's own use of rand() / srand() is
 * kept off the caller's state (initstate / setstate around every HIP call).
 * desc: desc_dim x n point-major; feat_out / desc_out
 * hold n points.  Standalone like pmx_voxel_grid;
 * pmx_last_error(NULL) on failure. */
int pmx_normal_space(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc, int desc_dim,
                     int normals_row, int64_t nb_sample, uint64_t seed, double epsilon, void* feat_out,
                     void* desc_out, int64_t* n_out, int64_t* n_recheck);

/* CovarianceSamplingDataPointsFilter (DataPointsFilters/CovarianceSampling.cpp:
 * 74-250, parameters CovarianceSampling.h:70-76; Gelfand et al. 2003): stability
 * sampling of a 3-D cloud with normals (desc rows normals_row .. normals_row +
 * 2): the nb_sample points that best constrain the six degrees of freedom of
 * the point-to-plane system.  In the reference's call order: rows != 4 is
 * PMX_E_BAD_PARAM (:77 only asserts; a release build would read the
 * homogeneous row as z); nb_sample >= n and n = 0 copy the input to the
 * outputs (:81), before any look at the normals; then normals_row < 0 or
 * normals_row + 3 > desc_dim is PMX_E_BAD_PARAM (:85).
 * Everything below is in T (the cloud's type) unless said otherwise, every
 * multiply and add rounded on its own, on the device and on the host alike;
 * only +, -, x, / and sqrt occur, so the two agree bit for bit.
 *   centre (:103-110)  each coordinate sum in fp64 over a fixed grid in a
 *     fixed order, divided by n in fp64, rounded to T.  The reference sums
 *     sequentially in T: the last bits of c may differ (divergence 1).
 *   L (:113-133)  torque_norm 0: 1.  1: the mean of sqrt((dx dx + dy dy) +
 *     dz dz), each term in T, the sum in fp64 (fixed order), divided by n,
 *     rounded to T.  2: half the largest of the three extents max - min, the
 *     reference's value exactly.
 *   v_i (:142-148, :169-173)  inv = T(1.0 / double(L)); v_i = [inv * ((p_i - c)
 *     x n_i) ; n_i], each cross-product component a * b - c * d.
 *   cov (:152)  the 21 upper-triangle sums of v_r * v_c, each product in T,
 *     accumulated in fp64 in a fixed order, then mirrored.
 *   basis  The reference takes the eigenvectors of Eigen's non-symmetric
 *     EigenSolver (:158-160), whose column order and signs are implementation-
 *     defined.  With basis NULL the library defines them (divergence 2): cyclic
 *     Jacobi on the symmetric cov in double on the host, eigenvalues ascending
 *     (list 0 serves the least constrained direction), each vector's largest
 *     component positive, rounded to T.  A supplied basis (36 doubles,
 *     row-major 6 x 6, column k is X_k, e.g. Eigen's) is rounded to T and used
 *     as given, in the caller's column order.
 *   projections (:189, :224)  m_k(i) = ((((v0 x0 + v1 x1) + v2 x2) + v3 x3) + v4
 *     x4) + v5 x5 with x = X_k; the reference's Eigen dot may add in another
 *     order (divergence 3).
 *   lists (:177-193)  list k holds the point indices by falling fabs(m_k), ties
 *     by rising index (std::list::sort is stable): a stable device sort on the
 *     inverted bit pattern of fabs(m).
 *   picks (:195-229), on the host, literally: t[6] in T from 0; k the first
 *     index of the smallest t; fronts of list k already sampled are dropped;
 *     the front is picked; t[j] += m_j * m_j for all six j with the picked
 *     point's signed projections.  Every entry read from a list is a distinct
 *     point that ends up sampled, so no list is read past position nb_sample
 *     and only that many entries of each list reach the host.
 *   columns (:233-249)  the picks move to the front by the swapCols / mapidx
 *     sequence of pmx_octree_grid's methods 0 and 1, stale lookups included.
 * Given the centre, L and basis, the selection and the output column order are
 * the reference's, bit for bit; report (may be NULL) returns those three as
 * used — center and lnorm as doubles holding T values, eigvec the basis after
 * rounding to T (row-major, column k is X_k) — with cov, eigval (the Jacobi
 * eigenvalues of cov, ascending, whichever basis is used) and depth, the
 * deepest 1-based list position read (<= nb_sample).  An early exit reports
 * zeros.
 * Also PMX_E_BAD_PARAM: nb_sample < 1; torque_norm outside 0..2; n >= 2^31; a
 * non-finite coordinate or normal, with a message naming the first such point;
 * L = 0 under torque_norm 1 or 2 (every point at the centroid); a supplied
 * basis with an entry that is not finite in T.  Projections that overflow T
 * are outside the contract.  The filter draws nothing from rand(); the GPU
 * runtime's own use of it is kept off the caller's state (initstate / setstate
 * around every HIP call, as pmx_normal_space).  No atomics: deterministic.
 * desc: desc_dim x n point-major; feat_out / desc_out hold n points.
 * Standalone like pmx_voxel_grid; pmx_last_error(NULL) on failure. */
typedef struct pmx_covs_report {
    double center[3];
    double lnorm;
    double cov[36];
    double eigval[6];
    double eigvec[36];
    int64_t depth;
} pmx_covs_report;
int pmx_covariance_sampling(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc,
                            int desc_dim, int normals_row, int64_t nb_sample, int torque_norm, const double* basis,
                            void* feat_out, void* desc_out, int64_t* n_out, pmx_covs_report* report);

/* IncidenceAngleDataPointsFilter (DataPointsFilters/IncidenceAngle.cpp:67-73):
 * angles[i] = acos(normalized(obs_i) . normal_i), in T: normalized() is a
 * sequential squared sum, a square root and a divide and leaves a zero vector
 * as it is (Eigen 3.3), the dot is a sequential sum, the normal is taken as it
 * comes.  normals, obs: span x n point-major T (span = 2 or 3, else
 * PMX_E_BAD_PARAM); angles_out: n values.  The device acos is within a few ulp
 * of the host library's, not bit-equal.  n = 0 is a result.  Standalone like
 * pmx_voxel_grid; pmx_last_error(NULL) on failure. */
int pmx_incidence_angles(int device, int dtype, const void* normals, const void* obs, int span, int64_t n,
                         void* angles_out);

/* SphericalityDataPointsFilter (DataPointsFilters/Sphericality.cpp:128-176):
 * per point the three eigenvalues sorted ascending (e0 <= e1 <= e2), then
 *   NaN for all three outputs when e2 < numeric_limits<T>::min(), e1 < 0 or e0 < 0,
 *   0 when e1 < numeric_limits<T>::min(),
 *   else unstructureness = e0 / e2, structureness = (e1 / e2) * ((e1 - e0) /
 *   sqrt(e0 * e0 + e1 * e1)), sphericality = unstructureness - structureness,
 * evaluated in T in that order: bit-identical to the reference (NaN
 * eigenvalues aside: their sort order is unspecified there).  eig_values:
 * 3 x n point-major T; sph_out: n values, always written; unstruct_out /
 * struct_out: n values each, written when flags asks (else may be NULL).
 * Standalone like pmx_voxel_grid; pmx_last_error(NULL) on failure. */
enum { PMX_SPH_UNSTRUCTURENESS = 1, PMX_SPH_STRUCTURENESS = 2 };
int pmx_sphericality(int device, int dtype, const void* eig_values, int64_t n, unsigned flags, void* sph_out,
                     void* unstruct_out, void* struct_out);

/* RemoveSensorBiasDataPointsFilter (DataPointsFilters/RemoveSensorBias.cpp:
 * 108-127; getCoefficients / diffDist / ratioCurvature :132-187; constants
 * RemoveSensorBias.h:94-113).  A point is kept when its incidence angle inc =
 * desc[inc_row] is not NaN, inc >= 0 and inc < angle_threshold — the caller
 * passes T(degrees / 180. * M_PI), compared in T.  A kept point moves along its
 * observation direction obs = desc[obs_row .. obs_row + D): p + T(correction) *
 * normalized(obs), correction = k1 * diffDist + k2 * ratioCurvature of the
 * depth |obs| (formed in T) and inc, in double except the tan / cos / sin of
 * inc, which are T calls as in the reference.  sensor_type: 0 Sick LMS-1xx,
 * 1 Velodyne HDL-32E.  The kept points come out in their input order with
 * their descriptors unchanged and the homogeneous row copied (the compaction
 * of pmx_keep_filter); the kept set is exact.  The correction cancels eight
 * digits, so for a double cloud sin / cos / tan of inc, erf and the two powers
 * are rounded once from double-double arithmetic (about 104 bits: correctly
 * rounded barring exact values within about 2^-100 of a rounding tie; inc in
 * [0, pi / 2], erf's argument up to 3, i.e. depths to some 60 m; the device
 * library's function beyond); a float cloud takes tanf / cosf / sinf.
 * feat_out / desc_out hold n points.  n = 0 and a kept count of 0 are
 * results.  PMX_E_BAD_PARAM for rows other than 3 or 4, inc_row or obs_row
 * (+ D rows) outside desc, a sensor_type outside {0, 1}.  Standalone like
 * pmx_voxel_grid; pmx_last_error(NULL) on failure. */
int pmx_remove_sensor_bias(int device, int dtype, const void* feat, int rows, int64_t n, const void* desc,
                           int desc_dim, int inc_row, int obs_row, int sensor_type, double angle_threshold,
                           void* feat_out, void* desc_out, int64_t* n_out);

/* ----------------------------------------------------- transformations --- */
/* Transformation::compute (PointMatcher.h Transformation; TransformationsImpl.cpp:
 * 49-87 RigidTransformation, :157-195 SimilarityTransformation, :215-231
 * PureTranslation) on a whole cloud: feat_out = params * feat, and R * d for
 * every listed descriptor span, R the top-left D x D block of params (D = rows
 * - 1).  It checks nothing of params: checkParameters is the caller's (the host
 * chain's Transformation classes, include/pmx_icp.h).
 *   feat        rows x n point-major T, rows 3 or 4
 *   params      rows x rows row-major T, as pmx_match's T_iter
 *   desc        desc_dim x n point-major T, or NULL with desc_dim 0
 *   span_rows   n_spans row offsets into desc, each naming D rows to rotate
 *               ("normals", "observationDirections"); at most
 *               PMX_TRANSFORM_MAX_SPANS, inside desc, not overlapping
 *   feat_out    rows x n; desc_out desc_dim x n (NULL with desc_dim 0).  An
 *               output may be its own input (identical or disjoint arrays).
 *   kernel_ms   (may be NULL) the kernel's own time from HIP events on the
 *               call's stream, without the copies
 * Every feature row r, the homogeneous one included, is ((P_r0 x + P_r1 y) +
 * P_r2 z) + P_r3 h, in 2-D (P_r0 x + P_r1 y) + P_r2 h; every span row the same
 * sequential sum over R's row; every multiply and add in T and rounded on its
 * own.  NaN and infinities go through the expression like any other value.
 * Descriptor rows outside the spans come out bit-identical: they are copied on
 * the host and never cross the bus.  n = 0 is a result.  PMX_E_BAD_PARAM for
 * rows other than 3 or 4, a span that leaves desc or overlaps another, spans
 * given without desc (desc_dim 0), more than PMX_TRANSFORM_MAX_SPANS spans;
 * the checks hold for an empty cloud too.  Standalone like pmx_voxel_grid;
 * pmx_last_error(NULL) on failure. */
enum { PMX_TRANSFORM_MAX_SPANS = 8 };
int pmx_transform_cloud(int device, int dtype, const void* feat, int rows, int64_t n, const void* params,
                        const void* desc, int desc_dim, const int* span_rows, int n_spans, void* feat_out,
                        void* desc_out, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* PMX_H */

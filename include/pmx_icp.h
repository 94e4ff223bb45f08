/*
 * pmx_icp.h — C ABI of the host ICP chain (libpmx_icp.so).
 *
 * A flat front-end over the C++ restatement of PointMatcher<T>::ICP
 * (libpointmatcher_amd/csrc/host/pm_icp.h) for non-C++ callers (the Python
 * tests and bench, a ctypes / cgo / JNI binding).  The chain is configured
 * exactly like the reference: ICPChainBase::setDefault (ICP.cpp:99-113) or a
 * libpointmatcher YAML chain (ICPChainBase::loadFromYaml, ICP.cpp:116-167).
 *
 * Clouds: rows x n point-major T arrays (rows = D + 1, homogeneous row last);
 * reference normals D x M point-major or NULL.  Transforms: rows x rows
 * row-major T.
 *
 * Errors: 0 on success, otherwise the negative code of the exception the
 * reference would throw; pmx_icp_last_error() holds its message.
 */
#ifndef PMX_ICP_H
#define PMX_ICP_H

#include <stdint.h>

#include "pmx.h" /* pmx_allreduce_fn / pmx_allgather_fn */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmx_icp pmx_icp;

enum {
    PMX_ICP_OK = 0,
    PMX_ICP_CONVERGENCE_ERROR = -1,   /* PointMatcher<T>::ConvergenceError */
    PMX_ICP_INVALID_PARAMETER = -3,   /* Parametrizable::InvalidParameter */
    PMX_ICP_TRANSFORMATION_ERROR = -4,/* TransformationError */
    PMX_ICP_INVALID_ELEMENT = -5,     /* InvalidElement (unknown module name) */
    PMX_ICP_INVALID_MODULE_TYPE = -6, /* ICPChainBase::InvalidModuleType */
    PMX_ICP_CONFIGURATION_ERROR = -7, /* ConfigurationError / YAML syntax */
    PMX_ICP_INVALID_FIELD = -8,       /* DataPoints::InvalidField (a data filter's missing descriptor) */
    PMX_ICP_RUNTIME_ERROR = -10       /* std::runtime_error (incl. HIP/RCCL failures) */
};

typedef struct pmx_icp_stats {
    int64_t iterations;            /* IterationsCount */
    int64_t point_count_touched;   /* PointCountTouched (pair evaluations) */
    double overlap_ratio;          /* OverlapRatio = weightedPointUsedRatio */
    double point_used_ratio;
    int64_t kept;                  /* ErrorElements columns of the last iteration */
    int64_t rejected_matches, rejected_points;
    double convergence_duration;   /* s, wall clock of the loop */
    double reference_preprocessing_duration;
    double reading_preprocessing_duration;
    int max_iterations_reached;
} pmx_icp_stats;

/* dtype: 0 = float, 1 = double; device: HIP ordinal */
int pmx_icp_create(int dtype, int device, pmx_icp** out);
void pmx_icp_destroy(pmx_icp* icp);
const char* pmx_icp_last_error(const pmx_icp* icp);

/* The parameter documentation of a registered outlier filter, one line per
 * parameter as the reference's Parametrizable dumps it (Parametrizable.cpp:51-74):
 * "- name (default: v) - doc[ - min: a][ - max: b]".  PMX_ICP_INVALID_ELEMENT for
 * an unknown name, PMX_ICP_INVALID_PARAMETER when cap is too small. */
int pmx_icp_outlier_filter_doc(int dtype, const char* name, char* out, int cap);
/* The same dump for a registered data points filter. */
int pmx_icp_data_points_filter_doc(int dtype, const char* name, char* out, int cap);
int pmx_icp_set_default(pmx_icp* icp);
int pmx_icp_load_yaml(pmx_icp* icp, const char* yaml_text);
/* multi-GPU: call before the first compute; uid from pmx_comm_unique_id */
int pmx_icp_comm_init(pmx_icp* icp, const void* uid128, int nranks, int rank);
/* multi-rank over the caller's host collectives (pmx_comm_init_host in pmx.h):
 * every rank passes its shard of the reading to compute/prepare */
int pmx_icp_comm_init_host(pmx_icp* icp, int nranks, int rank, pmx_allreduce_fn allreduce, pmx_allgather_fn allgather,
                           void* user);
int pmx_icp_keep_trace(pmx_icp* icp, int on);

/* ICP::compute (ICP.cpp:265-449): T_out = transform of reading into reference */
int pmx_icp_compute(pmx_icp* icp, const void* reading, int rows, int64_t N, const void* reference, int64_t M,
                    const void* ref_normals, const void* T_init, void* T_out);

/* DataPoints descriptors (PointMatcher.h:207-358) for the next compute /
 * prepare: cloud 0 = reading, 1 = reference; span rows x n points,
 * point-major, dtype of the ICP (e.g. the reading's "maxSearchDist" for
 * KDTreeVarDistMatcher).  Consumed by that call. */
int pmx_icp_add_descriptor(pmx_icp* icp, int cloud, const char* name, int span, const void* values, int64_t n);

/* DataPoints::load (IO.cpp:374-389; loadCSV :535-800, loadVTK :948-1252):
 * a .csv or .vtk cloud with the reference's label mapping; features
 * (rows x n, homogeneous row last) and descriptors (desc_dim x n), both
 * point-major.  Errors: PMX_ICP_RUNTIME_ERROR, message in
 * pmx_cloud_last_error(). */
typedef struct pmx_cloud pmx_cloud;
int pmx_cloud_load(const char* path, int dtype, pmx_cloud** out);
void pmx_cloud_destroy(pmx_cloud* cloud);
const char* pmx_cloud_last_error(void);
int pmx_cloud_info(const pmx_cloud* cloud, int64_t* n, int* rows, int* desc_dim, int* n_feature_labels,
                   int* n_descriptor_labels);
/* which: 0 feature labels, 1 descriptor labels */
int pmx_cloud_label(const pmx_cloud* cloud, int which, int i, char* name, int cap, int* span);
int pmx_cloud_data(const pmx_cloud* cloud, void* features, void* descriptors);

/* the same loop in phases (bench: time the iterations alone) */
int pmx_icp_prepare(pmx_icp* icp, const void* reading, int rows, int64_t N, const void* reference, int64_t M,
                    const void* ref_normals, const void* T_init);
/* run up to n iterations; *done = 1 once a checker stopped the loop */
int pmx_icp_iterate(pmx_icp* icp, int n, int* done);
int pmx_icp_finish(pmx_icp* icp, void* T_out);
/* the filtered reading moved by the last compute's result, T_out * readingFiltered,
 * in the caller's frame: rows x n; *n the filtered reading's size
 * (what transformation->compute(readingFiltered, T_out) returns for the
 * features; capacity in T values, at least n * rows; feat_out NULL: *n and
 * *rows alone, nothing is launched).  While the device still holds the
 * filtered reading (the device loop, or the module calls without
 * readingStepDataPointsFilters) nothing is uploaded: the device applies T_iter
 * to its resident reading, which the chain keeps centred on the reference
 * mean, and adds the mean back in the same kernel as one more separately
 * rounded step (pmx_transform_reading_offset, include/pmx.h); after a finished
 * device loop T_iter itself is read on the device.  Otherwise
 * pmx_transform_cloud runs on the host copy of the filtered reading with the
 * full T_out; the two agree within a few units in the last place of the
 * largest coordinate.  With a borrowed reading (pmx_icp_compute's arrays) the
 * host copy is the caller's array, which must then still be alive.
 * PMX_ICP_RUNTIME_ERROR before any compute (a state error). */
int pmx_icp_reading_transformed(pmx_icp* icp, void* feat_out, int64_t capacity, int64_t* n, int* rows);

int pmx_icp_stats_get(const pmx_icp* icp, pmx_icp_stats* out);
/* errorMinimizer->getCovariance() (PointMatcher.h:553, ErrorMinimizer.cpp:
 * 266-270) after a compute: 6 x 6 row-major T into cov36.  With
 * PointToPlaneWithCovErrorMinimizer the estimate of the last iteration,
 * sensorStdDev^2 H^-1 Q H^-1 (PointToPlaneWithCov.cpp:72-162; max * I for a
 * 2-D ICP, :91-92), computed once when the loop stops; zeros for every other
 * minimiser. */
int pmx_icp_covariance(pmx_icp* icp, void* cov36);
/* errorMinimizer->getOverlap() and getResidualError() (PointMatcher.h:552-554)
 * for the last iteration of the last compute.  The chain keeps the filtered
 * clouds' "simpleSensorNoise" (reading and reference, or the ICPSequence map)
 * and the reference's "densities" when present (from a data filter such as
 * SimpleSensorNoiseDataPointsFilter / SurfaceNormalDataPointsFilter, or
 * pmx_icp_add_descriptor); on the first call after the loop stopped they are
 * uploaded and the sums taken on the device from the match still resident
 * there (pmx_match_quality / pmx_loop_quality, include/pmx.h: the branches and
 * the one difference from the reference's scan), then cached until the next
 * prepare / set_map.  An ICP that never calls them launches nothing for them.
 * Without any noise descriptor the overlap is the weighted used ratio
 * (pmx_icp_stats.overlap_ratio, which always stays that ratio, ICP.cpp:435).
 * PointToPlane (and WithCov), PointToPoint and PointToPointSimilarity; any
 * other minimiser returns the base class's weighted used ratio and max().
 * Before a compute has stopped: PMX_ICP_RUNTIME_ERROR with the reference's
 * text (PointToPlane.cpp:384).  A multi-rank ICP calls them on every rank. */
int pmx_icp_overlap(pmx_icp* icp, double* overlap);
int pmx_icp_residual_error(pmx_icp* icp, double* residual);
/* errorMinimizer->getErrorElements() (PointMatcher.h:549-551, ErrorMinimizer.cpp:
 * 58-193): the pairs the last iteration of the last compute kept, one column
 * per pair, the reading index rising and the link rank rising within it.
 * Lazy like the two calls above: the first call after a checker stopped the ICP
 * compacts the match still resident on the device (pmx_error_elements_prepare /
 * pmx_loop_error_elements_prepare, include/pmx.h, by the path that ran), then
 * the result is cached until the next prepare / set_map; an ICP that never
 * asks launches and retains nothing.  Before any compute: zero columns and no
 * error (the reference's default-constructed lastErrorElements).  A chain that
 * kept nothing: PMX_ICP_CONVERGENCE_ERROR.  A multi-rank ICP returns its shard.
 *   pmx_icp_error_elements_info        columns, rows, the two descriptor
 *                                      dimensions and the rejected counts
 *   pmx_icp_error_elements             columns <= capacity (else
 *                                      PMX_ICP_INVALID_PARAMETER); any pointer may
 *                                      be NULL: reading / reference rows x P T
 *                                      (point-major, the reference's centred
 *                                      frame), dists, weights P T, ids (into the
 *                                      filtered reference), reading_index (into
 *                                      the filtered reading) P int32
 *   pmx_icp_error_elements_descriptor  one labelled descriptor of the columns,
 *                                      span x P T into out (capacity in
 *                                      values; out NULL: only *span, 0 when the
 *                                      cloud has no such descriptor); cloud 0
 *                                      reading, 1 reference
 * The descriptors are gathered from the filtered clouds of the last prepare
 * (with readingStepDataPointsFilters the last iteration's step reading; for a
 * sequence the held map); the reading's "normals" and "observationDirections"
 * are rotated by T_refMean_dataIn and the last match's T_iter, each component
 * (m0 n0 + m1 n1) + m2 n2 in T.  Arrays passed by pointer to prepare / compute
 * without a data filter on their side (the reference's normals) are read in
 * place at the first call: keep them valid until then. */
typedef struct pmx_icp_elements_info {
    int64_t columns;
    int rows, reading_desc_dim, reference_desc_dim;
    int64_t rejected_matches, rejected_points;
} pmx_icp_elements_info;
int pmx_icp_error_elements_info(pmx_icp* icp, pmx_icp_elements_info* info);
int pmx_icp_error_elements(pmx_icp* icp, int64_t capacity, void* reading, void* reference, void* dists, int32_t* ids,
                           void* weights, int32_t* reading_index);
int pmx_icp_error_elements_descriptor(pmx_icp* icp, int cloud, const char* name, void* out, int64_t capacity,
                                      int* span);
/* Inspection: the descriptor `name` of a cloud (rows x n, T) after the chain's
 * readingDataPointsFilters (cloud 0) or referenceDataPointsFilters (cloud 1),
 * with the descriptors staged for that cloud.  *n_out the filtered point count,
 * *span the descriptor's rows (0: absent); out (may be NULL to size) receives
 * n_out * span point-major T values, capacity in values.  Filters that run on
 * the GPU need one. */
int pmx_icp_filtered_descriptor(pmx_icp* icp, int cloud, const void* feat, int rows, int64_t n, const char* name,
                                void* out, int64_t capacity, int64_t* n_out, int* span);
/* T_iter after each iteration (rows x rows each), returns count written */
int pmx_icp_trace_get(const pmx_icp* icp, void* out, int max_iters);
/* HIP-event device time of the match kernel over the last iterations */
int pmx_icp_timing(pmx_icp* icp, int on);
int pmx_icp_timing_read(pmx_icp* icp, double* match_ms, int64_t* match_launches);
/* quantile window statistics of the device loop (pmx_loop_select_stats):
 * iterations since the last prepare whose TrimmedDist / MedianDist quantile
 * was resolved inside the match's key window, and iterations that ran the
 * radix passes.  Diagnostics only (no reference counterpart). */
int pmx_icp_select_stats(pmx_icp* icp, uint64_t* window_hits, uint64_t* window_misses);
/* per-iteration diagnostics of the device loop since the last prepare
 * (pmx_loop_diag): 4 int64 per iteration for iterations [first, first +
 * count).  Diagnostics only (no reference counterpart). */
int pmx_icp_loop_diag(pmx_icp* icp, int first, int count, int64_t* out);
/* multi-rank: the context's collectives and loop synchronisations since
 * creation (pmx_comm_stats, pmx_comm_loop_stats).  Diagnostics only. */
int pmx_icp_comm_stats(pmx_icp* icp, uint64_t* allreduces, uint64_t* allgathers, uint64_t* verdict_syncs,
                       uint64_t* async_iterations, uint64_t* stalls);

/* ICPSequence (PointMatcher.h:730-764, ICP.cpp:455-609).  set_map replaces
 * ICPSequence::setMap: the map is centred on its mean, filtered by the
 * referenceDataPointsFilters and indexed once; it stays resident on the
 * device.  accepted = 0 for an empty map (ignored, as the reference).
 * Descriptors staged with pmx_icp_add_descriptor(cloud = 1) go to the map.
 * sequence_compute replaces ICPSequence::compute(cloudIn, T_refIn_dataIn)
 * (T_init may be NULL: identity): the reading against the resident map; with
 * no map T_out is the identity.  sequence_prepare is its first phase
 * (prepared = 0 without a map), followed by pmx_icp_iterate / pmx_icp_finish.
 * get_map: the prefiltered map in global coordinates (ICP.cpp:543-554),
 * rows x n features, point-major, into `features` of `capacity` values;
 * features NULL returns n and rows only, a capacity below n * rows is
 * PMX_ICP_INVALID_PARAMETER (nothing written).  A load_yaml / set_default
 * re-indexes a held map (ICP.cpp:520-539). */
int pmx_icp_set_map(pmx_icp* icp, const void* map, int rows, int64_t M, const void* normals, int* accepted);
int pmx_icp_clear_map(pmx_icp* icp);
int pmx_icp_has_map(const pmx_icp* icp, int* has);
int pmx_icp_get_map(pmx_icp* icp, void* features, int64_t capacity, int64_t* n, int* rows);
int pmx_icp_sequence_prepare(pmx_icp* icp, const void* reading, int rows, int64_t N, const void* T_init,
                             int* prepared);
int pmx_icp_sequence_compute(pmx_icp* icp, const void* reading, int rows, int64_t N, const void* T_init,
                             void* T_out);

/* Transformation (PointMatcher.h; Transformation.cpp:60-79, TransformationsImpl.cpp:
 * 49-272): what the reference's applications call on the cloud once the ICP has
 * returned its parameters (transformation->compute(cloud, T)).  Registered
 * names: "RigidTransformation", "SimilarityTransformation", "PureTranslation";
 * any other is PMX_ICP_INVALID_ELEMENT.  A failed create leaves its message in
 * pmx_transformation_last_error(NULL) (per thread); every other call in the
 * handle's.  The ICP loop does not use these objects: its transform stays fused
 * into the match.
 *   check_parameters    *ok = checkParameters(params), params rows x rows
 *                       row-major T.  Rigid: |1 - det R| <= 0.001 in T;
 *                       Similarity: always 1; PureTranslation: the matrix with
 *                       its translation column zeroed isApprox(Identity)
 *                       (Eigen's rule: ||A - I||_F^2 <= p^2 min(||A||_F^2,
 *                       ||I||_F^2), p 1e-5 float / 1e-12 double).
 *   correct_parameters  out = correctParameters(params) (rows x rows).  Rigid
 *                       3-D: columns 1 and 2 normalised, c0 = c1 x c2, c1 = c2 x
 *                       c0; 2-D: a = (p00 + p11) / 2, b = (-p10 + p01) / 2, both
 *                       divided by sqrt(a a + b b), PMX_ICP_TRANSFORMATION_ERROR
 *                       when |p00 - p11| or |p10 + p01| exceeds 0.001 (a
 *                       reflection).  Similarity: params.  PureTranslation: the
 *                       left block the identity, the bottom row 0 .. 0 1.
 *                       Both are host arithmetic in T and need no GPU.
 *   compute             feat_out = params * feat on the device
 *                       (pmx_transform_cloud, include/pmx.h), and for Rigid and
 *                       Similarity the rotation block times every descriptor
 *                       labelled "normals" or "observationDirections"; every
 *                       other descriptor row, and with PureTranslation all of
 *                       them, bit-identical.  The descriptors come as
 *                       pmx_cloud_data returns them (desc_dim x n point-major)
 *                       with their labels as pmx_cloud_label lists them (names
 *                       and spans, the spans summing to desc_dim).  An output
 *                       may be its own input.  PMX_ICP_TRANSFORMATION_ERROR when
 *                       check_parameters refuses params (nothing is written),
 *                       PMX_ICP_INVALID_PARAMETER when params_rows != rows,
 *                       PMX_ICP_INVALID_FIELD for a rotated label whose span is
 *                       not rows - 1, PMX_ICP_RUNTIME_ERROR without a GPU. */
typedef struct pmx_transformation pmx_transformation;
int pmx_transformation_create(const char* name, int dtype, int device, pmx_transformation** out);
void pmx_transformation_destroy(pmx_transformation* t);
const char* pmx_transformation_last_error(const pmx_transformation* t);
int pmx_transformation_check_parameters(pmx_transformation* t, const void* params, int rows, int* ok);
int pmx_transformation_correct_parameters(pmx_transformation* t, const void* params, int rows, void* out);
int pmx_transformation_compute(pmx_transformation* t, const void* feat, int rows, int64_t n, const void* params,
                               int params_rows, const void* desc, int desc_dim, const char* const* label_names,
                               const int* label_spans, int n_labels, void* feat_out, void* desc_out);

#ifdef __cplusplus
}
#endif
#endif

"""ctypes binding of the C ABI in include/pmx.h (libpointmatcher_amd/lib/libpmx.so).

This is plumbing for Python callers (tests, bench, smoke): every call goes to
the HIP library.  There is no CPU fallback — if the library or a GPU is
missing, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(HERE, "lib")
# PMX_LIB_VARIANT: a kernel-variant build under lib/<variant>/ (tuning
# experiments through this module only; the host chain links lib/libpmx.so)
LIBPMX = os.path.join(LIBDIR, os.environ.get("PMX_LIB_VARIANT", ""), "libpmx.so")
LIBPMX_ICP = os.path.join(LIBDIR, "libpmx_icp.so")

PMX_F32, PMX_F64 = 0, 1
PMX_OK = 0
PMX_E_NO_POINTS = -1
PMX_E_EMPTY_QUANTILE = -2
PMX_E_BAD_PARAM = -3
PMX_E_TRANSFORMATION = -4
PMX_E_CONVERGENCE = -5
PMX_E_HIP = -10
PMX_E_RCCL = -11
PMX_E_STATE = -12
PMX_E_NO_DEVICE = -13


class ConvergenceError(RuntimeError):
    """PointMatcher<T>::ConvergenceError (pointmatcher/PointMatcher.h:83-87)."""


class InvalidParameter(RuntimeError):
    """Parametrizable::InvalidParameter (pointmatcher/Parametrizable.h:101-104)."""


class TransformationError(RuntimeError):
    """TransformationError (pointmatcher/PointMatcher.h:148-151)."""


class PmxError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [("kept", C.c_int64), ("nonzero_weights", C.c_int64),
                ("rejected_matches", C.c_int64), ("rejected_points", C.c_int64),
                ("sum_w", C.c_double), ("limit", C.c_double), ("n_total", C.c_int64),
                ("visited", C.c_int64), ("fallback_queries", C.c_int64)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# device-resident loop (pmx_loop_*)
FILTER_KIND = {"default": 0, "NullOutlierFilter": 1, "MaxDistOutlierFilter": 2, "MinDistOutlierFilter": 3,
               "MedianDistOutlierFilter": 4, "TrimmedDistOutlierFilter": 5, "VarTrimmedDistOutlierFilter": 6,
               "SurfaceNormalOutlierFilter": 8, "GenericDescriptorOutlierFilter": 9}  # (9: filter_p[i] = soft, larger_than, threshold)
CHECK_KIND = {"CounterTransformationChecker": 0, "DifferentialTransformationChecker": 1,
              "BoundTransformationChecker": 2}


class LoopCfg(C.Structure):
    _fields_ = [("knn", C.c_int), ("max_dist", C.c_double), ("n_filters", C.c_int),
                ("filter_kind", C.c_int * 8), ("filter_p", (C.c_double * 3) * 8), ("minimizer", C.c_int),
                ("n_checkers", C.c_int), ("checker_kind", C.c_int * 8), ("checker_p", (C.c_double * 3) * 8),
                ("keep_trace", C.c_int),
                # PMX_FILTER_ROBUST (include/pmx.h)
                ("robust_fct", C.c_int), ("robust_estimator", C.c_int), ("robust_p2pl", C.c_int),
                ("robust_nb_iter_for_scale", C.c_int), ("robust_first_call", C.c_int),
                ("robust_tuning", C.c_double), ("robust_approx", C.c_double), ("robust_berg_target", C.c_double),
                # PMX_FORCE_* of PointToPlane
                ("force", C.c_int)]


class LoopStatus(C.Structure):
    _fields_ = [("iterations", C.c_int), ("done", C.c_int), ("reason", C.c_int), ("error", C.c_int),
                ("point_count_touched", C.c_int64), ("last", Stats), ("T_iter", C.c_double * 16),
                ("cond", (C.c_double * 2) * 8)]


# host-staged collectives (pmx_comm_init_host)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
COLL_F64, COLL_U32, COLL_U64 = 0, 1, 2
COLL_SUM, COLL_MAX = 0, 1
_COLL_CT = {COLL_F64: C.c_double, COLL_U32: C.c_uint32, COLL_U64: C.c_uint64}


class HostComm:
    """A transport for pmx_comm_init_host: allreduce(np_array, op) reduces the
    array in place over the ranks ("sum" / "max"), allgather(np_uint8_array)
    returns the nranks concatenated blocks.  The ctypes callbacks stay alive
    with this object (keep it referenced for the life of the context)."""

    def __init__(self, nranks, rank, allreduce, allgather):
        self.nranks, self.rank = nranks, rank
        self.errors = []
        self.calls = {"allreduce": 0, "allgather": 0}  # (callbacks made, every context on this transport)

        def _ar(user, buf, count, typ, op):
            self.calls["allreduce"] += 1
            try:
                a = np.ctypeslib.as_array(C.cast(buf, C.POINTER(_COLL_CT[typ])), shape=(count,))
                allreduce(a, "max" if op == COLL_MAX else "sum")
                return 0
            except Exception as e:  # (an exception must not cross the C frame)
                self.errors.append(repr(e))
                return 1

        def _ag(user, send, recv, nbytes):
            self.calls["allgather"] += 1
            try:
                a = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,))
                out = np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(nbytes * nranks,))
                out[:] = allgather(a.copy())
                return 0
            except Exception as e:
                self.errors.append(repr(e))
                return 1

        self.ar = ALLREDUCE_FN(_ar)
        self.ag = ALLGATHER_FN(_ag)


def gloo_host_comm():
    """HostComm over the default torch.distributed process group (gloo on the
    CPU): the multi-rank test path on one GPU.  Integers travel as int64."""
    import torch
    import torch.distributed as dist

    def allreduce(a, op):
        t = torch.from_numpy(a.astype(np.float64) if a.dtype == np.float64 else a.astype(np.int64))
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)
        a[:] = t.numpy().astype(a.dtype)

    def allgather(a):
        t = torch.from_numpy(a)
        outs = [torch.empty_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(outs, t)
        return torch.cat(outs).numpy()

    return HostComm(dist.get_world_size(), dist.get_rank(), allreduce, allgather)


class Quality(C.Structure):
    """pmx_quality (include/pmx.h): getResidualError / getOverlap's sums."""
    _fields_ = [("residual", C.c_double), ("overlap_num", C.c_int64), ("overlap_den", C.c_int64),
                ("links", C.c_int64), ("dist_sum", C.c_double), ("median_density", C.c_double), ("branch", C.c_int)]


class ElementsInfo(C.Structure):
    """pmx_elements_info (include/pmx.h): the counts of a prepared getErrorElements."""
    _fields_ = [("columns", C.c_int64), ("rejected_matches", C.c_int64), ("rejected_points", C.c_int64)]


class ErrorElements:
    """ErrorMinimizer::getErrorElements' columns as numpy arrays (pmx_error_elements):
    reading / reference (P, rows), ref_normals (P, rows - 1) or None, dists, weights
    (P,), ids, reading_index, link_rank (P,) int32, and the two rejected counts."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def columns(self):
        return len(self.dists)


FORCE_KIND = {None: 0, "none": 0, "2D": 1, "4DOF": 2}  # PMX_FORCE_*

MINIMIZER_KIND = {"PointToPlaneErrorMinimizer": 0, "PointToPointErrorMinimizer": 1,
                  "PointToPlaneWithCovErrorMinimizer": 2, "PointToPointSimilarityErrorMinimizer": 3}

_lib = None

EXPORTS = [
    "pmx_ctx_create", "pmx_ctx_destroy", "pmx_ctx_set_option", "pmx_last_error", "pmx_device_count", "pmx_version",
    "pmx_comm_unique_id", "pmx_comm_init", "pmx_comm_init_host", "pmx_comm_size", "pmx_comm_stats", "pmx_comm_loop_stats", "pmx_set_reference", "pmx_set_reference_centred", "pmx_set_reference_mean_centred", "pmx_set_reading", "pmx_set_search", "pmx_match",
    "pmx_outlier_default", "pmx_outlier_null", "pmx_outlier_maxdist", "pmx_outlier_mindist",
    "pmx_outlier_mediandist", "pmx_outlier_trimmed", "pmx_outlier_vartrimmed", "pmx_outlier_robust",
    "pmx_robust_scale", "pmx_set_reading_radii", "pmx_set_reading_normals", "pmx_outlier_surface_normal",
    "pmx_set_reference_weight_descriptor", "pmx_outlier_generic_descriptor",
    "pmx_p2plane_system", "pmx_p2plane_system_forced", "pmx_p2point_system", "pmx_p2point_similarity_system", "pmx_p2plane_covariance", "pmx_loop_covariance", "pmx_set_reading_noise", "pmx_set_reference_descriptors", "pmx_match_quality", "pmx_loop_quality",
    "pmx_get_step_transform", "pmx_error_elements_prepare", "pmx_error_elements", "pmx_loop_error_elements_prepare", "pmx_get_matches", "pmx_get_weights", "pmx_vartrim_partial_sums",
    "pmx_get_shape", "pmx_grid_level_records", "pmx_timing_enable", "pmx_timing_read", "pmx_sync",
    "pmx_loop_begin", "pmx_loop_run", "pmx_loop_trace", "pmx_loop_select_stats", "pmx_loop_diag", "pmx_surface_normals",
    "pmx_sampling_surface_normals", "pmx_voxel_grid", "pmx_keep_filter", "pmx_octree_grid",
    "pmx_normal_space", "pmx_covariance_sampling",
    "pmx_incidence_angles", "pmx_sphericality", "pmx_remove_sensor_bias", "pmx_transform_cloud",
    "pmx_transform_reading", "pmx_transform_reading_offset",
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPMX):
            raise PmxError(f"{LIBPMX} not built (run __graft_entry__.build() or make -C libpointmatcher_amd)")
        l = C.CDLL(LIBPMX, mode=C.RTLD_GLOBAL)
        l.pmx_last_error.restype = C.c_char_p
        l.pmx_version.restype = C.c_char_p
        l.pmx_last_error.argtypes = [C.c_void_p]
        l.pmx_ctx_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.pmx_ctx_destroy.argtypes = [C.c_void_p]
        l.pmx_ctx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        l.pmx_comm_unique_id.argtypes = [C.c_void_p]
        l.pmx_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        l.pmx_comm_init_host.argtypes = [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, ALLGATHER_FN, C.c_void_p]
        l.pmx_comm_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pmx_comm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        l.pmx_comm_loop_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        l.pmx_set_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        l.pmx_set_reference_centred.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        l.pmx_set_reference_mean_centred.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                                     C.c_void_p]
        l.pmx_set_reading.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        l.pmx_set_search.argtypes = [C.c_void_p, C.c_int]
        l.pmx_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                C.POINTER(C.c_uint64)]
        l.pmx_outlier_default.argtypes = [C.c_void_p]
        l.pmx_outlier_null.argtypes = [C.c_void_p, C.c_int]
        for f in ("maxdist", "mindist", "mediandist", "trimmed"):
            getattr(l, "pmx_outlier_" + f).argtypes = [C.c_void_p, C.c_int, C.c_double]
        l.pmx_outlier_vartrimmed.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
        l.pmx_outlier_robust.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                         C.c_int]
        l.pmx_robust_scale.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        l.pmx_set_reading_radii.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_set_reading_normals.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_outlier_surface_normal.argtypes = [C.c_void_p, C.c_int, C.c_double]
        l.pmx_set_reference_weight_descriptor.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_outlier_generic_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
        l.pmx_p2plane_system.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        l.pmx_p2plane_system_forced.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        l.pmx_p2point_system.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(Stats)]
        l.pmx_p2point_similarity_system.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(C.c_double), C.POINTER(Stats)]
        l.pmx_p2plane_covariance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        l.pmx_loop_covariance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        l.pmx_set_reading_noise.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_set_reference_descriptors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pmx_match_quality.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Quality)]
        l.pmx_loop_quality.argtypes = [C.c_void_p, C.c_int, C.POINTER(Quality)]
        l.pmx_get_step_transform.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_error_elements_prepare.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ElementsInfo)]
        l.pmx_error_elements.argtypes = [C.c_void_p] * 9
        l.pmx_loop_error_elements_prepare.argtypes = [C.c_void_p, C.POINTER(ElementsInfo)]
        l.pmx_get_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pmx_get_weights.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_vartrim_partial_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        l.pmx_get_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        l.pmx_grid_level_records.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        l.pmx_timing_enable.argtypes = [C.c_void_p, C.c_int]
        l.pmx_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_double)]
        l.pmx_sync.argtypes = [C.c_void_p]
        l.pmx_loop_begin.argtypes = [C.c_void_p, C.POINTER(LoopCfg), C.c_void_p]
        l.pmx_loop_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(LoopStatus)]
        l.pmx_loop_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        l.pmx_loop_select_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        l.pmx_loop_diag.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        l.pmx_surface_normals.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_double,
                                          C.c_uint] + [C.c_void_p] * 6 + [C.POINTER(C.c_int64)]
        l.pmx_voxel_grid.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                     C.POINTER(C.c_double), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_int64)]
        l.pmx_keep_filter.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        l.pmx_octree_grid.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64,
                                      C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        l.pmx_normal_space.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int64, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        l.pmx_covariance_sampling.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                              C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int64), C.POINTER(CovsReport)]
        l.pmx_incidence_angles.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        l.pmx_sphericality.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_uint, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
        l.pmx_remove_sensor_bias.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_int64)]
        l.pmx_transform_cloud.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_double)]
        l.pmx_transform_reading.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pmx_transform_reading_offset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pmx_sampling_surface_normals.argtypes = ([C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                                    C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint]
                                                   + [C.c_void_p] * 6 + [C.POINTER(C.c_int64)] * 2)
        _lib = l
    return _lib


def device_count():
    return lib().pmx_device_count()


PMX_SN_SMOOTH = 1


def surface_normals(points, knn=5, max_dist=np.inf, smooth=False, device=0):
    """SurfaceNormalDataPointsFilter (DataPointsFilters/SurfaceNormal.cpp:80-290) on
    the GPU (pmx_surface_normals).  points: (n, rows) float32/float64 with the
    homogeneous row last.  Returns a dict of point-major arrays: normals (n, D),
    densities (n,), eig_values (n, D), eig_vectors (n, D*D), matched_ids (n, knn),
    mean_dists (n,), and the degenerate count."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    n, rows = pts.shape
    D = rows - 1
    dt = pts.dtype
    out = {"normals": np.empty((n, D), dt), "densities": np.empty(n, dt), "eig_values": np.empty((n, D), dt),
           "eig_vectors": np.empty((n, D * D), dt), "matched_ids": np.empty((n, knn), dt),
           "mean_dists": np.empty(n, dt)}
    deg = C.c_int64(0)
    l = lib()
    rc = l.pmx_surface_normals(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n, int(knn),
                               float(max_dist), PMX_SN_SMOOTH if smooth else 0, _ptr(out["normals"]),
                               _ptr(out["densities"]), _ptr(out["eig_values"]), _ptr(out["eig_vectors"]),
                               _ptr(out["matched_ids"]), _ptr(out["mean_dists"]), C.byref(deg))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    out["degenerate"] = deg.value
    return out


SSN_NORMALS, SSN_DENSITIES, SSN_EIGVALUES, SSN_EIGVECTORS, SSN_AVERAGE = 1, 2, 4, 8, 16
# RobustOutlierFilter functions / scale modes of one call (include/pmx.h PMX_RF_*, PMX_RS_*)
ROBUST_FCT = {"cauchy": 0, "welsch": 1, "sc": 2, "gm": 3, "tukey": 4, "huber": 5, "L1": 6, "student": 7}
RS_NONE, RS_MAD, RS_STD, RS_BERG_FIRST, RS_BERG_NEXT, RS_KEEP = range(6)


def sampling_surface_normals(points, descriptors=None, knn=7, sampling_method=0, ratio=0.5, max_box_dim=np.inf,
                             flags=SSN_NORMALS | SSN_AVERAGE, device=0):
    """SamplingSurfaceNormalDataPointsFilter (DataPointsFilters/SamplingSurfaceNormal.cpp:80-342)
    on the GPU (pmx_sampling_surface_normals).  points (n, rows) with the
    homogeneous row last; descriptors (n, desc_dim) or None.  Returns the kept
    points' features, descriptors, normals, densities, eig_values,
    eig_vectors (point-major) and the unfit count."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    D = rows - 1
    dd = 0 if descriptors is None else descriptors.shape[1]
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    out = {"features": np.empty((n, rows), dt), "descriptors": np.empty((n, dd), dt),
           "normals": np.empty((n, D), dt), "densities": np.empty(n, dt), "eig_values": np.empty((n, D), dt),
           "eig_vectors": np.empty((n, D * D), dt)}
    no, unfit = C.c_int64(0), C.c_int64(0)
    l = lib()
    rc = l.pmx_sampling_surface_normals(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n,
                                        _ptr(desc), dd, int(knn), int(sampling_method), float(ratio),
                                        float(max_box_dim), int(flags), _ptr(out["features"]),
                                        _ptr(out["descriptors"]) if dd else None, _ptr(out["normals"]),
                                        _ptr(out["densities"]), _ptr(out["eig_values"]), _ptr(out["eig_vectors"]),
                                        C.byref(no), C.byref(unfit))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    m = no.value
    res = {k: v[:m] for k, v in out.items()}
    res["unfit"] = unfit.value
    return res


def voxel_grid(points, descriptors=None, vsize=(1.0, 1.0, 1.0), use_centroid=True, average_descriptors=True,
               device=0):
    """VoxelGridDataPointsFilter (DataPointsFilters/VoxelGrid.cpp:60-343) on the
    GPU (pmx_voxel_grid).  points (n, rows) with the homogeneous row last;
    descriptors (n, desc_dim) or None.  Returns (features, descriptors) of
    the kept points, in index order."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    dd = 0 if descriptors is None else descriptors.shape[1]
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    of = np.empty((n, rows), dt)
    od = np.empty((n, dd), dt)
    vs = (C.c_double * 3)(*[float(v) for v in vsize])
    no = C.c_int64(0)
    l = lib()
    rc = l.pmx_voxel_grid(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n, _ptr(desc), dd,
                          vs, 1 if use_centroid else 0, 1 if average_descriptors else 0, _ptr(of),
                          _ptr(od) if dd else None, C.byref(no))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return of[:no.value], od[:no.value]


TRANSFORM_MAX_SPANS = 8  # PMX_TRANSFORM_MAX_SPANS


def transform_cloud(points, params, descriptors=None, spans=(), device=0, in_place=False, timing=False):
    """Transformation::compute on the GPU (pmx_transform_cloud): params * points,
    and the rotation block of params times every descriptor span listed in
    spans (row offsets, D = rows - 1 rows each).  points (n, rows) with the
    homogeneous row last, params (rows, rows), descriptors (n, desc_dim) or
    None.  Returns (features, descriptors or None), with timing=True also the
    kernel's own milliseconds.  in_place: the outputs are the (contiguous,
    float32 / float64) input arrays themselves.  It checks nothing of params:
    icp.Transformation does."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    P = np.ascontiguousarray(params, dtype=dt)
    if P.shape != (rows, rows):
        raise InvalidParameter(f"params must be ({rows}, {rows}), not {P.shape}")
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    dd = 0 if desc is None else desc.shape[1]
    if in_place:
        if pts is not points or (desc is not None and desc is not descriptors):
            raise InvalidParameter("in_place needs contiguous float32 / float64 arrays of one dtype")
        of, od = pts, desc
    else:
        of = np.empty((n, rows), dt)
        od = None if desc is None else np.empty((n, dd), dt)
    sp = (C.c_int * max(len(spans), 1))(*[int(s) for s in spans])
    ms = C.c_double(0.0)
    l = lib()
    rc = l.pmx_transform_cloud(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n, _ptr(P),
                               _ptr(desc), dd, sp, len(spans), _ptr(of), _ptr(od), C.byref(ms) if timing else None)
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return (of, od, ms.value) if timing else (of, od)


KEEP_SHADOW, KEEP_MAX_QUANTILE, KEEP_REMOVE_NAN, KEEP_CUT_DESCRIPTOR = range(4)  # PMX_KEEP_*


def keep_filter(points, descriptors, predicate, index=0, flag=0, value=0.0, device=0):
    """The keep-filters on the GPU (pmx_keep_filter, pmx_keep.hip): Shadow
    (Shadow.cpp:62-94; index = row offset of the normals in descriptors, value
    = sin(eps) in the cloud's type), MaxQuantileOnAxis (MaxQuantileOnAxis.cpp:
    65-98; index = dim, value = ratio), RemoveNaN (RemoveNaN.cpp:47-66) and
    CutAtDescriptorThreshold (CutAtDescriptorThreshold.cpp:61-102; index =
    descriptor row, flag = useLargerThan, value = threshold).  points (n, rows)
    with the homogeneous row last; descriptors (n, desc_dim) or None.  Returns
    (features, descriptors) of the kept points, in their input order."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    dd = 0 if descriptors is None else descriptors.shape[1]
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    of = np.empty((n, rows), dt)
    od = np.empty((n, dd), dt)
    no = C.c_int64(0)
    l = lib()
    rc = l.pmx_keep_filter(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n,
                           _ptr(desc) if dd else None, dd, int(predicate), int(index), int(flag), float(value),
                           _ptr(of), _ptr(od) if dd else None, C.byref(no))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return of[:no.value], od[:no.value]


OCTREE_FIRST, OCTREE_RANDOM, OCTREE_CENTROID, OCTREE_MEDOID = range(4)  # samplingMethod


def octree_grid(points, descriptors=None, max_point_by_node=1, max_size_by_node=0.0, sampling_method=OCTREE_FIRST,
                device=0):
    """OctreeGridDataPointsFilter (DataPointsFilters/OctreeGrid.cpp:48-366,
    utils/octree.hpp:229-385) on the GPU (pmx_octree_grid, pmx_octree.hip): one
    point per non-empty leaf of the octree (rows 4) or quadtree (rows 3), in
    the reference's visit order.  sampling_method 0 first, 1 random (draws
    from the process's rand() state between two srand(1)), 2 centroid, 3
    medoid; 0 and 1 are bit-identical to the reference, 2 and 3 are computed
    per leaf from the input cloud (include/pmx.h).  points (n, rows) with the
    homogeneous row last; descriptors (n, desc_dim) or None.  Returns
    (features, descriptors) of the kept points."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    dd = 0 if descriptors is None else descriptors.shape[1]
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    of = np.empty((n, rows), dt)
    od = np.empty((n, dd), dt)
    no = C.c_int64(0)
    l = lib()
    rc = l.pmx_octree_grid(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n,
                           _ptr(desc) if dd else None, dd, int(max_point_by_node), float(max_size_by_node),
                           int(sampling_method), _ptr(of), _ptr(od) if dd else None, C.byref(no))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return of[:no.value], od[:no.value]


def normal_space(points, descriptors, normals_row=0, nb_sample=5000, seed=1, epsilon=0.09817477042, device=0):
    """NormalSpaceDataPointsFilter (DataPointsFilters/NormalSpace.cpp:47-181) on
    the GPU (pmx_normal_space, pmx_nss.hip): nb_sample points drawn from the
    buckets of the normals' directions, bit-identical to the reference, column
    order included.  The shuffle draws n - 1 times from the process's rand()
    state; seed feeds the mt19937 of the picks; epsilon is cast to the cloud's
    type.  points (n, rows) with the homogeneous row last; descriptors
    (n, desc_dim) holding the normals at columns normals_row .. normals_row + 2.
    A 2-D cloud, nb_sample >= n and n = 0 return the cloud as it is.  Returns
    (features, descriptors, n_recheck): n_recheck points were evaluated on the
    host because the device could not certify their bucket (include/pmx.h)."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    dd = 0 if descriptors is None else descriptors.shape[1]
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    of = np.empty((n, rows), dt)
    od = np.empty((n, dd), dt)
    no, nr = C.c_int64(0), C.c_int64(0)
    l = lib()
    rc = l.pmx_normal_space(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n,
                            _ptr(desc) if dd else None, dd, int(normals_row), int(nb_sample), int(seed),
                            float(epsilon), _ptr(of), _ptr(od) if dd else None, C.byref(no), C.byref(nr))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return of[:no.value], od[:no.value], nr.value


class CovsReport(C.Structure):
    """pmx_covs_report of include/pmx.h."""
    _fields_ = [("center", C.c_double * 3), ("lnorm", C.c_double), ("cov", C.c_double * 36),
                ("eigval", C.c_double * 6), ("eigvec", C.c_double * 36), ("depth", C.c_int64)]


def covariance_sampling(points, descriptors, normals_row=0, nb_sample=5000, torque_norm=1, basis=None, device=0):
    """CovarianceSamplingDataPointsFilter (DataPointsFilters/CovarianceSampling.cpp:
    74-250) on the GPU (pmx_covariance_sampling, pmx_covs.hip): the nb_sample
    points that best constrain the six degrees of freedom of the point-to-plane
    system.  torque_norm 0 L = 1, 1 L = the mean distance from the centroid,
    2 L = half the largest extent.  basis: None for the library's own (Jacobi on
    the symmetric covariance, eigenvalues ascending, largest component positive)
    or a (6, 6) array whose column k is X_k, used as given after rounding to the
    cloud's type.  points (n, 4) with the homogeneous row last; descriptors
    (n, desc_dim) holding the normals at columns normals_row .. normals_row + 2.
    nb_sample >= n and n = 0 return the cloud as it is.  Returns (features,
    descriptors, report): report is a dict of center (3,), lnorm, cov (6, 6),
    eigval (6,), eigvec (6, 6) — the centre, L and basis as used — and depth,
    the deepest list position read (include/pmx.h).  eigval always holds the
    library's own eigenvalues of cov, ascending: with a supplied basis it does
    not correspond to the columns of eigvec."""
    pts = np.ascontiguousarray(points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    dt = pts.dtype
    n, rows = pts.shape
    dd = 0 if descriptors is None else descriptors.shape[1]
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    of = np.empty((n, rows), dt)
    od = np.empty((n, dd), dt)
    no = C.c_int64(0)
    rep = CovsReport()
    X = None
    if basis is not None:
        X = np.ascontiguousarray(basis, dtype=np.float64)
        if X.shape != (6, 6):
            raise InvalidParameter("covariance_sampling: the basis must be (6, 6), column k the vector X_k")
    l = lib()
    rc = l.pmx_covariance_sampling(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n,
                                   _ptr(desc) if dd else None, dd, int(normals_row), int(nb_sample), int(torque_norm),
                                   _ptr(X) if X is not None else None, _ptr(of), _ptr(od) if dd else None,
                                   C.byref(no), C.byref(rep))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    report = dict(center=np.array(rep.center), lnorm=float(rep.lnorm), cov=np.array(rep.cov).reshape(6, 6),
                  eigval=np.array(rep.eigval), eigvec=np.array(rep.eigvec).reshape(6, 6), depth=int(rep.depth))
    return of[:no.value], od[:no.value], report


def _float_array(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float32)
    return a


def incidence_angles(normals, observation_directions, device=0):
    """IncidenceAngleDataPointsFilter (IncidenceAngle.cpp:67-73) on the GPU
    (pmx_incidence_angles, pmx_sensor.hip): acos(normalized(obs) . normal) per
    point, in the arrays' type.  normals, observation_directions: (n, span),
    span 2 or 3.  Returns (n,)."""
    nrm = _float_array(normals)
    obs = _float_array(observation_directions, nrm.dtype)
    if nrm.ndim != 2 or obs.shape != nrm.shape:
        raise InvalidParameter("incidence_angles: normals and observation directions must be (n, span) alike")
    n, span = nrm.shape
    out = np.empty(n, nrm.dtype)
    l = lib()
    rc = l.pmx_incidence_angles(int(device), PMX_F64 if nrm.dtype == np.float64 else PMX_F32, _ptr(nrm), _ptr(obs),
                                span, n, _ptr(out))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return out


SPH_UNSTRUCTURENESS, SPH_STRUCTURENESS = 1, 2  # PMX_SPH_*


def sphericality(eig_values, keep_unstructureness=False, keep_structureness=False, device=0):
    """SphericalityDataPointsFilter (Sphericality.cpp:128-176) on the GPU
    (pmx_sphericality, pmx_sensor.hip).  eig_values: (n, 3), in any order.
    Returns a dict of (n,) arrays: sphericality, and unstructureness /
    structureness when asked."""
    ev = _float_array(eig_values)
    if ev.ndim != 2 or ev.shape[1] != 3:
        raise InvalidParameter("sphericality: eig_values must be (n, 3)")
    n, dt = ev.shape[0], ev.dtype
    out = {"sphericality": np.empty(n, dt)}
    if keep_unstructureness:
        out["unstructureness"] = np.empty(n, dt)
    if keep_structureness:
        out["structureness"] = np.empty(n, dt)
    flags = (SPH_UNSTRUCTURENESS if keep_unstructureness else 0) | (SPH_STRUCTURENESS if keep_structureness else 0)
    l = lib()
    rc = l.pmx_sphericality(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(ev), n, flags,
                            _ptr(out["sphericality"]), _ptr(out.get("unstructureness")),
                            _ptr(out.get("structureness")))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return out


def angle_threshold(degrees, dtype):
    """RemoveSensorBias's constructor (RemoveSensorBias.cpp:52): T(T(degrees) / 180. * M_PI)."""
    T = np.dtype(dtype).type
    return T(float(T(degrees)) / 180. * math.pi)


def remove_sensor_bias(points, descriptors, inc_row, obs_row, sensor_type=0, angle_threshold_deg=88.0, device=0):
    """RemoveSensorBiasDataPointsFilter (RemoveSensorBias.cpp:108-187) on the GPU
    (pmx_remove_sensor_bias, pmx_sensor.hip).  points (n, rows) with the
    homogeneous row last; descriptors (n, desc_dim) holding the incidence
    angle in column inc_row and the observation direction in columns obs_row ..
    obs_row + D; sensor_type 0 (LMS-1xx) or 1 (HDL-32E).  Returns (features,
    descriptors) of the kept points, corrected, in their input order."""
    pts = _float_array(points)
    dt = pts.dtype
    if pts.ndim != 2:
        raise InvalidParameter("remove_sensor_bias: points must be (n, rows)")
    n, rows = pts.shape
    desc = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=dt)
    if desc is not None and (desc.ndim != 2 or desc.shape[0] != n):
        raise InvalidParameter("remove_sensor_bias: descriptors must be (n, desc_dim) for the n points")
    dd = 0 if desc is None else desc.shape[1]
    of = np.empty((n, rows), dt)
    od = np.empty((n, dd), dt)
    no = C.c_int64(0)
    l = lib()
    rc = l.pmx_remove_sensor_bias(int(device), PMX_F64 if dt == np.float64 else PMX_F32, _ptr(pts), rows, n,
                                  _ptr(desc) if dd else None, dd, int(inc_row), int(obs_row), int(sensor_type),
                                  float(angle_threshold(angle_threshold_deg, dt)), _ptr(of), _ptr(od) if dd else None,
                                  C.byref(no))
    if rc != PMX_OK:
        raise_for(rc, l.pmx_last_error(None).decode())
    return of[:no.value], od[:no.value]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raise_for(code, msg=""):
    if code == PMX_OK:
        return
    if code in (PMX_E_NO_POINTS, PMX_E_EMPTY_QUANTILE, PMX_E_CONVERGENCE):
        raise ConvergenceError(msg)
    if code == PMX_E_BAD_PARAM:
        raise InvalidParameter(msg)
    if code == PMX_E_TRANSFORMATION:
        raise TransformationError(msg)
    raise PmxError(f"pmx error {code}: {msg}")


class Context:
    """One device context (one ICP object / one rank)."""

    def __init__(self, device=0, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self._l = lib()
        h = C.c_void_p()
        rc = self._l.pmx_ctx_create(device, PMX_F64 if self.dtype == np.float64 else PMX_F32, C.byref(h))
        if rc != PMX_OK:
            raise PmxError(f"pmx_ctx_create failed ({rc}: {self._l.pmx_last_error(None).decode()}); "
                           f"visible HIP devices: {device_count()}")
        self.h = h
        self.rows = None
        self.knn = None
        self.N = 0

    def set_option(self, name, value):
        """One developer option (README "Options"; pmx_ctx_set_option)."""
        self._chk(self._l.pmx_ctx_set_option(self.h, str(name).encode(), str(value).encode()))

    def level_records(self, level, normals=True):
        """Grid level `level`'s records (pmx_grid_level_records): original
        reference ids, points (n, 4) and, with normals, normals (n, 4)."""
        n = C.c_int64(0)
        self._chk(self._l.pmx_grid_level_records(self.h, int(level), C.byref(n), None, None, None))
        ids = np.zeros(n.value, np.int32)
        pts = np.zeros((n.value, 4), self.dtype)
        nrm = np.zeros((n.value, 4), self.dtype) if normals else None
        self._chk(self._l.pmx_grid_level_records(self.h, int(level), C.byref(n), _ptr(ids), _ptr(pts),
                                                 _ptr(nrm) if normals else None))
        return ids, pts, nrm

    def close(self):
        if self.h:
            self._l.pmx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != PMX_OK:
            raise_for(rc, self._l.pmx_last_error(self.h).decode())

    def _arr(self, a):
        return np.ascontiguousarray(a, dtype=self.dtype)

    # --- multi-GPU
    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        rc = lib().pmx_comm_unique_id(buf)
        if rc != PMX_OK:
            raise PmxError(f"pmx_comm_unique_id failed ({rc})")
        return bytes(buf)

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = (C.c_char * 128).from_buffer_copy(uid)
        self._chk(self._l.pmx_comm_init(self.h, buf, nranks, rank))

    def comm_init_host(self, comm: HostComm):
        self._comm = comm  # (the callbacks must outlive the context)
        self._chk(self._l.pmx_comm_init_host(self.h, comm.nranks, comm.rank, comm.ar, comm.ag, None))

    def comm_size(self):
        n, r, k = C.c_int(), C.c_int(), C.c_int()
        self._chk(self._l.pmx_comm_size(self.h, C.byref(n), C.byref(r), C.byref(k)))
        return n.value, r.value, k.value

    def comm_stats(self):
        """(all-reduces, all-gathers) this context has issued (pmx_comm_stats)."""
        a, g = C.c_uint64(), C.c_uint64()
        self._chk(self._l.pmx_comm_stats(self.h, C.byref(a), C.byref(g)))
        return a.value, g.value

    def comm_loop_stats(self):
        """(verdict syncs, async iterations, stalls) of the sharded device loop (pmx_comm_loop_stats)."""
        v, a, st = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._l.pmx_comm_loop_stats(self.h, C.byref(v), C.byref(a), C.byref(st)))
        return v.value, a.value, st.value

    # --- clouds
    def set_reference(self, feat, normals=None):
        feat = self._arr(feat)
        nrm = self._arr(normals) if normals is not None else None
        self.rows = feat.shape[1]
        self._ref_keep = (feat, nrm)
        self._chk(self._l.pmx_set_reference(self.h, _ptr(feat), feat.shape[1], feat.shape[0], _ptr(nrm)))

    def set_reading(self, feat, T0=None):
        feat = self._arr(feat)
        rows = feat.shape[1]
        T0 = self._arr(np.eye(rows) if T0 is None else T0)
        self.N = feat.shape[0]
        self._chk(self._l.pmx_set_reading(self.h, _ptr(feat), rows, feat.shape[0], _ptr(T0)))

    def set_reading_radii(self, radii):
        """KDTreeVarDistMatcher: one search radius per reading point (None clears)."""
        r = self._arr(radii) if radii is not None else None
        self._chk(self._l.pmx_set_reading_radii(self.h, _ptr(r) if r is not None else None))

    def set_reading_normals(self, normals):
        """SurfaceNormalOutlierFilter: the reading's normals, N x D in the order of
        set_reading's points (None clears; so does the next set_reading)."""
        n = self._arr(normals) if normals is not None else None
        if n is not None and n.shape != (self.N, self.rows - 1):
            raise InvalidParameter(f"reading normals must be {self.N} x {self.rows - 1}, not {n.shape}")
        self._chk(self._l.pmx_set_reading_normals(self.h, _ptr(n) if n is not None else None))

    def set_reference_weight_descriptor(self, desc):
        """GenericDescriptorOutlierFilter: the reference's one-row descriptor, M values
        in the order of set_reference's points, no NaN (None clears; so does the
        next set_reference)."""
        d = self._arr(desc).reshape(-1) if desc is not None else None
        ref = getattr(self, "_ref_keep", None)
        if d is not None and ref is not None and d.shape[0] != ref[0].shape[0]:
            raise InvalidParameter(f"the weight descriptor must have {ref[0].shape[0]} values, "
                                   f"not {d.shape[0]}")
        self._chk(self._l.pmx_set_reference_weight_descriptor(self.h, _ptr(d) if d is not None else None))

    # --- per-iteration
    def set_search(self, search_type: int):
        """0 = brute force, 1/2 = exact grid search (KDTreeMatcher searchType)."""
        self._chk(self._l.pmx_set_search(self.h, int(search_type)))

    def match(self, T, knn=1, max_dist=np.inf, epsilon=0.0):
        T = self._arr(T)
        v = C.c_uint64(0)
        self._chk(self._l.pmx_match(self.h, _ptr(T), knn, float(max_dist), float(epsilon), C.byref(v)))
        self.knn = knn
        return v.value

    def outlier_default(self):
        self._chk(self._l.pmx_outlier_default(self.h))

    def outlier(self, name, pos=0, **p):
        l, h = self._l, self.h
        if name == "NullOutlierFilter":
            rc = l.pmx_outlier_null(h, pos)
        elif name == "MaxDistOutlierFilter":
            rc = l.pmx_outlier_maxdist(h, pos, float(p.get("maxDist", 1.0)))
        elif name == "MinDistOutlierFilter":
            rc = l.pmx_outlier_mindist(h, pos, float(p.get("minDist", 1.0)))
        elif name == "MedianDistOutlierFilter":
            rc = l.pmx_outlier_mediandist(h, pos, float(p.get("factor", 3.0)))
        elif name == "TrimmedDistOutlierFilter":
            rc = l.pmx_outlier_trimmed(h, pos, float(p.get("ratio", 0.85)))
        elif name == "VarTrimmedDistOutlierFilter":
            rc = l.pmx_outlier_vartrimmed(h, pos, float(p.get("minRatio", 0.05)),
                                          float(p.get("maxRatio", 0.99)), float(p.get("lambda", 2.35)))
        else:
            raise InvalidParameter(f"unknown outlier filter {name}")
        self._chk(rc)

    def outlier_surface_normal(self, pos=0, eps=None, max_angle=1.57):
        """SurfaceNormalOutlierFilter: eps = cos(maxAngle) in the context's dtype
        (computed here from max_angle unless given)."""
        if eps is None:
            eps = np.cos(self.dtype.type(max_angle))
        self._chk(self._l.pmx_outlier_surface_normal(self.h, pos, float(eps)))

    def outlier_generic_descriptor(self, pos=0, soft=False, larger_than=True, threshold=0.1):
        """GenericDescriptorOutlierFilter on the descriptor of
        set_reference_weight_descriptor: hard (desc > threshold, or < with
        larger_than False; strict, in the context's dtype) or soft (desc / max)."""
        self._chk(self._l.pmx_outlier_generic_descriptor(self.h, pos, 1 if soft else 0, 1 if larger_than else 0,
                                                         float(threshold)))

    def outlier_robust(self, pos=0, fct="cauchy", tuning=1.0, approximation=np.inf, scale_mode=RS_MAD,
                       berg_target=0.0, point2plane=False):
        """One RobustOutlierFilter call with the scale mode given (the filter's
        iteration schedule is the caller's, as libpointmatcher_amd.icp does)."""
        self._chk(self._l.pmx_outlier_robust(self.h, pos, ROBUST_FCT[fct], float(tuning), float(approximation),
                                             int(scale_mode), float(berg_target), 1 if point2plane else 0))

    def robust_scale(self, pos=0):
        v = C.c_double()
        self._chk(self._l.pmx_robust_scale(self.h, pos, C.byref(v)))
        return v.value

    def p2plane_system(self):
        n = 6 if self.rows == 4 else 3
        A = np.zeros(n * n)
        b = np.zeros(n)
        st = Stats()
        self._chk(self._l.pmx_p2plane_system(self.h, _ptr(A), _ptr(b), C.byref(st)))
        return A.reshape(n, n), b, st

    def p2plane_system_forced(self, force):
        """PointToPlane's force2D ("2D") / force4DOF ("4DOF") normal equations for
        the last match (pmx_p2plane_system_forced): (A, b, stats), A 3 x 3 / 4 x 4."""
        f = FORCE_KIND[force]
        n = 4 if f == 2 else 3 if f == 1 or self.rows == 3 else 6
        A = np.zeros(n * n)
        b = np.zeros(n)
        st = Stats()
        self._chk(self._l.pmx_p2plane_system_forced(self.h, f, _ptr(A), _ptr(b), C.byref(st)))
        return A.reshape(n, n), b, st

    def p2point_system(self):
        D = self.rows - 1
        mp = np.zeros(D)
        mq = np.zeros(D)
        m = np.zeros(D * D)
        st = Stats()
        self._chk(self._l.pmx_p2point_system(self.h, _ptr(mp), _ptr(mq), _ptr(m), C.byref(st)))
        return mp, mq, m.reshape(D, D), st

    def p2point_similarity_system(self):
        """PointToPointSimilarityErrorMinimizer's sums for the last match:
        (mean_p, mean_q, m, sigma, stats), sigma = sum ||p - mean_p||^2 w."""
        D = self.rows - 1
        mp = np.zeros(D)
        mq = np.zeros(D)
        m = np.zeros(D * D)
        sigma = C.c_double()
        st = Stats()
        self._chk(self._l.pmx_p2point_similarity_system(self.h, _ptr(mp), _ptr(mq), _ptr(m), C.byref(sigma),
                                                        C.byref(st)))
        return mp, mq, m.reshape(D, D), sigma.value, st

    def p2plane_covariance(self, T_step):
        """The sums of PointToPlaneWithCovErrorMinimizer's estimate for the last
        match and the solved increment T_step (pmx_p2plane_covariance):
        (H, Q, pairs), 6 x 6 float64 each; cov = sigma^2 H^-1 Q H^-1."""
        T_step = self._arr(T_step)
        H, Q = np.zeros((6, 6)), np.zeros((6, 6))
        n = C.c_int64(0)
        self._chk(self._l.pmx_p2plane_covariance(self.h, _ptr(T_step), _ptr(H), _ptr(Q), C.byref(n)))
        return H, Q, n.value

    def loop_covariance(self):
        """The same for the last iteration of a finished device loop begun with
        PointToPlaneWithCovErrorMinimizer (pmx_loop_covariance)."""
        H, Q = np.zeros((6, 6)), np.zeros((6, 6))
        n = C.c_int64(0)
        self._chk(self._l.pmx_loop_covariance(self.h, _ptr(H), _ptr(Q), C.byref(n)))
        return H, Q, n.value

    def set_reading_noise(self, noise):
        """The reading's simpleSensorNoise, N values in set_reading's order (None clears)."""
        n = self._arr(noise).ravel() if noise is not None else None
        if n is not None and n.size != self.N:
            raise InvalidParameter(f"reading noise must have {self.N} values, not {n.size}")
        self._chk(self._l.pmx_set_reading_noise(self.h, _ptr(n)))

    def set_reference_descriptors(self, noise=None, densities=None):
        """The reference's simpleSensorNoise and densities, M values each in
        set_reference's order (None: absent)."""
        M = self._ref_keep[0].shape[0]
        arrs = [self._arr(a).ravel() if a is not None else None for a in (noise, densities)]
        for a in arrs:
            if a is not None and a.size != M:
                raise InvalidParameter(f"reference descriptors must have {M} values, not {a.size}")
        self._chk(self._l.pmx_set_reference_descriptors(self.h, _ptr(arrs[0]), _ptr(arrs[1])))

    def match_quality(self, minimizer="PointToPlaneErrorMinimizer", T_step=None):
        """getResidualError / getOverlap's sums for the last match (pmx_match_quality)."""
        q = Quality()
        T = self._arr(T_step) if T_step is not None else None
        self._chk(self._l.pmx_match_quality(self.h, _ptr(T), MINIMIZER_KIND[minimizer], C.byref(q)))
        return q

    def loop_quality(self, minimizer="PointToPlaneErrorMinimizer"):
        """The same for the last iteration of a finished device loop (pmx_loop_quality)."""
        q = Quality()
        self._chk(self._l.pmx_loop_quality(self.h, MINIMIZER_KIND[minimizer], C.byref(q)))
        return q

    def _fetch_elements(self, info, normals):
        P, r = info.columns, self.rows
        e = ErrorElements(reading=np.empty((P, r), self.dtype), reference=np.empty((P, r), self.dtype),
                          ref_normals=np.empty((P, r - 1), self.dtype) if normals else None,
                          dists=np.empty(P, self.dtype), ids=np.empty(P, np.int32), weights=np.empty(P, self.dtype),
                          reading_index=np.empty(P, np.int32), link_rank=np.empty(P, np.int32),
                          rejected_matches=info.rejected_matches, rejected_points=info.rejected_points)
        self._chk(self._l.pmx_error_elements(self.h, _ptr(e.reading), _ptr(e.reference),
                                             _ptr(e.ref_normals) if normals else None, _ptr(e.dists), _ptr(e.ids),
                                             _ptr(e.weights), _ptr(e.reading_index), _ptr(e.link_rank)))
        return e

    def error_elements(self, T_step=None, normals=None):
        """getErrorElements of the last match (pmx_error_elements_prepare, then
        pmx_error_elements).  T_step None: the match's own transform; normals
        None: the reference's normals when it has them."""
        info = ElementsInfo()
        T = self._arr(T_step) if T_step is not None else None
        self.last_elements_info = info  # (the counts come back with PMX_E_NO_POINTS too)
        self._chk(self._l.pmx_error_elements_prepare(self.h, _ptr(T), C.byref(info)))
        return self._fetch_elements(info, self._ref_keep[1] is not None if normals is None else normals)

    def loop_error_elements(self, normals=None):
        """The same for the last iteration of a finished device loop (pmx_loop_error_elements_prepare)."""
        info = ElementsInfo()
        self.last_elements_info = info
        self._chk(self._l.pmx_loop_error_elements_prepare(self.h, C.byref(info)))
        return self._fetch_elements(info, self._ref_keep[1] is not None if normals is None else normals)

    def get_matches(self):
        d = np.empty((self.N, self.knn), self.dtype)
        i = np.empty((self.N, self.knn), np.int32)
        self._chk(self._l.pmx_get_matches(self.h, _ptr(d), _ptr(i)))
        return d, i

    def get_weights(self):
        w = np.empty((self.N, self.knn), self.dtype)
        self._chk(self._l.pmx_get_weights(self.h, _ptr(w)))
        return w

    def vartrim_partial_sums(self):
        """The last VarTrimmedDist filter's partial sums (diagnostic)."""
        n = C.c_int64(0)
        self._chk(self._l.pmx_vartrim_partial_sums(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, self.dtype)
        self._chk(self._l.pmx_vartrim_partial_sums(self.h, _ptr(out), out.size, C.byref(n)))
        return out

    # --- timing
    def timing(self, on=True):
        self._chk(self._l.pmx_timing_enable(self.h, 1 if on else 0))

    def timing_read(self):
        ms = C.c_double()
        n = C.c_int64()
        o = C.c_double()
        self._chk(self._l.pmx_timing_read(self.h, C.byref(ms), C.byref(n), C.byref(o)))
        return ms.value, n.value

    def sync(self):
        self._chk(self._l.pmx_sync(self.h))

    # --- device-resident loop
    def loop_begin(self, knn=1, max_dist=np.inf, filters=(), minimizer="PointToPlaneErrorMinimizer",
                   checkers=(), T0=None, keep_trace=False, force=None):
        """filters: [(name, params...)], checkers: [(name, params...)] in chain order
        (Counter: max; Differential: rot, trans, smoothLength; Bound: rot, trans)."""
        cfg = LoopCfg()
        cfg.knn = knn
        cfg.max_dist = float(max_dist)
        cfg.n_filters = len(filters)
        for i, (name, *p) in enumerate(filters):
            cfg.filter_kind[i] = FILTER_KIND[name]
            for j, v in enumerate(p):
                cfg.filter_p[i][j] = float(v)
        cfg.minimizer = (2 if minimizer.startswith("PointToPlaneWithCov")
                         else 0 if minimizer.startswith("PointToPlane")
                         else 3 if minimizer.startswith("PointToPointSimilarity") else 1)
        cfg.n_checkers = len(checkers)
        for i, (name, *p) in enumerate(checkers):
            cfg.checker_kind[i] = CHECK_KIND[name]
            for j, v in enumerate(p):
                cfg.checker_p[i][j] = float(v)
        cfg.keep_trace = 1 if keep_trace else 0
        cfg.force = FORCE_KIND[force]
        T0 = self._arr(np.eye(self.rows) if T0 is None else T0)
        self._loop_keep = cfg
        self._chk(self._l.pmx_loop_begin(self.h, C.byref(cfg), _ptr(T0)))

    def loop_run(self, n):
        """Run up to n iterations; returns the status (raises the ICP's exception)."""
        st = LoopStatus()
        rc = self._l.pmx_loop_run(self.h, int(n), C.byref(st))
        self.last_loop_status = st
        self._chk(rc)
        return st

    def loop_select_stats(self):
        """(window hits, radix fallbacks) of the fused quantile window (pmx_spec.h)."""
        h, m = C.c_uint64(), C.c_uint64()
        self._chk(self._l.pmx_loop_select_stats(self.h, C.byref(h), C.byref(m)))
        return h.value, m.value

    def loop_diag(self, first, count):
        """Per-iteration diagnostics of the current loop (pmx_loop_diag): int64
        rows (grid level, window verdict 1/0/-1, pairs evaluated, full searches)."""
        out = np.zeros((count, 4), np.int64)
        self._chk(self._l.pmx_loop_diag(self.h, int(first), int(count), _ptr(out)))
        return out

    def transform_reading(self, T=None, normals=False, offset=None):
        """Transformation::compute on the resident reading (pmx_transform_reading):
        T * (the reading as the context holds it), (N, rows) in set_reading's
        order; nothing is uploaded.  T None: the finished device loop's T_iter,
        read on the device.  normals: also the rotation block times the
        resident reading normals, (N, rows - 1); (features, normals) is
        returned.  offset (rows - 1 values): added to each coordinate after the
        transform (pmx_transform_reading_offset)."""
        P = self._arr(T) if T is not None else None
        if P is not None and self.rows is not None and P.shape != (self.rows, self.rows):
            raise InvalidParameter(f"T must be ({self.rows}, {self.rows}), not {P.shape}")
        rows = self.rows or 4
        of = np.empty((self.N, rows), self.dtype)
        on = np.empty((self.N, rows - 1), self.dtype) if normals else None
        if offset is None:
            rc = self._l.pmx_transform_reading(self.h, _ptr(P), _ptr(of), _ptr(on))
        else:
            off = self._arr(offset).reshape(-1)
            if off.shape[0] != rows - 1:
                raise InvalidParameter(f"offset must have {rows - 1} values, not {off.shape[0]}")
            rc = self._l.pmx_transform_reading_offset(self.h, _ptr(P), _ptr(off), _ptr(of), _ptr(on))
        self._chk(rc)
        return (of, on) if normals else of

    def loop_T(self, st):
        r = self.rows
        return np.array(st.T_iter[:r * r], dtype=self.dtype).reshape(r, r)

    def loop_trace(self, first, count):
        r = self.rows
        out = np.empty((count, r, r), self.dtype)
        self._chk(self._l.pmx_loop_trace(self.h, int(first), int(count), _ptr(out)))
        return out

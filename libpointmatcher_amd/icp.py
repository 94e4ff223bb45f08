"""ctypes binding of the host ICP chain (include/pmx_icp.h, lib/libpmx_icp.so).

    icp = ICP(np.float32)
    icp.load_yaml(open("chain.yaml").read())     # or icp.set_default()
    T = icp.compute(reading, reference, ref_normals)
    aligned, _ = Transformation("RigidTransformation").compute(reading, T)

Clouds are (n, rows) arrays with the homogeneous row last (rows = D + 1) —
the memory layout of the reference's column-major (D+1) x n features.
Errors raise the Python mirrors of the reference exception types.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import ConvergenceError, InvalidParameter, TransformationError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "lib", os.environ.get("PMX_LIB_VARIANT", ""), "libpmx_icp.so")  # (variant: _capi.py)


class InvalidElement(RuntimeError):
    """InvalidElement (pointmatcher/Registrar.h:69-72): unknown module name."""


class InvalidField(RuntimeError):
    """DataPoints::InvalidField (pointmatcher/PointMatcher.h:213-216): a data
    filter did not find a descriptor it needs."""


class InvalidModuleType(RuntimeError):
    """ICPChainBase::InvalidModuleType (pointmatcher/ICP.cpp:158-166)."""


class ConfigurationError(RuntimeError):
    """PointMatcherSupport::ConfigurationError / YAML syntax."""


_ERR = {-1: ConvergenceError, -3: InvalidParameter, -4: TransformationError, -5: InvalidElement,
        -6: InvalidModuleType, -7: ConfigurationError, -8: InvalidField, -10: RuntimeError}


class IcpStats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("point_count_touched", C.c_int64),
                ("overlap_ratio", C.c_double), ("point_used_ratio", C.c_double), ("kept", C.c_int64),
                ("rejected_matches", C.c_int64), ("rejected_points", C.c_int64),
                ("convergence_duration", C.c_double), ("reference_preprocessing_duration", C.c_double),
                ("reading_preprocessing_duration", C.c_double), ("max_iterations_reached", C.c_int)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None


def lib():
    global _lib
    if _lib is None:
        _capi.lib()  # libpmx.so first (RTLD_GLOBAL)
        if not os.path.exists(LIB):
            raise _capi.PmxError(f"{LIB} not built")
        l = C.CDLL(LIB)
        l.pmx_icp_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.pmx_icp_destroy.argtypes = [C.c_void_p]
        l.pmx_icp_last_error.argtypes = [C.c_void_p]
        l.pmx_icp_last_error.restype = C.c_char_p
        l.pmx_icp_set_default.argtypes = [C.c_void_p]
        l.pmx_icp_load_yaml.argtypes = [C.c_void_p, C.c_char_p]
        l.pmx_icp_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        l.pmx_icp_comm_init_host.argtypes = [C.c_void_p, C.c_int, C.c_int, _capi.ALLREDUCE_FN, _capi.ALLGATHER_FN,
                                             C.c_void_p]
        l.pmx_icp_keep_trace.argtypes = [C.c_void_p, C.c_int]
        l.pmx_icp_outlier_filter_doc.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int]
        l.pmx_icp_data_points_filter_doc.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int]
        l.pmx_icp_add_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_int64]
        l.pmx_cloud_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        l.pmx_cloud_destroy.argtypes = [C.c_void_p]
        l.pmx_cloud_last_error.restype = C.c_char_p
        l.pmx_cloud_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pmx_cloud_label.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
        l.pmx_cloud_data.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pmx_icp_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        l.pmx_icp_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p]
        l.pmx_icp_iterate.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.pmx_icp_finish.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_icp_stats_get.argtypes = [C.c_void_p, C.POINTER(IcpStats)]
        l.pmx_icp_trace_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        l.pmx_icp_covariance.argtypes = [C.c_void_p, C.c_void_p]
        l.pmx_icp_overlap.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        l.pmx_icp_residual_error.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        l.pmx_icp_filtered_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_char_p,
                                                  C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        l.pmx_icp_timing.argtypes = [C.c_void_p, C.c_int]
        l.pmx_icp_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        l.pmx_icp_select_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        l.pmx_icp_comm_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 5
        l.pmx_icp_loop_diag.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        l.pmx_icp_error_elements_info.argtypes = [C.c_void_p, C.POINTER(IcpElementsInfo)]
        l.pmx_icp_error_elements.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        l.pmx_icp_error_elements_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_int64,
                                                        C.POINTER(C.c_int)]
        l.pmx_icp_set_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_int)]
        l.pmx_icp_clear_map.argtypes = [C.c_void_p]
        l.pmx_icp_has_map.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        l.pmx_icp_get_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        l.pmx_icp_sequence_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                               C.POINTER(C.c_int)]
        l.pmx_icp_sequence_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        l.pmx_icp_reading_transformed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_int)]
        l.pmx_transformation_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.pmx_transformation_destroy.argtypes = [C.c_void_p]
        l.pmx_transformation_last_error.argtypes = [C.c_void_p]
        l.pmx_transformation_last_error.restype = C.c_char_p
        l.pmx_transformation_check_parameters.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.pmx_transformation_correct_parameters.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        l.pmx_transformation_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                                 C.c_int, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


class IcpElementsInfo(C.Structure):
    """pmx_icp_elements_info (include/pmx_icp.h)."""
    _fields_ = [("columns", C.c_int64), ("rows", C.c_int), ("reading_desc_dim", C.c_int),
                ("reference_desc_dim", C.c_int), ("rejected_matches", C.c_int64), ("rejected_points", C.c_int64)]


class IcpErrorElements:
    """errorMinimizer->getErrorElements() as numpy arrays: reading / reference
    (P, rows) features, dists, weights (P,), ids, reading_index (P,) int32, the two
    rejected counts, and descriptor(cloud, name) -> (P, span) or None."""

    def __init__(self, icp, **kw):
        self._icp = icp
        self.__dict__.update(kw)

    @property
    def columns(self):
        return len(self.dists)

    def descriptor(self, cloud, name):
        return self._icp._elements_descriptor(cloud, name, self.columns)


def outlier_filter_doc(name, dtype=np.float32):
    """The parameter documentation of a registered outlier filter, as the
    reference prints a Parametrizable (one "- name (default: v) - doc - min: a -
    max: b" line per parameter)."""
    buf = C.create_string_buffer(8192)
    rc = lib().pmx_icp_outlier_filter_doc(1 if np.dtype(dtype) == np.float64 else 0, name.encode(), buf, len(buf))
    if rc:
        raise _ERR.get(rc, RuntimeError)(f"no documentation for outlier filter {name}")
    return buf.value.decode()


def data_points_filter_doc(name, dtype=np.float32):
    """The parameter documentation of a registered data points filter, in the
    form of outlier_filter_doc."""
    buf = C.create_string_buffer(8192)
    rc = lib().pmx_icp_data_points_filter_doc(1 if np.dtype(dtype) == np.float64 else 0, name.encode(), buf,
                                              len(buf))
    if rc:
        raise _ERR.get(rc, RuntimeError)(f"no documentation for data points filter {name}")
    return buf.value.decode()


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Cloud:
    """DataPoints loaded from a .csv / .vtk file (DataPoints::load, IO.cpp:374-389)."""

    def __init__(self, features, feature_labels, descriptors, descriptor_labels):
        self.features = features                  # (n, rows), homogeneous row last
        self.feature_labels = feature_labels      # [(name, span)]
        self.descriptors = descriptors            # (n, desc_dim)
        self.descriptor_labels = descriptor_labels

    def descriptor(self, name):
        off = 0
        for lab, span in self.descriptor_labels:
            if lab == name:
                return self.descriptors[:, off:off + span]
            off += span
        raise KeyError(name)

    def descriptor_exists(self, name):
        return any(lab == name for lab, _ in self.descriptor_labels)


def load_cloud(path, dtype=np.float32):
    l = lib()
    dt = np.dtype(dtype)
    h = C.c_void_p()
    rc = l.pmx_cloud_load(str(path).encode(), 1 if dt == np.float64 else 0, C.byref(h))
    if rc:
        raise _ERR.get(rc, RuntimeError)(l.pmx_cloud_last_error().decode())
    try:
        n, rows, dd, nfl, ndl = C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        l.pmx_cloud_info(h, C.byref(n), C.byref(rows), C.byref(dd), C.byref(nfl), C.byref(ndl))
        labels = []
        for which, cnt in ((0, nfl.value), (1, ndl.value)):
            ls = []
            for i in range(cnt):
                buf = C.create_string_buffer(256)
                span = C.c_int()
                l.pmx_cloud_label(h, which, i, buf, 256, C.byref(span))
                ls.append((buf.value.decode(), span.value))
            labels.append(ls)
        f = np.empty((n.value, rows.value), dt)
        d = np.empty((n.value, dd.value), dt)
        l.pmx_cloud_data(h, _p(f), _p(d) if dd.value else None)
        return Cloud(f, labels[0], d, labels[1])
    finally:
        l.pmx_cloud_destroy(h)


class Transformation:
    """A registered Transformation (PointMatcher.h; TransformationsImpl.cpp:49-272):
    "RigidTransformation", "SimilarityTransformation" or "PureTranslation".

        T = icp.compute(reading, reference, normals)
        aligned = Transformation("RigidTransformation").compute(reading_cloud, T)

    check_parameters and correct_parameters are host arithmetic and need no
    GPU; compute runs on the GPU and raises without one."""

    def __init__(self, name, dtype=np.float32, device=0):
        self.dtype = np.dtype(dtype)
        self.name = name
        self._l = lib()
        h = C.c_void_p()
        rc = self._l.pmx_transformation_create(name.encode(), 1 if self.dtype == np.float64 else 0, int(device),
                                               C.byref(h))
        if rc:
            raise _ERR.get(rc, RuntimeError)(self._l.pmx_transformation_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._l.pmx_transformation_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise _ERR.get(rc, RuntimeError)(self._l.pmx_transformation_last_error(self.h).decode())

    def _params(self, T):
        P = np.ascontiguousarray(T, dtype=self.dtype)
        if P.ndim != 2 or P.shape[0] != P.shape[1]:
            raise InvalidParameter(f"transformation parameters must be a square matrix, not {P.shape}")
        return P

    def check_parameters(self, T):
        P = self._params(T)
        ok = C.c_int(0)
        self._chk(self._l.pmx_transformation_check_parameters(self.h, _p(P), P.shape[0], C.byref(ok)))
        return bool(ok.value)

    def correct_parameters(self, T):
        P = self._params(T)
        out = np.empty_like(P)
        self._chk(self._l.pmx_transformation_correct_parameters(self.h, _p(P), P.shape[0], _p(out)))
        return out

    def compute(self, cloud_or_features, T, descriptors=None, descriptor_labels=None):
        """The transformed copy of a Cloud (a Cloud is returned), or of a
        features array (n, rows) with optional descriptors (n, desc_dim) and
        their labels [(name, span)]: (features, descriptors or None) is
        returned.  The inputs are left as they are."""
        is_cloud = isinstance(cloud_or_features, Cloud)
        if is_cloud:
            if descriptors is not None or descriptor_labels is not None:
                raise ValueError("a Cloud carries its own descriptors and labels")
            cloud = cloud_or_features
            feat, descriptors, descriptor_labels = cloud.features, cloud.descriptors, cloud.descriptor_labels
            if descriptors is not None and descriptors.shape[1] == 0:
                descriptors = None
        else:
            feat = cloud_or_features
        f = np.ascontiguousarray(feat, dtype=self.dtype)
        if f.ndim != 2:
            raise InvalidParameter("features must be (n, rows)")
        n, rows = f.shape
        P = self._params(T)
        d = None if descriptors is None else np.ascontiguousarray(descriptors, dtype=self.dtype)
        if d is not None and (d.ndim != 2 or d.shape[0] != n):
            raise InvalidParameter("descriptors must be (n, desc_dim)")
        dd = 0 if d is None else d.shape[1]
        labels = list(descriptor_labels or [])
        names = (C.c_char_p * max(len(labels), 1))(*[str(name).encode() for name, _ in labels])
        spans = (C.c_int * max(len(labels), 1))(*[int(span) for _, span in labels])
        of = np.empty_like(f)
        od = None if d is None else np.empty_like(d)
        self._chk(self._l.pmx_transformation_compute(self.h, _p(f), rows, n, _p(P), P.shape[0], _p(d), dd, names,
                                                     spans, len(labels), _p(of), _p(od)))
        if is_cloud:
            return Cloud(of, list(cloud.feature_labels), od if od is not None else np.empty((n, 0), self.dtype),
                         list(cloud.descriptor_labels))
        return of, od


class ICP:
    """PointMatcher<T>::ICP on the MI355X path (one object per rank / thread)."""

    def __init__(self, dtype=np.float32, device=0):
        self.dtype = np.dtype(dtype)
        self._l = lib()
        h = C.c_void_p()
        rc = self._l.pmx_icp_create(1 if self.dtype == np.float64 else 0, device, C.byref(h))
        if rc:
            raise RuntimeError("pmx_icp_create failed")
        self.h = h
        self.rows = None

    def close(self):
        if getattr(self, "h", None):
            self._l.pmx_icp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            msg = self._l.pmx_icp_last_error(self.h).decode()
            raise _ERR.get(rc, RuntimeError)(msg)

    # --- configuration
    def set_default(self):
        self._chk(self._l.pmx_icp_set_default(self.h))

    def load_yaml(self, text: str):
        self._chk(self._l.pmx_icp_load_yaml(self.h, text.encode()))

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = (C.c_char * 128).from_buffer_copy(uid)
        self._chk(self._l.pmx_icp_comm_init(self.h, buf, nranks, rank))

    def comm_init_host(self, comm):
        """Multi-rank over a _capi.HostComm (e.g. _capi.gloo_host_comm())."""
        self._comm = comm  # (the callbacks must outlive the ICP object)
        self._chk(self._l.pmx_icp_comm_init_host(self.h, comm.nranks, comm.rank, comm.ar, comm.ag, None))

    def keep_trace(self, on=True):
        self._chk(self._l.pmx_icp_keep_trace(self.h, 1 if on else 0))

    def add_descriptor(self, cloud, name, values):
        """Stage a descriptor (n,) or (n, span) for the next compute / prepare;
        cloud: "reading" or "reference" (e.g. the reading's "maxSearchDist"
        of KDTreeVarDistMatcher)."""
        if cloud not in ("reading", "reference"):
            raise ValueError(f'cloud must be "reading" or "reference", not {cloud!r}')
        v = np.ascontiguousarray(values, dtype=self.dtype)
        span = 1 if v.ndim == 1 else v.shape[1]
        self._chk(self._l.pmx_icp_add_descriptor(self.h, 0 if cloud == "reading" else 1, name.encode(), span, _p(v),
                                                 v.shape[0]))

    # --- run
    def _args(self, reading, reference, normals, T_init):
        rd = np.ascontiguousarray(reading, dtype=self.dtype)
        ref = np.ascontiguousarray(reference, dtype=self.dtype)
        nrm = np.ascontiguousarray(normals, dtype=self.dtype) if normals is not None else None
        rows = rd.shape[1]
        if ref.shape[1] != rows:
            raise ValueError("reading and reference must have the same number of rows")
        Ti = np.ascontiguousarray(np.eye(rows) if T_init is None else T_init, dtype=self.dtype)
        self.rows = rows
        self._keep = (rd, ref, nrm, Ti)
        return rd, ref, nrm, Ti, rows

    def compute(self, reading, reference, normals=None, T_init=None):
        rd, ref, nrm, Ti, rows = self._args(reading, reference, normals, T_init)
        out = np.zeros((rows, rows), self.dtype)
        self._chk(self._l.pmx_icp_compute(self.h, _p(rd), rows, rd.shape[0], _p(ref), ref.shape[0], _p(nrm),
                                          _p(Ti), _p(out)))
        return out

    __call__ = compute

    def prepare(self, reading, reference, normals=None, T_init=None):
        rd, ref, nrm, Ti, rows = self._args(reading, reference, normals, T_init)
        self._chk(self._l.pmx_icp_prepare(self.h, _p(rd), rows, rd.shape[0], _p(ref), ref.shape[0], _p(nrm),
                                          _p(Ti)))

    def iterate(self, n=1):
        done = C.c_int(0)
        self._chk(self._l.pmx_icp_iterate(self.h, n, C.byref(done)))
        return bool(done.value)

    def finish(self):
        out = np.zeros((self.rows, self.rows), self.dtype)
        self._chk(self._l.pmx_icp_finish(self.h, _p(out)))
        return out

    def reading_transformed(self):
        """The filtered reading moved by the last compute's result, (n, rows) in
        the caller's frame (pmx_icp_reading_transformed): what
        Transformation.compute(filtered_reading, T) returns, without the upload
        while the device still holds the filtered reading.  Raises RuntimeError
        before any compute."""
        n, rows = C.c_int64(0), C.c_int(0)
        self._chk(self._l.pmx_icp_reading_transformed(self.h, None, 0, C.byref(n), C.byref(rows)))
        out = np.empty((n.value, rows.value), self.dtype)
        self._chk(self._l.pmx_icp_reading_transformed(self.h, _p(out), out.size, C.byref(n), C.byref(rows)))
        return out

    # --- introspection
    def stats(self):
        s = IcpStats()
        self._l.pmx_icp_stats_get(self.h, C.byref(s))
        return s

    def trace(self, max_iters=100000):
        it = self.stats().iterations
        out = np.zeros((max(it, 1), self.rows, self.rows), self.dtype)
        n = self._l.pmx_icp_trace_get(self.h, _p(out), min(it, max_iters))
        return out[:n]

    def covariance(self):
        """errorMinimizer->getCovariance() of the last compute (pmx_icp_covariance):
        6 x 6, the estimate of PointToPlaneWithCovErrorMinimizer (translation
        first, then the rotation angles), zeros for every other minimiser."""
        out = np.zeros((6, 6), self.dtype)
        self._chk(self._l.pmx_icp_covariance(self.h, _p(out)))
        return out

    def overlap(self):
        """errorMinimizer->getOverlap() of the last compute (pmx_icp_overlap): from
        the clouds' simpleSensorNoise / densities when present, else the weighted
        used ratio."""
        v = C.c_double()
        self._chk(self._l.pmx_icp_overlap(self.h, C.byref(v)))
        return v.value

    def residual_error(self):
        """errorMinimizer->getResidualError() of the last compute (pmx_icp_residual_error)."""
        v = C.c_double()
        self._chk(self._l.pmx_icp_residual_error(self.h, C.byref(v)))
        return v.value

    def error_elements(self):
        """errorMinimizer->getErrorElements() of the last compute (pmx_icp_error_elements*):
        the kept pairs, computed on the first call after the ICP stopped and cached
        until the next prepare / set_map; zero columns before any compute."""
        info = IcpElementsInfo()
        self._chk(self._l.pmx_icp_error_elements_info(self.h, C.byref(info)))
        P, r = info.columns, info.rows if info.rows else (self.rows or 4)
        e = IcpErrorElements(self, reading=np.empty((P, r), self.dtype), reference=np.empty((P, r), self.dtype),
                             dists=np.empty(P, self.dtype), ids=np.empty(P, np.int32),
                             weights=np.empty(P, self.dtype), reading_index=np.empty(P, np.int32),
                             rejected_matches=info.rejected_matches, rejected_points=info.rejected_points,
                             reading_desc_dim=info.reading_desc_dim, reference_desc_dim=info.reference_desc_dim)
        self._chk(self._l.pmx_icp_error_elements(self.h, P, _p(e.reading), _p(e.reference), _p(e.dists), _p(e.ids),
                                                 _p(e.weights), _p(e.reading_index)))
        return e

    def _elements_descriptor(self, cloud, name, columns):
        which = 0 if cloud == "reading" else 1
        span = C.c_int(0)
        self._chk(self._l.pmx_icp_error_elements_descriptor(self.h, which, name.encode(), None, 0, C.byref(span)))
        if span.value == 0:
            return None
        out = np.empty((columns, span.value), self.dtype)
        self._chk(self._l.pmx_icp_error_elements_descriptor(self.h, which, name.encode(), _p(out), out.size,
                                                            C.byref(span)))
        return out

    def filtered_descriptor(self, cloud, points, name):
        """The descriptor `name` of `points` after the chain's reading
        ("reading") or reference filters (pmx_icp_filtered_descriptor): (n, span)
        array, or None when the filtered cloud has no such descriptor."""
        pts = np.ascontiguousarray(points, dtype=self.dtype)
        which = 0 if cloud == "reading" else 1
        n, span = C.c_int64(0), C.c_int(0)
        # (sized by the caller's cloud: filters only remove points; span <= 16 covers every descriptor here)
        out = np.empty(pts.shape[0] * 16, self.dtype)
        self._chk(self._l.pmx_icp_filtered_descriptor(self.h, which, _p(pts), pts.shape[1], pts.shape[0],
                                                      name.encode(), _p(out), out.size, C.byref(n), C.byref(span)))
        if span.value == 0:
            return None
        return out[:n.value * span.value].reshape(n.value, span.value).copy()

    def timing(self, on=True):
        self._chk(self._l.pmx_icp_timing(self.h, 1 if on else 0))

    def select_stats(self):
        """(window hits, window misses) of the device loop since the last prepare."""
        h, m = C.c_uint64(), C.c_uint64()
        self._chk(self._l.pmx_icp_select_stats(self.h, C.byref(h), C.byref(m)))
        return h.value, m.value

    def loop_diag(self, first, count):
        """Per-iteration diagnostics of the device loop since the last prepare
        (pmx_icp_loop_diag): int64 rows [grid level, window verdict (1 hit, 0
        radix passes, -1 no window), pairs evaluated, full searches]."""
        out = np.zeros((count, 4), np.int64)
        self._chk(self._l.pmx_icp_loop_diag(self.h, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out

    def comm_stats(self):
        """Multi-rank diagnostics since creation: {allreduces, allgathers, verdict_syncs,
        async_iterations, stalls} (pmx_icp_comm_stats)."""
        v = [C.c_uint64() for _ in range(5)]
        self._chk(self._l.pmx_icp_comm_stats(self.h, *[C.byref(x) for x in v]))
        keys = ("allreduces", "allgathers", "verdict_syncs", "async_iterations", "stalls")
        return dict(zip(keys, (x.value for x in v)))

    def timing_read(self):
        ms = C.c_double()
        n = C.c_int64()
        self._chk(self._l.pmx_icp_timing_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class ICPSequence(ICP):
    """PointMatcher<T>::ICPSequence (PointMatcher.h:730-764, ICP.cpp:455-609):
    the map is centred, filtered and indexed once by set_map and stays on the
    device; compute(reading, T_init) matches each new reading against it."""

    def set_map(self, cloud, normals=None):
        """ICPSequence::setMap; False for an empty cloud (ignored)."""
        m = np.ascontiguousarray(cloud, dtype=self.dtype)
        nrm = np.ascontiguousarray(normals, dtype=self.dtype) if normals is not None else None
        ok = C.c_int(0)
        self._chk(self._l.pmx_icp_set_map(self.h, _p(m), m.shape[1], m.shape[0], _p(nrm), C.byref(ok)))
        return bool(ok.value)

    def clear_map(self):
        self._chk(self._l.pmx_icp_clear_map(self.h))

    def has_map(self):
        h = C.c_int(0)
        self._chk(self._l.pmx_icp_has_map(self.h, C.byref(h)))
        return bool(h.value)

    def get_map(self):
        """The prefiltered map in global coordinates (getPrefilteredMap), (n, rows)."""
        n = C.c_int64(0)
        rows = C.c_int(0)
        self._chk(self._l.pmx_icp_get_map(self.h, None, 0, C.byref(n), C.byref(rows)))
        out = np.zeros((n.value, rows.value), self.dtype)  # (sized by the library: the held map's rows)
        self._chk(self._l.pmx_icp_get_map(self.h, _p(out), out.size, C.byref(n), C.byref(rows)))
        return out

    def _rd(self, reading, T_init):
        rd = np.ascontiguousarray(reading, dtype=self.dtype)
        rows = rd.shape[1]
        Ti = np.ascontiguousarray(np.eye(rows) if T_init is None else T_init, dtype=self.dtype)
        self.rows = rows
        self._keep = (rd, Ti)
        return rd, Ti, rows

    def compute(self, reading, T_init=None):
        """ICPSequence::compute(cloudIn, T_refIn_dataIn); identity without a map."""
        rd, Ti, rows = self._rd(reading, T_init)
        out = np.zeros((rows, rows), self.dtype)
        self._chk(self._l.pmx_icp_sequence_compute(self.h, _p(rd), rows, rd.shape[0], _p(Ti), _p(out)))
        return out

    __call__ = compute

    def prepare(self, reading, T_init=None):
        """The first phase of compute (then iterate / finish); False without a map."""
        rd, Ti, rows = self._rd(reading, T_init)
        ok = C.c_int(0)
        self._chk(self._l.pmx_icp_sequence_prepare(self.h, _p(rd), rows, rd.shape[0], _p(Ti), C.byref(ok)))
        return bool(ok.value)

    def compute_with_reference(self, reading, reference, normals=None, T_init=None):
        """ICP::compute on this object (the map is re-indexed by the next sequence compute)."""
        return ICP.compute(self, reading, reference, normals, T_init)

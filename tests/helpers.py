"""Shared test helpers (test infrastructure)."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


class DenseKit:
    """The host form of csrc/common/pmx_dense.h (tests/dense_shim.cpp, plain
    C++: what the per-module path runs) through ctypes.  Arrays go in and come
    out in `dtype` (float32 / float64), row-major."""

    def __init__(self, lib):
        self._l = lib

    def _f(self, name, dtype):
        return getattr(self._l, f"pmd_{name}_" + ("f32" if np.dtype(dtype) == np.float32 else "f64"))

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def solve_underdetermined(self, A, b, dtype):
        A = np.ascontiguousarray(A, dtype=dtype)
        b = np.ascontiguousarray(b, dtype=dtype)
        x = np.zeros(len(b), dtype)
        self._f("solve_underdetermined", dtype)(self._p(A), self._p(b), len(b), self._p(x))
        return x

    def qr_rank(self, A, dtype):
        A = np.ascontiguousarray(A, dtype=dtype)
        return int(self._f("qr_rank", dtype)(self._p(A), A.shape[0]))

    def p2plane_transform(self, x, rows, dtype):
        x = np.ascontiguousarray(x, dtype=dtype)
        out = np.zeros((rows, rows), dtype)
        self._f("p2plane_transform", dtype)(rows, self._p(x), self._p(out))
        return out

    def p2plane_step(self, A, b, rows, dtype):
        """solve + increment, the step of PointToPlaneErrorMinimizer: (dT, x)."""
        x = self.solve_underdetermined(A, b, dtype)
        return self.p2plane_transform(x, rows, dtype), x

    def p2point_transform(self, m, mp, mq, dtype):
        m = np.ascontiguousarray(m, dtype=dtype)
        D = m.shape[0]
        mp = np.ascontiguousarray(mp, dtype=dtype)
        mq = np.ascontiguousarray(mq, dtype=dtype)
        out = np.zeros((D + 1, D + 1), dtype)
        self._f("p2point_transform", dtype)(D + 1, self._p(m), self._p(mp), self._p(mq), self._p(out))
        return out

    def p2point_similarity_transform(self, m, mp, mq, sigma, dtype):
        m = np.ascontiguousarray(m, dtype=dtype)
        D = m.shape[0]
        mp = np.ascontiguousarray(mp, dtype=dtype)
        mq = np.ascontiguousarray(mq, dtype=dtype)
        out = np.zeros((D + 1, D + 1), dtype)
        sc = ctypes.c_float if np.dtype(dtype) == np.float32 else ctypes.c_double
        self._f("p2point_similarity_transform", dtype)(D + 1, self._p(m), self._p(mp), self._p(mq),
                                                       sc(float(np.dtype(dtype).type(sigma))), self._p(out))
        return out

    def jacobi_svd(self, A, dtype):
        """(U, S, V, nonzero singular values): A = U diag(S) V^T, S descending."""
        A = np.ascontiguousarray(A, dtype=dtype)
        n = A.shape[0]
        U, S, V = np.zeros((n, n), dtype), np.zeros(n, dtype), np.zeros((n, n), dtype)
        nz = self._f("jacobi_svd", dtype)(self._p(A), n, self._p(U), self._p(S), self._p(V))
        return U, S, V, int(nz)


_dense_kit = None


def dense_kit():
    """Build tests/dense_shim.cpp into a temporary directory (once per process)
    and load it.  Raises FileNotFoundError without g++."""
    global _dense_kit
    if _dense_kit is None:
        cxx = shutil.which("g++")
        if cxx is None:
            raise FileNotFoundError("g++")
        tmp = tempfile.mkdtemp(prefix="pmx_dense_shim_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libdense_shim.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "libpointmatcher_amd", "csrc"),
                               os.path.join(TESTS, "dense_shim.cpp"), "-o", so])
        _dense_kit = DenseKit(ctypes.CDLL(so))
    return _dense_kit


_match_plan = None


def match_plan():
    """Build tests/match_plan_shim.cpp the way dense_kit builds its shim and
    return plan(facts) -> dict: plan_grid_match (csrc/pmx_match_plan.h) on a
    dict of facts (missing ones: 0)."""
    global _match_plan
    if _match_plan is None:
        cxx = shutil.which("g++")
        if cxx is None:
            raise FileNotFoundError("g++")
        tmp = tempfile.mkdtemp(prefix="pmx_match_plan_shim_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libmatch_plan_shim.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "libpointmatcher_amd", "csrc"),
                               os.path.join(TESTS, "match_plan_shim.cpp"), "-o", so])
        lib = ctypes.CDLL(so)
        facts = ("grid_mode", "knn", "N", "reuse_on", "nbr_on", "safe_valid", "have_match", "ids_grid", "prev_knn",
                 "same_level", "nbr_prev", "level_normals", "loop_on", "tile_dispatch", "window_on", "step_counters",
                 "have_counters")
        fields = ("form", "run", "reuse", "kt", "nbr", "nbr_normals", "window", "counter_sum", "safe_valid", "nbr_prev")

        def plan(f):
            assert set(f) <= set(facts), set(f) - set(facts)
            a = (ctypes.c_longlong * len(facts))(*[int(f.get(k, 0)) for k in facts])
            out = (ctypes.c_int * len(fields))()
            lib.pmx_plan_grid_match(a, out)
            return dict(zip(fields, out))

        _match_plan = plan
    return _match_plan


def hom(a, dtype=None):
    a = np.asarray(a)
    dtype = dtype or a.dtype
    return np.hstack([a, np.ones((a.shape[0], 1))]).astype(dtype)


def pca_normals(pts, k=10):
    """Unit normals by PCA over the k nearest neighbours (scipy cKDTree) —
    stands in for the reference's SurfaceNormal filter when a test needs
    reference normals on a cloud that has none."""
    from scipy.spatial import cKDTree

    tree = cKDTree(pts)
    _, idx = tree.query(pts, k=k)
    nb = pts[idx]
    c = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c)
    w, v = np.linalg.eigh(cov)
    return v[:, :, 0]


def quat(R):
    """Eigen Quaternion(Matrix3) -> (x, y, z, w)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def angular_distance(Ra, Rb):
    a, b = quat(Ra), quat(Rb)
    a = a / np.linalg.norm(a)
    b = b / np.linalg.norm(b)
    d = abs(np.dot(a, b))
    return 2 * np.arccos(min(1.0, d))


def validate3d(T, V, tol):
    """utest/utest.h:64-85: translation-norm difference and rotation angle."""
    dt = abs(np.linalg.norm(V[:3, 3]) - np.linalg.norm(T[:3, 3]))
    da = angular_distance(np.asarray(T[:3, :3], np.float64), np.asarray(V[:3, :3], np.float64))
    return dt < tol and da < tol, dt, da


def validate2d(T, V, tol):
    """utest/utest.h:49-62: translation norm and acos(T00)."""
    dt = abs(np.linalg.norm(V[:2, 2]) - np.linalg.norm(T[:2, 2]))
    da = abs(np.arccos(np.clip(V[0, 0], -1, 1)) - np.arccos(np.clip(T[0, 0], -1, 1)))
    return dt < tol and da < tol, dt, da


def rel_displacement(curT, refT, pts):
    """utest/utest.cpp:139-153: median |curT p - refT p| / median |curT p|."""
    P = hom(pts, np.float64).T
    a = np.abs(np.asarray(curT, np.float64) @ P - np.asarray(refT, np.float64) @ P)
    b = np.abs(np.asarray(curT, np.float64) @ P)
    return np.median(a) / np.median(b)


def planar_grid():
    """utest/utest.cpp:167-183 (icpSingular): 10x10 grid, d=0.1, z=0 / z=1."""
    nX = nY = 10
    d = np.float32(0.1)
    oX = -(nX * d / 2)
    oY = -(nY * d / 2)
    pts = np.zeros((nX * nY, 4), np.float32)
    for x in range(nX):
        for y in range(nY):
            pts[x * nY + y] = [d * x + oX, d * y + oY, 0, 1]
    pts1 = pts.copy()
    pts1[:, 2] = 1
    return pts, pts1


# ---- the quantile select's reference and its adversarial key sets ----
TRIMMED, MEDIAN = "TrimmedDistOutlierFilter", "MedianDistOutlierFilter"


def quantile_rank(count, kind, ratio, dtype):
    """Matches.cpp:83-86 in T: int(T(count) * T(ratio)) clamped to count - 1,
    ratio == 1 the maximum; Median: count // 2 (Matches.cpp:110-120)."""
    T = np.dtype(dtype).type
    if kind == MEDIAN:
        return count // 2
    q = T(ratio)
    if q == T(1):
        return count - 1
    return min(int(T(count) * q), count - 1)


def quantile_value(d, kind, ratio, dtype):
    """The order statistic itself: the finite distances (not +inf,
    Matches.cpp:71) sorted, read at quantile_rank.  Raises LookupError when
    nothing is finite ("no outlier to filter")."""
    d = np.asarray(d, dtype=dtype)
    fin = np.sort(d[d != np.inf], axis=None)
    if fin.size == 0:
        raise LookupError("no outlier to filter")
    return fin[quantile_rank(fin.size, kind, ratio, dtype)]


def quantile_limit(d, kind, ratio, dtype):
    """(limit, weights) of TrimmedDist (ratio) / MedianDist (ratio = its
    factor; limit = factor * median in T, OutlierFiltersImpl.cpp:121-122) by a
    plain sort; weights = d <= limit, in d's shape."""
    T = np.dtype(dtype).type
    v = quantile_value(d, kind, ratio, dtype)
    limit = T(ratio) * v if kind == MEDIAN else v
    return limit, (np.asarray(d, dtype=dtype) <= limit).astype(dtype)


def select_filters(dtype):
    """The filters every select case runs: Trimmed at a ratio that gives rank
    0, two inner ratios, the largest T below 1, and 1 (the maximum); Median."""
    T = np.dtype(dtype).type
    below1 = float(np.nextafter(T(1), T(0)))
    return [(TRIMMED, 1e-6), (TRIMMED, 0.3), (TRIMMED, 0.85), (TRIMMED, below1), (TRIMMED, 1.0), (MEDIAN, 3.0)]


def filter_params(kind, p):
    return {"factor": p} if kind == MEDIAN else {"ratio": p}


SELECT_SIZES = (1, 2, 15, 16, 17, 4095, 4096, 4097, 8193, 40_000, 262_145)
SELECT_KEY_SETS = ("lastdigit", "equal", "zero", "two_values", "decades")


def select_reading_x(tag, n, dtype):
    """x coordinates of n reading points whose squared distances to one
    reference point at the origin, d_i = fl(x_i^2), form the key set `tag`."""
    T = np.dtype(dtype).type
    i = np.arange(n)
    if tag == "lastdigit":  # keys that share every digit but the last one or two
        return (T(1) + i.astype(dtype) * T(2.0 ** (-23 if T is np.float32 else -52))).astype(dtype)
    if tag == "equal":
        return np.full(n, 0.5, dtype)
    if tag == "zero":
        return np.zeros(n, dtype)
    if tag == "two_values":  # 80 % at 2^-4, 20 % at 2^-2, interleaved
        return np.where(i % 5 == 4, T(0.25), T(0.0625)).astype(dtype)
    if tag == "decades":
        return np.power(T(10), np.linspace(-18, 3, n, dtype=dtype)).astype(dtype)
    raise KeyError(tag)


def select_reading(x):
    """The reading of select_reading_x's points: (n, 4), on the x axis."""
    rd = np.zeros((len(x), 4), x.dtype)
    rd[:, 0] = x
    rd[:, 3] = 1
    return rd


def max_dist_keeping(x, m):
    """A matcher maxDist between the m-th and the (m+1)-th smallest |x| (their
    geometric mean): exactly m points stay within it."""
    s = np.sort(np.abs(np.asarray(x, np.float64)))
    return float(np.sqrt(s[m - 1] * s[m]))


def matched_dists(x, max_dist=np.inf):
    """What the matcher returns for select_reading(x) against the origin:
    fl(x^2), +inf beyond maxDist (squared in T, as libnabo does); (n, 1)."""
    T = x.dtype.type
    d = (x * x).astype(x.dtype)
    if np.isfinite(max_dist):
        d = np.where(d <= T(max_dist) * T(max_dist), d, T(np.inf)).astype(x.dtype)
    return d.reshape(-1, 1)


def key_bits(d):
    """IEEE bit patterns of non-negative distances (the select's keys)."""
    d = np.ascontiguousarray(d)
    return d.view(np.uint32 if d.dtype == np.float32 else np.uint64).ravel()


CHAIN_P2PLANE = """
readingDataPointsFilters:
  - IdentityDataPointsFilter:
matcher:
  KDTreeMatcher:
    knn: {knn}
    epsilon: 0
    maxDist: {maxdist}
outlierFilters:
{filters}
errorMinimizer:
  {minimizer}
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: {maxit}
{diff}
inspector:
  NullInspector
logger:
  NullLogger
"""


def chain_yaml(knn=1, maxdist="inf", filters=(("TrimmedDistOutlierFilter", {"ratio": 0.85}),),
               minimizer="PointToPlaneErrorMinimizer", maxit=40, differential=None, bound=None):
    if filters:
        fl = []
        for name, p in filters:
            if p:
                fl.append(f"  - {name}:\n" + "".join(f"      {k}: {v}\n" for k, v in p.items()))
            else:
                fl.append(f"  - {name}\n")
        ftxt = "".join(fl)
    else:
        ftxt = ""
    diff = ""
    if differential:
        diff = ("  - DifferentialTransformationChecker:\n" +
                "".join(f"      {k}: {v}\n" for k, v in differential.items()))
    if bound:
        diff += ("  - BoundTransformationChecker:\n" +
                 "".join(f"      {k}: {v}\n" for k, v in bound.items()))
    return CHAIN_P2PLANE.format(knn=knn, maxdist=maxdist, filters=ftxt, minimizer=minimizer, maxit=maxit,
                                diff=diff)

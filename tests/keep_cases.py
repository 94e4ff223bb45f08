"""Independent numpy references for the keep-filters: Shadow,
MaxQuantileOnAxis, RemoveNaN, CutAtDescriptorThreshold (device,
csrc/pmx_keep.hip) and MaxDensity, MaxPointCount (host chain, on libc rand()).

Nothing here is imported from the package under test or from the oracle
wrapper.  Each function restates one reference file with file:line notes, every
operation in the arrays' own type and in the reference's order (numpy rounds
each elementwise multiply and add on its own: no fused multiply-add).

Eigen's rules used below (Eigen 3.3):
  dot / squaredNorm of a 2- or 3-vector: a sequential sum c0 + c1 (+ c2)
  normalized(): z = squaredNorm(); z > 0 ? v / sqrt(z) : v   (Dot.h) — a zero
                vector stays zero, a NaN vector stays NaN
"""
import ctypes
import math

import numpy as np

_libc = ctypes.CDLL(None)
_libc.rand.restype = ctypes.c_int
_libc.srand.argtypes = [ctypes.c_uint]
RAND_MAX = 2147483647  # glibc

BLOCK = 256  # points per block of the device compaction (csrc/pmx_keep.hip kKeepBlock)


def srand(seed):
    _libc.srand(seed)


# --------------------------------------------------------------- predicates --
def _seq_dot(a, b):
    s = a[:, 0] * b[:, 0]
    for r in range(1, a.shape[1]):
        s = s + a[:, r] * b[:, r]
    return s


def normalized(v):
    z = _seq_dot(v, v)
    with np.errstate(all="ignore"):
        q = v / np.sqrt(z)[:, None]
    return np.where((z > 0)[:, None], q, v)


def sin_eps(eps, dtype):
    """The Shadow constructor's sin(eps) in T (Shadow.cpp:47)."""
    T = np.dtype(dtype).type
    return T(math.sin(float(T(eps))))


def shadow_value(points, normals):
    """|normalized(normal) . normalized(point)| per point (Shadow.cpp:80-84)."""
    D = points.shape[1] - 1
    assert normals.shape[1] == D and normals.dtype == points.dtype
    with np.errstate(all="ignore"):
        dot = _seq_dot(normalized(normals), normalized(points[:, :D]))
    return np.where(dot < 0, -dot, dot)  # anyabs, Functions.h:44-50


def shadow_keep(points, normals, sin_e):
    return shadow_value(points, normals) > points.dtype.type(sin_e)  # Shadow.cpp:86


def quantile_rank(n, ratio, dtype):
    """size_t(n * ratio), the product in T (MaxQuantileOnAxis.cpp:73, 82)."""
    T = np.dtype(dtype).type
    return min(int(T(n) * T(ratio)), n - 1)


def max_quantile_limit(values, ratio):
    """nth_element at that rank (MaxQuantileOnAxis.cpp:82-83), by np.partition."""
    r = quantile_rank(len(values), ratio, values.dtype)
    return np.partition(values, r)[r]


def max_quantile_keep(points, dim, ratio):
    v = np.ascontiguousarray(points[:, dim])
    if len(v) == 0:
        return np.zeros(0, bool)
    return v < max_quantile_limit(v, ratio)  # strict: MaxQuantileOnAxis.cpp:89


def remove_nan_keep(points):
    """(col == col).all() over every feature row (RemoveNaN.cpp:55-57)."""
    return (points == points).all(axis=1)


def cut_descriptor_keep(desc, row, use_larger_than, threshold):
    """CutAtDescriptorThreshold.cpp:76-99: useLargerThan keeps value <=
    threshold (the larger ones are cut), else value >= threshold."""
    v = desc[:, row]
    t = desc.dtype.type(threshold)
    return v <= t if use_larger_than else v >= t


def compact(points, desc, keep):
    return points[keep], (desc[keep] if desc is not None else None)


# ------------------------------------------------------- rand()-driven ones --
def _rand_unit():
    # (float)rand() / (float)RAND_MAX
    return np.float32(_libc.rand()) / np.float32(RAND_MAX)


def max_density_keep(dens, max_density):
    """MaxDensity.cpp:72-101 on the process's rand() state; dens: (n,) in T.
    nbSaturatedPts / nbPointsIn is an integer division."""
    T = dens.dtype.type
    md = T(max_density)
    n = len(dens)
    keep = np.ones(n, bool)
    if n == 0:
        return keep
    last = dens.max()
    nsat = int((dens == last).sum())
    for i in range(n):
        if dens[i] > md:
            r = _rand_unit()
            accept = np.float32(md / dens[i])
            if dens[i] == last:
                accept = np.float32(accept * np.float32(1 - nsat // n))
            keep[i] = r < accept
    return keep


def max_point_count_sources(n, max_count, seed):
    """MaxPointCount.cpp:70-101: the source column of every output column.
    `const auto feat = cloud.features.col(j)` is a view, so the "switch" writes
    column idx over column j and then column j (already overwritten) back over
    column idx: only column j changes.  None when the filter does nothing."""
    N = n - 1
    if n == 0 or max_count > N:
        return None
    srand(seed)
    src = np.arange(n)
    for j in range(max_count):
        r = np.float32(np.float32(_libc.rand()) / np.float32(RAND_MAX))
        idx = j + int(np.float32(N - j) * r)
        src[j] = src[idx]
    return src[:max_count]


# ------------------------------------------------------------------- scenes --
def pattern_keep(tag, n):
    """Keep patterns where a ballot prefix or a block offset error shows."""
    i = np.arange(n)
    if tag == "all":
        return np.ones(n, bool)
    if tag == "none":
        return np.zeros(n, bool)
    if tag == "alternating":
        return i % 2 == 0
    if tag == "first":
        return i == 0
    if tag == "last":
        return i == n - 1
    if tag == "wave_hole":  # one whole wave dropped between two kept waves, in every block
        return (i % BLOCK) // 64 != 1
    raise KeyError(tag)


PATTERNS = ["all", "none", "alternating", "first", "last", "wave_hole"]
SIZES = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 100003]


def tagged_cloud(n, rows, desc_dim, dtype, seed=0):
    """Random features (homogeneous row 1) and descriptors; every value distinct
    enough that a misplaced column shows."""
    rng = np.random.default_rng(seed + 7 * n + rows)
    f = rng.normal(0, 1, (n, rows)).astype(dtype)
    f[:, rows - 1] = 1
    d = rng.normal(0, 1, (n, desc_dim)).astype(dtype) if desc_dim else None
    return f, d


def shadow_scene(n, D, dtype, sin_e, seed=1, margin=1e-3):
    """Points and unit-ish normals whose |value - sin(eps)| exceeds margin *
    value: drawn at random, then every point inside the margin is moved onto
    its normal's direction (value 1).  The caller asserts the margin."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 3, (n, D))
    nr = rng.normal(0, 1, (n, D))
    pts = np.hstack([p, np.ones((n, 1))]).astype(dtype)
    nr = nr.astype(dtype)
    v = shadow_value(pts, nr).astype(np.float64)
    near = np.abs(v - float(sin_e)) <= 4 * margin * np.maximum(v, float(sin_e))
    pts[near, :D] = nr[near] * dtype(2)
    return pts, nr


def margin_ok(points, normals, sin_e, margin=1e-3):
    v = shadow_value(points, normals).astype(np.float64)
    return np.abs(v - float(sin_e)) > margin * v

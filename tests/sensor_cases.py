"""Independent numpy references, tolerance bars and case builders for the
sensor-bias family of data filters: IncidenceAngle, Sphericality and
RemoveSensorBias (device, csrc/pmx_sensor.hip).

Nothing here is imported from the package under test or from the oracle
wrapper.  Each function restates one reference file with file:line notes, every
operation in the type the reference gives it and in its order (numpy rounds
each elementwise multiply and add on its own: no fused multiply-add).  Eigen's
dot / squaredNorm / normalized() rules are those of keep_cases.py.

Bars.  The device acos / tanf / cosf / sinf / exp are not bit-equal to the
host library's, so IncidenceAngle and the bias correction are compared
within a bar computed here from the reference alone: the reference is
evaluated at the nominal input and again with the argument of its
transcendental moved by +-1 ulp of T (the dot for IncidenceAngle; the incidence
angle and the depth for the correction); the bar is 4 x the largest spread plus
4 ulp of T at the result (IncidenceAngle) or at |p| (the corrected point).  The
margin of 4 stands for the few-ulp accuracy of device math functions.
Sphericality and the kept set of RemoveSensorBias are exact.
"""
import math

import numpy as np

from keep_cases import BLOCK, PATTERNS, normalized, pattern_keep, _seq_dot  # noqa: F401

SIZES = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1]
DTYPES = [np.float32, np.float64]

_exp = np.vectorize(math.exp, otypes=[np.float64])


# ------------------------------------------- correctly rounded double math --
# The double correction cancels: one ulp in cos(theta), erf(.) or a pow moves
# it by millions of ulp (test_sensor_reference.py shows it), and numpy's and the
# C library's cos / tan / erf / pow are neither correctly rounded nor the same
# from one machine to the next.  So, for double arguments, the reference takes
# these functions correctly rounded: evaluated here in double-double arithmetic
# (about 104 bits, error-free sums and products) and rounded once, which is
# the correctly rounded value barring exact values within about 2^-100 of a
# rounding tie.
# test_sensor_reference.py pins every one of them against exact rational
# arithmetic and within one ulp of the C library's.
def _two_sum(a, b):
    s = a + b
    v = s - a
    return s, (a - (s - v)) + (b - v)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b  # Dekker's split, 2^27 + 1
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    return _two_sum(p, e + (a[0] * b[1] + a[1] * b[0]))


def _dd_add(a, b):
    s, e = _two_sum(a[0], b[0])
    return _two_sum(s, e + (a[1] + b[1]))


def _dd_div_d(a, d):
    q = a[0] / d
    p, e = _two_prod(q, d)
    return _two_sum(q, (((a[0] - p) - e) + a[1]) / d)


def _dd_div(a, b):
    q = a[0] / b[0]
    r = _dd_add(a, tuple(-v for v in _dd_mul(b, (q, np.zeros_like(q)))))
    return _two_sum(q, (r[0] + r[1]) / b[0])


_PIO2 = (1.5707963267948966, 6.123233995736766e-17)
_TWO_OVER_SQRT_PI = (1.1283791670955126, 1.533545961316588e-17)


def _dd_sincos(x):
    """(sin, cos) of x in [0, pi / 2] as double-doubles: the Taylor series of
    the argument folded into [0, pi / 4], nested from the fifteenth term."""
    x = np.asarray(x, np.float64)
    assert np.all((x >= 0) & (x <= _PIO2[0]))
    fold = x > 0.7853981633974483
    zero, one = np.zeros_like(x), np.ones_like(x)
    fh, fl = _two_sum(np.full_like(x, _PIO2[0]), -x)
    fh, fl = _two_sum(fh, fl + _PIO2[1])
    r = (np.where(fold, fh, x), np.where(fold, fl, zero))
    y = _dd_mul(r, r)
    c, s = (one, zero), (one, zero)
    for n in range(15, 0, -1):
        c = _dd_add((one, zero), tuple(-v for v in _dd_div_d(_dd_mul(y, c), float((2 * n - 1) * (2 * n)))))
        s = _dd_add((one, zero), tuple(-v for v in _dd_div_d(_dd_mul(y, s), float((2 * n) * (2 * n + 1)))))
    s = _dd_mul(s, r)
    return ((np.where(fold, c[0], s[0]), np.where(fold, c[1], s[1])),
            (np.where(fold, s[0], c[0]), np.where(fold, s[1], c[1])))


def cr_sin_cos_tan(x):
    """sin, cos, tan of doubles in [0, pi / 2], correctly rounded."""
    s, c = _dd_sincos(x)
    with np.errstate(all="ignore"):
        t = _dd_div(s, c)
    return s[0], c[0], t[0]


def cr_erf(x):
    """erf of doubles in [0, 3], correctly rounded: 2 / sqrt(pi) * sum of
    (-1)^n x^(2n+1) / (n! (2n+1)), 80 terms."""
    x = np.asarray(x, np.float64)
    assert np.all((x >= 0) & (x <= 3))
    zero = np.zeros_like(x)
    y = _dd_mul((x, zero), (x, zero))
    t, acc = (x, zero), (x, zero)
    for n in range(1, 80):
        t = _dd_div_d(_dd_mul(t, y), float(n))
        q = _dd_div_d(t, float(2 * n + 1))
        acc = _dd_add(acc, q if n % 2 == 0 else tuple(-v for v in q))
    return _dd_mul(acc, (np.full_like(x, _TWO_OVER_SQRT_PI[0]), np.full_like(x, _TWO_OVER_SQRT_PI[1])))[0]


def cr_pow3(x):
    """x^3 of doubles, correctly rounded."""
    x = np.asarray(x, np.float64)
    return _dd_mul(_two_prod(x, x), (x, np.zeros_like(x)))[0]


def cr_pow3_2(x):
    """x^(3/2) of positive doubles, correctly rounded."""
    x = np.asarray(x, np.float64)
    s = np.sqrt(x)
    p, e = _two_prod(s, s)
    root = _two_sum(s, ((x - p) - e) / (2. * s))
    return _dd_mul(root, (x, np.zeros_like(x)))[0]


# ----------------------------------------------------------- IncidenceAngle --
def incidence_dot(normals, obs):
    """normalized(obs) . normal, sequential in T (IncidenceAngle.cpp:70-72)."""
    assert normals.dtype == obs.dtype and normals.shape == obs.shape
    with np.errstate(all="ignore"):
        return _seq_dot(normalized(obs), normals)


def incidence_angles(normals, obs):
    with np.errstate(all="ignore"):
        return np.arccos(incidence_dot(normals, obs))  # acos in T


def incidence_bar(normals, obs):
    """4 x the spread of acos over dot -+ 1 ulp, plus 4 ulp of the result."""
    T = normals.dtype.type
    dot = incidence_dot(normals, obs)
    ref = np.arccos(dot)
    spread = np.zeros_like(ref)
    for to in (-np.inf, np.inf):
        with np.errstate(all="ignore"):
            moved = np.arccos(np.nextafter(dot, T(to)))
        spread = np.maximum(spread, np.abs(moved - ref))
    return T(4) * spread + T(4) * np.spacing(np.abs(ref))


def incidence_scene(n, D, dtype, seed=3):
    """Unit normals and observation directions of length 0.5 .. 30 with
    |dot| <= 0.999 (the caller asserts it): drawn at random, a pair past the
    limit gets its observation direction turned a quarter."""
    rng = np.random.default_rng(seed + 11 * n + D)
    nr = rng.normal(0, 1, (n, D))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    ob = rng.normal(0, 1, (n, D))
    ob /= np.linalg.norm(ob, axis=1, keepdims=True)
    bad = np.abs((nr * ob).sum(axis=1)) > 0.99
    ob[bad] = np.roll(nr[bad], 1, axis=1) * np.array([1, -1, 1][:D])
    ob *= rng.uniform(0.5, 30, (n, 1))
    return nr.astype(dtype), ob.astype(dtype)


# ------------------------------------------------------------- Sphericality --
def sphericality(eig):
    """(sphericality, unstructureness, structureness) per point, in T
    (Sphericality.cpp:128-176).  eig: (n, 3), any order, no NaN."""
    T = eig.dtype.type
    tiny = np.finfo(eig.dtype).tiny  # numeric_limits<T>::min()
    e = np.sort(eig, axis=1)
    e0, e1, e2 = e[:, 0], e[:, 1], e[:, 2]
    nan = (e2 < tiny) | (e1 < 0) | (e0 < 0)
    zero = ~nan & (e1 < tiny)
    with np.errstate(all="ignore"):
        u = e0 / e2
        s = (e1 / e2) * ((e1 - e0) / np.sqrt(e0 * e0 + e1 * e1))
        sph = u - s
    out = []
    for v in (sph, u, s):
        v = np.where(zero, T(0), v)
        out.append(np.where(nan, T(np.nan), v).astype(eig.dtype))
    return tuple(out)


SPH_TABLE = [
    # eigenvalues, branch
    ((0, 0, 0), "nan"), ((0, 0, 1), "zero"), ((1, 1, 1), "value"), ((-1, 1, 2), "nan"), ((1, -1e-3, 2), "nan"),
    ((1, 2, 4), "value"), ((4, 1, 2), "value"), ((2, 4, 1), "value"), ((0, 1, 2), "value"), ((0, 3, 0), "zero"),
    ((0.25, 0.5, 0.125), "value"), ((5, 0, 7), "value"), ((1e-3, 1e3, 1), "value"),
]


def sphericality_scene(n, dtype, seed=5):
    """Random unsorted triples over six decades with every branch mixed in: the
    table above, triples below numeric_limits<T>::min() and negative ones."""
    rng = np.random.default_rng(seed + n)
    e = (10.0 ** rng.uniform(-3, 3, (n, 3))).astype(dtype)
    tiny = np.finfo(dtype).tiny
    special = [list(t) for t, _ in SPH_TABLE] + [[tiny / 2, tiny / 4, 0], [tiny / 2, 0, 1], [tiny, tiny, tiny],
                                                 [tiny, 2 * tiny, 1], [-0.0, 1, 2], [1, 2, -tiny]]
    for j, i in enumerate(range(0, n, 3)):
        e[i] = np.asarray(special[j % len(special)], dtype)
    return e


# --------------------------------------------------------- RemoveSensorBias --
SENSORS = {0: (0.0075049, 6.08040951e+00, 3.17921789e-03),   # LMS_1XX: aperture, k1, k2 (RemoveSensorBias.h:107-109)
           1: (0.0014835, 1.03211569e+01, 7.07893371e-03)}   # HDL_32E (:111-113)
TAU = 50e-9             # s, pulse length (RemoveSensorBias.h:94-97)
PULSE_INTENSITY = 0.39
LAMBDA_LIGHT = 905e-9
C_LIGHT = 299792458.0
EPSILON = 1e-5          # RemoveSensorBias.cpp:158


def angle_threshold(degrees, dtype):
    """The constructor's T(T(degrees) / 180. * M_PI) (RemoveSensorBias.cpp:52)."""
    T = np.dtype(dtype).type
    return T(float(T(degrees)) / 180. * math.pi)


def coefficients(depth, theta, aperture):
    """a1, a2, a3 of getCoefficients (RemoveSensorBias.cpp:132-153).  depth:
    float64 array; theta: array of the cloud's type, whose tan / cos / sin are
    taken in that type and widen where they meet a double.  theta in
    [0, pi / 2], aperture * sqrt(A) <= 3 (the correctly rounded functions'
    ranges: every kept angle, depths to some 60 m)."""
    assert depth.dtype == np.float64
    c = C_LIGHT
    sigma = TAU / math.sqrt(2. * math.pi)
    w0 = LAMBDA_LIGHT / (math.pi * aperture)
    valid = (theta >= 0) & (theta <= _PIO2[0])  # (NaN: false) the others are never kept: NaN coefficients
    theta = np.where(valid, theta, theta.dtype.type(0))
    if theta.dtype == np.float64:
        sn, cs, tn = cr_sin_cos_tan(theta)
    else:  # float calls, widened
        assert np.tan(theta).dtype == theta.dtype
        tn = np.tan(theta).astype(np.float64)
        cs = np.cos(theta).astype(np.float64)
        sn = np.sin(theta).astype(np.float64)
    with np.errstate(all="ignore"):
        A = 2. * np.power(depth * tn, 2) / math.pow(sigma * c, 2) + 2. / math.pow(aperture, 2)
        K1 = cr_pow3(cs)
        K2 = 3. * np.power(cs, 2) * sn
        x = aperture * np.sqrt(A)
        valid &= x <= 3
        L1 = (PULSE_INTENSITY * np.power(w0 / (aperture * depth * cs), 2) * math.sqrt(math.pi) *
              cr_erf(np.where(valid, x, 0.)) / (2. * cr_pow3_2(A)))
        L2 = PULSE_INTENSITY * np.power(w0 / (aperture * depth * cs), 2) * K2 / (2. * A)
        a1 = -(2. * tn * depth *
               (L1 * K2 - 2. * L2 * aperture * _exp(-A * math.pow(aperture, 2)))) / (math.pow(sigma, 2) * c)
        a2 = (-L1 * 2. * A * K1 *
              (np.power(sigma * c * cs, 2) * A + 2. * np.power(cs * depth, 2) - 2. * np.power(depth, 2)) /
              (2 * np.power(c * cs, 2) * math.pow(sigma, 4) * A))
        a3 = (L1 * K2 * depth * tn * (math.pow(sigma * c, 2) * A - 2. * np.power(depth * tn, 2)) /
              (math.pow(sigma, 6) * math.pow(c, 3) * A))
    return tuple(np.where(valid, a, np.nan) for a in (a1, a2, a3))


def discriminant(depth, theta, sensor_type):
    a1, a2, a3 = coefficients(depth, theta, SENSORS[sensor_type][0])
    return 4 * np.power(a2, 2) - 12 * a1 * a3


def correction(depth, theta, sensor_type):
    """k1 * diffDist + k2 * ratioCurvature, in double (RemoveSensorBias.cpp:119, 155-187)."""
    aperture, k1, k2 = SENSORS[sensor_type]
    n = len(theta)  # (a and b = getCoefficients(depth, 0., aperture) in one evaluation)
    a1, a2, a3 = coefficients(np.concatenate([depth, depth]), np.concatenate([theta, np.zeros_like(theta)]), aperture)
    b2 = a2[n:]
    a1, a2, a3 = a1[:n], a2[:n], a3[:n]
    with np.errstate(all="ignore"):
        t = (-2 * a2 - np.sqrt(4 * np.power(a2, 2) - 12 * a1 * a3)) / (6 * a3)
        tmax = np.where(theta.astype(np.float64) < EPSILON, 0., t)
        diff = tmax * C_LIGHT / 2.
        ratio = 1. - 2 * b2 / (2 * a2 + 6 * tmax * a3)
        return k1 * diff + k2 * ratio


def bias_keep(inc, threshold):
    """not isnan(inc) and inc >= 0 and inc < angleThreshold (RemoveSensorBias.cpp:117)."""
    with np.errstate(invalid="ignore"):
        return ~np.isnan(inc) & (inc >= 0) & (inc < inc.dtype.type(threshold))


def bias_corrected(points, inc, obs, sensor_type, move_theta=0.0, move_depth=0.0):
    """Every point corrected as if it were kept (RemoveSensorBias.cpp:110-123):
    p + T(correction) * normalized(obs), depth = |obs| formed in T.
    move_theta / move_depth (scalars or one per point): -inf or +inf moves that
    argument of the correction by one ulp of T (the bars)."""
    T = points.dtype.type
    D = points.shape[1] - 1
    assert obs.shape[1] == D and obs.dtype == points.dtype and inc.dtype == points.dtype
    with np.errstate(all="ignore"):
        depth = np.sqrt(_seq_dot(obs, obs))
        mt = np.broadcast_to(np.asarray(move_theta, points.dtype), inc.shape)
        md = np.broadcast_to(np.asarray(move_depth, points.dtype), inc.shape)
        theta = np.where(mt == 0, inc, np.nextafter(inc, mt))
        depth = np.where(md == 0, depth, np.nextafter(depth, md))
        corr = correction(depth.astype(np.float64), theta, sensor_type).astype(points.dtype)
        out = points.copy()
        out[:, :D] = points[:, :D] + corr[:, None] * normalized(obs)
    return out


def remove_sensor_bias(points, desc, inc_row, obs_row, sensor_type, threshold):
    """(features, descriptors, keep) of the filter: the kept points corrected,
    their descriptors unchanged, in their input order."""
    D = points.shape[1] - 1
    inc = np.ascontiguousarray(desc[:, inc_row])
    keep = bias_keep(inc, threshold)
    out = bias_corrected(points[keep], inc[keep], np.ascontiguousarray(desc[keep, obs_row:obs_row + D]), sensor_type)
    return out, desc[keep], keep


def bias_bar(points, desc, inc_row, obs_row, sensor_type):
    """Per point and coordinate: 4 x the largest spread of the corrected point
    over theta -+ 1 ulp and depth -+ 1 ulp, plus 4 ulp of T at |p|."""
    T = points.dtype.type
    D = points.shape[1] - 1
    inc = np.ascontiguousarray(desc[:, inc_row])
    obs = np.ascontiguousarray(desc[:, obs_row:obs_row + D])
    moves = ((0, 0), (-np.inf, 0), (np.inf, 0), (0, -np.inf), (0, np.inf))  # nominal first; one evaluation for all
    n = len(points)
    out = bias_corrected(np.tile(points, (5, 1)), np.tile(inc, 5), np.tile(obs, (5, 1)), sensor_type,
                         move_theta=np.repeat([m[0] for m in moves], n), move_depth=np.repeat([m[1] for m in moves], n))
    ref = out[:n]
    spread = np.zeros_like(ref)
    for k in range(1, 5):
        spread = np.maximum(spread, np.abs(out[k * n:(k + 1) * n] - ref))
    norm = np.sqrt((points[:, :D].astype(np.float64) ** 2).sum(axis=1)).astype(points.dtype)
    return T(4) * spread + T(4) * np.spacing(norm)[:, None]


DROPPED = ["nan", "negative", "threshold", "above"]  # what a dropped point's angle is, in turn


def bias_scene(n, D, dtype, wide, keep, threshold_deg=88.0, seed=9):
    """A cloud for RemoveSensorBias: descriptors [tag, incidenceAngles,
    observationDirections (D)] and, wide, five more random rows (widths 2 + D
    and 2 + D + 5).  keep (n bools) is imposed through the angle row: kept
    points get an angle in [1e-3, threshold - 1e-3], dropped ones a NaN, a
    negative angle, exactly the threshold or a larger angle, in turn.
    Observation directions are sensor - point, 1 .. 30 long.
    Returns points, desc, inc_row, obs_row."""
    rng = np.random.default_rng(seed + 13 * n + D + (5 if wide else 0))
    T = np.dtype(dtype).type
    thr = angle_threshold(threshold_deg, dtype)
    direction = rng.normal(0, 1, (n, D))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    p = direction * rng.uniform(1, 30, (n, 1))
    pts = np.hstack([p, np.ones((n, 1))]).astype(dtype)
    inc = rng.uniform(1e-3, float(thr) - 1e-3, n).astype(dtype)
    drop = np.nonzero(~keep)[0]
    for j, i in enumerate(drop):
        inc[i] = {"nan": T(np.nan), "negative": T(-0.25), "threshold": thr,
                  "above": T(float(thr) + 0.01)}[DROPPED[j % len(DROPPED)]]
    cols = [np.arange(n, dtype=dtype)[:, None], inc[:, None], (-pts[:, :D]).astype(dtype)]
    if wide:
        cols.append(rng.normal(0, 1, (n, 5)).astype(dtype))
    return pts, np.ascontiguousarray(np.hstack(cols)) if n else np.zeros((0, 2 + D + (5 if wide else 0)), dtype), 1, 2

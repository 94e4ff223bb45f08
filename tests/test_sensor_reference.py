"""The numpy references of sensor_cases.py (IncidenceAngle, Sphericality,
RemoveSensorBias) pinned on hand-checkable values, without a GPU, and the
tolerance bars the GPU tests use: finite and non-zero for every case, so a GPU
failure cannot hide behind an infinite bar, and every case away from the
ill-conditioned corners.
"""
import math

import numpy as np
import pytest

import keep_cases as kc
import sensor_cases as sc


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_incidence_angle_by_hand(dtype):
    T = dtype
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 0]], T)
    obs = np.array([[0, 0, 2], [3, 0, 0], [0, 0, 0], [0, 0, -5], [0, 3, 4]], T)
    got = sc.incidence_angles(nrm, obs)
    # head-on, grazing, a zero observation vector (it stays zero: the dot is 0), from behind, 3-4-5
    want = [T(0), np.arccos(T(0)), np.arccos(T(0)), np.arccos(T(-1)), np.arccos(T(3) / T(5))]
    assert got.dtype == np.dtype(T) and list(got) == want
    assert float(got[1]) == pytest.approx(math.pi / 2, rel=1e-6) and float(got[3]) == pytest.approx(math.pi, rel=1e-6)
    got2 = sc.incidence_angles(nrm[:, 1:], obs[:, 1:])  # 2-D: the same vectors without x
    assert list(got2[[0, 3, 4]]) == [want[0], want[3], want[4]]


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_sphericality_by_hand(dtype):
    T = dtype
    eig = np.array([t for t, _ in sc.SPH_TABLE], T)
    sph, un, st = sc.sphericality(eig)
    for i, (t, branch) in enumerate(sc.SPH_TABLE):
        if branch == "nan":
            assert np.isnan(sph[i]) and np.isnan(un[i]) and np.isnan(st[i]), t
        elif branch == "zero":
            assert sph[i] == 0 and un[i] == 0 and st[i] == 0, t
        else:
            assert np.isfinite(sph[i]) and sph[i] == un[i] - st[i], t
    row = {t: i for i, (t, _) in enumerate(sc.SPH_TABLE)}
    i = row[(1, 1, 1)]
    assert (sph[i], un[i], st[i]) == (1, 1, 0)  # 1 - 0
    i = row[(1, 2, 4)]
    want_s = (T(2) / T(4)) * ((T(2) - T(1)) / np.sqrt(T(1) * T(1) + T(2) * T(2)))
    assert un[i] == T(0.25) and st[i] == want_s and sph[i] == T(0.25) - want_s
    for t in [(4, 1, 2), (2, 4, 1)]:  # the order of the triple does not matter
        assert (sph[row[t]], un[row[t]], st[row[t]]) == (sph[i], un[i], st[i])
    i = row[(0, 1, 2)]  # e0 = 0: a perfect plane or line, u = 0, s = (1 / 2) * (1 / 1)
    assert (sph[i], un[i], st[i]) == (T(-0.5), 0, T(0.5))
    tiny = np.finfo(T).tiny
    sph, _, _ = sc.sphericality(np.array([[tiny / 2, tiny / 2, tiny / 2], [tiny / 2, tiny / 2, 1], [tiny, tiny, tiny]], T))
    # below min(): NaN; two below and one above: 0; all at min(): the squares underflow, (e1 - e0) / sqrt(0) = 0 / 0
    assert np.isnan(sph[0]) and sph[1] == 0 and np.isnan(sph[2])


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("sensor", [0, 1])
def test_bias_correction_small_angle(dtype, sensor):
    """theta < 1e-5: Tmax = 0, so diffDist = 0 and the correction is
    k2 * (1 - b2 / a2); at theta = 0 a == b and it is exactly 0."""
    T = dtype
    aperture, k1, k2 = sc.SENSORS[sensor]
    depth = np.array([1.0, 7.5, 30.0])
    for theta in (T(0), T(5e-6)):
        th = np.full(3, theta, T)
        _, a2, _ = sc.coefficients(depth, th, aperture)
        _, b2, _ = sc.coefficients(depth, np.zeros(3, T), aperture)
        got = sc.correction(depth, th, sensor)
        assert np.array_equal(got, k2 * (1. - 2 * b2 / (2 * a2)))
        if theta == 0:
            assert np.array_equal(a2, b2) and np.all(got == 0)
    # past the switch the first term is there
    assert np.all(np.abs(sc.correction(depth, np.full(3, 0.5, T), sensor)) > 1e-5)


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_bias_correction_magnitude(dtype):
    """Sanity against the model's published scale: millimetres at 30 degrees,
    centimetres at 80, growing with the angle."""
    th = np.array([0.1, 0.5, 1.0, 1.4], dtype)
    for sensor in (0, 1):
        c = -sc.correction(np.full(4, 10.0), th, sensor)
        assert np.all(np.diff(c) > 0) and 1e-5 < c[0] < 1e-4 and 5e-4 < c[1] < 2e-3 and 1e-2 < c[3] < 1e-1


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_bias_keep_rule(dtype):
    T = dtype
    thr = sc.angle_threshold(88., T)
    inc = np.array([np.nan, -0.25, -0.0, 0, 0.5, np.nextafter(thr, T(0)), thr, np.nextafter(thr, T(4)), np.inf], T)
    assert list(sc.bias_keep(inc, thr)) == [False, False, True, True, True, True, False, False, False]
    assert float(thr) == pytest.approx(88 / 180 * math.pi, rel=1e-6)
    pts = np.ones((9, 4), T)
    desc = np.hstack([np.arange(9, dtype=T)[:, None], inc[:, None], -pts[:, :3]])
    f, d, keep = sc.remove_sensor_bias(pts, desc, 1, 2, 0, thr)
    assert list(d[:, 0]) == [2, 3, 4, 5] and np.array_equal(f[:, 3], np.ones(4, T))
    assert np.array_equal(f[:2], pts[2:4])  # theta = 0: the correction is exactly 0


def _bias_cases():
    for dtype in sc.DTYPES:
        for D in (2, 3):
            for n in sc.SIZES:
                for tag in ("all", "alternating"):
                    yield dtype, D, n, tag


def test_bars_are_finite_and_cases_well_conditioned():
    for dtype in sc.DTYPES:
        T = dtype
        thr = sc.angle_threshold(88., T)
        for D in (2, 3):
            for n in sc.SIZES:
                nrm, obs = sc.incidence_scene(n, D, T)
                bar = sc.incidence_bar(nrm, obs)
                assert np.all(np.isfinite(bar)) and np.all(bar > 0)
                assert np.all(np.abs(sc.incidence_dot(nrm, obs)) <= 0.999)
                assert np.all(bar <= 64 * np.finfo(T).eps * np.pi)  # 1 / sqrt(1 - 0.999^2) = 22
    for dtype, D, n, tag in _bias_cases():
        keep = kc.pattern_keep(tag, n)
        thr = sc.angle_threshold(88., dtype)
        for wide in (False, True):
            for sensor in (0, 1):
                pts, desc, ir, orow = sc.bias_scene(n, D, dtype, wide, keep)
                assert desc.shape == (n, 2 + D + (5 if wide else 0))
                assert np.array_equal(sc.bias_keep(desc[:, ir], thr), keep)
                inc = desc[keep, ir]
                assert np.all(inc >= 1e-3) and np.all(inc <= float(thr) - 1e-3 + 1e-6)
                depth = np.sqrt((desc[keep, orow:orow + D].astype(np.float64) ** 2).sum(axis=1))
                assert np.all(sc.discriminant(depth, np.ascontiguousarray(inc), sensor) > 0)
                bar = sc.bias_bar(pts[keep], desc[keep], ir, orow, sensor)
                assert np.all(np.isfinite(bar)) and np.all(bar > 0)


# ------------------------------------------- correctly rounded double math --
_SQRT_PI = "1.77245385090551602729816748334114518279754945612238712821381"


def _series(x, kind):
    """sin / cos / erf of a double in exact rational arithmetic, to 2^-160."""
    from fractions import Fraction
    x = Fraction(x)
    y, total, n = x * x, Fraction(0), 0
    term = Fraction(1) if kind == "cos" else x
    while abs(term) > Fraction(1, 2 ** 160):
        total += term / (2 * n + 1) if kind == "erf" else term
        n += 1
        term = -term * y / {"cos": (2 * n - 1) * (2 * n), "sin": (2 * n) * (2 * n + 1), "erf": n}[kind]
    return total * 2 / Fraction(_SQRT_PI) if kind == "erf" else total


def test_correctly_rounded_functions_against_exact_arithmetic():
    from fractions import Fraction
    rng = np.random.default_rng(4)
    th = np.concatenate([rng.uniform(0, 1.5707, 120), [0, 1e-3, 0.7853981633974483, 0.7853981633974484, 1.5359]])
    s, c, t = sc.cr_sin_cos_tan(th)
    for x, gs, gc, gt in zip(th, s, c, t):
        es, ec = _series(float(x), "sin"), _series(float(x), "cos")
        assert (gs, gc, gt) == (float(es), float(ec), float(es / ec)), x
        assert abs(gc - math.cos(x)) <= np.spacing(gc) and abs(gt - math.tan(x)) <= np.spacing(gt)
    x = np.concatenate([rng.uniform(0, 3, 60), [0, 1.41, 3]])
    for v, g in zip(x, sc.cr_erf(x)):
        assert g == float(_series(float(v), "erf")), v
        assert abs(g - math.erf(v)) <= np.spacing(g)
    a = 10.0 ** rng.uniform(3, 7, 100)
    for v, g3, g32 in zip(a, sc.cr_pow3(1 / np.sqrt(a)), sc.cr_pow3_2(a)):
        w = float(1 / np.sqrt(v))
        assert g3 == float(Fraction(w) ** 3)
        # x^(3/2) = q: the nearest double to sqrt(x^3), decided by squaring its neighbours' midpoints
        lo, hi = (Fraction(g32) + Fraction(float(np.nextafter(g32, 0)))) / 2, \
                 (Fraction(g32) + Fraction(float(np.nextafter(g32, np.inf)))) / 2
        assert lo * lo < Fraction(v) ** 3 < hi * hi


def test_one_ulp_of_cos_moves_the_double_correction_past_its_bar():
    """Why the double reference takes correctly rounded functions: the bar of
    a double cloud is a few ulp of |p|, and a cos(theta) one ulp off — inside
    any math library's accuracy — moves the reference itself far past it."""
    n = 255
    pts, desc, ir, orow = sc.bias_scene(n, 3, np.float64, False, np.ones(n, bool))
    inc, obs = np.ascontiguousarray(desc[:, ir]), np.ascontiguousarray(desc[:, orow:orow + 3])
    ref = sc.bias_corrected(pts, inc, obs, 1)
    bar = sc.bias_bar(pts, desc, ir, orow, 1)
    true = sc.cr_sin_cos_tan
    try:
        sc.cr_sin_cos_tan = lambda x: (lambda s, c, t: (s, np.nextafter(c, np.inf), t))(*true(x))
        off = sc.bias_corrected(pts, inc, obs, 1)
    finally:
        sc.cr_sin_cos_tan = true
    assert (np.abs(off - ref)[:, :3] / bar[:, :3]).max() > 1e4

"""IncidenceAngle, Sphericality and RemoveSensorBias on the GPU
(pmx_incidence_angles, pmx_sphericality, pmx_remove_sensor_bias;
csrc/pmx_sensor.hip) against the numpy references of sensor_cases.py.

Bars: Sphericality bit-identical (NaNs by position); the kept count, kept
indices, descriptors and homogeneous row of RemoveSensorBias bit-identical (the
keep decision uses no transcendental); IncidenceAngle and the corrected
coordinates within the bars of sensor_cases.py, derived from the reference
alone (4 x its spread over +-1 ulp of the transcendental's argument plus 4 ulp)
and checked finite, non-zero and well-conditioned in test_sensor_reference.py.
Every test prints the largest deviation as a fraction of its bar.
"""
import numpy as np
import pytest

import keep_cases as kc
import sensor_cases as sc
from libpointmatcher_amd import _capi

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(a.view(u), b.view(u))


def same_values(a, b):
    """Equal bit for bit, any NaN for a NaN."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and same_bits(np.where(na, 0, a), np.where(nb, 0, b))


# ----------------------------------------------------------- IncidenceAngle --
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_incidence_angles(dtype, D):
    worst = 0.0
    for n in sc.SIZES:
        nrm, obs = sc.incidence_scene(n, D, dtype)
        assert np.all(np.abs(sc.incidence_dot(nrm, obs)) <= 0.999)
        got = _capi.incidence_angles(nrm, obs)
        want, bar = sc.incidence_angles(nrm, obs), sc.incidence_bar(nrm, obs)
        assert got.shape == (n,) and got.dtype == np.dtype(dtype)
        frac = np.abs(got - want) / bar
        worst = max(worst, float(frac.max()) if n else 0.0)
        assert np.all(frac <= 1), f"n {n}: {frac.max()} of the bar"
    print(f"incidence angle {np.dtype(dtype).name} D {D}: largest deviation {worst:.3f} of the bar")


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_incidence_angles_exact_cases(dtype):
    """|dot| = 1, 0 and a zero observation vector.  The dot is exact there, so
    the bar has no spread term (and none could be formed past |dot| = 1): head-on
    is exactly 0, the others within the bar's 4 ulp of the result."""
    T = dtype
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], T)
    obs = np.array([[0, 0, 4], [0, 0, -2], [8, 0, 0], [0, 0, 0]], T)
    for cols in (slice(0, 3), slice(1, 3)):
        got = _capi.incidence_angles(nrm[:, cols], obs[:, cols])
        want = sc.incidence_angles(nrm[:, cols], obs[:, cols])
        assert got[0] == 0 and want[0] == 0
        assert np.all(np.abs(got[1:] - want[1:]) <= dtype(4) * np.spacing(want[1:]))


# ------------------------------------------------------------- Sphericality --
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_sphericality_bit_identical(dtype):
    for n in sc.SIZES:
        eig = sc.sphericality_scene(n, dtype)
        sph, un, st = sc.sphericality(eig)
        if n >= 63:
            nan = np.isnan(sph)
            assert nan.any() and (sph == 0).any() and (~nan & (sph != 0)).any()  # every branch
        got = _capi.sphericality(eig, keep_unstructureness=True, keep_structureness=True)
        assert same_values(got["sphericality"], sph), n
        assert same_values(got["unstructureness"], un), n
        assert same_values(got["structureness"], st), n
        only = _capi.sphericality(eig)
        assert list(only) == ["sphericality"] and same_values(only["sphericality"], sph)
        one = _capi.sphericality(eig, keep_structureness=True)
        assert list(one) == ["sphericality", "structureness"] and same_values(one["structureness"], st)


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_sphericality_table(dtype):
    eig = np.array([t for t, _ in sc.SPH_TABLE], dtype)
    got = _capi.sphericality(eig, True, True)
    for name, want in zip(("sphericality", "unstructureness", "structureness"), sc.sphericality(eig)):
        assert same_values(got[name], want), name


# --------------------------------------------------------- RemoveSensorBias --
def check_bias(got, pts, desc, ir, orow, sensor, keep, what):
    gf, gd = got
    D = pts.shape[1] - 1
    thr = sc.angle_threshold(88., pts.dtype)
    ef, ed, ekeep = sc.remove_sensor_bias(pts, desc, ir, orow, sensor, thr)
    assert np.array_equal(ekeep, keep), what
    assert len(gf) == int(keep.sum()) and len(gd) == len(gf), what
    assert same_bits(gd, ed), what                      # descriptors (the tag row: the kept indices) unchanged
    assert same_bits(gf[:, D], pts[keep][:, D]), what   # the homogeneous row
    if not len(gf):
        return 0.0
    bar = sc.bias_bar(pts[keep], desc[keep], ir, orow, sensor)[:, :D]
    frac = np.abs(gf[:, :D] - ef[:, :D]) / bar
    assert np.all(frac <= 1), f"{what}: {frac.max()} of the bar"  # (a NaN on either side fails here)
    return float(frac.max())


@pytest.mark.parametrize("sensor", [0, 1])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_remove_sensor_bias(dtype, D, sensor):
    """Every size around the wave and the block, every keep pattern imposed
    through the incidence-angle row, descriptor widths 2 + D and 2 + D + 5.

    Measured on the MI355X, largest deviation as a fraction of the bar: float
    0.083 - 0.125; double 0.000 (bit-equal: both sides take the double
    functions correctly rounded, sensor_cases.py)."""
    worst = 0.0
    for wide in (False, True):
        for n in sc.SIZES:
            for tag in sc.PATTERNS:
                keep = kc.pattern_keep(tag, n)
                pts, desc, ir, orow = sc.bias_scene(n, D, dtype, wide, keep)
                what = f"{np.dtype(dtype).name} D {D} sensor {sensor} wide {wide} n {n} {tag}"
                got = _capi.remove_sensor_bias(pts, desc, ir, orow, sensor, 88.0)
                frac = check_bias(got, pts, desc, ir, orow, sensor, keep, what)
                worst = max(worst, frac)
    print(f"sensor bias {np.dtype(dtype).name} D {D} sensor {sensor}: largest deviation {worst:.3f} of the bar")


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_remove_sensor_bias_every_point_dropped(dtype):
    n = kc.BLOCK + 1
    pts, desc, ir, orow = sc.bias_scene(n, 3, dtype, False, np.zeros(n, bool))
    for fill in (None, np.nan):  # NaN, negative, the threshold and above in turn; then every angle NaN
        if fill is not None:
            desc[:, ir] = fill
        gf, gd = _capi.remove_sensor_bias(pts, desc, ir, orow)
        assert gf.shape == (0, 4) and gd.shape == (0, desc.shape[1])


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_remove_sensor_bias_zero_angle_is_exact(dtype):
    """theta < 1e-5 takes Tmax = 0; at theta = 0 the two coefficient sets are
    the same numbers and the correction is exactly 0: the points stay."""
    for D in (2, 3):
        n = 65
        pts, desc, ir, orow = sc.bias_scene(n, D, dtype, True, np.ones(n, bool))
        desc[:, ir] = 0
        desc[::2, ir] = -0.0
        gf, gd = _capi.remove_sensor_bias(pts, desc, ir, orow, 1)
        assert same_bits(gf, pts) and same_bits(gd, desc)
        ef, _, _ = sc.remove_sensor_bias(pts, desc, ir, orow, 1, sc.angle_threshold(88., dtype))
        assert same_bits(ef, pts)


@pytest.mark.parametrize("sensor", [0, 1])
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_remove_sensor_bias_small_angle_switch(dtype, sensor):
    """Kept points on both sides of the switch at theta < 1e-5
    (RemoveSensorBias.cpp:158-166), next to ordinary ones at 0.3.  Below it
    Tmax = 0 and the correction is k2 * (1 - b2 / a2), asserted of the reference
    here.  Just above it the root's numerator -2 a2 - sqrt(4 a2^2 - 12 a1 a3)
    cancels to exactly 0 in double, so the two branches give the same number
    there (asserted too): the value of epsilon cannot be read off the results,
    only that neither branch yields a NaN or leaves the bar."""
    for D in (2, 3):
        n = 64
        pts, desc, ir, orow = sc.bias_scene(n, D, dtype, False, np.ones(n, bool))
        desc[:, ir] = np.tile(np.array([5e-6, 9.99e-6, 1.01e-5, 0.3], dtype), n // 4)
        inc = np.ascontiguousarray(desc[:, ir])
        below, near = inc < 1e-5, inc < 1e-4
        aperture, _, k2 = sc.SENSORS[sensor]
        depth = np.sqrt(sc._seq_dot(desc[:, orow:orow + D], desc[:, orow:orow + D])).astype(np.float64)
        _, a2, _ = sc.coefficients(depth, inc, aperture)
        _, b2, _ = sc.coefficients(depth, np.zeros(n, dtype), aperture)
        want = sc.correction(depth, inc, sensor)
        assert below.sum() == n // 2 and near.sum() == 3 * n // 4
        assert np.array_equal(want[near], (k2 * (1. - 2 * b2 / (2 * a2)))[near])
        assert np.all(np.abs(want[near]) < 1e-9) and np.all(np.abs(want[~near]) > 1e-4)
        got = _capi.remove_sensor_bias(pts, desc, ir, orow, sensor)
        frac = check_bias(got, pts, desc, ir, orow, sensor, np.ones(n, bool), f"{np.dtype(dtype).name} D {D}")
        print(f"small angles {np.dtype(dtype).name} D {D} sensor {sensor}: {frac:.3f} of the bar")


# -------------------------------------------------------------------- errors --
def test_bad_parameters():
    keep = np.ones(10, bool)
    pts, desc, ir, orow = sc.bias_scene(10, 3, np.float32, False, keep)
    nrm, obs = sc.incidence_scene(10, 3, np.float32)
    bad = [
        lambda: _capi.incidence_angles(np.ones((10, 4), np.float32), np.ones((10, 4), np.float32)),   # span 4
        lambda: _capi.incidence_angles(nrm[:, :1], obs[:, :1]),                                       # span 1
        lambda: _capi.remove_sensor_bias(pts, desc, 5, orow),       # the angle row past the 5 descriptor rows
        lambda: _capi.remove_sensor_bias(pts, desc, -1, orow),
        lambda: _capi.remove_sensor_bias(pts, desc, ir, 3),         # rows 3 .. 5 of 5
        lambda: _capi.remove_sensor_bias(pts, desc, ir, -1),
        lambda: _capi.remove_sensor_bias(pts, None, 0, 0),
        lambda: _capi.remove_sensor_bias(pts, desc, ir, orow, 2),   # sensor type
        lambda: _capi.remove_sensor_bias(pts, desc, ir, orow, -1),
        lambda: _capi.remove_sensor_bias(np.ones((10, 5), np.float32), desc, ir, orow),
        lambda: _capi.remove_sensor_bias(pts[:0], desc[:0], ir, orow, 2),   # the same checks on an empty cloud
    ]
    bad += [
        lambda: _capi.remove_sensor_bias(pts[:, 0], desc, ir, orow),         # 1-D points
        lambda: _capi.remove_sensor_bias(pts, desc[:5], ir, orow),           # fewer descriptor rows than points
        lambda: _capi.remove_sensor_bias(pts, desc[:, 0], ir, orow),         # 1-D descriptors
    ]
    for call in bad:
        with pytest.raises(_capi.InvalidParameter) as e:
            call()
        assert str(e.value)
    with pytest.raises(_capi.InvalidParameter, match="cannot remove bias for sensorType id 2"):
        _capi.remove_sensor_bias(pts, desc, ir, orow, 2)
    # an empty cloud itself is a result
    gf, gd = _capi.remove_sensor_bias(pts[:0], desc[:0], ir, orow)
    assert gf.shape == (0, 4) and gd.shape == (0, 5)
    assert _capi.incidence_angles(nrm[:0], obs[:0]).shape == (0,)
    assert _capi.sphericality(np.zeros((0, 3), np.float64))["sphericality"].shape == (0,)

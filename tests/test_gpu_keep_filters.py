"""The keep-filters on the GPU (pmx_keep_filter, csrc/pmx_keep.hip) against the
numpy references of keep_cases.py, bit for bit, and the five icp_data
configurations that use them, run unchanged.

Bars: kept count, features and descriptors identical to the reference (the
predicates are evaluated in T in the reference's order on both sides; the
Shadow scenes keep every decision 1e-3 away from the threshold, asserted here
from the reference alone); the icp_data runs below the project's bar, the
reference's own (utest/utest.cpp:81-160: median relative displacement < 3 %).
"""
import ctypes

import numpy as np
import pytest

import keep_cases as kc
from helpers import hom, rel_displacement
from libpointmatcher_amd import _capi
from libpointmatcher_amd.icp import ICP

pytestmark = pytest.mark.gpu

_libc = ctypes.CDLL(None)
DTYPES = [np.float32, np.float64]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(a.view(u), b.view(u))


def check(got, pts, desc, keep, what):
    gf, gd = got
    ef, ed = kc.compact(pts, desc, keep)
    assert len(gf) == int(keep.sum()), what
    assert same_bits(gf, ef), what
    if desc is not None:
        assert same_bits(gd, ed), what
    else:
        assert gd.shape == (len(ef), 0), what


# ---------------------------------------------------------------- compaction --
@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compaction_patterns(dtype, rows):
    """Every size around the wave and the block, every keep pattern, descriptor
    widths 0, 1 and 7.  The pattern is imposed through RemoveNaN (a NaN in one
    feature row of each dropped point), and again through
    CutAtDescriptorThreshold where there is a descriptor to carry it."""
    for desc_dim in (0, 1, 7):
        for n in kc.SIZES:
            base_f, base_d = kc.tagged_cloud(n, rows, desc_dim, dtype)
            for tag in kc.PATTERNS:
                keep = kc.pattern_keep(tag, n)
                what = f"{np.dtype(dtype).name} rows {rows} desc {desc_dim} n {n} {tag}"
                f = base_f.copy()
                f[~keep, (n + rows) % rows] = np.nan
                assert np.array_equal(kc.remove_nan_keep(f), keep)
                check(_capi.keep_filter(f, base_d, _capi.KEEP_REMOVE_NAN), f, base_d, keep, "RemoveNaN " + what)
                if desc_dim:
                    d = base_d.copy()
                    row = desc_dim - 1
                    d[:, row] = np.where(keep, 0.25, 0.75)
                    assert np.array_equal(kc.cut_descriptor_keep(d, row, True, 0.5), keep)
                    check(_capi.keep_filter(base_f, d, _capi.KEEP_CUT_DESCRIPTOR, index=row, flag=1, value=0.5),
                          base_f, d, keep, "Cut " + what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_at_descriptor_threshold_senses_and_equality(dtype):
    n = 2 * kc.BLOCK + 1
    f, d = kc.tagged_cloud(n, 4, 3, dtype)
    d[:, 1] = np.resize(np.array([-1.0, 0.5, 0.5, 2.0, np.inf, -np.inf, np.nan], dtype), n)
    for larger in (True, False):
        keep = kc.cut_descriptor_keep(d, 1, larger, 0.5)
        assert keep[1] and keep[2]  # equality is kept in both senses
        assert not keep[6]          # a NaN is cut in both
        check(_capi.keep_filter(f, d, _capi.KEEP_CUT_DESCRIPTOR, index=1, flag=int(larger), value=0.5), f, d, keep,
              f"larger {larger}")


# -------------------------------------------------------------------- Shadow --
@pytest.mark.parametrize("eps", [0.1, 1.2])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shadow_equals_reference(dtype, D, eps):
    n = 2 * kc.BLOCK + 1 + 777
    s = kc.sin_eps(eps, dtype)
    pts, nrm = kc.shadow_scene(n, D, dtype, s)
    ok = kc.margin_ok(pts, nrm, s)
    assert ok.all(), f"{(~ok).sum()} points within 1e-3 of the threshold"
    keep = kc.shadow_keep(pts, nrm, s)
    assert 0 < keep.sum() < n
    rng = np.random.default_rng(5)
    desc = rng.normal(0, 1, (n, 2 + D + 1)).astype(dtype)  # normals at row offset 2
    desc[:, 2:2 + D] = nrm
    check(_capi.keep_filter(pts, desc, _capi.KEEP_SHADOW, index=2, value=float(s)), pts, desc, keep, "shadow")


@pytest.mark.parametrize("dtype", DTYPES)
def test_shadow_exact_case(dtype):
    """normal (0, 0, 1) against (3, 4, 0) and (0, 0, 2), eps 0: the values are
    exactly 0 and 1; 0 > 0 is false."""
    pts = np.array([[3, 4, 0, 1], [0, 0, 2, 1]], dtype)
    nrm = np.array([[0, 0, 1], [0, 0, 1]], dtype)
    assert list(kc.shadow_value(pts, nrm)) == [0.0, 1.0]
    gf, gd = _capi.keep_filter(pts, nrm, _capi.KEEP_SHADOW, index=0, value=0.0)
    assert same_bits(gf, pts[1:]) and same_bits(gd, nrm[1:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_shadow_zero_and_nan_vectors(dtype):
    """normalized() of a zero vector is the zero vector (value 0: dropped at any
    eps >= 0); a NaN vector stays NaN and fails the comparison."""
    pts = np.array([[0, 0, 0, 1], [1, 2, 2, 1], [0, 0, 0, 1], [1, 2, 2, 1], [1, 2, 2, 1], [0, 0, 5, 1]], dtype)
    nrm = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0], [1, 2, 2], [np.nan, 0, 1], [0, 0, -1]], dtype)
    for s in (0.0, float(kc.sin_eps(0.1, dtype))):
        keep = kc.shadow_keep(pts, nrm, s)
        assert list(keep) == [False, False, False, True, False, True]
        check(_capi.keep_filter(pts, nrm, _capi.KEEP_SHADOW, index=0, value=s), pts, nrm, keep, f"sin {s}")


# --------------------------------------------------------- MaxQuantileOnAxis --
def quantile_axes(n, dtype):
    rng = np.random.default_rng(n)
    T = np.dtype(dtype).type
    ties = np.where(rng.uniform(0, 1, n) < 0.9, T(0.375), rng.normal(0, 1, n).astype(dtype))
    zeros = np.resize(np.array([-0.0, 0.0, -0.0, 0.0, 0.0, -1.5, 2.5], dtype), n)
    negative = -np.abs(rng.normal(3, 1, n)).astype(dtype)
    edge = np.concatenate([negative[:n // 2], np.abs(negative[n // 2:])])  # rank n/2 - 1 | n/2: the sign boundary
    return {"random": rng.normal(0, 10, n).astype(dtype), "ties": ties.astype(dtype),
            "equal": np.full(n, -2.5, dtype), "zeros": zeros, "negative": negative, "edge": edge.astype(dtype)}


@pytest.mark.parametrize("dim", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_max_quantile_equals_partition(dtype, dim):
    lo, hi = 0.0000001, 0.9999999  # the parameter's bounds (MaxQuantileOnAxis.h:61)
    for n in (1, 1000, 100003):
        for name, axis in quantile_axes(n, dtype).items():
            if n > 1000 and name not in ("random", "ties", "edge"):
                continue  # (many blocks: the cases where the keys differ)
            pts, desc = kc.tagged_cloud(n, 4, 1, dtype, seed=dim)
            pts[:, dim] = axis
            for ratio in (lo, 0.25, 0.4995, 0.5, 0.72, hi):  # (0.4995 | 0.5: "edge"'s last negative | first positive)
                keep = kc.max_quantile_keep(pts, dim, ratio)
                what = f"{name} n {n} ratio {ratio}"
                if name == "equal" or ratio == lo:
                    assert not keep.any(), what  # strict <: the ties with the limit go, the minimum included
                got = _capi.keep_filter(pts, desc, _capi.KEEP_MAX_QUANTILE, index=dim, value=ratio)
                check(got, pts, desc, keep, what)


def test_max_quantile_limit_inside_the_tie_and_signed_zeros():
    n = 1000
    ax = quantile_axes(n, np.float32)
    lim = kc.max_quantile_limit(ax["ties"], 0.5)
    assert lim == np.float32(0.375)  # 90 % of the axis: every tied point goes
    assert kc.max_quantile_keep(ax["ties"][:, None], 0, 0.5).sum() == (ax["ties"] < lim).sum() < n // 10
    pts = np.ones((n, 4), np.float32)
    pts[:, 0] = ax["zeros"]
    keep = kc.max_quantile_keep(pts, 0, 0.5)
    assert kc.max_quantile_limit(ax["zeros"], 0.5) == 0  # either zero
    assert np.array_equal(keep, ax["zeros"] == np.float32(-1.5))  # -0 < +0 is false: no zero is kept
    check(_capi.keep_filter(pts, None, _capi.KEEP_MAX_QUANTILE, index=0, value=0.5), pts, None, keep, "zeros")


# ----------------------------------------------------------------- RemoveNaN --
@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_nan_inspects_every_feature_row(dtype, rows):
    n = kc.BLOCK + 9
    pts, desc = kc.tagged_cloud(n, rows, 2, dtype)
    for r in range(rows):  # the homogeneous row included
        pts[3 + 5 * r, r] = np.nan
        pts[4 + 5 * r, r] = np.inf
        pts[5 + 5 * r, r] = -np.inf
    desc[0, 0] = np.nan  # descriptors are not inspected
    keep = kc.remove_nan_keep(pts)
    assert keep.sum() == n - rows and keep[0]
    check(_capi.keep_filter(pts, desc, _capi.KEEP_REMOVE_NAN), pts, desc, keep, "nan rows")


# -------------------------------------------------------------------- errors --
def test_bad_parameters():
    pts, desc = kc.tagged_cloud(10, 4, 3, np.float32)
    bad = [
        dict(points=pts, descriptors=desc, predicate=_capi.KEEP_MAX_QUANTILE, index=4, value=0.5),
        dict(points=pts, descriptors=desc, predicate=_capi.KEEP_MAX_QUANTILE, index=-1, value=0.5),
        dict(points=np.ones((10, 5), np.float32), descriptors=None, predicate=_capi.KEEP_REMOVE_NAN),
        dict(points=np.ones((10, 2), np.float32), descriptors=None, predicate=_capi.KEEP_REMOVE_NAN),
        dict(points=pts, descriptors=desc, predicate=_capi.KEEP_SHADOW, index=-1, value=0.1),
        dict(points=pts, descriptors=desc, predicate=_capi.KEEP_SHADOW, index=1, value=0.1),   # rows 1..3 of 3
        dict(points=pts, descriptors=None, predicate=_capi.KEEP_SHADOW, index=0, value=0.1),
        dict(points=pts, descriptors=desc, predicate=_capi.KEEP_CUT_DESCRIPTOR, index=3),
        dict(points=pts, descriptors=desc, predicate=9),
    ]
    for kw in bad:
        with pytest.raises(_capi.InvalidParameter):
            _capi.keep_filter(**kw)
    # the same checks on an empty cloud; an empty cloud itself is a result
    with pytest.raises(_capi.InvalidParameter):
        _capi.keep_filter(pts[:0], desc[:0], _capi.KEEP_MAX_QUANTILE, index=4, value=0.5)
    gf, gd = _capi.keep_filter(pts[:0], desc[:0], _capi.KEEP_MAX_QUANTILE, index=0, value=0.5)
    assert gf.shape == (0, 4) and gd.shape == (0, 3)


# --------------------------------------------------------------------- chain --
CONFIGS = ["defaultShadowDataPointsFilter", "defaultMaxDensityDataPointsFilter",
           "defaultMaxQuantileOnAxisDataPointsFilter", "defaultMaxPointCountDataPointsFilter",
           "defaultRemoveNaNDataPointsFilter"]


@pytest.mark.parametrize("name", CONFIGS)
def test_icp_data_config_unchanged(golden, name):
    """utest.cpp:81-160, as tests/test_gpu_ssn.py runs the other configs."""
    g, kat = golden
    icp = ICP(np.float32)
    try:
        icp.load_yaml(kat["icp_data_configs"][name])
        _libc.srand(1)
        T = icp.compute(hom(g["vtk1"], np.float32), hom(g["vtk0"], np.float32), None)
        err = rel_displacement(T, np.array(kat["icp_data_ref_trans"][name]), g["vtk1"])
        print(f"{name}: rel err {err:.4f}, iterations {icp.stats().iterations}")
    finally:
        icp.close()
    assert err < kat["icp_data_rel_tol"]


def test_chain_shadow_keeps_the_reference_points(golden):
    """The reading chain of defaultShadowDataPointsFilter against the numpy
    Shadow on the normals the same chain computes without its Shadow entry."""
    g, kat = golden
    text = kat["icp_data_configs"]["defaultShadowDataPointsFilter"]
    entry = "  - ShadowDataPointsFilter:\n       eps: 0.00001\n"
    assert entry in text
    rd = hom(g["vtk1"], np.float32)
    icp = ICP(np.float32)
    try:
        icp.load_yaml(text.replace(entry, ""))
        nrm = icp.filtered_descriptor("reading", rd, "normals")
        icp.load_yaml(text)
        kept = icp.filtered_descriptor("reading", rd, "normals")
    finally:
        icp.close()
    assert nrm.shape == (len(rd), 3)
    keep = kc.shadow_keep(rd, nrm, kc.sin_eps(0.00001, np.float32))
    assert len(kept) == int(keep.sum())
    assert same_bits(kept, nrm[keep])


def test_chain_max_quantile_keeps_the_reference_points(golden):
    g, kat = golden
    text = kat["icp_data_configs"]["defaultMaxQuantileOnAxisDataPointsFilter"]
    rd = hom(g["vtk1"], np.float32)
    icp = ICP(np.float32)
    try:
        icp.load_yaml(text)
        icp.add_descriptor("reading", "tag", np.arange(len(rd)).astype(np.float32))
        tag = icp.filtered_descriptor("reading", rd, "tag")
    finally:
        icp.close()
    keep = kc.max_quantile_keep(rd, 0, 0.72)
    assert 0 < keep.sum() < len(rd)
    assert np.array_equal(tag[:, 0].astype(int), np.nonzero(keep)[0])

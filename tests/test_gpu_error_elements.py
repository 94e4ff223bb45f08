"""ErrorMinimizer::getErrorElements on the GPU, at the C ABI:
pmx_error_elements_prepare / pmx_error_elements.

The yardstick is error_elements_cases.restate applied to the independent
mirrors (pmx_get_matches, pmx_get_weights) and the test's own host clouds.
Every output is a copy of a stored value or xform3's transform, so every
comparison is exact.

Reading sizes sit where a 64-lane ballot and a 256-thread block scan can go
wrong (1, 63, 64, 65, 256, 257, 1000, 4099), k is 1, 4 and 17 (the
wave-per-query match).  A rejecting chain must leave 0 < P < k N and an `inf`
case at least one inf, checked on the mirrors before comparing; with a single
reading point no P lies strictly between 0 and k at k = 1 and a radius cannot
be met and missed at once, so the two guards apply from 63 points up.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import error_elements_cases as E  # noqa: E402
import quality_cases as Q  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SIZES = [1, 63, 64, 65, 256, 257, 1000, 4099]
KS = [1, 4, 17]
CHAINS = ["radius", "trim", "maxdist", "robust", "generic", "normal"]
RADIUS = 0.03  # about a fifth of the reading points have no reference point this near
T_OTHER = Q.rigid(-0.003, 0.002, 0.004, [0.001, 0.002, -0.002])


def weight_descriptor(M, dtype):
    """Negative, zero and positive values: soft weights keep the first, drop the second."""
    d = np.random.default_rng(11).normal(0, 1, M)
    d[::3] = 0
    assert (d < 0).any() and (d > 0).any()
    return d.astype(dtype)


def reading_normals(n, dtype):
    v = np.random.default_rng(5 + n).normal(0, 1, (n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), dtype=dtype)


def run_chain(ctx, chain, knn, dtype, n_rd):
    from libpointmatcher_amd import _capi
    if chain == "normal":
        ctx.set_reading_normals(reading_normals(n_rd, dtype))
    ctx.match(np.asarray(Q.T_AT, dtype), knn=knn, max_dist=RADIUS if chain == "radius" else np.inf)
    if chain == "trim":
        ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    elif chain == "maxdist":
        ctx.outlier("MaxDistOutlierFilter", 0, maxDist=0.03)
    elif chain == "robust":  # real weights; the approximation zeroes the far pairs
        ctx.outlier_robust(0, "cauchy", 0.5, 1.5, _capi.RS_MAD, 0.0)
    elif chain == "generic":
        ctx.outlier_generic_descriptor(0, soft=True)
    elif chain == "normal":
        ctx.outlier_surface_normal(0, max_angle=1.2)
    # ("radius": the empty chain, w = dist != inf)


def mirrors_and_want(ctx, T, rd, ref, nrm):
    d, ids = ctx.get_matches()
    w = ctx.get_weights()
    return d, w, E.restate(d, ids, w, E.step_reading(T, rd), ref, nrm)


def compare(ctx, tag, chain, rd, ref, nrm, knn, guard):
    from libpointmatcher_amd import _capi
    dtype = rd.dtype
    try:
        st = ctx.p2plane_system()[2]
    except _capi.ConvergenceError:  # (one reading point has no robust scale: the minimiser has nothing either)
        assert not guard, tag
        st = None
    d, w, want = mirrors_and_want(ctx, Q.T_AT, rd, ref, nrm)
    P = len(want["dists"])
    print(f"{tag}: P {P} of {d.size} inf {int(np.isinf(d).sum())} rejM {want['rejected_matches']} "
          f"rejP {want['rejected_points']} neg {int((want['weights'] < 0).sum())}")
    if guard:
        assert 0 < P < d.size, tag
        if chain == "radius":
            assert np.isinf(d).any(), tag
        if chain == "generic":
            assert (want["weights"] < 0).any() and ((w == 0) & ~np.isinf(d)).any(), tag
    if P == 0:  # (never under the guard)
        info = _capi.ElementsInfo()
        assert ctx._l.pmx_error_elements_prepare(ctx.h, None, C.byref(info)) == _capi.PMX_E_NO_POINTS, tag
        assert (info.columns, info.rejected_matches, info.rejected_points) == (
            0, want["rejected_matches"], want["rejected_points"]), tag
        return
    got = ctx.error_elements()
    info = ctx.last_elements_info
    if st is not None:
        assert (info.columns, info.rejected_matches, info.rejected_points) == (
            st.kept, st.rejected_matches, st.rejected_points), tag
    assert got.columns == P and got.reading.dtype == dtype, tag
    E.assert_equal(got, want, tag)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("chain", CHAINS)
def test_columns_match_restatement(dtype, search, chain):
    from libpointmatcher_amd import _capi
    ctx = _capi.Context(0, dtype)
    ctx.set_search(search)
    _, ref, nrm = Q.clouds(64, dtype)
    ctx.set_reference(ref, nrm)
    if chain == "generic":
        ctx.set_reference_weight_descriptor(weight_descriptor(len(ref), dtype))
    for n_rd in SIZES:
        rd = Q.clouds(n_rd, dtype)[0]
        for knn in KS:
            ctx.set_reading(rd)
            run_chain(ctx, chain, knn, dtype, n_rd)
            compare(ctx, f"{np.dtype(dtype).name} search {search} {chain} N {n_rd} k {knn}", chain, rd, ref, nrm,
                    knn, guard=n_rd >= 63)
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("search", [0, 1])
def test_two_dimensional_cloud(dtype, search):
    from libpointmatcher_amd import _capi
    rd3, ref3, nrm3 = Q.clouds(257, dtype)
    rd, ref = np.ascontiguousarray(rd3[:, [0, 1, 3]]), np.ascontiguousarray(ref3[:, [0, 1, 3]])
    ang = np.random.default_rng(2).uniform(0, 2 * np.pi, len(ref))
    nrm = np.ascontiguousarray(np.c_[np.cos(ang), np.sin(ang)], dtype=dtype)
    T = np.eye(3)
    T[:2, :2] = Q.rot(0, 0, 0.004)[:2, :2]
    T[:2, 2] = [0.002, -0.001]
    T = np.asarray(T, dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_search(search)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    for knn in (1, 4):
        ctx.match(T, knn=knn)
        ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
        d, ids = ctx.get_matches()
        want = E.restate(d, ids, ctx.get_weights(), E.step_reading(T, rd), ref, nrm)
        assert 0 < len(want["dists"]) < d.size
        got = ctx.error_elements()
        assert got.reading.shape == (len(want["dists"]), 3) and got.ref_normals.shape[1] == 2
        E.assert_equal(got, want, f"2-D k {knn}")
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["first", "last"])
def test_only_one_point_keeps_a_link(dtype, which):
    """Every reading point but the first / the last lies beyond the search radius."""
    from libpointmatcher_amd import _capi
    rd, ref, nrm = Q.clouds(257, dtype)
    keep = 0 if which == "first" else len(rd) - 1
    far = np.ones(len(rd), bool)
    far[keep] = False
    rd = rd.copy()
    rd[far, :3] += np.asarray([5.0, 5.0, 5.0], dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    for knn in (1, 4):
        ctx.match(np.asarray(Q.T_AT, dtype), knn=knn, max_dist=0.2)
        d, w, want = mirrors_and_want(ctx, Q.T_AT, rd, ref, nrm)
        assert np.isinf(d[far]).all() and not np.isinf(d[keep]).any()
        got = ctx.error_elements()
        assert got.columns == knn and (got.reading_index == keep).all()
        assert got.rejected_points == len(rd) - 1 and got.rejected_matches == 0
        E.assert_equal(got, want, f"{which} k {knn}")
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_explicit_step_transform(dtype):
    from libpointmatcher_amd import _capi
    rd, ref, nrm = Q.clouds(1000, dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.match(np.asarray(Q.T_AT, dtype), knn=4)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    d, w, want = mirrors_and_want(ctx, Q.T_AT, rd, ref, nrm)
    same = ctx.error_elements(T_step=np.asarray(Q.T_AT, dtype))
    E.assert_equal(same, want, "T_step = T_iter")
    E.assert_equal(ctx.error_elements(), want, "NULL")
    other = ctx.error_elements(T_step=np.asarray(T_OTHER, dtype))
    want_other = dict(want, reading=E.step_reading(T_OTHER, rd)[want["reading_index"]])
    assert not np.array_equal(want_other["reading"], want["reading"])
    E.assert_equal(other, want_other, "T_step other")
    ctx.close()


def fetch_rc(ctx, normals=False):
    """pmx_error_elements' status with one small buffer per column of `columns` capacity."""
    P = max(int(ctx.last_elements_info.columns), 1) if hasattr(ctx, "last_elements_info") else 1
    buf = np.zeros((P, 4), np.float64)
    n = np.zeros((P, 3), np.float64)
    return ctx._l.pmx_error_elements(ctx.h, None, None, n.ctypes.data_as(C.c_void_p) if normals else None,
                                     buf.ctypes.data_as(C.c_void_p), None, None, None, None)


def test_states():
    from libpointmatcher_amd import _capi
    rd, ref, nrm = Q.clouds(130, np.float32)
    ctx = _capi.Context(0, np.float32)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    info = _capi.ElementsInfo()
    assert ctx._l.pmx_error_elements_prepare(ctx.h, None, C.byref(info)) == _capi.PMX_E_STATE  # no match
    assert fetch_rc(ctx) == _capi.PMX_E_STATE
    T = np.asarray(Q.T_AT, np.float32)
    ctx.match(T, knn=1)
    assert fetch_rc(ctx) == _capi.PMX_E_STATE  # a match, no prepare
    e = ctx.error_elements()
    assert e.columns == 130 and fetch_rc(ctx) == _capi.PMX_OK
    ctx.match(T, knn=1)
    assert fetch_rc(ctx) == _capi.PMX_E_STATE  # a new match
    ctx.error_elements()
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    assert fetch_rc(ctx) == _capi.PMX_E_STATE  # a new chain
    ctx.error_elements()
    ctx.set_reading(rd)
    assert fetch_rc(ctx) == _capi.PMX_E_STATE  # a new reading
    # a chain that rejects everything: the counts come back with the error
    ctx.match(T, knn=2)
    ctx.outlier("MaxDistOutlierFilter", 0, maxDist=1e-6)
    assert ctx._l.pmx_error_elements_prepare(ctx.h, None, C.byref(info)) == _capi.PMX_E_NO_POINTS
    assert (info.columns, info.rejected_matches, info.rejected_points) == (0, 260, 130)
    assert fetch_rc(ctx) == _capi.PMX_E_STATE
    with pytest.raises(_capi.ConvergenceError):
        ctx.error_elements()
    ctx.close()
    # the normals of a reference without normals
    ctx = _capi.Context(0, np.float32)
    ctx.set_reference(ref)
    ctx.set_reading(rd)
    ctx.match(T, knn=1)
    e = ctx.error_elements()
    assert e.ref_normals is None and e.columns == 130
    assert fetch_rc(ctx, normals=True) == _capi.PMX_E_BAD_PARAM
    ctx.close()

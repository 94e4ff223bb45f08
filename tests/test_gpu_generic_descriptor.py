"""GenericDescriptorOutlierFilter on the GPU through the C ABI
(pmx_set_reference_weight_descriptor, pmx_outlier_generic_descriptor;
gd_weight in csrc/pmx_weight.h, the maximum in csrc/pmx_generic.hip).

The filter's weights are restated here in numpy over the ids pmx_get_matches
returns (OutlierFiltersImpl.cpp:312-374): no neighbour 0; hard desc[id] >
threshold or < threshold, strict, in T; soft desc[id], then every entry divided
in T by the maximum over all k x N entries, the zeros included.  Bars: the
weights bit-equal to the restatement (soft x robust: the robust factor's own
tolerance, tests/test_gpu_robust.py); hard chains' systems as the 0/1 chains of
tests/test_gpu_kernels.py (1e-12 relative, counts equal); soft chains' as
test_weighted_systems of tests/test_gpu_robust.py (1e-9 relative, counts
equal).  Shapes: 3000 reading points against 4000 reference points.
"""
import numpy as np
import pytest

import force_cases as fc
from libpointmatcher_amd import _capi as P
from libpointmatcher_amd.synth import reading_cloud, reference_cloud

pytestmark = pytest.mark.gpu

N, M = 3000, 4000
THR = 0.5
DTYPES = [np.float32, np.float64]
RTOL = {np.float32: 1e-6, np.float64: 1e-12}  # (robust weights, tests/test_gpu_robust.py)
MODES = {"gt": dict(soft=False, larger_than=True), "lt": dict(soft=False, larger_than=False),
         "soft": dict(soft=True, larger_than=True)}


def descriptor(dtype, m=M, seed=3):
    """seeded values in (0.05, 1), 50 of them exactly the threshold"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 1.0, m).astype(dtype)
    v[rng.choice(m, 50, replace=False)] = dtype(THR)
    return v


def restate(desc, ids, mode):
    dtype = desc.dtype.type
    valid = ids >= 0
    v = desc[np.where(valid, ids, 0)]
    if mode == "gt":
        return np.where(valid & (v > dtype(THR)), 1, 0).astype(dtype)
    if mode == "lt":
        return np.where(valid & (v < dtype(THR)), 1, 0).astype(dtype)
    w = np.where(valid, v, dtype(0)).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w / w.max()).astype(dtype)  # (a division in T by the maximum over every entry)


def small_T(dtype, rows=4):
    c, s = np.cos(0.01), np.sin(0.01)
    T = np.eye(rows)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:rows - 1, rows - 1] = [0.008, -0.006, 0.004][:rows - 1]
    return T.astype(dtype)


def setup(dtype, search=1, desc=None, dim=3):
    ref, nrm = reference_cloud(M, dtype)
    rd = reading_cloud(N, dtype)
    if dim == 2:
        ref = np.ascontiguousarray(ref[:, [0, 1, 3]])
        rd = np.ascontiguousarray(rd[:, [0, 1, 3]])
        nrm = None
    ctx = P.Context(0, dtype)
    ctx.set_search(search)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    desc = descriptor(dtype) if desc is None else desc
    ctx.set_reference_weight_descriptor(desc)
    return ctx, ref, nrm, rd, desc


def match_losing_some(ctx, T, k):
    """matched with a maxDist that leaves about 5 % of the entries without a
    neighbour (the 0.95 quantile of the unlimited match's distances)"""
    ctx.match(T, knn=k)
    d0, _ = ctx.get_matches()
    md = float(np.sqrt(np.quantile(d0.astype(np.float64), 0.95)))
    ctx.match(T, knn=k, max_dist=md)
    d, i = ctx.get_matches()
    lost = (i < 0).mean()
    assert 0.01 < lost < 0.20, lost
    assert np.array_equal(i < 0, np.isinf(d))
    return d, i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("k", [1, 3, 20])
def test_weights_bit_equal(oracle, dtype, search, k):
    ctx, ref, nrm, rd, desc = setup(dtype, search)
    try:
        d, i = match_losing_some(ctx, small_T(dtype), k)
        _, wt = oracle.outlier_chain([("TrimmedDistOutlierFilter", {"ratio": 0.8})], d)
        for mode, p in MODES.items():
            ow = restate(desc, i, mode)
            if mode != "soft":
                assert (desc[i[i >= 0]] == dtype(THR)).any() and 0 < ow.sum() < ow.size
            ctx.outlier_generic_descriptor(0, threshold=THR, **p)
            w = ctx.get_weights()
            assert w.tobytes() == ow.tobytes(), (mode, "position 0")
            ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.8)
            ctx.outlier_generic_descriptor(1, threshold=THR, **p)
            w = ctx.get_weights()
            assert w.tobytes() == (wt * ow).tobytes(), (mode, "position 1")
            if mode == "soft":
                # the maximum the device divided by, as its weights imply it: the entries of
                # weight 1 at position 0 are exactly those whose descriptor is numpy's maximum
                ctx.outlier_generic_descriptor(0, soft=True)
                w0 = ctx.get_weights()
                m = desc[i[i >= 0]].max()
                assert np.array_equal(w0 == 1, (i >= 0) & (desc[np.where(i >= 0, i, 0)] == m)) and (w0 == 1).any()
    finally:
        ctx.close()


def test_weights_2d():
    dtype = np.float32
    ctx, ref, nrm, rd, desc = setup(dtype, 1, dim=2)
    try:
        d, i = match_losing_some(ctx, small_T(dtype, 3), 3)
        for mode, p in MODES.items():
            ctx.outlier_generic_descriptor(0, threshold=THR, **p)
            assert ctx.get_weights().tobytes() == restate(desc, i, mode).tobytes(), mode
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_soft_times_robust(oracle, dtype):
    k = 3
    ctx, ref, nrm, rd, desc = setup(dtype)
    try:
        d, i = match_losing_some(ctx, small_T(dtype), k)
        r = oracle.make_robust({"robustFct": "cauchy", "scaleEstimator": "mad", "tuning": 1.0})
        _, wr = oracle.robust_weights(r, d, i)
        ow = wr * restate(desc, i, "soft")
        for order in ("soft first", "robust first"):
            if order == "soft first":
                ctx.outlier_generic_descriptor(0, soft=True)
                ctx.outlier_robust(1, "cauchy", 1.0, np.inf, P.RS_MAD, 0.0)
            else:
                ctx.outlier_robust(0, "cauchy", 1.0, np.inf, P.RS_MAD, 0.0)
                ctx.outlier_generic_descriptor(1, soft=True)
            w = ctx.get_weights()
            np.testing.assert_allclose(w, ow, rtol=RTOL[dtype], atol=RTOL[dtype], err_msg=order)
            assert np.array_equal(w == 0, ow == 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_maximum_of_negative_descriptors(dtype):
    desc = -descriptor(dtype)
    ctx, ref, nrm, rd, _ = setup(dtype, desc=desc)
    try:
        T = small_T(dtype)
        # every entry valid: m is the (negative) maximum, every weight >= 1
        ctx.match(T, knn=3)
        _, i = ctx.get_matches()
        assert (i >= 0).all()
        ctx.outlier_generic_descriptor(0, soft=True)
        w = ctx.get_weights()
        m = desc[i].max()
        assert m < 0 and w.tobytes() == (desc[i] / m).astype(dtype).tobytes() and (w >= 1).all()
        # an entry without a neighbour: m = 0, the weights -inf and NaN (IEEE, unguarded).
        # Only the weights' mirror is read: no system is run on them.
        d, i = match_losing_some(ctx, T, 3)
        ctx.outlier_generic_descriptor(0, soft=True)
        w = ctx.get_weights()
        ow = restate(desc, i, "soft")
        assert np.isnan(ow[i < 0]).all() and np.isneginf(ow[i >= 0]).all()
        assert np.array_equal(w, ow, equal_nan=True)
    finally:
        ctx.close()


def stats_equal(st, ost):
    assert st.kept == ost.kept and st.nonzero_weights == ost.nonzero_weights
    assert st.rejected_matches == ost.rejected_matches and st.rejected_points == ost.rejected_points


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,search", [(1, 1), (3, 1), (3, 0)])
@pytest.mark.parametrize("mode", ["gt", "lt", "soft"])
def test_systems(oracle, dtype, k, search, mode):
    tol = 1e-9 if mode == "soft" else 1e-12
    ctx, ref, nrm, rd, desc = setup(dtype, search)
    try:
        T = small_T(dtype)
        d, i = match_losing_some(ctx, T, k)
        ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.8)
        ctx.outlier_generic_descriptor(1, threshold=THR, **MODES[mode])
        _, wt = oracle.outlier_chain([("TrimmedDistOutlierFilter", {"ratio": 0.8})], d)
        w = wt * restate(desc, i, mode)
        assert ctx.get_weights().tobytes() == w.tobytes()
        step = oracle.transform(T, rd)
        A, b, st = ctx.p2plane_system()
        rc, oA, ob, ost = oracle.p2plane_system(step, ref, nrm, d, i, w)
        assert rc == 0
        np.testing.assert_allclose(A, oA, rtol=tol, atol=tol * np.abs(oA).max())
        np.testing.assert_allclose(b, ob, rtol=tol, atol=tol * np.abs(ob).max())
        stats_equal(st, ost)
        np.testing.assert_allclose(st.sum_w, ost.sum_w, rtol=1e-9)
        # forced forms: 4-DOF is the 6-DOF system's block, 2-D against the restatement
        A4, b4, st4 = ctx.p2plane_system_forced("4DOF")
        assert np.array_equal(A4, A[2:, 2:]) and np.array_equal(b4, b[2:])
        stats_equal(st4, ost)
        A2, b2, st2 = ctx.p2plane_system_forced("2D")
        wA, wb, kept = fc.forced_system(step, ref, np.ascontiguousarray(nrm[:, :3]), i, d, w, "2D")
        assert st2.kept == kept
        stats_equal(st2, ost)
        np.testing.assert_allclose(A2, wA, rtol=tol, atol=tol * np.abs(wA).max())
        np.testing.assert_allclose(b2, wb, rtol=tol, atol=tol * np.abs(wb).max())
        # point-to-point: the moments' rotation and translation against the oracle's step
        mp, mq, m, stp = ctx.p2point_system()
        rc, dT, ostp = oracle.p2point(step, ref, d, i, w)
        assert rc == 0
        stats_equal(stp, ostp)
        np.testing.assert_allclose(stp.sum_w, ostp.sum_w, rtol=1e-9)
        U, S, Vt = np.linalg.svd(m)
        R = U @ Vt
        if np.linalg.det(R) < 0:
            Vt[-1] *= -1
            R = U @ Vt
        ptol = 1e-5 if dtype == np.float32 else 1e-11
        assert np.abs(R - dT[:3, :3]).max() < ptol
        assert np.abs((mq - R @ mp) - dT[:3, 3]).max() < ptol
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["lt", "soft"])
@pytest.mark.parametrize("k", [1, 3])
def test_covariance_counts_the_kept_pairs(oracle, mode, k):
    dtype = np.float32
    ctx, ref, nrm, rd, desc = setup(dtype)
    try:
        T = small_T(dtype)
        d, i = match_losing_some(ctx, T, k)
        ctx.outlier_generic_descriptor(0, threshold=THR, **MODES[mode])
        ctx.outlier("TrimmedDistOutlierFilter", 1, ratio=0.8)
        _, wt = oracle.outlier_chain([("TrimmedDistOutlierFilter", {"ratio": 0.8})], d)
        w = wt * restate(desc, i, mode)
        A, b, st = ctx.p2plane_system()
        H, Q, pairs = ctx.p2plane_covariance(np.eye(4, dtype=dtype))
        kept = int((np.isfinite(d) & (w != 0)).sum())
        assert pairs == kept == st.kept and 0 < kept < w.size
    finally:
        ctx.close()


def test_errors():
    dtype = np.float32
    ref, nrm = reference_cloud(M, dtype)
    ctx = P.Context(0, dtype)
    try:
        ctx.set_reference(ref, nrm)
        ctx.set_reading(reading_cloud(N, dtype))
        ctx.match(np.eye(4, dtype=dtype), knn=1)
        state = f"pmx error {P.PMX_E_STATE}:"
        with pytest.raises(P.PmxError, match=state):  # no descriptor uploaded
            ctx.outlier_generic_descriptor(0)
        ctx.set_reference_weight_descriptor(descriptor(dtype))
        ctx.outlier_generic_descriptor(0)
        with pytest.raises(P.InvalidParameter, match="one GenericDescriptorOutlierFilter"):  # PMX_E_BAD_PARAM
            ctx.outlier_generic_descriptor(1, soft=True)
        ctx.outlier_generic_descriptor(0, soft=True)  # (position 0 starts a new chain)
        ctx.set_reference(ref, nrm)  # a new reference clears the descriptor
        ctx.match(np.eye(4, dtype=dtype), knn=1)
        with pytest.raises(P.PmxError, match=state):
            ctx.outlier_generic_descriptor(0)
        ctx.set_reference_weight_descriptor(descriptor(dtype))
        ctx.set_reference_weight_descriptor(None)  # NULL clears it
        with pytest.raises(P.PmxError, match=state):
            ctx.outlier_generic_descriptor(0)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_search_type_switched_after_the_upload(dtype):
    """the descriptor uploaded under brute force, the match then run on the grid
    (and back): every level got its copy at the upload, whatever the search type was"""
    ref, nrm = reference_cloud(M, dtype)
    rd = reading_cloud(N, dtype)
    desc = descriptor(dtype)
    ctx = P.Context(0, dtype)
    try:
        ctx.set_search(0)
        ctx.set_reference(ref, nrm)
        ctx.set_reading(rd)
        ctx.set_reference_weight_descriptor(desc)
        for search in (1, 0, 1):
            ctx.set_search(search)
            d, i = match_losing_some(ctx, small_T(dtype), 3)
            for mode, p in MODES.items():
                ctx.outlier_generic_descriptor(0, threshold=THR, **p)
                assert ctx.get_weights().tobytes() == restate(desc, i, mode).tobytes(), (search, mode)
            A, b, st = ctx.p2plane_system()  # (soft: the maximum and the weighted sums ran)
            assert st.kept == int((i >= 0).sum())
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_reference_and_descriptor_on_one_context(dtype):
    """a second reference of the same size reuses the level buffers: its matches must read
    the second descriptor in the second reference's order, and nothing before its upload"""
    rd = reading_cloud(N, dtype)
    ctx = P.Context(0, dtype)
    try:
        for seed, shift in ((3, 0.0), (4, 0.37)):
            ref, nrm = reference_cloud(M, dtype)
            ref = ref.copy()
            ref[:, 0] += dtype(shift)
            ref = np.ascontiguousarray(ref[::-1]) if shift else ref  # (another order of the points)
            nrm = np.ascontiguousarray(nrm[::-1]) if shift else nrm
            desc = descriptor(dtype, seed=seed)
            ctx.set_reference(ref, nrm)
            ctx.set_reading(rd)
            ctx.match(small_T(dtype), knn=3)
            with pytest.raises(P.PmxError, match=f"pmx error {P.PMX_E_STATE}:"):  # (the last reference's is gone)
                ctx.outlier_generic_descriptor(0, soft=True)
            ctx.set_reference_weight_descriptor(desc)
            d, i = match_losing_some(ctx, small_T(dtype), 3)
            for mode, p in MODES.items():
                ctx.outlier_generic_descriptor(0, threshold=THR, **p)
                assert ctx.get_weights().tobytes() == restate(desc, i, mode).tobytes(), (seed, mode)
    finally:
        ctx.close()


def test_soft_maximum_over_rccl_at_one_rank():
    """a communicator issues every collective: the maximum's fp64 max all-reduce over RCCL
    leaves the weights bit-equal and counts one all-reduce"""
    dtype = np.float32
    ref, nrm = reference_cloud(M, dtype)
    desc = descriptor(dtype)
    ctx = P.Context(0, dtype)
    try:
        ctx.comm_init(P.Context.unique_id(), 1, 0)
        ctx.set_reference(ref, nrm)
        ctx.set_reading(reading_cloud(N, dtype))
        ctx.set_reference_weight_descriptor(desc)
        d, i = match_losing_some(ctx, small_T(dtype), 3)
        a0, g0 = ctx.comm_stats()
        ctx.outlier_generic_descriptor(0, soft=True)
        a1, g1 = ctx.comm_stats()
        assert (a1 - a0, g1 - g0) == (1, 0)
        assert ctx.get_weights().tobytes() == restate(desc, i, "soft").tobytes()
        ctx.outlier_generic_descriptor(0, soft=False, threshold=THR)
        assert ctx.comm_stats() == (a1, g1)  # (a hard filter adds none)
    finally:
        ctx.close()

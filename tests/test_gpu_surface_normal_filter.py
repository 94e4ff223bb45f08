"""SurfaceNormalOutlierFilter (OutlierFiltersImpl.cpp:225-285) on the GPU:
the module path's weights, the chain product, and whole ICPs through the
device loop and the module calls.

The CPU oracle has no such filter, so the checker is the numpy restatement
below, written in the test's dtype with the arithmetic order the library
fixes (include/pmx.h, pmx_snormal.h): every product and sum rounded
separately, a rotated component (m0 n0 + m1 n1) + m2 n2, squared norm and dot
product summed left to right, norm = sqrt, each component divided by the norm,
|dot| < eps rejects.  It is composed with the oracle's primitives (transform,
knn, outlier_chain, p2plane_system + p2plane_solve, p2point, robust_weights)
into the reference ICP of chains that hold the filter: the weights of an
iteration are outlier_chain(other filters) * restatement.

Bars: weights bit-identical; whole ICPs with equal iteration counts, equal
kept / rejected pairs and the final transform within 1e-5 (float) / 1e-12
(double), the bars of test_gpu_loop.py.
"""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

from helpers import angular_distance, chain_yaml
from libpointmatcher_amd import _capi
from libpointmatcher_amd.icp import ICP, ICPSequence
from libpointmatcher_amd.synth import reading_cloud, reference_cloud, t_gt

pytestmark = pytest.mark.gpu

SN = "SurfaceNormalOutlierFilter"
TRIM = ("TrimmedDistOutlierFilter", {"ratio": 0.85})
TOL = {np.float32: 1e-5, np.float64: 1e-12}
DIFF = dict(minDiffRotErr=0.001, minDiffTransErr=0.01, smoothLength=4)
MAX_ANGLE = 0.6
P2PLANE, P2POINT = "PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer"


def eps_of(dtype, max_angle=MAX_ANGLE):
    return np.cos(np.dtype(dtype).type(max_angle))


# ------------------------------------------------------------ restatement --
def rotate(R, n):
    """R n per point in n's dtype: (m0 n0 + m1 n1) + m2 n2 (2-D: two terms)."""
    D = n.shape[1]
    R = np.asarray(R, n.dtype)
    cols = []
    for c in range(D):
        s = R[c, 0] * n[:, 0] + R[c, 1] * n[:, 1]
        if D == 3:
            s = s + R[c, 2] * n[:, 2]
        cols.append(s)
    return np.stack(cols, 1)


def unit(v):
    sq = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    if v.shape[1] == 3:
        sq = sq + v[:, 2] * v[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(sq)[:, None]


def sn_weights(rn0, T_iter, ref_nrm, ids, eps):
    """The filter's weights (N, k).  rn0: the reading's normals after R_0 (N, D)."""
    D = rn0.shape[1]
    a = unit(rotate(np.asarray(T_iter)[:D, :D], rn0))
    w = np.zeros(ids.shape, rn0.dtype)
    for y in range(ids.shape[1]):
        id_ = ids[:, y]
        ok = id_ >= 0
        b = unit(ref_nrm[np.where(ok, id_, 0)])
        dot = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
        if D == 3:
            dot = dot + a[:, 2] * b[:, 2]
        with np.errstate(invalid="ignore"):
            rej = np.abs(dot) < eps
        w[:, y] = np.where(ok & ~rej, 1, 0)
    return w


def rot3(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def rigid(rows, R, t):
    T = np.eye(rows)
    T[:rows - 1, :rows - 1] = R
    T[:rows - 1, rows - 1] = t
    return T


# ------------------------------------------------------------------ inputs --
_CACHE = {}


def clouds(oracle, M=4000, N=3000):
    """Reference with normals, reading, and the reading's normals: the
    reference normal of each reading point's nearest neighbour at the true
    pose, brought into the reading's frame; a fixed 30 % of them turned by a
    seeded angle in [0.3, 1.5] rad about a seeded axis (float64; cast per test)."""
    key = (M, N)
    if key not in _CACHE:
        ref, nrm = reference_cloud(M, np.float64)
        rd = reading_cloud(N, np.float64)
        Tg = t_gt()
        _, ids, _ = oracle.knn(ref, oracle.transform(Tg, rd), k=1)
        rn = nrm[ids[:, 0]] @ Tg[:3, :3]  # (R_gt^T n per point)
        rng = np.random.default_rng(77)
        turn = rng.permutation(N)[: (3 * N) // 10]
        ang = rng.uniform(0.3, 1.5, turn.size)
        ax = rng.normal(size=(turn.size, 3))
        for j, a, x in zip(turn, ang, ax):
            rn[j] = rot3(x, a) @ rn[j]
        _CACHE[key] = (ref, nrm, rd, rn)
    return _CACHE[key]


def clouds2d(M=1500, N=1000):
    t = np.linspace(0, 2 * np.pi, M, endpoint=False)
    r = 1 + 0.2 * np.sin(5 * t)
    dr = np.cos(5 * t)
    x, y = np.cos(t) * r, np.sin(t) * r
    tx, ty = dr * np.cos(t) - r * np.sin(t), dr * np.sin(t) + r * np.cos(t)
    nrm = np.stack([ty, -tx], 1)  # (not unit length: the filter normalises)
    ref = np.stack([x, y, np.ones_like(t)], 1)
    rng = np.random.default_rng(9)
    pick = np.sort(rng.permutation(M)[:N])
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, -s], [s, c]])
    rd = ref[pick].copy()
    rd[:, :2] = ref[pick, :2] @ R.T + [0.02, -0.01]
    rn = nrm[pick] @ R.T
    turn = rng.permutation(N)[: (3 * N) // 10]
    for j, a in zip(turn, rng.uniform(0.3, 1.5, turn.size)):
        ca, sa = np.cos(a), np.sin(a)
        rn[j] = np.array([[ca, -sa], [sa, ca]]) @ rn[j]
    return ref, nrm, rd, rn


def poses(rows):
    """A non-trivial T0 (rotation 0.2 rad) and T_iter (rotation 0.1 rad)."""
    if rows == 4:
        return (rigid(4, rot3([0, 0, 1], 0.2), [0.1, -0.2, 0.05]),
                rigid(4, rot3([1, 2, 3], 0.1), [0.02, 0.01, -0.03]))
    r = lambda a: np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return rigid(3, r(0.2), [0.05, -0.02]), rigid(3, r(0.1), [0.01, 0.02])


def context(monkeypatch, dtype, opts=""):
    monkeypatch.setenv("PMX_OPTS", opts)
    return _capi.Context(0, dtype)


def matched(ctx, ref, nrm, rd, rn, dtype, knn, max_dist, normals=True):
    """set_reference .. match on ctx; returns (T0, T_iter, rn0, dists, ids)."""
    rows = ref.shape[1]
    T0, Ti = (np.asarray(t, dtype) for t in poses(rows))
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd, T0)
    if normals:
        ctx.set_reading_normals(rn)
    ctx.match(Ti, knn=knn, max_dist=max_dist)
    d, ids = ctx.get_matches()
    return T0, Ti, rotate(T0[:rows - 1, :rows - 1], rn), d, ids


# -------------------------------------------------- 1. weights, module path --
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("nbr", [0, 1])
@pytest.mark.parametrize("max_dist", [np.inf, 0.5])
@pytest.mark.parametrize("knn", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weights_bit_identical(monkeypatch, oracle, dtype, knn, max_dist, nbr, order):
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    ctx = context(monkeypatch, dtype, f"nbr_cache={nbr},reading_order={order}")
    _, Ti, rn0, d, ids = matched(ctx, ref, nrm, rd, rn, dtype, knn, max_dist)
    eps = eps_of(dtype)
    ctx.outlier_surface_normal(0, eps=eps)
    w = ctx.get_weights()
    ctx.close()
    want = sn_weights(rn0, Ti, nrm, ids, eps)
    none = ids < 0
    print(f"rejected {1 - want.mean():.3f}, no neighbour {none.mean():.3f}, mismatches {(w != want).sum()}")
    assert np.array_equal(none, np.isinf(d))
    assert none.any() == np.isfinite(max_dist) and not none.all()
    assert 0 < want.sum() < want.size
    assert np.array_equal(w, want)
    assert not w[none].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["2d", "wave"])
def test_weights_2d_and_just_past_one_wave(monkeypatch, oracle, dtype, case):
    if case == "2d":
        ref, nrm, rd, rn = (a.astype(dtype) for a in clouds2d())
    else:  # N = 65, M = 130
        ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
        ref, nrm, rd, rn = ref[:130], nrm[:130], rd[:65], rn[:65]
    for knn in (1, 2):
        ctx = context(monkeypatch, dtype)
        _, Ti, rn0, d, ids = matched(ctx, ref, nrm, rd, rn, dtype, knn, np.inf)
        eps = eps_of(dtype)
        ctx.outlier_surface_normal(0, eps=eps)
        w = ctx.get_weights()
        A, b, st = ctx.p2plane_system()
        ctx.close()
        want = sn_weights(rn0, Ti, nrm, ids, eps)
        assert 0 < want.sum() < want.size
        assert np.array_equal(w, want)
        assert st.kept == st.nonzero_weights == int(want.sum())
        assert st.rejected_matches == want.size - int(want.sum())


# -------------------------------------------------------- 2. chain product --
@pytest.mark.parametrize("first", ["trimmed", "normal"])
@pytest.mark.parametrize("knn", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chain_product_and_statistics(monkeypatch, oracle, dtype, knn, first):
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    ctx = context(monkeypatch, dtype)
    T0, Ti, rn0, d, ids = matched(ctx, ref, nrm, rd, rn, dtype, knn, 0.5)
    eps = eps_of(dtype)
    if first == "trimmed":
        ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
        ctx.outlier_surface_normal(1, eps=eps)
    else:
        ctx.outlier_surface_normal(0, eps=eps)
        ctx.outlier("TrimmedDistOutlierFilter", 1, ratio=0.85)
    w = ctx.get_weights()
    A, b, st = ctx.p2plane_system()
    mp, mq, m, st2 = ctx.p2point_system()
    # the same chain without the normal filter: its quantile is unchanged
    ctx.match(Ti, knn=knn, max_dist=0.5)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    _, _, st_plain = ctx.p2plane_system()
    ctx.close()
    rc, wt = oracle.outlier_chain([TRIM], d)
    assert rc == 0
    want = wt * sn_weights(rn0, Ti, nrm, ids, eps)
    assert np.array_equal(w, want)
    assert st.limit == st_plain.limit and st_plain.kept > st.kept
    # ErrorElements counts on the product of the weights (ErrorMinimizer.cpp:133-192)
    fin = np.isfinite(d)
    kept = (want != 0) & fin
    for s in (st, st2):
        assert s.kept == kept.sum() and s.nonzero_weights == (want != 0).sum()
        assert s.rejected_matches == (fin & (want == 0)).sum()
        assert s.rejected_points == (~kept.any(axis=1)).sum()
        assert s.sum_w == kept.sum()
    step = oracle.transform(Ti, oracle.transform(T0, rd))
    rc, oA, ob, ost = oracle.p2plane_system(step, ref, nrm, d, ids, want)
    assert rc == 0 and ost.kept == st.kept
    assert np.allclose(A, oA, rtol=1e-12, atol=1e-12 * abs(oA).max())
    assert np.allclose(b, ob, rtol=1e-12, atol=1e-12 * abs(ob).max())


# ----------------------------------------------------------- 3. no normals --
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_without_normals_all_ones(monkeypatch, oracle, dtype):
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    eps = eps_of(dtype)
    ctx = context(monkeypatch, dtype)

    def weights():
        ctx.outlier_surface_normal(0, eps=eps)
        return ctx.get_weights()

    # no reading normals
    _, Ti, rn0, d, ids = matched(ctx, ref, nrm, rd, rn, dtype, 2, 0.5, normals=False)
    assert (ids < 0).any()
    assert np.array_equal(weights(), np.ones_like(d))
    # with them the filter acts; cleared, ones again
    ctx.set_reading_normals(rn)
    assert np.array_equal(weights(), sn_weights(rn0, Ti, nrm, ids, eps))
    ctx.set_reading_normals(None)
    assert np.array_equal(weights(), np.ones_like(d))
    # a new reading clears them too
    ctx.set_reading_normals(rn)
    matched(ctx, ref, nrm, rd, rn, dtype, 2, 0.5, normals=False)
    assert np.array_equal(weights(), np.ones_like(d))
    # a reference without normals
    matched(ctx, ref, None, rd, rn, dtype, 2, 0.5)
    assert np.array_equal(weights(), np.ones_like(d))
    ctx.close()


# ---------------------------------------------------------- 4. zero normal --
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_normal_is_kept(monkeypatch, oracle, dtype):
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    rn = rn.copy()
    eps = eps_of(dtype)
    ctx = context(monkeypatch, dtype)
    _, Ti, rn0, d, ids = matched(ctx, ref, nrm, rd, rn, dtype, 3, np.inf)
    ctx.outlier_surface_normal(0, eps=eps)
    before = ctx.get_weights()
    j = int(np.flatnonzero(before.sum(axis=1) == 0)[0])  # (a point the filter rejects entirely)
    rn[j] = 0
    ctx.set_reading_normals(rn)
    ctx.outlier_surface_normal(0, eps=eps)
    w = ctx.get_weights()
    ctx.close()
    rn0 = rn0.copy()
    rn0[j] = 0
    assert np.array_equal(w, sn_weights(rn0, Ti, nrm, ids, eps))
    assert (w[j] == 1).all()
    assert np.array_equal(np.delete(w, j, 0), np.delete(before, j, 0))


# ------------------------------------------------------------ 5. whole ICP --
def restated_icp(oracle, dtype, rd, ref, nrm, rn, filters, minimizer, maxit, diff, max_dist=np.inf, T_init=None):
    """ICP::compute (ICP.cpp:281-449) over the oracle's primitives, with the
    restated filter wherever `filters` names it.  Returns T, iterations and
    the last iteration's statistics."""
    dt = np.dtype(dtype).type
    rows = ref.shape[1]
    D = rows - 1
    mean = np.array([np.cumsum(ref[:, c], dtype=dtype)[-1] / dt(ref.shape[0]) for c in range(D)], dtype)
    refc = ref.copy()
    refc[:, :D] -= mean
    T_rm = np.eye(rows, dtype=dtype)
    T_rm[:D, D] = mean
    # T_refMean_dataIn = T_refIn_refMean^-1 T_init (ICP.cpp:345-346; the inverse is a pure translation)
    T0 = np.eye(rows, dtype=dtype) if T_init is None else np.array(T_init, dtype)
    T0[:D, D] = T0[:D, D] - mean
    rd0 = oracle.transform(T0, rd)
    rn0 = rotate(T0[:D, :D], rn) if rn is not None else None
    robust = None
    Ti = np.eye(rows, dtype=dtype)
    hist = [Ti.copy()]
    it, st = 0, None
    while True:
        step = oracle.transform(Ti, rd0)
        d, ids, _ = oracle.knn(refc, step, k=1, max_dist=max_dist)
        w = np.ones_like(d) if filters else (d != np.inf).astype(dtype)
        for name, p in filters:
            if name == SN:
                f = sn_weights(rn0, Ti, nrm, ids, eps_of(dtype, p.get("maxAngle", 1.57))) if rn0 is not None else 1
            elif name == "RobustOutlierFilter":
                robust = robust or oracle.make_robust(p)
                rc, f = oracle.robust_weights(robust, d, ids)
                assert rc == 0
            else:
                rc, f = oracle.outlier_chain([(name, p)], d)
                assert rc == 0
            w = w * f
        if minimizer == P2PLANE:
            rc, A, b, st = oracle.p2plane_system(step, refc, nrm, d, ids, w)
            assert rc == 0
            rc, dT = oracle.p2plane_solve(A, b, rows, dtype)
        else:
            rc, dT, st = oracle.p2point(step, refc, d, ids, w)
        assert rc == 0
        Ti = (dT @ Ti).astype(dtype)
        it += 1
        hist.append(Ti.copy())
        if it >= maxit:
            break
        if diff and len(hist) > diff["smoothLength"]:
            L = diff["smoothLength"]
            cr = sum(abs(angular_distance(hist[-1 - i][:3, :3], hist[-2 - i][:3, :3])) for i in range(L)) / L
            ct = sum(np.linalg.norm(hist[-1 - i][:D, D].astype(np.float64) - hist[-2 - i][:D, D]) for i in range(L)) / L
            if cr < diff["minDiffRotErr"] and ct < diff["minDiffTransErr"]:
                break
    return (T_rm @ Ti @ T0).astype(dtype), it, st


def run_icp(monkeypatch, mode, dtype, yaml, rd, ref, nrm, rn, T_init=None):
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if mode == "loop" else "0")
    monkeypatch.delenv("PMX_OPTS", raising=False)
    icp = ICP(dtype)
    icp.load_yaml(yaml)
    if rn is not None:
        icp.add_descriptor("reading", "normals", rn)
    T = icp.compute(rd, ref, nrm, T_init)
    try:  # (the device loop's diagnostics exist only if it ran)
        used_loop = bool(icp.loop_diag(0, 1)[0, 2] > 0)
    except RuntimeError:
        used_loop = False
    return T, icp.stats(), used_loop


ICP_CHAINS = {
    "p2plane_trim": ([TRIM, (SN, {"maxAngle": MAX_ANGLE})], P2PLANE),
    "p2point_maxdist": ([("MaxDistOutlierFilter", {"maxDist": 0.5}), (SN, {"maxAngle": MAX_ANGLE})], P2POINT),
    "robust": ([("RobustOutlierFilter", {"robustFct": "cauchy", "scaleEstimator": "mad", "tuning": 1}),
                (SN, {"maxAngle": MAX_ANGLE})], P2PLANE),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chain", list(ICP_CHAINS))
def test_icp_loop_equals_modules_equals_restated(monkeypatch, oracle, dtype, chain):
    filters, minimizer = ICP_CHAINS[chain]
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    # the restatement alone: the filter rejects a real share at iteration 0
    d0, i0, _ = oracle.knn(ref, rd, k=1)
    share = 1 - sn_weights(rn, np.eye(4, dtype=dtype), nrm, i0, eps_of(dtype)).mean()
    print(f"rejected at iteration 0: {share:.3f}")
    assert 0.10 <= share <= 0.60
    yaml = chain_yaml(filters=filters, minimizer=minimizer, maxit=25, differential=DIFF)
    To, ito, sto = restated_icp(oracle, dtype, rd, ref, nrm, rn, filters, minimizer, 25, DIFF)
    Tl, sl, used = run_icp(monkeypatch, "loop", dtype, yaml, rd, ref, nrm, rn)
    Tm, sm, _ = run_icp(monkeypatch, "modules", dtype, yaml, rd, ref, nrm, rn)
    print(f"iterations {sl.iterations} {sm.iterations} {ito}; kept {sl.kept} {sm.kept} {sto.kept}; "
          f"|Tl-Tm| {np.linalg.norm(Tl - Tm):.3g} |Tl-To| {np.linalg.norm(Tl - To):.3g}")
    assert used, "the loop-mode run fell back to module calls"
    assert sl.iterations == sm.iterations == ito
    assert sl.kept == sm.kept == sto.kept
    assert sl.rejected_matches == sm.rejected_matches == sto.rejected_matches
    assert np.linalg.norm(Tl - Tm) <= TOL[dtype]
    assert np.linalg.norm(Tl - To) <= TOL[dtype]
    # the filter acted: the same chain without it ends elsewhere
    plain = [f for f in filters if f[0] != SN]
    Tp, sp, _ = run_icp(monkeypatch, "loop", dtype, chain_yaml(filters=plain, minimizer=minimizer, maxit=25,
                                                              differential=DIFF), rd, ref, nrm, None)
    assert np.linalg.norm(Tl - Tp) > TOL[dtype]


def test_default_max_angle_is_1_57(monkeypatch, oracle):
    dtype = np.float32
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    runs = {}
    for tag, p in (("default", {}), ("1.57", {"maxAngle": 1.57}), ("1.0", {"maxAngle": 1.0})):
        yaml = chain_yaml(filters=[TRIM, (SN, p)], maxit=3)
        runs[tag] = run_icp(monkeypatch, "modules", dtype, yaml, rd, ref, nrm, rn)
    assert np.array_equal(runs["default"][0], runs["1.57"][0]) and runs["default"][1].kept == runs["1.57"][1].kept
    assert runs["default"][1].kept != runs["1.0"][1].kept


# -------------------------------------------------------- 6. loop fallback --
def test_two_filters_fall_back_to_module_calls(monkeypatch, oracle):
    dtype = np.float32
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    e = float(eps_of(dtype))
    ctx = context(monkeypatch, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.set_reading_normals(rn)
    with pytest.raises(_capi.InvalidParameter, match="one SurfaceNormalOutlierFilter"):
        ctx.loop_begin(filters=[(SN, e), (SN, e)], checkers=[("CounterTransformationChecker", 5)])
    ctx.loop_begin(filters=[("TrimmedDistOutlierFilter", 0.85), (SN, e)],
                   checkers=[("CounterTransformationChecker", 5)])
    assert ctx.loop_run(100).iterations == 5
    ctx.close()
    filters = [TRIM, (SN, {"maxAngle": MAX_ANGLE}), (SN, {"maxAngle": 1.2})]
    yaml = chain_yaml(filters=filters, maxit=25, differential=DIFF)
    To, ito, sto = restated_icp(oracle, dtype, rd, ref, nrm, rn, filters, P2PLANE, 25, DIFF)
    Tl, sl, used = run_icp(monkeypatch, "loop", dtype, yaml, rd, ref, nrm, rn)
    assert not used
    assert sl.iterations == ito and sl.kept == sto.kept
    assert np.linalg.norm(Tl - To) <= TOL[dtype]


# --------------------------------------------------------- 8. ICPSequence --
def test_icp_sequence(monkeypatch, oracle):
    dtype = np.float32
    monkeypatch.delenv("PMX_OPTS", raising=False)
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    yaml = chain_yaml(filters=[TRIM, (SN, {"maxAngle": MAX_ANGLE})], maxit=25, differential=DIFF)
    seq = ICPSequence(dtype)
    seq.load_yaml(yaml)
    assert seq.set_map(ref, nrm)
    # two scans: the reading, then the reading moved a little
    T2 = rigid(4, rot3([0, 1, 0], 0.01), [0.01, 0.0, -0.01]).astype(dtype)
    rd2 = (rd @ T2.T).astype(dtype)
    rn2 = (rn @ T2[:3, :3].T).astype(dtype)
    out = []
    for scan, normals in ((rd, rn), (rd2, rn2)):
        seq.add_descriptor("reading", "normals", normals)
        out.append(seq.compute(scan))
    fresh = ICP(dtype)
    fresh.load_yaml(yaml)
    fresh.add_descriptor("reading", "normals", rn2)
    Tf = fresh.compute(rd2, ref, nrm)
    assert np.linalg.norm(out[1] - Tf) <= TOL[dtype]
    # and the filter acted on the sequence path
    plain = ICPSequence(dtype)
    plain.load_yaml(chain_yaml(filters=[TRIM], maxit=25, differential=DIFF))
    assert plain.set_map(ref, nrm)
    plain.compute(rd)
    assert np.linalg.norm(plain.compute(rd2) - out[1]) > TOL[dtype]


# ------------------------------------- readingStepDataPointsFilters re-upload --
STEP_FILTER = "readingStepDataPointsFilters:\n  - IdentityDataPointsFilter\n"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_step_filter_reupload_and_initial_rotation(monkeypatch, oracle, dtype):
    """With a step filter the reading is re-uploaded every iteration from a
    host copy in <refMean>, whose normals the host rotates by T_refMean_dataIn;
    without one the device rotates them at the upload.  The reading is given
    in a frame turned by 1 rad, which T_init undoes, so that rotation
    matters; both paths must equal the restated reference (which applies R_0
    as the restatement fixes it)."""
    ref, nrm, rd, rn = clouds(oracle)
    Q = rigid(4, rot3([1, 1, 1], 1.0), [0.3, -0.2, 0.1])
    Qi = np.linalg.inv(Q)
    ref, nrm, rd, rn = ref.astype(dtype), nrm.astype(dtype), (rd @ Qi.T).astype(dtype), (rn @ Qi[:3, :3].T).astype(dtype)
    T_init = Q.astype(dtype)
    # (on the restatement alone: leaving the normals unrotated would reject another share)
    _, i0, _ = oracle.knn(ref, oracle.transform(T_init, rd), k=1)
    eye = np.eye(4, dtype=dtype)
    share = [1 - sn_weights(n, eye, nrm, i0, eps_of(dtype)).mean() for n in (rotate(T_init[:3, :3], rn), rn)]
    assert abs(share[0] - share[1]) > 0.05
    filters = [TRIM, (SN, {"maxAngle": MAX_ANGLE})]
    yaml = chain_yaml(filters=filters, maxit=25, differential=DIFF)
    To, ito, sto = restated_icp(oracle, dtype, rd, ref, nrm, rn, filters, P2PLANE, 25, DIFF, T_init=T_init)
    Ts, ss, used_s = run_icp(monkeypatch, "loop", dtype, STEP_FILTER + yaml, rd, ref, nrm, rn, T_init)
    Tl, sl, used_l = run_icp(monkeypatch, "loop", dtype, yaml, rd, ref, nrm, rn, T_init)
    print(f"iterations {ss.iterations} {sl.iterations} {ito}; kept {ss.kept} {sl.kept} {sto.kept}; "
          f"|Ts-To| {np.linalg.norm(Ts - To):.3g} |Tl-To| {np.linalg.norm(Tl - To):.3g}")
    assert not used_s and used_l  # (step filters take the module calls)
    assert ss.iterations == sl.iterations == ito
    assert ss.kept == sl.kept == sto.kept
    assert ss.rejected_matches == sl.rejected_matches == sto.rejected_matches
    assert np.linalg.norm(Ts - To) <= TOL[dtype]
    assert np.linalg.norm(Tl - To) <= TOL[dtype]


# ------------------------------------------- 7. two ranks on the one GPU --
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(n, world, rank):
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


SHARD_CHAINS = {"trim": [TRIM], "trim_sn": [TRIM, (SN, {"maxAngle": MAX_ANGLE})]}
SHARD_ITERS = 8


def _sn_rank(rank, world, port, outdir):
    """One rank: its own process and pmx_ctx on device 0, the reading's
    contiguous shard with the shard's normals, the collectives over the host
    callbacks with gloo as the transport (tests/test_gpu_multirank.py)."""
    os.environ.pop("PMX_OPTS", None)
    os.environ["PMX_DEVICE_LOOP"] = "1"
    import torch  # noqa: F401 (its HIP runtime first, as bench.py does)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import oracle_py

        dtype = np.float32
        ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle_py))
        lo, hi = _shard(rd.shape[0], world, rank)
        shard, shard_n = np.ascontiguousarray(rd[lo:hi]), np.ascontiguousarray(rn[lo:hi])
        comm = _capi.gloo_host_comm()
        e = float(eps_of(dtype))
        res = {}
        for tag, filters in SHARD_CHAINS.items():
            # whole ICP through the host chain (device loop)
            icp = ICP(dtype)
            icp.comm_init_host(comm)
            icp.load_yaml(chain_yaml(filters=filters, maxit=25, differential=DIFF))
            icp.add_descriptor("reading", "normals", shard_n)
            T = icp.compute(shard, ref, nrm)
            s = icp.stats()
            res[f"icp_{tag}"] = np.concatenate([T.astype(np.float64).ravel(), [s.iterations, s.kept]])
            icp.close()
            loop_filters = [("TrimmedDistOutlierFilter", 0.85)] + ([(SN, e)] if tag == "trim_sn" else [])
            # collectives: one iteration of module calls, then a fixed number
            # of device-loop iterations with the quantile from the radix passes
            # (spec_select=0: the same collectives every iteration) and with
            # the exchanged window (default)
            for opt in ("0", "1"):
                ctx = _capi.Context(0, dtype)
                ctx.set_option("spec_select", opt)
                ctx.comm_init_host(comm)
                ctx.set_reference(ref, nrm)
                ctx.set_reading(shard)
                ctx.set_reading_normals(shard_n)
                c0 = ctx.comm_stats()
                ctx.match(np.eye(4, dtype=dtype), knn=1)
                ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
                if tag == "trim_sn":
                    ctx.outlier_surface_normal(1, eps=e)
                _, _, st = ctx.p2plane_system()
                c1 = ctx.comm_stats()
                ctx.set_reading(shard)
                ctx.set_reading_normals(shard_n)
                c2 = ctx.comm_stats()
                ctx.loop_begin(filters=loop_filters, checkers=[("CounterTransformationChecker", SHARD_ITERS)])
                ls = ctx.loop_run(SHARD_ITERS)
                c3 = ctx.comm_stats()
                hits, misses = ctx.loop_select_stats()
                stalls = ctx.comm_loop_stats()[2]
                res[f"coll_{tag}_{opt}"] = np.array([c1[0] - c0[0], c1[1] - c0[1], c3[0] - c2[0], c3[1] - c2[1],
                                                     ls.iterations, hits, misses, stalls, st.kept, ls.last.kept])
                ctx.close()
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu(oracle, tmp_path):
    dtype = np.float32
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_sn_rank, args=(i, 2, port, str(tmp_path))) for i in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.exitcode is None:
            p.kill()
    assert codes == [0, 0], codes
    r = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds(oracle))
    for tag, filters in SHARD_CHAINS.items():
        np.testing.assert_array_equal(r[0][f"icp_{tag}"], r[1][f"icp_{tag}"])  # every rank the same transform
        To, ito, sto = restated_icp(oracle, dtype, rd, ref, nrm, rn, filters, P2PLANE, 25, DIFF)
        a = r[0][f"icp_{tag}"]
        frob = np.linalg.norm(a[:16].reshape(4, 4) - To.astype(np.float64))
        print(f"{tag}: iterations {int(a[16])}/{ito} kept {int(a[17])}/{sto.kept} |dT| = {frob:.3g}")
        assert frob <= TOL[dtype]
        assert int(a[16]) == ito and int(a[17]) == sto.kept
    assert np.linalg.norm(r[0]["icp_trim"][:16] - r[0]["icp_trim_sn"][:16]) > TOL[dtype]  # (the filter acted)
    passes = 3  # (radix passes of a float quantile: one histogram all-reduce each)
    for rank in (0, 1):
        for opt in ("0", "1"):
            plain = [int(v) for v in r[rank][f"coll_trim_{opt}"]]
            sn = [int(v) for v in r[rank][f"coll_trim_sn_{opt}"]]
            print(f"rank {rank} spec_select={opt}: [Trimmed] {plain} [Trimmed, SurfaceNormal] {sn}")
            assert sn[8] < plain[8] and sn[9] < plain[9]  # (fewer pairs kept: the filter ran on the shards)
            # one iteration of module calls: the same collectives
            assert sn[:2] == plain[:2] and sn[0] >= 1
            assert sn[4] == plain[4] == SHARD_ITERS
            if opt == "0":  # radix passes every iteration: identical counts
                assert sn[2:4] == plain[2:4]
                assert sn[3] == 0 and sn[2] % (1 + passes) == 0 and sn[2] // (1 + passes) >= SHARD_ITERS
            # per iteration, net of what a window miss or a stall adds (the
            # two chains' quantiles move differently, so their misses may):
            # the window's all-gather and the system's all-reduce, no more
            for ar, ag, _, hits, misses, stalls in (plain[2:8], sn[2:8]):
                if opt == "1":
                    assert ar == ag + passes * misses + stalls
                    assert ag <= SHARD_ITERS + 1 + 2 * 4 * stalls

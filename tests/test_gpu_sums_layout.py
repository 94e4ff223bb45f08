"""The minimisers' result block (csrc/pmx_sums.h) read by every one of its
readers: the reduction kernels write it, the module path reads it back on the
host (Context.p2plane_system / p2point_system / p2point_similarity_system,
p2plane_covariance) and the device loop's step reads it on the device
(finalize_step_kernel / loop_step_kernel).  For one match every reader must
see the same statistics and the same system.

Cloud (sums_cloud): about 300 reference points with normals on a curved
surface (3-D) or curve (2-D), 257 reading points (one more than a block of
the reductions: the grid-stride tail and a second block's partials) on the
same surface after a small rigid motion, the whole scene centred at the
origin.  Every tenth reading point is lifted 0.5 off the surface, past the
MaxDistOutlierFilter of every chain here (0.2), so rejected matches and
rejected points are not zero; test_cloud_fills_every_statistic asserts that on
the CPU through the oracle.

Forms: point-to-plane with 0/1 weights (the packed upper triangle),
point-to-plane behind a RobustOutlierFilter (the full asymmetric A),
point-to-point in two passes, point-to-point similarity (sigma behind the
moments); float and double, 2-D and 3-D, knn 1 and 2.  The module path's
values and a one-iteration device loop (Counter 1) come from the same context.

Bounds: the five statistics are equal exactly.  The loop's first T_iter
against the step recomputed in float64 numpy from the module path's sums:
the project's bar, ||dT||_F <= 1e-5 (float) / 1e-12 (double), as
tests/test_gpu_step_degenerate.py states it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import step_cases as sc

DTYPES = [np.float32, np.float64]
FORMS = ["p2plane", "p2plane_robust", "p2point", "similarity"]
MINIMIZER = {"p2plane": "PointToPlaneErrorMinimizer", "p2plane_robust": "PointToPlaneErrorMinimizer",
             "p2point": "PointToPointErrorMinimizer", "similarity": "PointToPointSimilarityErrorMinimizer"}
STATS = ("kept", "nonzero_weights", "rejected_matches", "rejected_points", "sum_w")
MAX_DIST = 0.2
N_READING = 257
ROBUST_TUNING = 0.05  # (cauchy on the squared distance, scale 1: weights between ~0.2 and 1 on this cloud)


def _height(x, y):
    return 0.25 * np.sin(2.0 * x) + 0.2 * np.cos(2.5 * y) + 0.15 * x * y


def _surface(u, D):
    """Points and unit normals of the surface at the parameters u."""
    if D == 3:
        x, y = u[:, 0], u[:, 1]
        p = np.stack([x, y, _height(x, y)], 1)
        n = np.stack([-(0.5 * np.cos(2.0 * x) + 0.15 * y), -(-0.5 * np.sin(2.5 * y) + 0.15 * x), np.ones_like(x)], 1)
    else:
        x = u[:, 0]
        p = np.stack([x, 0.3 * np.sin(2.0 * x) + 0.2 * x * x], 1)
        n = np.stack([-(0.6 * np.cos(2.0 * x) + 0.4 * x), np.ones_like(x)], 1)
    return p, n / np.linalg.norm(n, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def sums_cloud(D, dtype):
    """(reading, reference, normals) in dtype, homogeneous points."""
    rng = np.random.default_rng(257 + D)
    if D == 3:
        g = np.stack(np.meshgrid(np.linspace(-1, 1, 17), np.linspace(-1, 1, 18), indexing="ij"), -1).reshape(-1, 2)
        u_ref = g + rng.uniform(-0.02, 0.02, g.shape)
    else:
        u_ref = np.linspace(-1, 1, 300)[:, None] + rng.uniform(-0.002, 0.002, (300, 1))
    ref, nrm = _surface(u_ref, D)
    p, n = _surface(rng.uniform(-0.95, 0.95, (N_READING, D - 1)), D)
    p = p + rng.normal(scale=0.004, size=p.shape)
    p[::10] += 0.5 * n[::10]  # 26 of 257 beyond MAX_DIST
    centre = ref.mean(0)
    ref, p = ref - centre, p - centre
    p = p - p[np.arange(N_READING) % 10 != 0].mean(0)  # (the kept pairs' centroid near the origin)
    rd = sc.move(p, D, rot=(0.8e-2, -1.1e-2, 1.3e-2), trans=(1.2e-2, -0.9e-2, 0.7e-2))
    return sc.hom(rd.astype(dtype), dtype), sc.hom(ref.astype(dtype), dtype), np.ascontiguousarray(nrm, dtype=dtype)


def stats_of(st):
    return tuple(getattr(st, f) for f in STATS)


# -------------------------------------------------------------------- the CPU --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("knn", [1, 2])
def test_cloud_fills_every_statistic(oracle, dtype, D, knn):
    """Precondition of the GPU tests below, on the reference side: none of the
    five statistics is zero on this cloud, for either minimiser."""
    rd, ref, nrm = sums_cloud(D, dtype)
    assert len(rd) == N_READING and 290 <= len(ref) <= 310
    assert np.abs(ref[:, :D].mean(0)).max() < 1e-6
    d, ids, _ = oracle.knn(ref, rd, k=knn)
    rc, w = oracle.outlier_chain([("MaxDistOutlierFilter", {"maxDist": MAX_DIST})], d)
    assert rc == 0
    rc, A, b, st = oracle.p2plane_system(rd, ref, nrm, d, ids, w)
    assert rc == 0
    rc, _, st2 = oracle.p2point(rd, ref, d, ids, w)
    assert rc == 0
    print(f"D={D} knn={knn} {np.dtype(dtype).name}: {stats_of(st)} cond2(A) {np.linalg.cond(A):.3g}")
    for s in (st, st2):
        assert all(v > 0 for v in stats_of(s))
        assert s.rejected_points >= 26 and s.kept < knn * N_READING
    assert stats_of(st)[:4] == stats_of(st2)[:4]


# -------------------------------------------------------------------- the GPU --
def loop_cfg_robust(P, knn):
    """pmx_loop_cfg of [MaxDist, Robust cauchy without a scale estimator], Counter 1
    (Context.loop_begin has no robust parameters)."""
    cfg = P.LoopCfg()
    cfg.knn = knn
    cfg.max_dist = float("inf")
    cfg.n_filters = 2
    cfg.filter_kind[0] = P.FILTER_KIND["MaxDistOutlierFilter"]
    cfg.filter_p[0][0] = MAX_DIST
    cfg.filter_kind[1] = 7  # PMX_FILTER_ROBUST
    cfg.robust_fct = P.ROBUST_FCT["cauchy"]
    cfg.robust_estimator = 0  # PMX_RSE_NONE
    cfg.robust_first_call = 1
    cfg.robust_tuning = ROBUST_TUNING
    cfg.robust_approx = float("inf")
    cfg.minimizer = 0
    cfg.n_checkers = 1
    cfg.checker_kind[0] = P.CHECK_KIND["CounterTransformationChecker"]
    cfg.checker_p[0][0] = 1.0
    cfg.keep_trace = 1
    return cfg


@functools.lru_cache(maxsize=None)
def run_form(form, dtype, D, knn, onepass=None):
    """One context: the module path's sums and statistics of the match at the
    identity, the covariance sums (3-D point-to-plane), then a one-iteration
    device loop.  -> dict(sums, stats, cov, loop_stats, T)."""
    from libpointmatcher_amd import _capi as P
    rd, ref, nrm = sums_cloud(D, dtype)
    rows = D + 1
    ctx = P.Context(0, dtype)
    try:
        if onepass is not None:
            ctx.set_option("p2p_onepass", onepass)
        ctx.set_reference(ref, nrm)
        ctx.set_reading(rd)
        ctx.match(np.eye(rows, dtype=dtype), knn=knn)
        ctx.outlier("MaxDistOutlierFilter", 0, maxDist=MAX_DIST)
        if form == "p2plane_robust":
            ctx.outlier_robust(1, "cauchy", ROBUST_TUNING, np.inf, P.RS_NONE, 0.0)
        out = {"cov": None}
        if form in ("p2plane", "p2plane_robust"):
            *sums, st = ctx.p2plane_system()
            if D == 3:
                A, b = sums
                T_step = sc.increment64(np.linalg.solve(A.astype(dtype).astype(np.float64),
                                                        b.astype(dtype).astype(np.float64)), rows).astype(dtype)
                out["cov"] = ctx.p2plane_covariance(T_step)
        elif form == "p2point":
            *sums, st = ctx.p2point_system()
        else:
            *sums, st = ctx.p2point_similarity_system()
        out["sums"], out["stats"] = sums, stats_of(st)
        if form == "p2plane_robust":
            cfg = loop_cfg_robust(P, knn)
            T0 = np.eye(rows, dtype=dtype)
            ctx._chk(ctx._l.pmx_loop_begin(ctx.h, C.byref(cfg), T0.ctypes.data_as(C.c_void_p)))
        else:
            ctx.loop_begin(knn=knn, filters=[("MaxDistOutlierFilter", MAX_DIST)], minimizer=MINIMIZER[form],
                           checkers=[("CounterTransformationChecker", 1)], keep_trace=True)
        ls = ctx.loop_run(1)
        assert ls.iterations == 1 and ls.done
        out["loop_stats"] = stats_of(ls.last)
        out["T"] = ctx.loop_T(ls)
        assert np.array_equal(out["T"], ctx.loop_trace(0, 1)[0])
        return out
    finally:
        ctx.close()


def step64(form, sums, dtype, rows):
    """The step in float64 numpy from the module path's sums, cast to T as the
    step casts them."""
    t = lambda a: np.asarray(a).astype(dtype).astype(np.float64)
    if form in ("p2plane", "p2plane_robust"):
        A, b = sums
        return sc.increment64(np.linalg.solve(t(A), t(b)), rows)
    if form == "p2point":
        mp, mq, m = sums
        return sc.kabsch(t(m), t(mp), t(mq))[0]
    mp, mq, m, sigma = sums
    return sc.kabsch(t(m), t(mp), t(mq), sigma=float(t(sigma)))[0]


CASES = [(f, dt, D, k) for f in FORMS for dt in DTYPES for D in (2, 3) for k in (1, 2)]


# (a) the module path's host readback and the loop's device step read the same statistics
@pytest.mark.gpu
@pytest.mark.parametrize("form,dtype,D,knn", CASES)
def test_statistics_agree(form, dtype, D, knn):
    r = run_form(form, dtype, D, knn)
    print(f"{form} {np.dtype(dtype).name} D={D} knn={knn}: module {r['stats']} loop {r['loop_stats']}")
    assert all(v > 0 for v in r["stats"])  # (not the equality of zeros)
    assert r["stats"] == r["loop_stats"]
    if form != "p2plane_robust":  # 0/1 weights: the sum of the weights is the kept count
        assert r["stats"][4] == r["stats"][0]
    else:
        assert 0 < r["stats"][4] < r["stats"][0]


# (b) ... and the same system: the loop's step against float64 numpy on the module path's sums
@pytest.mark.gpu
@pytest.mark.parametrize("form,dtype,D,knn", CASES)
def test_step_from_module_sums(form, dtype, D, knn):
    dn = np.dtype(dtype).name
    r = run_form(form, dtype, D, knn)
    want = step64(form, r["sums"], dtype, D + 1)
    gap = np.linalg.norm(r["T"].astype(np.float64) - want)
    print(f"{form} {dn} D={D} knn={knn}: |T_loop - step64(module sums)| = {gap:.3g}, |step| = "
          f"{np.linalg.norm(want - np.eye(D + 1)):.3g}")
    assert np.linalg.norm(want - np.eye(D + 1)) > 1e-3  # the step moved
    assert gap <= sc.BAR[dn]


# (c) double: the one-pass layout (raw moments) and the two passes' hold the same sums
@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("knn", [1, 2])
def test_onepass_equals_two_passes(D, knn):
    one = run_form("p2point", np.float64, D, knn, onepass=1)
    two = run_form("p2point", np.float64, D, knn, onepass=0)
    gap = np.linalg.norm(one["T"] - two["T"])
    print(f"D={D} knn={knn}: |T_onepass - T_twopass| = {gap:.3g}; {one['loop_stats']}")
    assert all(v > 0 for v in one["loop_stats"])
    assert one["loop_stats"] == two["loop_stats"] == two["stats"]
    assert gap <= sc.BAR["float64"]
    want = step64("p2point", two["sums"], np.float64, D + 1)
    assert np.linalg.norm(one["T"] - want) <= sc.BAR["float64"]


# (d) the covariance area behind the system: symmetric sums over the same kept pairs
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["p2plane", "p2plane_robust"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knn", [1, 2])
def test_covariance_area(form, dtype, knn):
    r = run_form(form, dtype, 3, knn)
    H, Q, pairs = r["cov"]
    assert np.array_equal(H, H.T) and np.array_equal(Q, Q.T)
    assert np.isfinite(H).all() and np.isfinite(Q).all() and np.diag(H).min() > 0 and np.diag(Q).min() > 0
    assert pairs == r["stats"][0]

"""One step of the device-resident ICP loop (finalize_step_kernel /
loop_step_kernel: csrc/pmx_step.h over csrc/common/pmx_dense.h) on degenerate
geometry — floors, corridors, lines, thin slabs — against references that
share no code with the kit or the oracle (tests/step_cases.py): an exact
rational solve of the structurally rank-deficient normal equations, the rigid
increment in float64, Kabsch with the determinant rule in float64.

Every test isolates one step: the module path's sums of iteration 0
(Context.p2plane_system / p2point_system: float64, held to the oracle at 1e-12
elsewhere) are cast to T as the step casts them and solved independently; the
result is compared with the first T_iter of a device loop on the same context
(Counter 1).  The Context API re-centres nothing: the coordinates are what
step_cases wrote.  The match must be the identity (asserted on get_matches);
the chain is empty or TrimmedDist 1.0.  The same preconditions (structural
zeros, sub-system rank, conditioning targets, identity match by brute force)
are asserted on the CPU through the oracle in tests/test_dense_kit.py.

Bounds.  Loop against the host kit (the module path's code) and the oracle:
the project's bar, ||dT||_F <= 1e-5 (float) / 1e-12 (double).  Loop against
the exact solution:
    ||x - x_exact|| <= K_SOLVE n eps_T cond2(A_r) ||x_exact||,  K_SOLVE = 1.8,
x read back out of T_iter (step_cases.step_vector), cond2 from the reference
side in float64.  K_SOLVE is 8 x the largest ratio measured on the CPU for the
host kit and the oracle (0.22, a 2-D rank-2 wall in double; 3-D table 0.047,
switch systems 0.0014; tests/test_dense_kit.py lists them); it was fixed
before any device result was seen.  Point-to-point against float64 Kabsch:
||T - T_kabsch||_F <= K_P2P eps_T, K_P2P = 34 = 8 x 4.3 (the kit's largest
deviation on these cases, the 3-D reflection in double).

Scope.  Every kept-pair centroid here lies within a few spreads of the origin.
Overlaps far off centre, where the one-pass point-to-point form (p2p_onepass,
double) loses digits to cancellation, are a separate piece of work and
deliberately not covered.
"""
import numpy as np
import pytest

import step_cases as sc
from helpers import chain_yaml, dense_kit

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
P2PLANE, P2P, SIM = "PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer", "PointToPointSimilarityErrorMinimizer"


def one_step(dtype, rd, ref, nrm, minimizer, trimmed=False, options=None):
    """(module sums of iteration 0, first T_iter of the device loop, matches)
    on one context.  Asserts the identity match with unit weights."""
    from libpointmatcher_amd import _capi
    rows = ref.shape[1]
    ctx = _capi.Context(0, dtype)
    try:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        ctx.set_reference(ref, nrm)
        ctx.set_reading(rd)
        ctx.match(np.eye(rows, dtype=dtype), knn=1)
        if trimmed:
            ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=1.0)
        else:
            ctx.outlier_default()
        d, ids = ctx.get_matches()
        assert np.array_equal(ids[:, 0], np.arange(len(rd)))  # precondition: the match is the identity
        w = ctx.get_weights()
        assert (w == 1).all()
        if minimizer == P2PLANE:
            sums = ctx.p2plane_system()
        elif minimizer == P2P:
            sums = ctx.p2point_system()
        else:
            sums = ctx.p2point_similarity_system()
        assert sums[-1].kept == len(rd)
        ctx.loop_begin(knn=1, filters=[("TrimmedDistOutlierFilter", 1.0)] if trimmed else (), minimizer=minimizer,
                       checkers=[("CounterTransformationChecker", 1)], keep_trace=True)
        st = ctx.loop_run(1)
        assert st.iterations == 1 and st.done
        T = ctx.loop_T(st)
        assert np.array_equal(T, ctx.loop_trace(0, 1)[0])
        return sums, T, (d, ids, w)
    finally:
        ctx.close()


def check_p2plane_step(oracle, At, bt, x_exact, live, T, dtype, tag):
    """The loop's first T_iter against the exact solution (K_SOLVE bound), the
    host kit and the oracle (the project's bar)."""
    dn = np.dtype(dtype).name
    rows = T.shape[0]
    x_dev = sc.step_vector(T)
    ratio = sc.solve_ratio(x_dev, x_exact, At, live, dtype)
    dT_kit, x_kit = dense_kit().p2plane_step(At, bt, rows, dtype)
    rc, dT_o = oracle.p2plane_solve(At, bt, rows, dtype)
    assert rc == 0
    g_kit = np.linalg.norm(T.astype(np.float64) - dT_kit.astype(np.float64))
    g_o = np.linalg.norm(T.astype(np.float64) - dT_o.astype(np.float64))
    g_x = np.linalg.norm(T.astype(np.float64) - sc.increment64(x_exact, rows))
    print(f"{tag} {dn}: cond2 {sc.cond2(At, live):.3g} |x| {np.linalg.norm(x_exact):.3g} ratio {ratio:.3g} "
          f"(host kit {sc.solve_ratio(x_kit, x_exact, At, live, dtype):.3g}); |T - kit| {g_kit:.3g} "
          f"|T - oracle| {g_o:.3g} |T - exact| {g_x:.3g}")
    assert ratio <= sc.K_SOLVE, tag
    assert g_kit <= sc.BAR[dn] and g_o <= sc.BAR[dn], tag
    return x_dev


# ------------------------------------------- point-to-plane, exact rank 1 - 6 --
# Each case depends on the branch it targets:
#  * ranks 1 - 5 (3-D) and 1 - 2 (2-D): A is singular, so llt() fails or leaves a
#    non-positive / garbage diagonal.  If well_conditioned() returned true here,
#    llt_solve would divide by that diagonal: inf / NaN or values of order
#    1 / eps in the null directions, against a bound of ~1e-8 |x| — the K_SOLVE
#    assertion fails (a NaN fails every <=).
#  * the same ranks: a basic solution (the free variables set to zero after the
#    QR's column permutation, instead of the minimal norm) differs from the
#    minimal-norm one wherever the live sub-system is not what the pivoting
#    kept; with zero rows / columns exact the two coincide only if the solver
#    drops exactly the null columns, which is what the exact reference states.
#    A basic solution that keeps a null column (any other choice) puts a
#    non-zero of order |x| into x[zero]; x_exact[zero] = 0 exactly, so the
#    bound fails.  The motion's null-space part (in-plane slide of the floor,
#    slide along the corridor) is of the size of x itself, so a solver that
#    "recovers" it instead of leaving it alone fails the same way.
#  * rank 6 and 2-D rank 3 are the full-rank controls of the same geometry
#    family: LLT on both device branches.
RANKS = [(3, r) for r in range(1, 7)] + [(2, r) for r in range(1, 4)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,rank", RANKS)
def test_plane_exact_rank(oracle, dtype, D, rank):
    rd, ref, nrm, zero = (sc.plane3d_case if D == 3 else sc.plane2d_case)(rank, dtype)
    # (the odd ranks run the TrimmedDist 1.0 chain, the even ones the empty chain)
    (A, b, st), T, _ = one_step(dtype, rd, ref, nrm, P2PLANE, trimmed=rank % 2 == 1)
    At, bt, x_exact, live = sc.check_structure(A, b, zero, dtype)  # before looking at the loop's result
    assert len(live) == rank
    x_dev = check_p2plane_step(oracle, At, bt, x_exact, live, T, dtype, f"D={D} rank {rank}")
    # the null directions are left alone (part of the bound above; printed for the record)
    print(f"   null directions {zero}: max |x| = {np.abs(x_dev[zero]).max() if zero else 0.0:.3g}")


# Identity: b = 0 exactly, so x = 0 on either branch (rank 3: the
# rank-deficient solve, 0 <= 0 keeps the QR solution; rank 6: LLT) and
# angle_axis(0, 0) = I: the first T_iter is the identity bit for bit.  A
# shortcut firing on the singular floor divides 0 by a zero / garbage pivot
# (NaN -> the NaN rule keeps R = I but t = NaN), which fails the equality.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,rank", [(3, 3), (3, 6), (2, 2)])
def test_identity_step_is_exact(dtype, D, rank):
    _, ref, nrm, _ = (sc.plane3d_case if D == 3 else sc.plane2d_case)(rank, dtype)
    (A, b, st), T, _ = one_step(dtype, ref, ref, nrm, P2PLANE)
    assert not b.any()
    assert np.array_equal(T, np.eye(D + 1, dtype=dtype))


# ------------------------------------------------ the well_conditioned switch --
# lambda_min(A) / ||A||_F lands within a factor 2 of each target, on both sides
# of the shortcut's 1e-3 (float) / 1e-9 (double) switch; every system is full
# rank under Eigen's rule, so with or without the shortcut the step is the LLT
# solve and must reproduce the exact full solve.  A shortcut bound that were
# wrong by a constant would move the switch but not the answer; what fails
# here is a device branch that does not end in the same llt_solve (e.g. the QR
# branch calling a full-rank system deficient: the minimal-norm solve would
# zero the weakest direction, an error of order |x| against a bound of at most
# 1.8 * 6 * eps * cond2 ~ 0.1 |x| (float, cond2 9e4) and far less at the other
# targets).  Together with the exact-rank table above (where the shortcut must
# not fire) both sides of the decision are pinned.
@pytest.mark.parametrize("dtype,target", [(np.float32, t) for t in sc.SWITCH_TARGETS["float32"]] +
                         [(np.float64, t) for t in sc.SWITCH_TARGETS["float64"]])
def test_well_conditioned_switch(oracle, dtype, target):
    rd, ref, nrm = sc.switch_case(target, dtype)
    (A, b, st), T, _ = one_step(dtype, rd, ref, nrm, P2PLANE)
    At, bt = A.astype(dtype), b.astype(dtype)
    ratio = sc.conditioning_ratio(At)
    print(f"target {target:g}: lambda_min / |A|_F = {ratio:.4g}")
    assert target / 2 <= ratio <= target * 2  # precondition: the landing
    assert dense_kit().qr_rank(At, dtype) == 6  # full rank under Eigen's rule
    x_exact, live = sc.exact_min_norm(At, bt)
    assert live == list(range(6))
    check_p2plane_step(oracle, At, bt, x_exact, live, T, dtype, f"switch {target:g}")


# ------------------------------------------------ robust chain on a floor --
# RobustOutlierFilter makes the chain "full": the sums are the asymmetric
# NF x NF product (w F) F^T and the rank-3 floor goes through
# loop_solve_rank_deficient(res, full = 1).  If the flag were ignored there,
# the 36 + 6 doubles would be read as the packed upper triangle (21 + 6): b
# and most of A come from the wrong words and the step no longer equals the
# module path's, which solves the same sums on the host.
@pytest.mark.parametrize("dtype", DTYPES)
def test_robust_chain_on_a_floor(monkeypatch, oracle, dtype):
    from libpointmatcher_amd.icp import ICP
    dn = np.dtype(dtype).name
    rd, ref, nrm, zero = sc.plane3d_case(3, dtype)
    filters = (("RobustOutlierFilter", {"robustFct": "cauchy", "scaleEstimator": "mad", "tuning": 1.0}),)
    yaml = chain_yaml(filters=filters, maxit=1)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
        icp = ICP(dtype)
        icp.load_yaml(yaml)
        try:
            out[mode] = (icp.compute(rd, ref, nrm), icp.stats())
        finally:
            icp.close()
    (Tl, sl), (Tm, sm) = out["1"], out["0"]
    cfg = oracle.make_cfg(filters=filters, counter_max=1)
    rc, To, so, _ = oracle.icp(cfg, rd, ref, normals=nrm)
    assert rc == 0
    assert sl.iterations == sm.iterations == so.iterations == 1
    assert sl.kept == sm.kept == so.kept == len(rd)
    f = [np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) for a, b in ((Tl, Tm), (Tl, To), (Tm, To))]
    print(f"{dn}: |loop - modules| {f[0]:.3g} |loop - oracle| {f[1]:.3g} |modules - oracle| {f[2]:.3g}")
    assert max(f) <= sc.BAR[dn]
    # the step moved (so equality is not the equality of identities) and left the in-plane slide alone
    x = sc.step_vector(Tl)
    assert np.linalg.norm(x) > 1e-4 and np.abs(x[zero]).max() <= sc.BAR[dn]


# ------------------------------------------------------------- point to point --
def p2p_step(dtype, case, minimizer, options=None):
    rd, ref = sc.p2p_case(case, dtype)
    sums, T, match = one_step(dtype, rd, ref, None, minimizer, options=options)
    if minimizer == SIM:
        mp, mq, m, sigma, st = sums
        want, d, S = sc.kabsch(m.astype(dtype), mp.astype(dtype), mq.astype(dtype), sigma=dtype(sigma))
        kit = dense_kit().p2point_similarity_transform(m, mp, mq, sigma, dtype)
    else:
        mp, mq, m, st = sums
        want, d, S = sc.kabsch(m.astype(dtype), mp.astype(dtype), mq.astype(dtype))
        kit = dense_kit().p2point_transform(m, mp, mq, dtype)
    return rd, ref, T, want, d, S, kit, (mp, mq, m.astype(dtype)), match


def onepass_options(dtype):
    """float has the two-pass form only; double runs both (p2p_onepass, the rigid minimiser's)."""
    return [None] if dtype == np.float32 else [{"p2p_onepass": 0}, {"p2p_onepass": 1}]


# coplanar: one singular value is 0 (m has an exactly zero row); the rotation
# is unique only through the determinant rule, so a kit that built R from two
# singular directions, or took the wrong sign of the third, is off by a mirror
# (||dT|| ~ 2).  reflection / reflection2d: det(U V^T) = -1 (asserted on the
# reference side as d = -1); with the reflection pass removed the step is the
# mirror: det(R) = -1 and ||T - T_kabsch|| ~ 2 against 34 eps.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,minimizer", [("coplanar", P2P), ("coplanar", SIM), ("reflection", P2P),
                                            ("reflection", SIM), ("reflection2d", P2P)])
def test_p2point_against_kabsch(oracle, dtype, case, minimizer):
    dn = np.dtype(dtype).name
    eps = sc.EPS[dn]
    got = []
    for opt in (onepass_options(dtype) if minimizer == P2P else [None]):
        rd, ref, T, want, d, S, kit, _, (dist, ids, w) = p2p_step(dtype, case, minimizer, opt)
        D = ref.shape[1] - 1
        assert d == (1.0 if case == "coplanar" else -1.0)  # precondition: the reflection pass must (not) engage
        if case == "coplanar":
            assert S[2] <= 4 * eps * S[0] and S[1] > 0.1 * S[0]
        else:
            assert S[-1] > 1e-4 * S[0] and S[-2] - S[-1] > 0.1 * S[0]
        T64 = T.astype(np.float64)
        dev = np.linalg.norm(T64 - want) / eps
        g_kit = np.linalg.norm(T64 - kit.astype(np.float64))
        print(f"{case} {dn} {minimizer} {opt}: d {d:+.0f} |T - T_kabsch| = {dev:.3g} eps, |T - kit| = {g_kit:.3g}")
        assert dev <= sc.K_P2P
        assert g_kit <= sc.BAR[dn]
        R = T64[:D, :D]
        assert np.linalg.det(R) > 0
        if minimizer == SIM:
            # the scale against the same formula in float64 (kabsch: (s_0 + .. + d s_last) / sigma)
            assert abs(np.linalg.det(R) ** (1.0 / D) - np.linalg.det(want[:D, :D]) ** (1.0 / D)) <= sc.K_P2P * eps
        else:
            assert abs(np.linalg.det(R) - 1.0) <= sc.K_P2P * eps
            rc, To, _ = oracle.p2point(rd, ref, dist, ids, w)
            assert rc == 0 and np.linalg.norm(T64 - To.astype(np.float64)) <= sc.BAR[dn]
        got.append(T64)
    if len(got) == 2:  # double: the two-pass and the one-pass forms agree on these centred inputs
        assert np.linalg.norm(got[0] - got[1]) <= sc.BAR[dn]


# collinear: two zero singular values, R is not unique.  Any minimiser must
# return a rotation that maps the reading's line direction onto the
# reference's and the centroids onto each other; a kit without the
# determinant rule may return the mirror (det = -1).
@pytest.mark.parametrize("dtype", DTYPES)
def test_p2point_collinear_properties(oracle, dtype):
    dn = np.dtype(dtype).name
    tol = sc.K_P2P * sc.EPS[dn]
    got = []
    for opt in onepass_options(dtype):
        rd, ref, T, _, _, S, kit, (mp, mq, mT), (dist, ids, w) = p2p_step(dtype, "collinear", P2P, opt)
        assert S[1] <= 4 * sc.EPS[dn] * S[0]
        T64 = T.astype(np.float64)
        R = T64[:3, :3]
        assert np.linalg.norm(R.T @ R - np.eye(3)) <= tol
        assert abs(np.linalg.det(R) - 1.0) <= tol
        U, _, Vt = np.linalg.svd(mT.astype(np.float64))
        assert np.linalg.norm(R @ Vt[0] - U[:, 0]) <= tol
        assert np.linalg.norm(R @ mp + T64[:3, 3] - mq) <= tol
        # loop, modules (the host kit on the module sums) and oracle agree
        assert np.linalg.norm(T64 - kit.astype(np.float64)) <= sc.BAR[dn]
        rc, To, _ = oracle.p2point(rd, ref, dist, ids, w)
        assert rc == 0 and np.linalg.norm(T64 - To.astype(np.float64)) <= sc.BAR[dn]
        got.append(T64)
    if len(got) == 2:
        assert np.linalg.norm(got[0] - got[1]) <= sc.BAR[dn]

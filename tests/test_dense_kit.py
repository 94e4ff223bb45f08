"""The shared dense kit of the ICP step (csrc/common/pmx_dense.h) as the host
chain compiles it (tests/dense_shim.cpp through helpers.dense_kit), and the
oracle's restatement (oracle/pmo_dense.inc), against references that share no
code with either (tests/step_cases.py): an exact rational solve of the
structurally rank-deficient systems, the rigid increment in float64, Kabsch
with the determinant rule in float64.  No GPU.

The same scenes are the GPU cases of tests/test_gpu_step_degenerate.py; their
preconditions (identity match by brute force, exact structural zeros, the
sub-system's rank, the conditioning targets of the well_conditioned switch)
are asserted here on the oracle's sums, so they can be checked without a GPU.

Bound of a T-precision solve against the exact solution:
    ||x - x_exact|| <= K n eps_T cond2(A_r) ||x_exact||
(A_r the live sub-system, cond2 in float64 from the T-valued entries, x read
back out of the increment by step_cases.step_vector for the oracle, which
returns only the matrix).  Measured ratios ||x - x_exact|| / (n eps_T cond2
||x_exact||), the largest over both dtypes of each group:
    exact-rank table, 3-D ranks 1..6:  host kit 0.047   oracle 0.047
    exact-rank table, 2-D ranks 1..3:  host kit 0.22    oracle 0.22
    well_conditioned switch targets:   host kit 0.0014  oracle 0.0011
(host kit: the larger of x itself and x read back out of its increment; the two
sides are bit-identical on every case, |dT kit - dT oracle| = 0.)
K_SOLVE = 8 x 0.22 = 1.8: the 8 covers another sqrt / division rounding and
another sum order; it is not taken from any device result.  The ratios are
below 1 because n eps cond2 is a worst-case bound; on the ill-conditioned
switch systems (cond2 up to 9e4 in float, 9e12 in double) the solve is far
better than the bound because b is consistent with a small step.

Point-to-point: the deviation of the kit's transform from float64 Kabsch,
||T - T_kabsch||_F / eps_T, measured per case (larger of both dtypes; rigid /
similarity): coplanar 2.5 / 3.9, reflection 4.3 / 3.0, reflection2d 1.5 / 3.4;
K_P2P = 8 x 4.3 = 34 (eps_T units).
"""
import shutil

import numpy as np
import pytest

import step_cases as sc
from helpers import dense_kit

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ builds tests/dense_shim.cpp")

DTYPES = [np.float32, np.float64]
K_SOLVE, K_P2P = sc.K_SOLVE, sc.K_P2P  # (1.8 and 34: the docstring)


def unit_match(rd, ref):
    """ids / dists / weights of the identity match, as the matcher and an empty filter chain give them."""
    n = len(rd)
    D = ref.shape[1] - 1
    ids = np.arange(n, dtype=np.int32).reshape(n, 1)
    d = ((rd[:, :D] - ref[:, :D]) ** 2).sum(1, dtype=rd.dtype).reshape(n, 1)
    return d, ids, np.ones((n, 1), rd.dtype)


def oracle_system(oracle, rd, ref, nrm):
    d, ids, w = unit_match(rd, ref)
    rc, A, b, st = oracle.p2plane_system(rd, ref, nrm, d, ids, w)
    assert rc == 0 and st.kept == len(rd)
    return A, b


def solve_both(oracle, At, bt, rows, dtype):
    """(host kit x, host kit dT, oracle dT)."""
    kit = dense_kit()
    dT, x = kit.p2plane_step(At, bt, rows, dtype)
    rc, dTo = oracle.p2plane_solve(At, bt, rows, dtype)
    assert rc == 0
    return x, dT, dTo


def check_solve(oracle, At, bt, x_exact, live, rows, dtype, tag):
    dn = np.dtype(dtype).name
    x, dT, dTo = solve_both(oracle, At, bt, rows, dtype)
    rk = sc.solve_ratio(x, x_exact, At, live, dtype)
    rk_m = sc.solve_ratio(sc.step_vector(dT), x_exact, At, live, dtype)
    ro = sc.solve_ratio(sc.step_vector(dTo), x_exact, At, live, dtype)
    gap = np.linalg.norm(dT.astype(np.float64) - dTo.astype(np.float64))
    print(f"{tag} {dn}: cond2 {sc.cond2(At, live):.3g} |x| {np.linalg.norm(x_exact):.3g} ratio kit {rk:.3g} "
          f"(through the matrix {rk_m:.3g}) oracle {ro:.3g}; |dT kit - oracle| {gap:.3g}")
    assert max(rk, rk_m, ro) <= K_SOLVE, tag
    # a disagreement between the oracle's restatement and the kit is a finding
    assert gap <= sc.BAR[dn], tag
    # the increment against its float64 restatement (16 eps_T: nine entries of
    # magnitude <= 1, each a few roundings), and the solve's error carried through
    err = np.linalg.norm(dT.astype(np.float64) - sc.increment64(x, rows))
    assert err <= 16 * sc.EPS[dn], (tag, err)
    return x


# ------------------------------------------------------- the reference itself --
def test_exact_min_norm_known_answers():
    # Hilbert 4 x 4 with the solution (1, -2, 3, -4), embedded in rows / columns 0, 2, 3, 5 of a 6 x 6
    H = np.array([[1.0 / (i + j + 1) for j in range(4)] for i in range(4)])
    live = [0, 2, 3, 5]
    A = np.zeros((6, 6))
    A[np.ix_(live, live)] = H
    want = np.zeros(6)
    want[live] = [1, -2, 3, -4]
    from fractions import Fraction
    b = np.zeros(6)
    # (b from the float entries of H exactly, so that the rational solve returns `want` exactly)
    for r, i in enumerate(live):
        b[i] = float(sum(Fraction(float(H[r, c])) * Fraction(int(want[live[c]])) for c in range(4)))
    x, lv = sc.exact_min_norm(A, b)
    assert lv == live
    assert np.allclose(x, want, rtol=1e-13, atol=0)  # (b was rounded once to float64; cond(H4) ~ 1.6e4)
    assert not x[[1, 4]].any()
    with pytest.raises(ArithmeticError):
        sc.exact_min_norm(np.ones((3, 3)), np.ones(3))
    # a float64 lstsq agrees on a mildly conditioned case
    rng = np.random.default_rng(0)
    B = rng.normal(size=(3, 3))
    A = np.zeros((6, 6))
    A[np.ix_([1, 2, 4], [1, 2, 4])] = B @ B.T
    b = A @ rng.normal(size=6)
    x, _ = sc.exact_min_norm(A, b)
    assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], rtol=1e-9, atol=1e-12)


# --------------------------------------------------------- exact-rank table --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,rank", [(3, r) for r in range(1, 7)] + [(2, r) for r in range(1, 4)])
def test_exact_rank_table(oracle, dtype, D, rank):
    rd, ref, nrm, zero = (sc.plane3d_case if D == 3 else sc.plane2d_case)(rank, dtype)
    assert 100 <= len(rd) <= 2000
    assert sc.identity_match(rd, ref)
    A, b = oracle_system(oracle, rd, ref, nrm)
    At, bt, x_exact, live = sc.check_structure(A, b, zero, dtype)
    assert len(live) == rank
    # Eigen's rule sees the same rank (FullPivHouseholderQR::rank of the T-valued matrix)
    assert dense_kit().qr_rank(At, dtype) == rank
    x = check_solve(oracle, At, bt, x_exact, live, D + 1, dtype, f"D={D} rank {rank}")
    assert not x[zero].any()  # the minimal-norm solution leaves the null directions alone, exactly


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", [3, 6])
def test_identity_is_exact(oracle, dtype, rank):
    _, ref, nrm, _ = sc.plane3d_case(rank, dtype)
    A, b = oracle_system(oracle, ref, ref, nrm)
    assert not b.any()
    x, dT, dTo = solve_both(oracle, A.astype(dtype), b.astype(dtype), 4, dtype)
    assert not x.any()
    assert np.array_equal(dT, np.eye(4, dtype=dtype)) and np.array_equal(dTo, np.eye(4, dtype=dtype))


# ------------------------------------------------ the well_conditioned switch --
@pytest.mark.parametrize("dtype,target", [(np.float32, t) for t in sc.SWITCH_TARGETS["float32"]] +
                         [(np.float64, t) for t in sc.SWITCH_TARGETS["float64"]])
def test_switch_targets(oracle, dtype, target):
    rd, ref, nrm = sc.switch_case(target, dtype)
    assert sc.identity_match(rd, ref)
    A, b = oracle_system(oracle, rd, ref, nrm)
    At, bt = A.astype(dtype), b.astype(dtype)
    ratio = sc.conditioning_ratio(At)
    print(f"target {target:g}: tilt {sc.tilt_for(target):.4g} lambda_min / |A|_F = {ratio:.4g}")
    assert target / 2 <= ratio <= target * 2
    # full rank under Eigen's rule: the host path and the oracle take LLT
    assert dense_kit().qr_rank(At, dtype) == 6
    x_exact, live = sc.exact_min_norm(At, bt)
    assert live == list(range(6))
    check_solve(oracle, At, bt, x_exact, live, 4, dtype, f"switch {target:g}")


# ------------------------------------------------------------------ increment --
@pytest.mark.parametrize("dtype", DTYPES)
def test_increment_matches_float64(dtype):
    kit = dense_kit()
    eps = sc.EPS[np.dtype(dtype).name]
    rng = np.random.default_rng(4)
    for scale in (1e-6, 1e-3, 0.3, 2.0):
        for _ in range(20):
            x = (rng.normal(size=6) * scale).astype(dtype)
            got = kit.p2plane_transform(x, 4, dtype)
            assert np.linalg.norm(got.astype(np.float64) - sc.increment64(x, 4)) <= 16 * eps * max(1.0, scale)
            x2 = x[:3]
            got = kit.p2plane_transform(x2, 3, dtype)
            assert np.linalg.norm(got.astype(np.float64) - sc.increment64(x2, 3)) <= 16 * eps * max(1.0, scale)
    assert np.array_equal(kit.p2plane_transform(np.zeros(6), 4, dtype), np.eye(4, dtype=dtype))
    assert np.array_equal(kit.p2plane_transform(np.zeros(3), 3, dtype), np.eye(3, dtype=dtype))
    # PointToPlane.cpp:286-292: a NaN step keeps the identity rotation
    got = kit.p2plane_transform(np.array([np.nan, 0, 0, 1, 2, 3]), 4, dtype)
    assert np.array_equal(got[:3, :3], np.eye(3, dtype=dtype)) and np.array_equal(got[:3, 3], [1, 2, 3])


# ------------------------------------------------------------------------ SVD --
@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi_svd_rank_deficient(dtype):
    kit = dense_kit()
    eps = sc.EPS[np.dtype(dtype).name]
    rng = np.random.default_rng(8)
    for n in (2, 3, 6):
        for r in range(0, n + 1):
            B = rng.normal(size=(n, r)) @ rng.normal(size=(r, n)) if r else np.zeros((n, n))
            A = B.astype(dtype)
            U, S, V, nz = kit.jacobi_svd(A, dtype)
            U, S, V = U.astype(np.float64), S.astype(np.float64), V.astype(np.float64)
            nrm = max(np.linalg.norm(A), 1.0)
            assert np.linalg.norm(U @ np.diag(S) @ V.T - A) <= 30 * n * eps * nrm, (n, r)
            assert np.linalg.norm(U.T @ U - np.eye(n)) <= 30 * n * eps and np.linalg.norm(V.T @ V - np.eye(n)) <= 30 * n * eps
            assert (S >= 0).all() and (np.diff(S) <= 0).all()
            assert np.abs(S - np.linalg.svd(A.astype(np.float64), compute_uv=False)).max() <= 30 * n * eps * nrm
            assert nz <= n


# ------------------------------------------------------------- point to point --
def p2p_kit_and_reference(rd, ref, dtype, similarity):
    kit = dense_kit()
    mp, mq, m, sigma = sc.p2point_sums(rd, ref, dtype)
    mT = m.astype(dtype)
    if similarity:
        got = kit.p2point_similarity_transform(mT, mp, mq, sigma, dtype)
        want, d, S = sc.kabsch(mT, mp, mq, sigma=dtype(sigma))
    else:
        got = kit.p2point_transform(mT, mp, mq, dtype)
        want, d, S = sc.kabsch(mT, mp, mq)
    return got, want, d, S, (mp, mq, mT)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("similarity", [False, True])
@pytest.mark.parametrize("case", ["coplanar", "reflection", "reflection2d"])
def test_p2point_against_kabsch(oracle, dtype, case, similarity):
    dn = np.dtype(dtype).name
    rd, ref = sc.p2p_case(case, dtype)
    D = ref.shape[1] - 1
    assert sc.identity_match(rd, ref)
    got, want, d, S, _ = p2p_kit_and_reference(rd, ref, dtype, similarity)
    # the case is what it says: coplanar pairs -> a zero singular value, no
    # reflection; the mirrored cases -> det(U V^T) = -1, and no tiny non-zero gap
    assert d == (1.0 if case == "coplanar" else -1.0)
    if case == "coplanar":
        assert S[2] <= 4 * sc.EPS[dn] * S[0] and S[1] > 0.1 * S[0]
    else:
        assert S[-1] > 1e-4 * S[0] and S[-2] - S[-1] > 0.1 * S[0]
    dev = np.linalg.norm(got.astype(np.float64) - want) / sc.EPS[dn]
    print(f"{case} {dn} similarity={similarity}: S {S} d {d:+.0f} |T - T_kabsch|_F = {dev:.3g} eps")
    assert dev <= K_P2P
    R = got.astype(np.float64)[:D, :D]
    s = np.linalg.det(R) ** (1.0 / D)
    assert np.linalg.det(R) > 0  # a rotation (scaled), never the mirror
    if similarity:
        assert abs(s - np.linalg.det(want[:D, :D]) ** (1.0 / D)) <= K_P2P * sc.EPS[dn]
    else:
        assert abs(np.linalg.det(R) - 1.0) <= K_P2P * sc.EPS[dn]
        d_, ids, w = unit_match(rd, ref)
        rc, To, st = oracle.p2point(rd, ref, d_, ids, w)
        assert rc == 0
        assert np.linalg.norm(To.astype(np.float64) - got.astype(np.float64)) <= sc.BAR[dn]


@pytest.mark.parametrize("dtype", DTYPES)
def test_p2point_collinear_properties(oracle, dtype):
    """Two zero singular values: R is not unique; what Kabsch requires of any
    minimiser is that R is a rotation, maps the reading's line direction onto
    the reference's and the centroids onto each other."""
    dn = np.dtype(dtype).name
    tol = K_P2P * sc.EPS[dn]
    rd, ref = sc.p2p_case("collinear", dtype)
    assert sc.identity_match(rd, ref)
    got, _, _, S, (mp, mq, mT) = p2p_kit_and_reference(rd, ref, dtype, False)
    assert S[1] <= 4 * sc.EPS[dn] * S[0]
    T = got.astype(np.float64)
    R = T[:3, :3]
    assert np.linalg.norm(R.T @ R - np.eye(3)) <= tol
    assert abs(np.linalg.det(R) - 1.0) <= tol
    U, _, Vt = np.linalg.svd(mT.astype(np.float64))
    assert np.linalg.norm(R @ Vt[0] - U[:, 0]) <= tol  # the line's direction
    assert np.linalg.norm(R @ mp.astype(np.float64) + T[:3, 3] - mq.astype(np.float64)) <= tol  # the centroids
    d_, ids, w = unit_match(rd, ref)
    rc, To, st = oracle.p2point(rd, ref, d_, ids, w)
    assert rc == 0 and np.linalg.norm(To.astype(np.float64) - T) <= sc.BAR[dn]

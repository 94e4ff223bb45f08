"""PointToPlaneErrorMinimizer's force2D / force4DOF on the GPU
(pmx_p2plane_system_forced, pmx_loop_cfg.force, the host chain's minimiser and
the two data filters of the reference's 4-DOF regression config) against the
numpy restatement of tests/force_cases.py.

Scenes (force_cases.scene): a floor and two walls, 2540 points (not a multiple
of 4 x 256: the U = 4 tail of the k = 1 loop runs), the reading the reference
under step_cases' motion (roll, pitch, yaw ~1e-3 rad, translation ~1e-3 on x, y
and z).  k = 1 with and without the neighbour records, k = 3 and k = 5 (the
reduction's three k ranges); chains TrimmedDist 0.85, TrimmedDist +
SurfaceNormal, Robust (cauchy, mad: the FULL form of the sums); both dtypes.

Bounds.
  * 4-DOF sums: rows and columns 2..5 of pmx_p2plane_system, np.array_equal.
  * 2-D sums against the restatement on the GPU's own matches and weights: the
    expression tests/test_gpu_kernels.py holds pmx_p2plane_system to against
    the oracle, rtol 1e-12 and atol 1e-12 max|.|.
  * One step against the exact rational solve: step_cases.K_SOLVE, as
    tests/test_gpu_step_degenerate.py; host step and device step against the
    host kit on the same sums: step_cases.BAR.
  * Whole ICP, 8 Counter iterations: 2 x the distance ||T - T_restated||_F of
    the UNFORCED chain from the same restatement with the flags off, measured
    on an MI355X on this scene with the unforced code of the parent commit
    (which this change leaves as it was):
        float32  module path 1.18659e-07  device loop 1.18659e-07
        float64  module path 2.7756e-17   device loop 2.7756e-17
    (UNFORCED below).  The forced modes solve sub-problems of the same sums with
    the same solver; the factor covers the different iterate path.  Module
    path and device loop agree at step_cases.BAR with equal iteration counts.
    Measured for the forced modes (module path and device loop alike):
        float32  4DOF 1.82866e-08  2D 3.25651e-08   (bound 2.37e-07)
        float64  4DOF 0            2D 9.19976e-19   (bound 5.55e-17)
    The restatement composes T_iter = dT T_iter and the final transform with
    force_cases.matmul_seq, one rounding per product and sum.  With numpy's `@`
    (BLAS, fused multiply-adds) in its place the float64 figures were 5.55e-17
    unforced, 2.78e-17 for 4DOF and 2.48e-16 for 2D, the last one past twice the
    first: the restated force2D iterates left the library's by one unit in the
    last place of the rotation's entries from the second iteration on, while
    every iterate of the sequential composition stays within 3e-18 of them.
  * The reference's force4DOFForPointToPlaneMinimizer.yaml on cloud.00001 ->
    cloud.00000: the median relative displacement against the stored ref_trans
    below the reference's own 3 % (utest/utest.cpp:81-160).
"""
import ctypes

import numpy as np
import pytest

import force_cases as fc
import step_cases as sc
from helpers import chain_yaml, dense_kit, hom, rel_displacement

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
P2PL = "PointToPlaneErrorMinimizer"
MINIMIZER = {None: P2PL, "4DOF": P2PL + ":\n    force4DOF: 1\n", "2D": P2PL + ":\n    force2D: 1\n"}
TRIM = (("TrimmedDistOutlierFilter", {"ratio": 0.85}),)
ITERS = 8
# ||T - T_restated||_F of the unforced chain (module docstring)
UNFORCED = {"float32": {"0": 1.18659e-07, "1": 1.18659e-07}, "float64": {"0": 2.7756e-17, "1": 2.7756e-17}}

SHAPES = [(1, 1), (1, 0), (3, 1), (5, 1)]  # (knn, nbr_cache)
CHAINS = ["trim", "trim+sn", "robust"]


def run_chain(ctx, chain, nrm):
    from libpointmatcher_amd import _capi
    if chain == "none":
        ctx.outlier_default()
        return
    if chain == "robust":
        ctx.outlier_robust(0, "cauchy", tuning=1.0, scale_mode=_capi.RS_MAD)
        return
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    if chain == "trim+sn":
        ctx.outlier_surface_normal(1, max_angle=0.5)


def matched(dtype, knn, nbr, chain, parts="floor+walls", cloud=None):
    """A context with the scene matched at the identity and the chain applied."""
    from libpointmatcher_amd import _capi
    rd, ref, nrm = cloud if cloud is not None else fc.scene(dtype, parts)
    ctx = _capi.Context(0, dtype)
    ctx.set_option("nbr_cache", nbr)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    if chain == "trim+sn":
        ctx.set_reading_normals(nrm)  # (the reading is the moved reference, point for point)
    ctx.match(np.eye(ref.shape[1], dtype=dtype), knn=knn)
    run_chain(ctx, chain, nrm)
    return ctx, rd, ref, nrm


def stats_tuple(st):
    return tuple(getattr(st, f) for f, _ in st._fields_)


# ------------------------------------------------------------- 1, 2: the sums --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("knn,nbr", SHAPES)
def test_4dof_sums_are_the_6dof_block(dtype, chain, knn, nbr):
    ctx, rd, ref, nrm = matched(dtype, knn, nbr, chain)
    try:
        A6, b6, st6 = ctx.p2plane_system()
        A4, b4, st4 = ctx.p2plane_system_forced("4DOF")
        A0, b0, st0 = ctx.p2plane_system_forced(None)
    finally:
        ctx.close()
    assert 6 < st6.kept < rd.shape[0] * knn or chain == "robust"
    assert A6[2:, 2:].any() and b6[2:].any()
    assert np.array_equal(A4, A6[2:, 2:]) and np.array_equal(b4, b6[2:])
    assert stats_tuple(st4) == stats_tuple(st6)
    assert np.array_equal(A0, A6) and np.array_equal(b0, b6) and stats_tuple(st0) == stats_tuple(st6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("knn,nbr", SHAPES)
def test_2d_sums_against_restatement(dtype, chain, knn, nbr):
    ctx, rd, ref, nrm = matched(dtype, knn, nbr, chain)
    try:
        A6, b6, st6 = ctx.p2plane_system()
        A, b, st = ctx.p2plane_system_forced("2D")
        d, ids = ctx.get_matches()
        w = ctx.get_weights()
    finally:
        ctx.close()
    if chain == "robust":
        assert ((w != 0) & (w != 1)).any()  # (real weights: the FULL form)
    else:
        assert 0 < (w == 0).sum() < w.size
    wA, wb, kept = fc.forced_system(rd, ref, nrm, ids, d, w, "2D")  # (T_iter = I: the step reading is the reading)
    print(f"{np.dtype(dtype).name} {chain} k={knn} nbr={nbr}: kept {st.kept} max|dA| {np.abs(A - wA).max():.3g} "
          f"max|db| {np.abs(b - wb).max():.3g} (|A| {np.abs(wA).max():.3g} |b| {np.abs(wb).max():.3g})")
    assert st.kept == kept and stats_tuple(st) == stats_tuple(st6)
    np.testing.assert_allclose(A, wA, rtol=1e-12, atol=1e-12 * np.abs(wA).max())
    np.testing.assert_allclose(b, wb, rtol=1e-12, atol=1e-12 * np.abs(wb).max())
    # A's yaw / x / y block is the 6-DOF one's: the same products summed by the other form
    np.testing.assert_allclose(A, A6[2:5, 2:5], rtol=1e-12, atol=1e-12 * np.abs(A6).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_2d_b_is_not_the_6dof_block(dtype):
    """The mistake this mode invites.  With axis-aligned normals (the scene
    above) every pair has n_z = 0 or n_x = n_y = 0 and the z term of dot never
    meets a non-zero F; on a floor with tilted normals (step_cases.tilted_floor)
    d_z n_z != 0 multiplies n_x, n_y != 0, and b must come from the 2-D dot."""
    cloud = sc.tilted_floor(0.3, dtype)
    ctx, rd, ref, nrm = matched(dtype, 1, 1, "trim", cloud=cloud)
    try:
        A6, b6, st6 = ctx.p2plane_system()
        A, b, st = ctx.p2plane_system_forced("2D")
        d, ids = ctx.get_matches()
        w = ctx.get_weights()
    finally:
        ctx.close()
    wA, wb, kept = fc.forced_system(rd, ref, nrm, ids, d, w, "2D")
    w6A, w6b, _ = fc.forced_system(rd, ref, nrm, ids, d, w, None)
    assert st.kept == kept and 6 < kept < len(rd)
    np.testing.assert_allclose(A, wA, rtol=1e-12, atol=1e-12 * np.abs(wA).max())
    np.testing.assert_allclose(b, wb, rtol=1e-12, atol=1e-12 * np.abs(wb).max())
    np.testing.assert_allclose(b6, w6b, rtol=1e-12, atol=1e-12 * np.abs(w6b).max())
    gap = np.abs(b - b6[2:5]).max()
    print(f"{np.dtype(dtype).name}: b {b} 6-DOF block {b6[2:5]} gap {gap:.3g}")
    assert gap > 0.1 * np.abs(b6[2:5]).max()


# ------------------------------------------------------------------ 3: step --
def host_step(monkeypatch, dtype, rd, ref, nrm, force):
    """The first T_iter of the module path and of the device loop (Counter 1,
    the empty chain) through the host chain, identity T_init."""
    from libpointmatcher_amd.icp import ICP
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
        icp = ICP(dtype)
        icp.load_yaml(chain_yaml(filters=(), minimizer=MINIMIZER[force], maxit=1))
        try:
            out[mode] = icp.compute(rd, ref, nrm)
            assert icp.stats().iterations == 1
        finally:
            icp.close()
    return out


STEP_CASES = [("4DOF", "floor+walls", []), ("2D", "floor+walls", []), ("4DOF", "floor", [0, 1, 2]), ("2D", "wall", [2])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("force,parts,zero", STEP_CASES)
def test_step_full_rank_and_rank_deficient(monkeypatch, dtype, force, parts, zero):
    dn = np.dtype(dtype).name
    ctx, rd, ref, nrm = matched(dtype, 1, 1, "none", parts)
    try:
        d, ids = ctx.get_matches()
        assert np.array_equal(ids[:, 0], np.arange(len(rd)))  # precondition: the match is the identity
        A, b, st = ctx.p2plane_system_forced(force)
        assert st.kept == len(rd)
        # the device loop's step on the same context (pmx_loop_cfg.force)
        ctx.loop_begin(knn=1, minimizer=P2PL, checkers=[("CounterTransformationChecker", 1)], force=force)
        ls = ctx.loop_run(1)
        assert ls.iterations == 1 and ls.done
        T_ctx = ctx.loop_T(ls)
    finally:
        ctx.close()
    At, bt, x_exact, live = sc.check_structure(A, b, zero, dtype)  # before looking at any step
    assert len(live) == fc.NF[force] - len(zero)
    # the host step's solver (pm_icp.cpp: dense::solve_underdetermined on these sums) and the device loop's step,
    # each against the exact solution; the loop's transform against the exact one and the kit's x
    x_kit = dense_kit().solve_underdetermined(At, bt, dtype).astype(np.float64)
    x_dev = fc.step_vector(T_ctx, force)
    r_kit = sc.solve_ratio(x_kit, x_exact, At, live, dtype)
    r_dev = sc.solve_ratio(x_dev, x_exact, At, live, dtype)
    g_kit = np.linalg.norm(x_dev - x_kit)
    g_x = np.linalg.norm(T_ctx.astype(np.float64) - fc.transform64(x_exact, force))
    print(f"{force} {parts} {dn}: cond2 {sc.cond2(At, live):.3g} |x| {np.linalg.norm(x_exact):.3g} ratio loop {r_dev:.3g} "
          f"host kit {r_kit:.3g} |x - kit| {g_kit:.3g} |T - exact| {g_x:.3g} "
          f"null {np.abs(x_dev[zero]).max() if zero else 0:.3g}")
    assert r_dev <= sc.K_SOLVE and r_kit <= sc.K_SOLVE
    assert g_kit <= sc.BAR[dn] and g_x <= sc.BAR[dn]
    assert structure_ok(T_ctx, force)
    # the host chain's step (it centres the reference on its mean, so its sums are not the context's): the module
    # path's forced transform and the device loop's agree, and keep the structure
    steps = host_step(monkeypatch, dtype, rd, ref, nrm, force)
    g = np.linalg.norm(steps["0"].astype(np.float64) - steps["1"].astype(np.float64))
    print(f"   host chain: |modules - loop| {g:.3g}")
    assert g <= sc.BAR[dn] and structure_ok(steps["0"], force) and structure_ok(steps["1"], force)
    assert np.linalg.norm(fc.step_vector(steps["0"], force)) > 1e-4


# ------------------------------------------------ 4, 5: structure, whole ICP --
def structure_ok(T, force):
    ok = T[2, 0] == 0 and T[2, 1] == 0 and T[0, 2] == 0 and T[1, 2] == 0 and T[2, 2] == 1
    ok = ok and np.array_equal(T[3], np.array([0, 0, 0, 1], T.dtype))
    return bool(ok and (force != "2D" or T[2, 3] == 0))


def whole_icp(dtype, force, mode, monkeypatch, filters=TRIM, knn=1):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
    rd, ref, nrm = fc.scene(dtype)
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(knn=knn, filters=filters, minimizer=MINIMIZER[force], maxit=ITERS))
    try:
        T = icp.compute(rd, ref, nrm)
        return T, icp.stats().iterations
    finally:
        icp.close()


@pytest.fixture(scope="module")
def restated():
    """force_cases.icp on the scene, once per (dtype, force)."""
    out = {}

    def get(dtype, force):
        key = (np.dtype(dtype).name, force)
        if key not in out:
            rd, ref, nrm = fc.scene(dtype)
            out[key] = fc.icp(rd, ref, nrm, force, ITERS)
        return out[key]

    return get


@pytest.mark.parametrize("dtype", DTYPES)
def test_unforced_chain_violates_the_structure(monkeypatch, dtype):
    """The scene's motion has roll, pitch and z: the unforced chain recovers them."""
    T, it = whole_icp(dtype, None, "1", monkeypatch)
    assert it == ITERS and not structure_ok(T, "4DOF")
    assert abs(T[2, 0]) > 1e-4 and abs(T[2, 1]) > 1e-4 and abs(T[2, 3]) > 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("force", fc.FORCES)
def test_whole_icp(monkeypatch, restated, dtype, force):
    dn = np.dtype(dtype).name
    want = restated(dtype, force)
    got = {}
    for mode in ("0", "1"):
        T, it = whole_icp(dtype, force, mode, monkeypatch)
        assert it == ITERS
        assert structure_ok(T, force), (mode, T)
        err = np.linalg.norm(T.astype(np.float64) - want)
        print(f"{force} {dn} PMX_DEVICE_LOOP={mode}: |T - T_restated| {err:.3g} (bound {2 * UNFORCED[dn][mode]:.3g})")
        got[mode] = (T, err)
    # the forced step moved (yaw and translation of the motion's size), so this is not the equality of identities
    x = fc.step_vector(got["1"][0], force)
    assert abs(x[0]) > 5e-4 and np.linalg.norm(x[1:]) > 5e-4
    assert np.linalg.norm(got["0"][0].astype(np.float64) - got["1"][0].astype(np.float64)) <= sc.BAR[dn]
    for mode in ("0", "1"):
        assert got[mode][1] <= 2 * UNFORCED[dn][mode], mode


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("force", fc.FORCES)
@pytest.mark.parametrize("tag,filters,knn", [
    ("robust", (("RobustOutlierFilter", {"robustFct": "cauchy", "scaleEstimator": "mad", "tuning": 1.0}),), 1),
    ("trim k=3", TRIM, 3)])
def test_loop_and_modules_agree_on_other_chains(monkeypatch, dtype, force, tag, filters, knn):
    """The FULL form (a robust chain) and the gathered k range through both paths."""
    dn = np.dtype(dtype).name
    (Tm, im), (Tl, il) = [whole_icp(dtype, force, m, monkeypatch, filters, knn) for m in ("0", "1")]
    err = np.linalg.norm(Tm.astype(np.float64) - Tl.astype(np.float64))
    print(f"{force} {dn} {tag}: |modules - loop| {err:.3g}")
    assert im == il == ITERS and structure_ok(Tm, force) and structure_ok(Tl, force)
    assert err <= sc.BAR[dn]


# --------------------------------------------------------------- 6: errors --
@pytest.mark.parametrize("dtype", DTYPES)
def test_4dof_on_a_2d_context_is_refused(dtype):
    from libpointmatcher_amd import _capi
    ctx, rd, ref, nrm = matched(dtype, 1, 1, "trim", cloud=fc.scene2d(dtype))
    try:
        with pytest.raises(_capi.InvalidParameter):
            ctx.p2plane_system_forced("4DOF")
        with pytest.raises(_capi.InvalidParameter):
            ctx.loop_begin(knn=1, minimizer=P2PL, checkers=[("CounterTransformationChecker", 1)], force="4DOF")
        # force2D on a 2-D cloud changes nothing
        A, b, st = ctx.p2plane_system()
        A2, b2, st2 = ctx.p2plane_system_forced("2D")
        assert A.shape == (3, 3) and b.any()
        assert np.array_equal(A, A2) and np.array_equal(b, b2) and stats_tuple(st) == stats_tuple(st2)
    finally:
        ctx.close()


def test_force_with_the_covariance_is_refused():
    from libpointmatcher_amd import _capi
    ctx, rd, ref, nrm = matched(np.float32, 1, 1, "trim")
    try:
        for force in fc.FORCES:
            with pytest.raises(_capi.InvalidParameter):
                ctx.loop_begin(knn=1, minimizer="PointToPlaneWithCovErrorMinimizer",
                               checkers=[("CounterTransformationChecker", 1)], force=force)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["0", "1"])
def test_force2d_on_a_2d_cloud_equals_unforced(monkeypatch, dtype, mode):
    from libpointmatcher_amd.icp import ICP, ConfigurationError
    monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
    rd, ref, nrm = fc.scene2d(dtype)
    out = []
    for force in (None, "2D"):
        icp = ICP(dtype)
        icp.load_yaml(chain_yaml(filters=TRIM, minimizer=MINIMIZER[force], maxit=4))
        try:
            out.append(icp.compute(rd, ref, nrm))
            assert icp.stats().iterations == 4
        finally:
            icp.close()
    assert np.array_equal(out[0], out[1]) and not np.array_equal(out[0], np.eye(3, dtype=dtype))
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(filters=TRIM, minimizer=MINIMIZER["4DOF"], maxit=4))
    try:
        with pytest.raises(ConfigurationError, match="force4DOF"):
            icp.compute(rd, ref, nrm)
    finally:
        icp.close()


# ------------------------------- 8: the reference's regression configurations --
_libc = ctypes.CDLL(None)


def run_config(golden, name):
    from libpointmatcher_amd.icp import ICP
    g, kat = golden
    icp = ICP(np.float32)
    icp.load_yaml(kat["icp_data_configs"][name])
    _libc.srand(1)
    try:
        T = icp.compute(hom(g["vtk1"], np.float32), hom(g["vtk0"], np.float32), None)
        it = icp.stats().iterations
    finally:
        icp.close()
    err = rel_displacement(T, np.array(kat["icp_data_ref_trans"][name]), g["vtk1"])
    print(f"{name}: rel err {err:.4f}, iterations {it}")
    return T, err, kat["icp_data_rel_tol"]


@pytest.mark.parametrize("mode", ["0", "1"])
def test_reference_4dof_config_unchanged(monkeypatch, golden, mode):
    """utest.cpp:81-160 with force4DOFForPointToPlaneMinimizer.yaml as it is."""
    monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
    T, err, tol = run_config(golden, "force4DOFForPointToPlaneMinimizer")
    assert structure_ok(T, "4DOF"), T
    assert not np.array_equal(T, np.eye(4, dtype=np.float32))
    assert tol == 0.03 and err < tol


@pytest.mark.parametrize("name", ["defaultObservationDirectionDataPointsFilter",
                                  "defaultOrientNormalsDataPointsFilter"])
def test_reference_filter_configs_unchanged(golden, name):
    T, err, tol = run_config(golden, name)
    assert err < tol

"""GenericDescriptorOutlierFilter chains through the whole ICP: the device
loop and the per-module path against a Python loop over the oracle functions
(oracle.knn, outlier_chain, p2plane_system / p2plane_solve, p2point) fed the
filter's weights restated in numpy (test_gpu_generic_descriptor.restate).

The oracle loop is ICP::compute's (ICP.cpp:291-312, 371-441) as oracle/pmo_impl.inc
restates it: the reference centred on its mean (sequential sums in T), the
reading moved into that frame, T_iter = dT T_iter in T with one rounding per
product and sum, the result T_ref T_iter T_refinv.  It shares nothing with the
library but the match and the minimisers' oracles, so a divisor or a
descriptor order wrong in both GPU paths alike does not pass.
Bar: 8 iterations, both GPU paths within 1e-5 (f32) / 1e-12 (f64) of the
oracle loop (README, Parity) and of each other.
"""
import numpy as np
import pytest

from helpers import chain_yaml
from libpointmatcher_amd.icp import ICP
from libpointmatcher_amd.synth import reading_cloud, reference_cloud
from test_gpu_generic_descriptor import THR, descriptor, restate

pytestmark = pytest.mark.gpu

N, M = 3000, 4000
ITERS = 8
TOL = {np.float32: 1e-5, np.float64: 1e-12}
TRIM = ("TrimmedDistOutlierFilter", {"ratio": 0.8})
NAME = "GenericDescriptorOutlierFilter"


def mm(A, B):
    """A B in T, every product and sum rounded once, the inner sums sequential"""
    n = A.shape[0]
    C = np.zeros((n, n), A.dtype)
    for r in range(n):
        for c in range(n):
            s = A[r, 0] * B[0, c]
            for k in range(1, n):
                s = s + A[r, k] * B[k, c]
            C[r, c] = s
    return C


def oracle_loop(oracle, rd, ref, nrm, desc, mode, minimizer, iters, k=1):
    dt = rd.dtype
    rows = rd.shape[1]
    D = rows - 1
    mean = np.array([np.cumsum(ref[:, r], dtype=dt)[-1] / dt.type(len(ref)) for r in range(D)], dt)
    Tm, Tmi = np.eye(rows, dtype=dt), np.eye(rows, dtype=dt)
    Tm[:D, D] = mean
    Tmi[:D, D] = -mean
    refc = ref.copy()
    refc[:, :D] = ref[:, :D] - mean
    rd0 = oracle.transform(Tmi, rd)
    T = np.eye(rows, dtype=dt)
    kept = 0
    for _ in range(iters):
        step = oracle.transform(T, rd0)
        d, ids, _ = oracle.knn(refc, step, k=k)
        rc, wt = oracle.outlier_chain([TRIM], d)
        assert rc == 0
        w = wt * restate(desc, ids, mode)
        if minimizer.startswith("PointToPlane"):
            rc, A, b, st = oracle.p2plane_system(step, refc, nrm, d, ids, w)
            assert rc == 0
            rc, dT = oracle.p2plane_solve(A, b, rows, dt)
        else:
            rc, dT, st = oracle.p2point(step, refc, d, ids, w)
        assert rc == 0
        kept = st.kept
        T = mm(dT, T)
    return mm(mm(Tm, T), Tmi), kept


def gpu_icp(monkeypatch, mode, text, rd, ref, nrm, desc, levels=None):
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if mode == "loop" else "0")
    icp = ICP(rd.dtype)
    icp.load_yaml(text)
    icp.add_descriptor("reference", "quality", desc)
    T = icp.compute(rd, ref, nrm)
    st = icp.stats()
    if levels is not None:  # the grid level of every iteration's match (device loop)
        levels.extend(icp.loop_diag(0, st.iterations)[:, 0].tolist())
    icp.close()
    return T, st


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("minimizer", ["PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer"])
@pytest.mark.parametrize("mode", ["gt", "lt", "soft"])
def test_both_paths_equal_the_oracle_loop(monkeypatch, oracle, dtype, minimizer, mode):
    ref, nrm = reference_cloud(M, dtype)
    rd = reading_cloud(N, dtype)
    desc = descriptor(dtype)
    p = {"descName": "quality", "threshold": THR, "useSoftThreshold": int(mode == "soft"),
         "useLargerThan": int(mode != "lt")}
    text = chain_yaml(filters=(TRIM, (NAME, p)), minimizer=minimizer, maxit=ITERS)
    To, kept = oracle_loop(oracle, rd, ref, nrm, desc, mode, minimizer, ITERS)
    Tl, sl = gpu_icp(monkeypatch, "loop", text, rd, ref, nrm, desc)
    Tm, sm = gpu_icp(monkeypatch, "modules", text, rd, ref, nrm, desc)
    el, em = np.linalg.norm(Tl.astype(np.float64) - To), np.linalg.norm(Tm.astype(np.float64) - To)
    print(f"{np.dtype(dtype).name} {minimizer} {mode}: |Tloop - To| {el:.3g} |Tmodules - To| {em:.3g} kept {kept}")
    assert sl.iterations == sm.iterations == ITERS
    assert sl.kept == sm.kept == kept
    assert el <= TOL[dtype] and em <= TOL[dtype]
    assert np.linalg.norm(Tl - Tm) <= TOL[dtype]


def test_loop_2d_point_to_point(monkeypatch, oracle):
    """a 2-D cloud (rows = 3) through the device loop, hard and soft"""
    dtype = np.float32
    ref3, _ = reference_cloud(M, dtype)
    ref = np.ascontiguousarray(ref3[:, [0, 1, 3]])
    rd = np.ascontiguousarray(reading_cloud(N, dtype)[:, [0, 1, 3]])
    desc = descriptor(dtype)
    for mode in ("gt", "soft"):
        p = {"descName": "quality", "threshold": THR, "useSoftThreshold": int(mode == "soft")}
        text = chain_yaml(filters=(TRIM, (NAME, p)), minimizer="PointToPointErrorMinimizer", maxit=ITERS)
        To, kept = oracle_loop(oracle, rd, ref, None, desc, mode, "PointToPointErrorMinimizer", ITERS)
        Tl, sl = gpu_icp(monkeypatch, "loop", text, rd, ref, None, desc)
        Tm, sm = gpu_icp(monkeypatch, "modules", text, rd, ref, None, desc)
        print(f"2-D {mode}: |Tloop - To| {np.linalg.norm(Tl - To):.3g} |Tmodules - To| {np.linalg.norm(Tm - To):.3g}")
        assert sl.kept == sm.kept == kept
        assert np.linalg.norm(Tl - To) <= TOL[dtype] and np.linalg.norm(Tm - To) <= TOL[dtype]


@pytest.mark.parametrize("mode", ["gt", "soft"])
def test_level_change_inside_the_loop(monkeypatch, oracle, mode):
    """Two grid levels of 0.25 and 8 points per cell, only the fine one built with
    the reference (first_ppc=0.25), k = 10 and a reading that starts 2 away: a
    fine-level search evaluates about 18 pairs per query, over 32 cells' worth,
    so the loop asks for the coarse level.  That level is built on demand, after
    the descriptor's upload, and gets its copy on the stream that builds it; the
    loop's later matches run on it and read that copy (grid_reuse=0: every query
    searches, so the level is judged at every iteration).  Asserted from the
    loop's diagnostics: it starts on level 0 and both levels ran."""
    dtype = np.float32
    k, iters = 10, 16
    monkeypatch.setenv("PMX_OPTS", "grid_levels=0.25:8,first_ppc=0.25,grid_reuse=0")
    ref, nrm = reference_cloud(M, dtype)
    rd = reading_cloud(N, dtype)
    rd[:, 0] += dtype(2.0)
    desc = descriptor(dtype)
    p = {"descName": "quality", "threshold": THR, "useSoftThreshold": int(mode == "soft")}
    text = chain_yaml(knn=k, filters=(TRIM, (NAME, p)), maxit=iters)
    levels = []
    Tl, sl = gpu_icp(monkeypatch, "loop", text, rd, ref, nrm, desc, levels)
    Tm, sm = gpu_icp(monkeypatch, "modules", text, rd, ref, nrm, desc)
    To, kept = oracle_loop(oracle, rd, ref, nrm, desc, mode, "PointToPlaneErrorMinimizer", iters, k=k)
    print(f"{mode}: levels {levels} |Tloop - To| {np.linalg.norm(Tl - To):.3g} |Tmodules - To| "
          f"{np.linalg.norm(Tm - To):.3g} kept {kept}")
    assert levels[0] == 0 and set(levels) == {0, 1}
    assert sl.iterations == sm.iterations == iters and sl.kept == sm.kept == kept
    assert np.linalg.norm(Tl - To) <= TOL[dtype] and np.linalg.norm(Tm - To) <= TOL[dtype]

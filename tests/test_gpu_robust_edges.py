"""RobustOutlierFilter on the GPU at its branch and scale edges: the device
(robust_weight / entry_weight of pmx_weight.h, the scale estimators of
pmx_robust.hip, the weighted reductions) held to the cases, the independent
numpy reference and the bars of tests/robust_cases.py.  Nothing here depends
on the oracle; tests/test_robust_reference.py holds the oracle to the same
cases on a CPU.

Each case first asserts that the match returns the intended distances bit for
bit and the intended ids, with both search types; then, per call of the
filter's schedule: the scale, the weights (zero / NaN / inf patterns equal
everywhere, exact values bit-equal, see robust_cases.check_call), the
ErrorElements counts and sum_w of the three minimisers' systems before and
after get_weights() against the counts of the reference weights, and, where
every kept weight is finite, the point-to-plane normal equations against an
fp64 accumulation in numpy.

sum_w: the device's and fsum's are fp64 sums of N k values of T, within
N k 2^-52 fsum of each other (tests/test_gpu_weight_forms.py), widened by the
weights' own rtol since the reference's weights are summed here, not the
device's.
"""
import math

import numpy as np
import pytest

import robust_cases as rc
from helpers import chain_yaml
from libpointmatcher_amd import _capi as P
from libpointmatcher_amd.icp import ICP

pytestmark = pytest.mark.gpu

CASES = rc.case_ids()
IDS = [f"{n}-{np.dtype(t).name}" for _, n, t in CASES]
FIELDS = ("nonzero_weights", "kept", "rejected_matches", "rejected_points")


def systems(ctx):
    """(name, Stats, (A, b) or None) of the three systems; Stats None where the
    minimiser reports no point to minimise"""
    out = []
    for name, f in (("p2plane", ctx.p2plane_system), ("p2point", ctx.p2point_system),
                    ("similarity", ctx.p2point_similarity_system)):
        try:
            r = f()
            out.append((name, r[-1], r[:2] if name == "p2plane" else None))
        except P.ConvergenceError as e:
            assert "no point to minimize" in str(e)
            out.append((name, None, None))
    return out


def p2plane_numpy(sc, w, kept):
    """PointToPlane's A, b (PointToPlane.cpp:171-243) for the kept entries: each
    term in T as the reference forms it, the sums in fp64"""
    i, s = np.nonzero(kept)
    p, j = sc.rd[i, :3], sc.ids[i, s]
    q, n, wv = sc.ref[j, :3], sc.nrm[j], w[i, s]
    F = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
    dl = p - q
    dot = (dl[:, 0] * n[:, 0] + dl[:, 1] * n[:, 1]) + dl[:, 2] * n[:, 2]
    wF = wv[:, None] * F
    assert wF.dtype == w.dtype and dot.dtype == w.dtype
    A = (wF[:, :, None] * F[:, None, :]).astype(np.float64).sum(0)
    b = -(wF * dot[:, None]).astype(np.float64).sum(0)
    return A, b


def check_systems(case, sc, x, w, stats, when):
    want, kept = rc.want_counts(sc.d, x.w)
    T = x.w.dtype.type
    with np.errstate(all="ignore"):
        fsum_ref = x.w[kept].astype(np.float64)
        fsum = math.fsum(fsum_ref) if np.isfinite(fsum_ref).all() else float(np.sum(fsum_ref))
    bound = (sc.d.size * 2.0 ** -52 + rc.TOL[T]) * abs(fsum)
    for name, st, Ab in stats:
        if want["kept"] == 0 or want["nonzero_weights"] == 0:
            assert st is None, (when, name)
            continue
        assert st is not None, (when, name)
        got = {f: getattr(st, f) for f in FIELDS}
        print(f"    {when}, {name}: {got}, sum_w {st.sum_w!r} (reference {fsum!r})")
        assert got == want, (when, name, got, want)
        if np.isfinite(fsum):
            assert abs(st.sum_w - fsum) <= bound, (when, name, st.sum_w, fsum, bound)
        else:
            assert np.isnan(st.sum_w) == np.isnan(fsum) and np.isinf(st.sum_w) == np.isinf(fsum), (when, name)
            if np.isinf(fsum):
                assert st.sum_w == fsum
        if Ab is not None and np.isfinite(fsum):
            A, b = p2plane_numpy(sc, w, kept)
            np.testing.assert_allclose(Ab[0], A, rtol=1e-9, atol=1e-9 * np.abs(A).max())
            np.testing.assert_allclose(Ab[1], b, rtol=1e-9, atol=1e-9 * np.abs(b).max())


@pytest.mark.parametrize("group,name,dtype", CASES, ids=IDS)
def test_device_on_edge_case(group, name, dtype):
    case = rc.get_case(group, name, dtype)
    tuning, target = rc.device_tuning(case)
    for k in case.ks:
        sc = rc.scene(case, dtype, k)
        exp = rc.expected(case, dtype, k)
        if exp is not None:
            print(f"{name} {np.dtype(dtype).name} k={k}: bands {rc.check_bands(case, exp)}")
        for search in (0, 1):
            ctx = P.Context(0, dtype)
            try:
                ctx.set_search(search)
                ctx.set_reference(sc.ref, sc.nrm)
                ctx.set_reading(sc.rd)
                ctx.match(np.eye(4, dtype=dtype), knn=k, max_dist=sc.max_dist)
                d, ids = ctx.get_matches()
                # the scene holds what the case is about: the intended match, bit for bit
                assert d.tobytes() == sc.d.tobytes() and np.array_equal(ids, sc.ids), (name, k, search)
                if case.raises:
                    assert exp is None
                    with pytest.raises(P.ConvergenceError, match="no outlier to filter"):
                        ctx.outlier_robust(0, case.fct, tuning, case.approx, rc.scale_mode(P, 1, case.scale, case.nb),
                                           target, point2plane=case.p2pl)
                        ctx.p2plane_system()
                    continue
                for call, x in enumerate(exp, 1):
                    ctx.outlier_robust(0, case.fct, tuning, case.approx, rc.scale_mode(P, call, case.scale, case.nb),
                                       target, point2plane=case.p2pl)
                    before = systems(ctx)
                    w = ctx.get_weights()
                    scale = ctx.robust_scale(0)
                    after = systems(ctx)
                    print(f"  search {search} call {call}: scale {scale!r}, {rc.band_counts(x)}")
                    rc.check_call(case, x, scale, w, f"device search {search} k {k} call {call}")
                    check_systems(case, sc, x, w, before, "before get_weights")
                    check_systems(case, sc, x, w, after, "after get_weights")
            finally:
                ctx.close()


LOOP = [(g, n, t) for g, n, t in CASES if g in ("thresholds", "median_ties") or (g == "underflow" and "welsch" in n)]


@pytest.mark.parametrize("group,name,dtype", LOOP, ids=[f"{n}-{np.dtype(t).name}" for _, n, t in LOOP])
def test_device_loop_equals_modules_on_edge_case(monkeypatch, group, name, dtype):
    """The same scene through ICP with the robust chain, two iterations: the
    device loop against the per-module calls, the bar of
    test_gpu_robust.py::test_robust_device_loop_equals_modules (same iterations,
    same kept, T within 1e-5 / 1e-12).  Of `underflow` the Welsch scenes run:
    every weight there is finite."""
    case = rc.get_case(group, name, dtype)
    sc = rc.scene(case, dtype, 1)
    yaml = chain_yaml(knn=1, filters=(("RobustOutlierFilter", case.params()),),
                      minimizer="PointToPointErrorMinimizer", maxit=2)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
        icp = ICP(dtype)
        try:
            icp.load_yaml(yaml)
            T = icp.compute(sc.rd, sc.ref, None)
            s = icp.stats()
            out[mode] = (T.astype(np.float64), s.iterations, s.kept)
        except P.ConvergenceError as e:   # (every weight 0: both paths must say so)
            out[mode] = (None, str(e), None)
        finally:
            icp.close()
    (Tl, il, kl), (Tm, im, km) = out["1"], out["0"]
    print(f"{name} {np.dtype(dtype).name}: loop {il} kept {kl}, modules {im} kept {km}")
    assert (Tl is None) == (Tm is None)
    assert il == im and kl == km
    if Tl is not None:
        assert il == 2
        df = np.linalg.norm(Tl - Tm)
        print(f"  |dT| {df:.3g}")
        assert df <= (1e-5 if dtype == np.float32 else 1e-12)

"""PointToPlaneWithCovErrorMinimizer on the GPU: the covariance sums H and Q
(pmx_p2plane_covariance, pmx_loop_covariance) and ICP.covariance().

The yardstick is `restate` below: ErrorMinimizers/PointToPlaneWithCov.cpp:94-161
restated in numpy, the per-pair terms in the ICP's dtype in the reference's
order, the sums in float64, fed with the matches and weights read back
through pmx_get_matches / pmx_get_weights and the transforms of the trace.

Fixture: a box corner (three mutually orthogonal unit squares, exact axis
normals), the reading its points plus 0.01 noise under a small pose offset;
65 and 130 reading points (one wave plus a tail; past one block's first
round).  cond(H) of it is about 10; the tests assert <= 100.

Bars: H and Q relative to their Frobenius norm 1e-5 (f32) / 1e-12 (f64), the
project's parity bars; the covariance sigma^2 H^-1 Q H^-1 within
(2 cond(H) + 1) * bar, the first-order bound of a product with two inverses.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from helpers import chain_yaml  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {"float32": 1e-5, "float64": 1e-12}
COV, PLAIN = "PointToPlaneWithCovErrorMinimizer", "PointToPlaneErrorMinimizer"
DTYPES = [np.float32, np.float64]


# ------------------------------------------------------------------ fixture --
def box_corner(n_side=20):
    """Three unit squares on the planes x = 0, y = 0, z = 0: points and normals."""
    g = (np.arange(n_side) + 0.5) / n_side
    a, b = [v.ravel() for v in np.meshgrid(g, g, indexing="ij")]
    z = np.zeros_like(a)
    pts = np.concatenate([np.stack([z, a, b], 1), np.stack([a, z, b], 1), np.stack([a, b, z], 1)])
    nrm = np.concatenate([np.tile(e, (a.size, 1)) for e in np.eye(3)])
    return pts, nrm


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rigid(rx, ry, rz, t):
    T = np.eye(4)
    T[:3, :3] = rot(rx, ry, rz)
    T[:3, 3] = t
    return T


def clouds(n_rd, dtype, seed=3, centre=True):
    """(reading n_rd x 4, reference M x 4, normals M x 3): the reference centred
    on its mean when `centre` (what a context is given), the reading the box's
    points plus noise under the inverse of a small pose about that centre."""
    rng = np.random.default_rng(seed + n_rd)
    ref, nrm = box_corner()
    faces = rng.integers(0, 3, n_rd)
    uv = rng.uniform(0.05, 0.95, (n_rd, 2))
    rd = np.zeros((n_rd, 3))
    for f in range(3):
        m = faces == f
        rd[np.ix_(m, [c for c in range(3) if c != f])] = uv[m]
    rd += rng.normal(0, 0.01, rd.shape)
    off = ref.mean(0)
    ref = ref - off
    rd = rd - off
    pose = rigid(0.02, -0.015, 0.025, [0.01, -0.008, 0.012])
    rd = (np.linalg.inv(pose) @ np.c_[rd, np.ones(n_rd)].T).T[:, :3]
    if not centre:  # (the same geometry away from the origin: what an ICP is given)
        ref = ref + off
        rd = rd + off
    hom = lambda p: np.ascontiguousarray(np.c_[p, np.ones(len(p))], dtype=dtype)  # noqa: E731
    return hom(rd), hom(ref), np.ascontiguousarray(nrm, dtype=dtype)


# -------------------------------------------------------------- restatement --
def xform3(T, p):
    """The device's transform of the reading (pmx_p2plane.h xform3), in T's dtype."""
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] * p[:, 3]
                     for r in range(3)], 1)


def restate(p, q, n, T_step, dtype):
    """estimateCovariance's sums over the ErrorElements columns (p, q, n: K x 3
    in dtype): H, Q in float64 and the six parameters."""
    t = np.dtype(dtype).type
    Ts = np.asarray(T_step, dtype)
    beta = -np.arcsin(Ts[2, 0])
    alpha = np.arctan2(Ts[2, 1], Ts[2, 2])
    gamma = np.arctan2(Ts[1, 0] / np.cos(beta), Ts[0, 0] / np.cos(beta))
    tx, ty, tz = Ts[0, 3], Ts[1, 3], Ts[2, 3]
    assert all(type(v) is t for v in (alpha, beta, gamma, tx))
    p0, p1, p2 = p.T
    q0, q1, q2 = q.T
    n0, n1, n2 = n.T
    rp = np.sqrt((p0 * p0 + p1 * p1) + p2 * p2)
    d0, d1, d2 = p0 / rp, p1 / rp, p2 / rp
    rq = np.sqrt((q0 * q0 + q1 * q1) + q2 * q2)
    e0, e1, e2 = q0 / rq, q1 / rq, q2 / rq
    na = n2 * d1 - n1 * d2
    nb = n0 * d2 - n2 * d0
    ng = n1 * d0 - n0 * d1
    E = n0 * ((((p0 - gamma * p1) + beta * p2) + tx) - q0)
    E = E + n1 * ((((gamma * p0 + p1) - alpha * p2) + ty) - q1)
    E = E + n2 * (((((-beta) * p0 + alpha * p1) + p2) + tz) - q2)
    Nr = n0 * ((d0 - gamma * d1) + beta * d2)
    Nr = Nr + n1 * ((gamma * d0 + d1) - alpha * d2)
    Nr = Nr + n2 * (((-beta) * d0 + alpha * d1) + d2)
    Nf = -((n0 * e0 + n1 * e1) + n2 * e2)
    er = E + rp * Nr
    a = np.stack([n0, n1, n2, rp * na, rp * nb, rp * ng], 1)
    u = np.stack([n0 * Nr, n1 * Nr, n2 * Nr, na * er, nb * er, ng * er], 1)
    v = np.stack([n0 * Nf, n1 * Nf, n2 * Nf, (rq * na) * Nf, (rq * nb) * Nf, (rq * ng) * Nf], 1)
    for x in (a, u, v):
        assert x.dtype == np.dtype(dtype)
    outer = lambda x: (x[:, :, None] * x[:, None, :]).astype(np.float64).sum(0)  # noqa: E731
    return outer(a), outer(u) + outer(v)


def restate_match(ctx, rd0, ref, nrm, T_at, T_step, dtype):
    """H, Q, pairs of the restatement for the context's current match and chain:
    rd0 the reading as the context holds it, T_at the transform the match ran at."""
    d, ids = ctx.get_matches()
    w = ctx.get_weights()
    kept = (d != np.inf) & (w != 0)
    qi, s = np.nonzero(kept)
    p = xform3(np.asarray(T_at, dtype), rd0)[qi]
    H, Q = restate(p, ref[ids[qi, s], :3], nrm[ids[qi, s]], T_step, dtype)
    return H, Q, int(kept.sum())


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


T_AT = rigid(0.004, -0.003, 0.005, [0.002, -0.001, 0.003])     # the match's transform
T_STEP = rigid(0.011, -0.017, 0.023, [0.004, -0.006, 0.005])   # alpha, beta, gamma all non-zero

CHAINS = {
    "trim": dict(filters=[("TrimmedDistOutlierFilter", dict(ratio=0.85))]),
    "maxdist": dict(max_dist=0.03, filters=[("MaxDistOutlierFilter", dict(maxDist=0.025))]),
    "trim_sn": dict(filters=[("TrimmedDistOutlierFilter", dict(ratio=0.85))], sn=0.3),
    "robust": dict(robust=True),
}


def run_chain(ctx, chain, knn, dtype, rd):
    c = CHAINS[chain]
    ctx.match(np.asarray(T_AT, dtype), knn=knn, max_dist=c.get("max_dist", np.inf))
    pos = 0
    for name, p in c.get("filters", []):
        ctx.outlier(name, pos, **p)
        pos += 1
    if "sn" in c:
        ctx.outlier_surface_normal(pos, max_angle=c["sn"])
    if c.get("robust"):
        from libpointmatcher_amd import _capi
        ctx.outlier_robust(0, "cauchy", 0.5, 1.5, _capi.RS_MAD, 0.0)  # (the approximation zeroes the far pairs)


def reading_normals(rd, ref, nrm):
    """The nearest reference normal, tilted for a third of the points so that
    the SurfaceNormal filter rejects some pairs."""
    d2 = ((rd[:, None, :3].astype(np.float64) - ref[None, :, :3]) ** 2).sum(2)
    out = nrm[d2.argmin(1)].astype(np.float64)
    out[::3] = out[::3] @ rot(0.0, 0.6, 0.5).T
    return out


# ------------------------------------------------------------ module path --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rd", [65, 130])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_module_path_matches_restatement(dtype, n_rd, chain):
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    rd, ref, nrm = clouds(n_rd, dtype)
    for knn in (1, 3, 5):
        for nbr_cache in (0, 1):
            for reading_order in (0, 1):
                ctx = _capi.Context(0, dtype)
                ctx.set_option("nbr_cache", nbr_cache)
                ctx.set_option("reading_order", reading_order)
                ctx.set_reference(ref, nrm)
                ctx.set_reading(rd)
                if "sn" in CHAINS[chain]:
                    ctx.set_reading_normals(reading_normals(rd, ref, nrm))
                run_chain(ctx, chain, knn, dtype, rd)
                ctx.p2plane_system()
                H, Q, pairs = ctx.p2plane_covariance(np.asarray(T_STEP, dtype))
                Hn, Qn, kept = restate_match(ctx, rd, ref, nrm, T_AT, T_STEP, dtype)
                d, _ = ctx.get_matches()
                ctx.close()
                tag = f"{dn} n={n_rd} {chain} knn={knn} nbr={nbr_cache} order={reading_order}"
                print(f"{tag}: pairs {pairs}/{kept} of {d.size} |dH|={rel(H, Hn):.3g} |dQ|={rel(Q, Qn):.3g} "
                      f"cond(H)={np.linalg.cond(Hn):.3g}")
                assert 6 < kept < d.size, tag  # (the chain rejects something and keeps enough)
                if chain == "maxdist":
                    assert np.isinf(d).any() and np.isfinite(d).any(), tag
                assert np.linalg.cond(Hn) <= 100, tag
                assert pairs == kept, tag
                assert rel(H, Hn) <= BAR[dn], tag
                assert rel(Q, Qn) <= BAR[dn], tag
                assert np.array_equal(H, H.T) and np.array_equal(Q, Q.T)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_kept_pair(dtype):
    from libpointmatcher_amd import _capi
    from libpointmatcher_amd.icp import ICP
    dn = np.dtype(dtype).name
    rd, ref, nrm = clouds(65, dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    I = np.eye(4, dtype=dtype)
    ctx.match(I, knn=1)
    d, _ = ctx.get_matches()
    lo, hi = np.sort(d.ravel().astype(np.float64))[:2]
    assert lo < hi
    max_dist = float(np.sqrt((lo + hi) / 2))  # (MaxDist compares the squared distance with maxDist^2)
    ctx.outlier("MaxDistOutlierFilter", 0, maxDist=max_dist)
    ctx.p2plane_system()
    H, Q, pairs = ctx.p2plane_covariance(np.asarray(T_STEP, dtype))
    Hn, Qn, kept = restate_match(ctx, rd, ref, nrm, I, T_STEP, dtype)
    ctx.close()
    assert pairs == kept == 1
    assert rel(H, Hn) <= BAR[dn] and rel(Q, Qn) <= BAR[dn]
    # the host chain: H is singular (rank 1); the inverse gives what it gives, nothing is raised
    rd_u, ref_u, _ = clouds(65, dtype, centre=False)
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(filters=[("MaxDistOutlierFilter", {"maxDist": max_dist})], minimizer=COV, maxit=1))
    icp.compute(rd_u, ref_u, nrm)
    assert icp.stats().kept == 1
    assert icp.covariance().shape == (6, 6)
    icp.close()


# --------------------------------------------------------------- whole ICP --
STEP_FILTER = "readingStepDataPointsFilters:\n  - IdentityDataPointsFilter\n"
TRIM = (("TrimmedDistOutlierFilter", {"ratio": 0.85}),)
DIFF = dict(minDiffRotErr=0.001, minDiffTransErr=0.01, smoothLength=2)


def seq_mean(ref, dtype):
    """The reference mean as ICP::compute forms it (ICP.cpp:291-292): each
    coordinate summed sequentially in T, divided by M."""
    t = np.dtype(dtype).type
    return np.array([np.cumsum(ref[:, r], dtype=dtype)[-1] / t(len(ref)) for r in range(3)], dtype)


def run_icp(dtype, rd, ref, nrm, minimizer, monkeypatch, device_loop=True, step_filter=False, sigma=None):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if device_loop else "0")
    icp = ICP(dtype)
    m = minimizer if sigma is None else f"{minimizer}:\n    sensorStdDev: {sigma}\n"
    y = chain_yaml(filters=TRIM, minimizer=m, maxit=12, differential=DIFF)
    icp.load_yaml((STEP_FILTER if step_filter else "") + y)
    icp.keep_trace()
    T = icp.compute(rd, ref, nrm)
    out = dict(T=T, trace=icp.trace(), cov=icp.covariance(), iters=icp.stats().iterations, kept=icp.stats().kept)
    icp.close()
    return out


def restate_icp(dtype, rd, ref, nrm, trace, sigma=0.01):
    """sigma^2 H^-1 Q H^-1 of the restatement in float64 at the last iteration's
    pose and increment, both from the trace; its H, Q and cond(H)."""
    from libpointmatcher_amd import _capi
    mean = seq_mean(ref, dtype)
    refc, rdc = ref.copy(), rd.copy()
    refc[:, :3] = ref[:, :3] - mean   # ICP.cpp:299, in T
    rdc[:, :3] = rd[:, :3] - mean     # T_refMean_dataIn = a pure translation: exact in T
    T_at = trace[-2] if len(trace) > 1 else np.eye(4, dtype=dtype)
    T_step = (trace[-1].astype(np.float64) @ np.linalg.inv(T_at.astype(np.float64))).astype(dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(refc, nrm)
    ctx.set_reading(rdc)
    ctx.match(T_at, knn=1)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    H, Q, kept = restate_match(ctx, rdc, refc, nrm, T_at, T_step, dtype)
    ctx.close()
    Hi = np.linalg.inv(H)
    return sigma * sigma * (Hi @ Q @ Hi), H, Q, kept


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rd", [65, 130])
def test_whole_icp_three_paths(dtype, n_rd, monkeypatch):
    dn = np.dtype(dtype).name
    rd, ref, nrm = clouds(n_rd, dtype, centre=False)
    plain = run_icp(dtype, rd, ref, nrm, PLAIN, monkeypatch)
    assert not plain["cov"].any()  # ErrorMinimizer::getCovariance: zeros
    paths = {"loop": dict(), "modules": dict(device_loop=False), "step_filter": dict(step_filter=True)}
    got = {k: run_icp(dtype, rd, ref, nrm, COV, monkeypatch, **kw) for k, kw in paths.items()}
    # the transforms are PointToPlane's, bit for bit
    assert got["loop"]["iters"] == plain["iters"] > 1
    assert np.array_equal(got["loop"]["T"], plain["T"])
    assert np.array_equal(got["loop"]["trace"], plain["trace"])
    cov_n, Hn, Qn, kept = restate_icp(dtype, rd, ref, nrm, got["loop"]["trace"])
    cond = np.linalg.cond(Hn)
    assert cond <= 100
    tol = (2 * cond + 1) * BAR[dn]
    for k, g in got.items():
        err = rel(g["cov"].astype(np.float64), cov_n)
        print(f"{dn} n={n_rd} {k}: iterations {g['iters']} kept {g['kept']}/{kept} cond(H)={cond:.3g} "
              f"|dcov|={err:.3g} tol={tol:.3g}")
        assert g["kept"] == kept
        assert err <= tol, k
    # the three paths' sums agree (read back through their covariances' inputs:
    # equal H and Q give equal products in T)
    for k in ("modules", "step_filter"):
        assert rel(got[k]["cov"].astype(np.float64), got["loop"]["cov"].astype(np.float64)) <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_paths_sums_agree(dtype):
    """H and Q of the device loop, of the module calls and of a re-uploaded
    reading (the step filters' path) agree within 1e-12."""
    from libpointmatcher_amd import _capi
    rd, ref, nrm = clouds(130, dtype)
    filters = [("TrimmedDistOutlierFilter", 0.85)]
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.loop_begin(filters=filters, minimizer=COV, checkers=[("CounterTransformationChecker", 4)], keep_trace=True)
    with pytest.raises(_capi.PmxError):  # PMX_E_STATE: not done yet
        ctx.loop_covariance()
    st = ctx.loop_run(2)
    assert not st.done
    with pytest.raises(_capi.PmxError):
        ctx.loop_covariance()
    st = ctx.loop_run(10)
    assert st.done and st.iterations == 4
    Hl, Ql, nl = ctx.loop_covariance()
    tr = ctx.loop_trace(0, 4)
    # a loop begun with plain PointToPlane keeps no increment: PMX_E_STATE
    ctx.loop_begin(filters=filters, checkers=[("CounterTransformationChecker", 2)])
    ctx.loop_run(5)
    with pytest.raises(_capi.PmxError):
        ctx.loop_covariance()
    ctx.close()
    I = np.eye(4, dtype=dtype)
    for reupload in (False, True):
        ctx = _capi.Context(0, dtype)
        ctx.set_reference(ref, nrm)
        ctx.set_reading(rd)
        T = I
        for it in range(4):
            if reupload:
                ctx.set_reading(rd)
            ctx.match(T, knn=1)
            ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
            A, b, _ = ctx.p2plane_system()
            assert np.array_equal(tr[it - 1] if it else I, T)
            dT = (tr[it].astype(np.float64) @ np.linalg.inv(T.astype(np.float64))).astype(dtype)
            T = tr[it]
        # (the loop's own increment is not observable; the trace's quotient is
        # within an ulp of T of it, which moves Q by about as much)
        H, Q, n = ctx.p2plane_covariance(dT)
        ctx.close()
        assert n == nl
        assert rel(H, Hl) <= 1e-12
        assert rel(Q, Ql) <= (1e-12 if dtype == np.float64 else 1e-5)


def test_sensor_std_dev_scales_exactly(monkeypatch):
    rd, ref, nrm = clouds(130, np.float64, centre=False)
    a = run_icp(np.float64, rd, ref, nrm, COV, monkeypatch, sigma=0.01)["cov"]
    b = run_icp(np.float64, rd, ref, nrm, COV, monkeypatch, sigma=0.05)["cov"]
    assert a.any()
    # 0.05^2 / 0.01^2 = 25 up to the two squares' own rounding
    np.testing.assert_allclose(b, 25.0 * a, rtol=4 * np.finfo(np.float64).eps, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_2d_icp_gives_max_identity(dtype):
    from libpointmatcher_amd.icp import ICP
    rng = np.random.default_rng(5)
    t = np.linspace(0, 1, 80)
    ref = np.concatenate([np.stack([t, np.zeros_like(t)], 1), np.stack([np.zeros_like(t), t], 1)])
    nrm = np.concatenate([np.tile([0.0, 1.0], (80, 1)), np.tile([1.0, 0.0], (80, 1))])
    rd = ref[::2] + rng.normal(0, 0.005, (80, 2)) + [0.01, -0.01]
    hom = lambda p: np.ascontiguousarray(np.c_[p, np.ones(len(p))], dtype=dtype)  # noqa: E731
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(filters=TRIM, minimizer=COV, maxit=5))
    icp.compute(hom(rd), hom(ref), np.ascontiguousarray(nrm, dtype=dtype))
    assert np.array_equal(icp.covariance(), np.finfo(dtype).max * np.eye(6, dtype=dtype))
    icp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_icp_sequence_second_scan(dtype):
    from libpointmatcher_amd.icp import ICPSequence
    dn = np.dtype(dtype).name
    rd1, ref, nrm = clouds(65, dtype, centre=False)
    rd2, _, _ = clouds(130, dtype, centre=False)
    seq = ICPSequence(dtype)
    seq.load_yaml(chain_yaml(filters=TRIM, minimizer=COV, maxit=12, differential=DIFF))
    seq.keep_trace()
    assert seq.set_map(ref, nrm)
    seq.compute(rd1)
    c1 = seq.covariance()
    seq.compute(rd2)
    c2 = seq.covariance()
    trace = seq.trace()
    seq.close()
    assert not np.array_equal(c1, c2)
    cov_n, Hn, _, _ = restate_icp(dtype, rd2, ref, nrm, trace)
    tol = (2 * np.linalg.cond(Hn) + 1) * BAR[dn]
    assert rel(c2.astype(np.float64), cov_n) <= tol


# ---------------------------------------------------------------- two ranks --
def _worker(rank, world, port, outdir):
    import torch  # noqa: F401  (first: its HIP runtime is the one the library binds to)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from libpointmatcher_amd import _capi
        from libpointmatcher_amd.icp import ICP
        from test_gpu_multirank import shard_range

        comm = _capi.gloo_host_comm()
        res = {}
        for dtype in DTYPES:
            dn = np.dtype(dtype).name
            rd, ref, nrm = clouds(130, dtype)
            lo, hi = shard_range(len(rd), world, rank)
            shard = np.ascontiguousarray(rd[lo:hi])
            ctx = _capi.Context(0, dtype)
            ctx.comm_init_host(comm)
            ctx.set_reference(ref, nrm)
            ctx.set_reading(shard)
            ctx.match(np.asarray(T_AT, dtype), knn=1)
            ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
            ctx.p2plane_system()
            H, Q, n = ctx.p2plane_covariance(np.asarray(T_STEP, dtype))
            ctx.close()
            res[f"{dn}_sums"] = np.concatenate([H.ravel(), Q.ravel(), [n]])
            rd_u, ref_u, _ = clouds(130, dtype, centre=False)
            for tag, minimizer in (("plain", PLAIN), ("cov", COV)):
                icp = ICP(dtype)
                icp.comm_init_host(comm)
                icp.load_yaml(chain_yaml(filters=TRIM, minimizer=minimizer, maxit=6))
                T = icp.compute(np.ascontiguousarray(rd_u[lo:hi]), ref_u, nrm)
                res[f"{dn}_{tag}"] = np.concatenate([T.astype(np.float64).ravel(), [icp.comm_stats()["allreduces"]]])
                icp.close()
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    from test_gpu_multirank import _free_port
    tmp = tmp_path_factory.mktemp("cov_mr")
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(i, 2, port, str(tmp))) for i in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.exitcode is None:
            p.kill()
    assert codes == [0, 0], codes
    return [dict(np.load(tmp / f"rank{i}.npz")) for i in range(2)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_ranks_equal_one(two_ranks, dtype):
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    rd, ref, nrm = clouds(130, dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.match(np.asarray(T_AT, dtype), knn=1)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    ctx.p2plane_system()
    H, Q, n = ctx.p2plane_covariance(np.asarray(T_STEP, dtype))
    ctx.close()
    for r in two_ranks:
        got = r[f"{dn}_sums"]
        assert int(got[72]) == n
        assert rel(got[:36].reshape(6, 6), H) <= 1e-12
        assert rel(got[36:72].reshape(6, 6), Q) <= 1e-12
        # the same transform, and exactly one more all-reduce per ICP
        assert np.array_equal(r[f"{dn}_cov"][:16], r[f"{dn}_plain"][:16])
        assert int(r[f"{dn}_cov"][16]) == int(r[f"{dn}_plain"][16]) + 1

"""PointToPointSimilarityErrorMinimizer on the GPU: the module sums
(pmx_p2point_similarity_system), the step on the per-module path and in the
device loop, the non-rigid plumbing, temporal reuse under scaling, ICPSequence
and the reference's own known answer (utest/utest.cpp:222-243).

The yardstick is the numpy restatement below of
ErrorMinimizers/PointToPointSimilarity.cpp:55-97: the per-pair terms in the
ICP's dtype in the reference's order, the sums in float64, numpy.linalg.svd in
the dtype, fed with the matches and weights read back through pmx_get_matches /
pmx_get_weights and the transforms of the trace.

Fixture: a few hundred points uniform in a box of extents 2 x 1.6 x 1.2 (2-D:
2 x 1.6), the reading a subset of them plus 0.002 noise under the inverse of a
similarity of scale 1.04; 65, 130 and 300 reading points (one wave plus a
tail, two waves plus a tail, more than one block).  cond(m) of it is about 3;
the step tests assert <= 100, so LAPACK's and the Jacobi SVD differ by a few
ulps only.

Bars: the sums sigma and m relative 1e-12 (only the fp64 summation order
differs), the means and every transform relative 1e-5 (f32) / 1e-12 (f64), the
project's parity bars.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from helpers import chain_yaml  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {"float32": 1e-5, "float64": 1e-12}
SUM_BAR = 1e-12
SIM, P2P = "PointToPointSimilarityErrorMinimizer", "PointToPointErrorMinimizer"
DTYPES = [np.float32, np.float64]
HERE = os.path.dirname(os.path.abspath(__file__))
TRIM75 = (("TrimmedDistOutlierFilter", {"ratio": 0.75}),)


# ------------------------------------------------------------------ fixture --
def rot3(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def similarity(D, scale, ang, t):
    """(D+1) x (D+1): scale * rotation and a translation."""
    T = np.eye(D + 1)
    if D == 3:
        T[:3, :3] = scale * rot3(ang, -0.7 * ang, 1.3 * ang)
    else:
        c, s = np.cos(ang), np.sin(ang)
        T[:2, :2] = scale * np.array([[c, -s], [s, c]])
    T[:D, D] = np.asarray(t, np.float64)[:D]
    return T


def hom(p, dtype):
    return np.ascontiguousarray(np.c_[p, np.ones(len(p))], dtype=dtype)


POSE_T = [0.012, -0.009, 0.007]


def clouds(n_rd, dtype, D=3, M=400, noise=0.002, scale=1.04, ang=0.01, off=(0.0, 0.0, 0.0), extent=1.0, seed=7):
    """(reading n_rd x (D+1), reference M x (D+1)): the reference uniform in a
    box about `off`, the reading n_rd of its points plus noise under the
    inverse of similarity(scale, ang, POSE_T) about `off`."""
    rng = np.random.default_rng(seed + n_rd + 1000 * D)
    ref = rng.uniform(-1, 1, (M, D)) * np.array([1.0, 0.8, 0.6])[:D] * extent
    rd = ref[rng.permutation(M)[:n_rd]] + rng.normal(0, noise * extent, (n_rd, D))
    pose = similarity(D, scale, ang, np.array(POSE_T) * extent)
    rd = (np.linalg.inv(pose) @ np.c_[rd, np.ones(n_rd)].T).T[:, :D]
    o = np.asarray(off, np.float64)[:D]
    return hom(rd + o, dtype), hom(ref + o, dtype)


# -------------------------------------------------------------- restatement --
def xform(T, p):
    """The device's transform of the reading (xform3), in T's dtype; (n, 3), z = 0 in 2-D."""
    D = T.shape[0] - 1
    if D == 3:
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] * p[:, 3]
                         for r in range(3)], 1)
    out = np.zeros((len(p), 3), p.dtype)
    for r in range(2):
        out[:, r] = (T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]
    return out


def pad3(q):
    return q if q.shape[1] == 3 else np.c_[q, np.zeros(len(q), q.dtype)]


def restate_means(p, q, w, dtype):
    """PointToPointSimilarity.cpp:57-62: w_sum_inv = 1 / w.sum(); sum(p w) * w_sum_inv, in T."""
    t = np.dtype(dtype).type
    winv = t(1) / t(w.astype(np.float64).sum())
    mp = (p * w[:, None]).astype(np.float64).sum(0).astype(dtype) * winv
    mq = (q * w[:, None]).astype(np.float64).sum(0).astype(dtype) * winv
    assert mp.dtype == np.dtype(dtype)
    return mp, mq


def restate_sums(p, q, w, mp, mq, dtype):
    """:66-73: sigma = sum ||pc||^2 w and m = sum (qc w) pc^T, terms in T, sums in float64."""
    pc, qc = p - mp, q - mq
    term = ((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2]) * w
    mt = (qc * w[:, None])[:, :, None] * pc[:, None, :]
    assert term.dtype == mt.dtype == np.dtype(dtype)
    return term.astype(np.float64).sum(), mt.astype(np.float64).sum(0)


def restate_step(mp, mq, m, sigma, dtype, D):
    """:74-97 in T: ((D+1) x (D+1) step, reflected?, unit scale?, cond(m))."""
    t = np.dtype(dtype).type
    mT = np.ascontiguousarray(m[:D, :D], dtype=dtype)
    U, S, Vt = np.linalg.svd(mT)
    assert U.dtype == np.dtype(dtype)
    cond = float(S[0] / S[-1])
    R = U @ Vt
    reflected = bool(np.linalg.det(R.astype(np.float64)) < 0)
    if reflected:
        Vt[D - 1] *= -1
        S[D - 1] *= -1
        R = U @ Vt
    sg = t(sigma)
    scale = S.sum(dtype=dtype) / sg
    unit = bool(sg < t(0.0001))
    if unit:
        scale = t(1)
    sR = (scale * R).astype(dtype)
    out = np.eye(D + 1, dtype=dtype)
    out[:D, :D] = sR
    out[:D, D] = mq[:D] - sR @ mp[:D]
    return out, reflected, unit, cond


def kept_pairs(ctx, rd0, ref, T_at, dtype):
    """ErrorElements of the context's current match and chain: the transformed
    reading points, their matched reference points and weights (K x 3, K x 3, K)."""
    d, ids = ctx.get_matches()
    w = ctx.get_weights()
    kept = (d != np.inf) & (w != 0)
    qi, s = np.nonzero(kept)
    p = xform(np.asarray(T_at, dtype), rd0)[qi]
    q = pad3(np.ascontiguousarray(ref[ids[qi, s], :ref.shape[1] - 1]))
    return p, q, np.ascontiguousarray(w[qi, s]), d


def restated_increment(ctx, rd0, ref, T_at, dtype):
    D = ref.shape[1] - 1
    p, q, w, _ = kept_pairs(ctx, rd0, ref, T_at, dtype)
    mp, mq = restate_means(p, q, w, dtype)
    sigma, m = restate_sums(p, q, w, mp, mq, dtype)
    return restate_step(mp, mq, m, sigma, dtype, D)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def scale_of(T):
    D = T.shape[0] - 1
    return float(np.linalg.det(np.asarray(T, np.float64)[:D, :D])) ** (1.0 / D)


# ------------------------------------------------------------ module path --
CHAINS = {
    "trim": dict(filters=[("TrimmedDistOutlierFilter", dict(ratio=0.75))]),
    "maxdist": dict(max_dist=0.05, filters=[("MaxDistOutlierFilter", dict(maxDist=0.015))]),
    "robust": dict(robust=True),
}


def run_chain(ctx, chain, knn, T_at, dtype):
    from libpointmatcher_amd import _capi
    c = CHAINS[chain]
    ctx.match(np.asarray(T_at, dtype), knn=knn, max_dist=c.get("max_dist", np.inf))
    for pos, (name, p) in enumerate(c.get("filters", [])):
        ctx.outlier(name, pos, **p)
    if c.get("robust"):
        ctx.outlier_robust(0, "cauchy", 0.5, 1.5, _capi.RS_MAD, 0.0)  # (the approximation zeroes the far pairs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_module_sums_match_restatement(dtype, D, chain):
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    # the match's transform scales: the kernels apply the matrix they are handed
    T_at = similarity(D, 1.03, 0.004, [0.002, -0.001, 0.003]).astype(dtype)
    for n_rd in (65, 130, 300):
        rd, ref = clouds(n_rd, dtype, D)
        for knn in (1, 2):
            ctx = _capi.Context(0, dtype)
            ctx.set_reference(ref)
            ctx.set_reading(rd)
            run_chain(ctx, chain, knn, T_at, dtype)
            mp, mq, m, sigma, st = ctx.p2point_similarity_system()
            # PointToPoint's entry point on the same match: the same means and moments
            mp1, mq1, m1, st1 = ctx.p2point_system()
            p, q, w, d = kept_pairs(ctx, rd, ref, T_at, dtype)
            ctx.close()
            tag = f"{dn} D={D} n={n_rd} {chain} knn={knn}"
            mpn, mqn = restate_means(p, q, w, dtype)
            # (the sums centred on the device's means, T values: a last-bit
            # difference of a mean would move every term)
            mpd, mqd = np.zeros(3, dtype), np.zeros(3, dtype)
            mpd[:D], mqd[:D] = mp, mq
            assert np.array_equal(mpd.astype(np.float64)[:D], mp) and np.array_equal(mqd.astype(np.float64)[:D], mq)
            sn, mn = restate_sums(p, q, w, mpd, mqd, dtype)
            print(f"{tag}: kept {st.kept}/{d.size} sigma {sigma:.6g} |dsigma|={abs(sigma - sn) / sn:.3g} "
                  f"|dm|={rel(m, mn[:D, :D]):.3g} |dmp|={rel(mp, mpn[:D]):.3g} |dmq|={rel(mq, mqn[:D]):.3g}")
            assert 6 < len(w) < d.size and st.kept == len(w), tag  # (the chain rejects something, keeps enough)
            if chain == "robust":
                assert ((w != 0) & (w != 1)).any(), tag  # (real-valued weights)
            assert rel(mp, mpn[:D]) <= BAR[dn] and rel(mq, mqn[:D]) <= BAR[dn], tag
            assert abs(sigma - sn) <= SUM_BAR * sn, tag
            assert rel(m, mn[:D, :D]) <= SUM_BAR, tag
            if D == 2:  # the embedding: the z terms are exactly zero
                assert not mn[2].any() and not mn[:, 2].any()
            assert np.array_equal(mp, mp1) and np.array_equal(mq, mq1) and np.array_equal(m, m1), tag
            assert st.asdict() == st1.asdict(), tag


# -------------------------------------------------------------- whole ICP --
def seq_mean(ref, dtype):
    """The reference mean as ICP::compute forms it (ICP.cpp:291-292): each
    coordinate summed sequentially in T, divided by M."""
    t = np.dtype(dtype).type
    D = ref.shape[1] - 1
    return np.array([np.cumsum(ref[:, r], dtype=dtype)[-1] / t(len(ref)) for r in range(D)], dtype)


def run_icp(dtype, rd, ref, monkeypatch, device_loop=True, minimizer=SIM, filters=TRIM75, maxit=30, differential=None,
            T_init=None, opts="", knn=1):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if device_loop else "0")
    monkeypatch.setenv("PMX_OPTS", opts)
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(knn=knn, filters=filters, minimizer=minimizer, maxit=maxit, differential=differential))
    icp.keep_trace()
    try:
        T = icp.compute(rd, ref, None, T_init)
        return dict(T=T, trace=icp.trace(), iters=icp.stats().iterations, kept=icp.stats().kept)
    finally:
        icp.close()


def check_steps(dtype, rd, ref, trace, filters=TRIM75, max_cond=100.0):
    """Every trace[i + 1] against the restated step applied to the GPU's own
    trace[i] (identity before the first); the branches the restatement took."""
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    R = ref.shape[1]
    D = R - 1
    mean = seq_mean(ref, dtype)
    refc, rdc = ref.copy(), rd.copy()
    refc[:, :D] = ref[:, :D] - mean   # ICP.cpp:299, in T
    rdc[:, :D] = rd[:, :D] - mean     # T_refMean_dataIn = a pure translation: exact in T
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(refc)
    ctx.set_reading(rdc)
    flags, worst = [], 0.0
    T_at = np.eye(R, dtype=dtype)
    for i in range(len(trace)):
        ctx.match(T_at, knn=1)
        for pos, (name, p) in enumerate(filters):
            ctx.outlier(name, pos, **p)
        if not filters:
            ctx.outlier_default()
        dT, reflected, unit, cond = restated_increment(ctx, rdc, refc, T_at, dtype)
        assert cond <= max_cond, (i, cond)
        want = (dT @ T_at).astype(dtype)
        err = rel(trace[i], want)
        worst = max(worst, err)
        assert err <= BAR[dn], (dn, i, err)
        flags.append((reflected, unit))
        T_at = np.ascontiguousarray(trace[i])
    ctx.close()
    return flags, worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 2])
def test_step_matches_restatement_per_iteration(dtype, D, monkeypatch):
    dn = np.dtype(dtype).name
    rd, ref = clouds(300, dtype, D, off=(0.3, -0.2, 0.1))
    diff = dict(minDiffRotErr=0.0005, minDiffTransErr=0.0005, smoothLength=3)
    got = {}
    for path in ("loop", "modules"):
        g = run_icp(dtype, rd, ref, monkeypatch, device_loop=path == "loop", differential=diff)
        assert 2 < g["iters"] == len(g["trace"])
        flags, worst = check_steps(dtype, rd, ref, g["trace"])
        assert not any(r or u for r, u in flags)
        print(f"{dn} D={D} {path}: iterations {g['iters']} kept {g['kept']} worst step error {worst:.3g} "
              f"scale {scale_of(g['T']):.6f}")
        got[path] = g
    assert got["loop"]["iters"] == got["modules"]["iters"]
    assert got["loop"]["kept"] == got["modules"]["kept"]
    assert rel(got["loop"]["T"], got["modules"]["T"]) <= BAR[dn]
    assert abs(scale_of(got["loop"]["T"]) - 1.04) < 0.01  # (noise: the exact-image test holds the bar)


def test_p2p_onepass_does_not_change_similarity(monkeypatch):
    # (the one-pass form is the rigid minimiser's, double only: LoopCfg.p2p_onepass)
    rd, ref = clouds(300, np.float64, 3)
    a = run_icp(np.float64, rd, ref, monkeypatch, opts="p2p_onepass=0", maxit=12)
    b = run_icp(np.float64, rd, ref, monkeypatch, opts="p2p_onepass=1", maxit=12)
    assert a["iters"] == b["iters"] == 12
    assert np.array_equal(a["trace"], b["trace"]) and np.array_equal(a["T"], b["T"])


# ---------------------------------------------------------------- branches --
def mirrored_strip(dtype, D):
    """A jittered lattice one cell thick in the last coordinate, and its mirror
    image in that coordinate as the reference: every point's nearest reference
    point is its own image (2 * 0.35 < the lattice's 0.8), so U V^T of the
    first iteration is a reflection.  cond(m) ~ 2 / 0.06."""
    rng = np.random.default_rng(11 + D)
    n = 5
    g = np.arange(n) - (n - 1) / 2
    if D == 3:
        a, b = [v.ravel() for v in np.meshgrid(g, g, indexing="ij")]
        pts = np.stack([a, b, np.zeros_like(a)], 1)
    else:
        pts = np.stack([g, np.zeros_like(g)], 1)
    pts[:, :D - 1] += rng.uniform(-0.1, 0.1, (len(pts), D - 1))
    pts[:, D - 1] = 0.35 * np.cos(2.4 * np.arange(len(pts)) + 0.5)
    ref = pts.copy()
    ref[:, D - 1] = -ref[:, D - 1]
    return hom(pts, dtype), hom(ref + 0.01, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("device_loop", [True, False])
def test_reflection_branch(dtype, D, device_loop, monkeypatch):
    rd, ref = mirrored_strip(dtype, D)
    g = run_icp(dtype, rd, ref, monkeypatch, device_loop=device_loop, filters=(), maxit=1)
    assert g["iters"] == 1 and g["kept"] == len(rd)
    flags, _ = check_steps(dtype, rd, ref, g["trace"], filters=())
    assert flags == [(True, False)]
    assert np.linalg.det(np.asarray(g["trace"][0], np.float64)[:D, :D]) > 0  # (a rotation, scaled)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("device_loop", [True, False])
def test_small_sigma_forces_unit_scale(dtype, device_loop, monkeypatch):
    # extent 5e-4 (a cloud 1e-3 wide): sigma ~ 225 * 1.7e-7 < 0.0001, although the reference is the
    # reading's image at scale 1.04
    rd, ref = clouds(300, dtype, 3, extent=5e-4)
    g = run_icp(dtype, rd, ref, monkeypatch, device_loop=device_loop, maxit=2)
    flags, _ = check_steps(dtype, rd, ref, g["trace"])
    assert flags == [(False, True)] * 2
    bar = BAR[np.dtype(dtype).name]
    assert abs(scale_of(g["trace"][0]) - 1.0) <= bar and abs(scale_of(g["T"]) - 1.0) <= bar


# ------------------------------------------------------------- exact image --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("device_loop", [True, False])
def test_exact_image_recovers_the_scale(dtype, D, device_loop, monkeypatch):
    dn = np.dtype(dtype).name
    rd, ref = clouds(300, dtype, D, noise=0.0)
    g = run_icp(dtype, rd, ref, monkeypatch, device_loop=device_loop, maxit=30)
    s = scale_of(g["T"])
    print(f"{dn} D={D} loop={device_loop}: scale {s:.12f} after {g['iters']} iterations")
    assert abs(s - 1.04) <= 1.04 * BAR[dn]
    # the loop's known answer: the accumulated scale passed 1.001 and the loop went on
    # (PMX_E_TRANSFORMATION with the determinant check)
    scales = np.array([scale_of(t) for t in g["trace"]])
    assert g["iters"] == 30 and (np.abs(scales[:-1] - 1.0) > 0.001).any()
    want = similarity(D, 1.04, 0.01, POSE_T)
    assert rel(g["T"], want) <= 10 * BAR[dn]  # (the clouds are rounded to T; 30 products of steps)


# ------------------------------------------------------ non-rigid plumbing --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("device_loop", [True, False])
def test_scaled_t_init(dtype, device_loop, monkeypatch):
    from libpointmatcher_amd.icp import TransformationError
    rd, ref = clouds(300, dtype, 3, scale=1.1, noise=0.0)
    T_init = similarity(3, 1.1, 0.0, [0, 0, 0])
    g = run_icp(dtype, rd, ref, monkeypatch, device_loop=device_loop, T_init=T_init, maxit=20)
    assert g["iters"] == 20
    assert abs(scale_of(g["T"]) - 1.1) <= 1.1 * BAR[np.dtype(dtype).name]
    with pytest.raises(TransformationError, match="rotation matrix is not orthogonal"):
        run_icp(dtype, rd, ref, monkeypatch, device_loop=device_loop, T_init=T_init, minimizer=P2P, maxit=20)


# ------------------------------------------------ temporal reuse under scaling --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knn", [1, 2])
def test_temporal_reuse_under_scaling(dtype, knn):
    """The device loop one iteration at a time: the matches with the temporal
    reuse certificate are bitwise those without it and those of the brute-force
    search at the same transforms."""
    from libpointmatcher_amd import _capi
    rd, ref = clouds(300, dtype, 3)
    iters = 10

    def loop_ctx(reuse):
        ctx = _capi.Context(0, dtype)
        ctx.set_option("grid_reuse", reuse)
        ctx.set_reference(ref)
        ctx.set_reading(rd)
        ctx.loop_begin(knn=knn, filters=[("TrimmedDistOutlierFilter", 0.75)], minimizer=SIM,
                       checkers=[("CounterTransformationChecker", iters)], keep_trace=True)
        return ctx

    a, b = loop_ctx(1), loop_ctx(0)
    c = _capi.Context(0, dtype)
    c.set_search(0)
    c.set_reference(ref)
    c.set_reading(rd)
    T_at = np.eye(4, dtype=dtype)
    certified = 0
    for i in range(iters):
        sa, sb = a.loop_run(1), b.loop_run(1)
        assert sa.iterations == sb.iterations == i + 1
        a.knn = b.knn = knn
        da, ia = a.get_matches()
        db, ib = b.get_matches()
        c.match(T_at, knn=knn)
        dc, ic = c.get_matches()
        assert np.array_equal(da, db) and np.array_equal(ia, ib), i
        assert np.array_equal(da, dc) and np.array_equal(ia, ic), i
        certified += len(rd) - int(a.loop_diag(i, 1)[0, 3])
        T_at = a.loop_trace(i, 1)[0]
        assert np.array_equal(T_at, b.loop_trace(i, 1)[0])
    for x in (a, b, c):
        x.close()
    assert abs(scale_of(T_at) - 1.0) > 0.01  # (the scale moved by more than 1 % overall)
    assert certified > 0  # (the certificate passed for some queries: reuse was exercised)


# ------------------------------------------------------------- ICPSequence --
@pytest.mark.parametrize("dtype", DTYPES)
def test_icp_sequence(dtype, monkeypatch):
    from libpointmatcher_amd.icp import ICPSequence
    dn = np.dtype(dtype).name
    rd, ref = clouds(300, dtype, 3, off=(0.3, -0.2, 0.1))
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    seq = ICPSequence(dtype)
    seq.load_yaml(chain_yaml(filters=TRIM75, minimizer=SIM, maxit=15))
    assert seq.set_map(ref)
    Ts = seq.compute(rd)
    Tr = seq.compute_with_reference(rd, ref)
    seq.close()
    assert abs(scale_of(Ts) - 1.04) < 0.01
    assert rel(Ts, Tr) <= BAR[dn]


# ----------------------------------------------- the reference's known answer --
@pytest.fixture(scope="module")
def car():
    rd = np.load(os.path.join(HERE, "golden", "clouds.npz"))["car400"]
    ref = np.load(os.path.join(HERE, "golden", "car400_scaled.npz"))["car400_scaled"]
    with open(os.path.join(HERE, "golden", "data", "defaultSimilarityPointToPointMinDistDataPointsFilter.yaml")) as f:
        yaml = f.read()
    assert rd.shape == ref.shape == (24989, 3)
    return rd, ref, yaml


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subsample", [False, True])
def test_reference_known_answer(car, dtype, subsample, monkeypatch):
    """utest/utest.cpp:222-243: car_cloud400 against car_cloud400_scaled with the
    reference's chain; |det(T)^(1/3) - 1.04| < 0.001, the reference's own bar."""
    from libpointmatcher_amd.icp import ICP
    rd, ref, yaml = car
    if subsample:
        rd = rd[np.sort(np.random.default_rng(1).permutation(24989)[:2000])]
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    icp = ICP(dtype)
    icp.load_yaml(yaml)
    T = icp.compute(hom(rd, dtype), hom(ref, dtype))
    st = icp.stats()
    icp.close()
    s = scale_of(T)
    print(f"{np.dtype(dtype).name} subsample={subsample}: scale {s:.7f} after {st.iterations} iterations, "
          f"kept {st.kept}")
    assert abs(s - 1.04) < 0.001

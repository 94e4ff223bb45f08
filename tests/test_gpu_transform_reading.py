"""Transformation::compute on the resident reading (pmx_transform_reading,
csrc/pmx_transform.hip transform_reading_kernel) through _capi.Context and
ICP / ICPSequence.reading_transformed.

Module path.  The bar is bit equality with a numpy restatement in the context's
dtype.  The context holds T0 * reading (pmx_set_reading; T0 the identity here,
applied through the same expression, which turns -0.0 into +0.0 and inf into
NaN where inf * 0 appears), so the restatement applies the expression twice:
`held = xf(I, reading)`, then `xf(T, held)`; every row r is
((T_r0 x + T_r1 y) + T_r2 z) + T_r3 w (2-D: (T_r0 x + T_r1 y) + T_r2 w), every
multiply and add a separate numpy operation.  NaNs compare by position (their
payload is the hardware's), everything else by bit pattern, signed zeros
included.  Sizes 1, 63 / 64 / 65 (the wave edge), 257 (one block and a tail of
one) and 4099 (17 blocks, where the slot order is a real permutation).  The
slot table is not readable through the context, so for 4099 the tests assert
instead that the reading is sorted along no axis: an output left in slot
(Morton) order could not equal the restatement.

Chain.  ICP.reading_transformed() against
Transformation("RigidTransformation").compute(filtered_reading, T) (the chain
has no reading filters: the filtered reading is the caller's), per coordinate
within K_ASSERT * eps_T * (max|coordinate| + max|mean|).  First-order bound
(DESIGN.md section 5t), u = eps / 2, rho = sqrt(3) >= the absolute row sum of a
rotation, A = max|coordinate| of the input and the output, M = max|mean_r|,
|t| <= A + M the centred-frame translation of T_iter:
  resident side   one centring rounding u (A + M) carried through a rotation
                  row (rho), the four-term sequential sum 4 u (rho (A + M) +
                  |t|), one un-centring rounding u A:  <= (5 rho + 5) u (A + M)
  reference side  finish()'s two matrix products leave (5 + 4 rho) u M + 5 u |t|
                  in T's translation, pmx_transform_cloud's four-term sum adds
                  4 u (rho A + |t| + (1 + rho) M):       <= (8 rho + 18) u (A + M)
  together (13 rho + 23) u (A + M) = 22.8 eps (A + M):  K_DERIVED = 23.
K_MEASURED is the worst ratio on the box-corner fixture (clouds(130)) over both
dtypes and the three paths, always against Transformation.compute (never
against the resident path itself), measured on an MI355X: 0.767 in float32 and
in float64 alike (one unit in the last place of a coordinate near 1 over a
scale of 1.304; the step-filter path, which is Transformation.compute's own
arithmetic, measures 0).  The tests assert K_ASSERT = min(2 * K_MEASURED,
K_DERIVED) = 1.534; the ICPSequence scans measured 0.78 (65 points, float32),
1.17 (65 points, float64) and 0.767 (130 points) against the same bar.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from helpers import chain_yaml  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SIZES = [1, 63, 64, 65, 257, 4099]
K_DERIVED = 23.0
K_MEASURED = 0.767
K_ASSERT = min(2.0 * K_MEASURED, K_DERIVED)


# ---------------------------------------------------------------- helpers --
def same_values(a, b):
    """Equal bit for bit (signed zeros included), any NaN for a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(u), np.where(nb, 0, b).view(u))


def xf(T, p):
    """The kernel's expression, every row, in the arrays' dtype."""
    assert T.dtype == p.dtype
    rows = p.shape[1]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(rows):
            if rows == 4:
                out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] * p[:, 3]
            else:
                out[:, r] = (T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]
    return out


def lin(T, v):
    """The rotation block's rows on D-vectors (the normals' form)."""
    assert T.dtype == v.dtype
    D = v.shape[1]
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(D):
            acc = T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]
            if D == 3:
                acc = acc + T[r, 2] * v[:, 2]
            out[:, r] = acc
    return out


def restate(T, rd):
    eye = np.eye(rd.shape[1], dtype=rd.dtype)
    return xf(T, xf(eye, rd))  # (the context holds T0 * reading, T0 = I)


def rotation(D, seed):
    rng = np.random.default_rng(seed)
    if D == 3:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        return q
    a = rng.uniform(0.2, 1.2)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def params(kind, D, dtype):
    rng = np.random.default_rng(11 + D)
    T = np.eye(D + 1)
    if kind == "rigid":
        T[:D, :D] = rotation(D, 21)
    elif kind == "similarity":
        T[:D, :D] = 1.04 * rotation(D, 22)
    else:  # a general affine map, the bottom row included
        T = rng.normal(size=(D + 1, D + 1))
    if kind != "affine":
        T[:D, D] = rng.normal(size=D)
    return np.ascontiguousarray(T, dtype=dtype)


KINDS = ["rigid", "similarity", "affine"]


def cloud(n, D, dtype, seed):
    rng = np.random.default_rng(seed)
    p = np.ones((n, D + 1))
    p[:, :D] = rng.normal(size=(n, D))
    return np.ascontiguousarray(p, dtype=dtype)


def sorted_along_an_axis(p):
    return any(np.all(np.diff(p[:, c]) >= 0) or np.all(np.diff(p[:, c]) <= 0) for c in range(p.shape[1] - 1))


def context(dtype, D, reading_order, rd, normals=None, comm=None):
    from libpointmatcher_amd import _capi
    ctx = _capi.Context(0, dtype)
    if comm is not None:
        ctx.comm_init_host(comm)
    ctx.set_option("reading_order", reading_order)
    ctx.set_reference(cloud(500, D, dtype, 5),
                      np.ascontiguousarray(np.tile(np.eye(D)[0], (500, 1)), dtype=dtype))
    ctx.set_reading(rd)
    if normals is not None:
        ctx.set_reading_normals(normals)
    return ctx


# ------------------------------------------------------------ module path --
@pytest.mark.parametrize("reading_order", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_path_bit_exact(dtype, D, n, reading_order):
    from libpointmatcher_amd import _capi
    rd = cloud(n, D, dtype, 100 + n)
    if n == 4099:
        assert not sorted_along_an_axis(rd)  # (an un-permuted output would differ: see the module docstring)
    ctx = context(dtype, D, reading_order, rd)
    for kind in KINDS:
        T = params(kind, D, dtype)
        got = ctx.transform_reading(T)
        assert got.shape == (n, D + 1) and got.dtype == np.dtype(dtype)
        assert np.array_equal(got, restate(T, rd)), kind
        assert np.array_equal(got, _capi.transform_cloud(rd, T)[0]), kind
    ctx.close()


@pytest.mark.parametrize("reading_order", [0, 1])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_normals(dtype, D, reading_order):
    from libpointmatcher_amd import _capi
    n = 4099
    rd = cloud(n, D, dtype, 7)
    nrm = np.ascontiguousarray(np.random.default_rng(8).normal(size=(n, D)), dtype=dtype)
    ctx = context(dtype, D, reading_order, rd, normals=nrm)
    eye = np.eye(D + 1, dtype=dtype)
    for kind in KINDS:
        T = params(kind, D, dtype)
        f, o = ctx.transform_reading(T, normals=True)
        assert np.array_equal(f, restate(T, rd)), kind
        assert o.shape == (n, D)
        assert np.array_equal(o, lin(T, lin(eye, nrm))), kind  # (the context holds R0 * normals, R0 = I)
    ctx.set_reading_normals(None)
    with pytest.raises(_capi.PmxError):  # PMX_E_STATE
        ctx.transform_reading(params("rigid", D, dtype), normals=True)
    ctx.set_reading(rd)  # (a new reading clears the last one's normals too)
    with pytest.raises(_capi.PmxError):
        ctx.transform_reading(params("rigid", D, dtype), normals=True)
    assert np.array_equal(ctx.transform_reading(params("rigid", D, dtype)), restate(params("rigid", D, dtype), rd))
    ctx.close()


@pytest.mark.parametrize("reading_order", [0, 1])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_and_signed_zero(dtype, D, reading_order):
    n = 257
    rd = cloud(n, D, dtype, 9)
    specials = [np.nan, np.inf, -np.inf, -0.0, 0.0]
    for i, v in enumerate(specials):
        for c in range(D):
            rd[3 * (i * D + c) + 1, c] = v
    rd[200, D] = np.nan  # the homogeneous row is a value like the others
    rd[201, D] = np.inf
    rd[202, :D] = -0.0
    ctx = context(dtype, D, reading_order, rd)
    for kind in KINDS:
        T = params(kind, D, dtype)
        want = restate(T, rd)
        # (an infinite coordinate meets a zero of T0 = I when the context takes the reading: its point is NaN)
        assert np.isnan(want).any() and np.isfinite(want).any()
        assert same_values(ctx.transform_reading(T), want), kind
    # the identity keeps -0.0 where the expression keeps it, bit for bit
    eye = np.eye(D + 1, dtype=dtype)
    assert same_values(ctx.transform_reading(eye), restate(eye, rd))
    ctx.close()


def test_no_reading_is_a_state_error():
    from libpointmatcher_amd import _capi
    ctx = _capi.Context(0, np.float32)
    with pytest.raises(_capi.PmxError):
        ctx.transform_reading(np.eye(4, dtype=np.float32))
    ctx.set_reference(cloud(100, 3, np.float32, 1))
    with pytest.raises(_capi.PmxError):
        ctx.transform_reading(np.eye(4, dtype=np.float32))
    ctx.close()


# ------------------------------------------------------------- loop's own T --
@pytest.mark.parametrize("dtype", DTYPES)
def test_loop_T_read_on_the_device(dtype):
    from libpointmatcher_amd import _capi
    from test_gpu_covariance import clouds
    rd, ref, nrm = clouds(130, dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    with pytest.raises(_capi.PmxError):  # PMX_E_STATE: a fresh reading, no loop
        ctx.transform_reading(None)
    ctx.loop_begin(filters=[("TrimmedDistOutlierFilter", 0.85)], checkers=[("CounterTransformationChecker", 4)])
    with pytest.raises(_capi.PmxError):  # begun, not run
        ctx.transform_reading(None)
    st = ctx.loop_run(2)
    assert not st.done
    with pytest.raises(_capi.PmxError):  # not done yet
        ctx.transform_reading(None)
    part = ctx.transform_reading(ctx.loop_T(st))  # (a host matrix is always taken)
    assert np.array_equal(part, restate(ctx.loop_T(st), rd))
    st = ctx.loop_run(10)
    assert st.done and st.iterations == 4
    T = ctx.loop_T(st)
    assert not np.array_equal(T, np.eye(4, dtype=dtype))
    own = ctx.transform_reading(None)
    assert np.array_equal(own, ctx.transform_reading(T))
    assert np.array_equal(own, restate(T, rd))
    assert not np.array_equal(own, part)
    ctx.set_reading(rd)  # a fresh reading: the finished loop's T_iter is not this reading's
    with pytest.raises(_capi.PmxError):
        ctx.transform_reading(None)
    ctx.close()


# ---------------------------------------------------------------- two ranks --
def _worker(rank, world, port, outdir):
    import torch  # noqa: F401  (first: its HIP runtime is the one the library binds to)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from libpointmatcher_amd import _capi
        from test_gpu_multirank import shard_range

        comm = _capi.gloo_host_comm()
        res = {}
        for dtype in DTYPES:
            dn = np.dtype(dtype).name
            rd = cloud(4099, 3, dtype, 31)
            nrm = np.ascontiguousarray(np.random.default_rng(32).normal(size=(4099, 3)), dtype=dtype)
            lo, hi = shard_range(len(rd), world, rank)
            ctx = context(dtype, 3, 1, np.ascontiguousarray(rd[lo:hi]), normals=np.ascontiguousarray(nrm[lo:hi]),
                          comm=comm)
            before = ctx.comm_stats()
            f, o = ctx.transform_reading(params("rigid", 3, dtype), normals=True)
            after = ctx.comm_stats()
            ctx.close()
            res[f"{dn}_f"], res[f"{dn}_n"] = f, o
            res[f"{dn}_coll"] = np.array([before[0], before[1], after[0], after[1]], np.int64)
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    from test_gpu_multirank import _free_port
    tmp = tmp_path_factory.mktemp("xfrd_mr")
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
    dn = np.dtype(dtype).name
    rd = cloud(4099, 3, dtype, 31)
    nrm = np.ascontiguousarray(np.random.default_rng(32).normal(size=(4099, 3)), dtype=dtype)
    ctx = context(dtype, 3, 1, rd, normals=nrm)
    f, o = ctx.transform_reading(params("rigid", 3, dtype), normals=True)
    ctx.close()
    assert np.array_equal(np.concatenate([r[f"{dn}_f"] for r in two_ranks]), f)
    assert np.array_equal(np.concatenate([r[f"{dn}_n"] for r in two_ranks]), o)
    for r in two_ranks:
        c = r[f"{dn}_coll"]
        assert c[0] == c[2] and c[1] == c[3]  # all-reduces, all-gathers: the call issues none


# -------------------------------------------------------------------- chain --
STEP_FILTER = "readingStepDataPointsFilters:\n  - IdentityDataPointsFilter\n"
TRIM = (("TrimmedDistOutlierFilter", {"ratio": 0.85}),)
DIFF = dict(minDiffRotErr=0.001, minDiffTransErr=0.01, smoothLength=2)
PATHS = {"loop": dict(), "modules": dict(device_loop=False), "step_filter": dict(step_filter=True)}


def run_icp(dtype, rd, ref, nrm, monkeypatch, device_loop=True, step_filter=False):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if device_loop else "0")
    icp = ICP(dtype)
    icp.load_yaml((STEP_FILTER if step_filter else "") + chain_yaml(filters=TRIM, maxit=12, differential=DIFF))
    icp.keep_trace()
    T = icp.compute(rd, ref, nrm)
    out = dict(T=T, moved=icp.reading_transformed(), trace=icp.trace(), iters=icp.stats().iterations)
    icp.close()
    return out


def bar(dtype, rd, want, ref):
    """eps_T * (max|coordinate| + max|mean|), and that scale."""
    from test_gpu_covariance import seq_mean
    scale = max(np.abs(rd[:, :3]).max(), np.abs(want[:, :3]).max()) + np.abs(seq_mean(ref, dtype)).max()
    return float(np.finfo(dtype).eps) * float(scale), float(scale)


@pytest.fixture(scope="module")
def rigid_compute():
    """Transformation.compute(filtered_reading, T): the yardstick, one object per dtype."""
    from libpointmatcher_amd.icp import Transformation
    ts = {np.dtype(d).name: Transformation("RigidTransformation", d) for d in DTYPES}
    yield lambda dtype, rd, T: ts[np.dtype(dtype).name].compute(rd, T)[0]
    for t in ts.values():
        t.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_three_paths(dtype, monkeypatch, rigid_compute):
    """The device-loop path (the resident reading, the loop's own T_iter), the
    module calls (the resident reading, the host's T_iter) and the step-filter
    path (the fallback: pmx_transform_cloud on the host copy with the full T)."""
    from test_gpu_covariance import clouds
    dn = np.dtype(dtype).name
    rd, ref, nrm = clouds(130, dtype, centre=False)
    got = {k: run_icp(dtype, rd, ref, nrm, monkeypatch, **kw) for k, kw in PATHS.items()}
    worst = 0.0
    for k, g in got.items():
        assert g["iters"] > 1
        assert g["moved"].shape == rd.shape  # (no reading filters: the filtered reading is the caller's)
        want = rigid_compute(dtype, rd, g["T"])
        unit, scale = bar(dtype, rd, want, ref)
        # the bound's assumption on T_iter's translation in the centred frame
        assert np.abs(g["trace"][-1][:3, 3]).max() <= scale
        ratio = float(np.abs(g["moved"].astype(np.float64) - want.astype(np.float64)).max()) / unit
        worst = max(worst, ratio)
        print(f"{dn} {k}: iterations {g['iters']} scale {scale:.4g} worst |diff| / (eps scale) = {ratio:.4g} "
              f"(asserted {K_ASSERT}, derived {K_DERIVED})")
        assert ratio <= K_ASSERT, k
        assert np.array_equal(g["moved"][:, 3], want[:, 3])  # (the homogeneous row: 1 on every path)
    # the fallbacks against the device-loop result, within the same bar
    for k in ("modules", "step_filter"):
        unit, _ = bar(dtype, rd, got["loop"]["moved"], ref)
        d = float(np.abs(got[k]["moved"].astype(np.float64) - got["loop"]["moved"].astype(np.float64)).max()) / unit
        print(f"{dn} {k} against loop: {d:.4g}")
        assert d <= K_ASSERT, k
    # the step-filter path is the fallback itself: Transformation.compute's arithmetic, bit for bit
    g = got["step_filter"]
    assert np.array_equal(g["moved"], rigid_compute(dtype, rd, g["T"]))
    print(f"{dn}: worst ratio against Transformation.compute {worst:.4g}")
    assert K_ASSERT <= K_DERIVED


@pytest.mark.parametrize("dtype", DTYPES)
def test_icp_sequence_second_scan(dtype, rigid_compute):
    from libpointmatcher_amd.icp import ICPSequence
    from test_gpu_covariance import clouds
    rd1, ref, nrm = clouds(65, dtype, centre=False)
    rd2, _, _ = clouds(130, dtype, centre=False)
    seq = ICPSequence(dtype)
    seq.load_yaml(chain_yaml(filters=TRIM, maxit=12, differential=DIFF))
    with pytest.raises(RuntimeError):
        seq.reading_transformed()
    assert seq.set_map(ref, nrm)
    with pytest.raises(RuntimeError):  # a map, no compute yet
        seq.reading_transformed()
    T1 = seq.compute(rd1)
    m1 = seq.reading_transformed()
    T2 = seq.compute(rd2)
    m2 = seq.reading_transformed()
    seq.close()
    for rd, T, m in ((rd1, T1, m1), (rd2, T2, m2)):
        assert m.shape == rd.shape
        want = rigid_compute(dtype, rd, T)
        unit, _ = bar(dtype, rd, want, ref)
        ratio = float(np.abs(m.astype(np.float64) - want.astype(np.float64)).max()) / unit
        print(f"{np.dtype(dtype).name} scan of {len(rd)}: {ratio:.4g}")
        assert ratio <= K_ASSERT


@pytest.mark.parametrize("dtype", DTYPES)
def test_before_any_compute_raises(dtype):
    from libpointmatcher_amd.icp import ICP
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(filters=TRIM, maxit=4))
    with pytest.raises(RuntimeError, match="no compute has run"):
        icp.reading_transformed()
    icp.close()

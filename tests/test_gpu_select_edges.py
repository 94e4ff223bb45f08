"""The exact order statistic behind Trimmed / Median (select_all_kernel, the
per-pass select_hist / select_pick kernels of the sharded path, and the
quantile window of pmx_spec.h) against a plain sort, bit for bit, on
adversarial keys and at every size where the code takes another path.

Crafted module-path cases: one reference point at the origin and the reading
on the x axis, brute-force search, so the distances are fl(x^2); the expected
values always come from the distances get_matches() returns.  The reference
(helpers.quantile_limit) is pinned against the CPU oracle on the same key
sets in tests/test_select_reference.py.

st.limit is the resolved order statistic (include/pmx.h: the last quantile
threshold); MedianDist scales it by its factor in the weights, so Median cases
assert st.limit against the statistic and factor * st.limit (in T) against the
reference's limit.
"""
import functools

import numpy as np
import pytest

from helpers import (MEDIAN, SELECT_KEY_SETS, SELECT_SIZES, TRIMMED, filter_params, max_dist_keeping, quantile_limit,
                     quantile_value, select_filters, select_reading, select_reading_x)
from libpointmatcher_amd import _capi as P
from libpointmatcher_amd.synth import reference_cloud

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOL = {np.float32: 1e-5, np.float64: 1e-12}  # (tests/test_gpu_loop.py)
ORIGIN = [[0, 0, 0, 1]]
THREE = [[0, 0, 0, 1], [-1, 0, 0, 1], [-2, 0, 0, 1]]


def passes(dtype):
    return 3 if np.dtype(dtype) == np.float32 else 6


def one_rank_comm(ctx):
    """sharded(c) in one process: every collective runs, over one rank."""
    ctx.comm_init_host(P.HostComm(1, 0, lambda a, op: None, lambda a: a))


def crafted(dtype, sharded=False, ref=ORIGIN):
    ctx = P.Context(0, dtype)
    if sharded:
        one_rank_comm(ctx)
    ctx.set_search(0)
    ctx.set_reference(np.asarray(ref, dtype))
    return ctx


def matched(ctx, x, knn=1, max_dist=np.inf):
    ctx.set_reading(select_reading(x))
    ctx.match(np.eye(4, dtype=x.dtype), knn=knn, max_dist=max_dist)
    return ctx.get_matches()[0]


def select(ctx, kind, p):
    """One select through the module path: (weights, the minimiser's stats);
    the minimiser call surfaces the iteration's error word."""
    ctx.outlier(kind, 0, **filter_params(kind, p))
    st = ctx.p2point_system()[3]
    return ctx.get_weights(), st


def check_select(ctx, d, kind, p):
    dtype = d.dtype
    T = dtype.type
    w, st = select(ctx, kind, p)
    limit, rw = quantile_limit(d, kind, p, dtype)
    value = quantile_value(d, kind, p, dtype)
    print(f"{kind} {p!r} n={d.size}: limit {st.limit!r} (sort {float(value)!r}), kept {st.kept} (sort {int(rw.sum())})")
    assert st.limit == float(value), (kind, p)
    assert (T(p) * T(st.limit) if kind == MEDIAN else T(st.limit)) == limit, (kind, p)
    assert np.array_equal(w, rw), (kind, p)
    assert st.kept == int(rw.sum())
    return st.limit


def check_both_paths(dtype, x, filters, knn=1, max_dist=np.inf, ref=ORIGIN, sharded=True, finite=None):
    """Every filter on select_all (one rank), then - sharded - on the per-pass
    kernels through a one-rank communicator: the same bits, the same limit,
    and one histogram all-reduce per pass."""
    ctx = crafted(dtype, ref=ref)
    d = matched(ctx, x, knn, max_dist)
    if finite is not None:
        assert int((d != np.inf).sum()) == finite
    limits = [check_select(ctx, d, kind, p) for kind, p in filters]
    ctx.close()
    if not sharded:
        return
    ctx = crafted(dtype, sharded=True, ref=ref)
    ds = matched(ctx, x, knn, max_dist)
    assert np.array_equal(ds, d)
    for (kind, p), lim in zip(filters, limits):
        ar0 = ctx.comm_stats()[0]
        ctx.outlier(kind, 0, **filter_params(kind, p))
        assert ctx.comm_stats()[0] - ar0 == passes(dtype)  # (the per-pass kernels ran)
        assert check_select(ctx, d, kind, p) == lim
    assert not ctx._comm.errors
    ctx.close()


# ---- 1. sizes: the scalar tail of load_keys, the select_blocks thresholds ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SELECT_SIZES)
@pytest.mark.parametrize("tag", ["lastdigit", "decades"])
def test_select_sizes(tag, n, dtype):
    check_both_paths(dtype, select_reading_x(tag, n, dtype), select_filters(dtype), sharded=n <= 40_000)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", ["lastdigit", "decades"])
def test_select_k3_not_a_multiple_of_16(tag, dtype):
    # n = k N = 4101: two blocks, the second one's last run of keys is 5 long
    x = select_reading_x(tag, 1367, dtype)
    check_both_paths(dtype, x, select_filters(dtype), knn=3, ref=THREE)


# ---- 2. every key set ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
@pytest.mark.parametrize("tag", SELECT_KEY_SETS)
def test_select_key_sets(tag, n, dtype):
    filters = select_filters(dtype) + ([(TRIMMED, 0.80)] if tag == "two_values" else [])
    check_both_paths(dtype, select_reading_x(tag, n, dtype), filters)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
def test_select_mostly_inf(n, dtype):
    x = select_reading_x("decades", n, dtype)
    for m in (1, 2, n // 100, n // 100 + 1):
        check_both_paths(dtype, x, select_filters(dtype), max_dist=max_dist_keeping(x, m), finite=m)


# ---- 3. one context, changing n: the re-zero of the arrival state ----
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_select_one_context_changing_n(dtype, sharded):
    ctx = crafted(dtype, sharded=sharded)
    for n in (40_000, 9000, 300_000, 3000, 9000):  # 8, 2, 64, 1, 2 blocks
        d = matched(ctx, select_reading_x("decades", n, dtype))
        check_select(ctx, d, TRIMMED, 0.85)
    # a select that errors (nothing finite), then a normal one: what the error
    # launch left in the bins and the arrival generations must not leak
    x = select_reading_x("decades", 9000, dtype)
    d = matched(ctx, x, max_dist=1e-30)
    assert np.all(d == np.inf)
    ctx.outlier(TRIMMED, 0, ratio=0.85)
    with pytest.raises(P.ConvergenceError, match="no outlier to filter"):
        ctx.p2point_system()
    d = matched(ctx, x)
    for kind, p in select_filters(dtype):
        check_select(ctx, d, kind, p)
    ctx.close()


# ---- 4. more than 256 selects in one context: the 8-bit generation wraps ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [9000, 3000])  # 2 blocks, 1 block
def test_select_generation_wrap(n, dtype):
    ctx = crafted(dtype)
    d = matched(ctx, select_reading_x("decades", n, dtype))
    for j in range(300):  # (launches 255-258 are the point)
        r = (j + 1) / 300
        w, st = select(ctx, TRIMMED, r)  # (a timed-out wait raises here)
        limit, rw = quantile_limit(d, TRIMMED, r, dtype)
        assert st.limit == float(limit), (j, r)
        assert np.array_equal(w, rw), (j, r)
    ctx.close()


# ---- 5. chain position > 0: still over every finite distance ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag,cut,ratio", [("two_values", 0.125, 0.85), ("decades", 1e-7, 0.3)])
def test_select_chain_position_one(oracle, tag, cut, ratio, dtype):
    T = np.dtype(dtype).type
    for sharded in (False, True):
        ctx = crafted(dtype, sharded=sharded)
        d = matched(ctx, select_reading_x(tag, 3000, dtype))
        ctx.outlier("MaxDistOutlierFilter", 0, maxDist=cut)
        ctx.outlier(TRIMMED, 1, ratio=ratio)
        ctx.p2point_system()
        w = ctx.get_weights()
        ctx.close()
        rw = (d <= T(np.power(float(T(cut)), 2.0))).astype(dtype) * quantile_limit(d, TRIMMED, ratio, dtype)[1]
        assert np.array_equal(w, rw)
        rc, ow = oracle.outlier_chain([("MaxDistOutlierFilter", {"maxDist": cut}), (TRIMMED, {"ratio": ratio})], d)
        assert rc == 0 and np.array_equal(w, ow)


# ---- device loop: the window against the oracle ----
def run_loop(monkeypatch, dtype, rd, ref, nrm, filt, minimizer, iters, spec, sharded=False):
    monkeypatch.setenv("PMX_OPTS", f"spec_select={spec}")
    ctx = P.Context(0, dtype)
    if sharded:
        one_rank_comm(ctx)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.loop_begin(knn=1, filters=[filt], minimizer=minimizer, checkers=[("CounterTransformationChecker", iters)],
                   keep_trace=True)
    st = ctx.loop_run(iters)
    out = dict(trace=ctx.loop_trace(0, st.iterations), stats=ctx.loop_select_stats(), kept=st.last.kept,
               it=st.iterations, T=ctx.loop_T(st), verdict=ctx.loop_diag(0, st.iterations)[:, 1].copy())
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def self_registration(dn, N):
    dtype = np.dtype(dn).type
    ref, nrm = reference_cloud(20_000, dtype)
    return np.ascontiguousarray(ref[:N]), ref, nrm


@functools.lru_cache(maxsize=None)
def twin_lattice(dn):
    """A 32^3 dyadic lattice (spacing 2^-6) and the same lattice with 80 % of
    the points moved by 2^-9 and 20 % by 2^-7 along z."""
    dtype = np.dtype(dn).type
    g = np.arange(32, dtype=np.float64) * 2.0 ** -6
    ref = np.ones((32 ** 3, 4))
    ref[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rd = ref.copy()
    rd[:, 2] += np.where(np.arange(len(rd)) % 5 == 4, 2.0 ** -7, 2.0 ** -9)
    return rd.astype(dtype), ref.astype(dtype), None


LOOP_FILTERS = {"trimmed": ((TRIMMED, 0.85), (TRIMMED, {"ratio": 0.85})),
                "median": ((MEDIAN, 3.0), (MEDIAN, {"factor": 3.0}))}


def loop_case(case, dn):
    """(reading, reference, normals, minimiser, iterations) of a loop case."""
    if case == "twin":
        return twin_lattice(dn) + ("PointToPointErrorMinimizer", 15)
    return self_registration(dn, int(case)) + ("PointToPlaneErrorMinimizer", 12)


# (4096 | 4097: the last window population read from LDS, the first from global
# memory, and the one-rank segment's cap; 16 384 | 16 385: the window's capacity)
LOOP_CASES = [("3000", "trimmed"), ("3000", "median"), ("10000", "trimmed"), ("10000", "median"),
              ("20000", "trimmed"), ("20000", "median"), ("4096", "trimmed"), ("4097", "trimmed"),
              ("16384", "trimmed"), ("16385", "trimmed"), ("twin", "trimmed")]
WINDOW_HOLDS = ("3000", "4096", "4097", "10000", "16384")   # kSpecCap = 16 384 keys
WINDOW_OVERFLOWS = ("16385", "20000")
SEGMENT_HOLDS = ("3000", "4096")                            # kSpecXCap = 4096 keys a segment
SEGMENT_OVERFLOWS = ("4097", "10000", "16384", "16385", "20000")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,filt", LOOP_CASES)
def test_window_loop_vs_oracle(monkeypatch, oracle, case, filt, dtype):
    dn = np.dtype(dtype).name
    rd, ref, nrm, minimizer, iters = loop_case(case, dn)
    gf, of = LOOP_FILTERS[filt]
    on = run_loop(monkeypatch, dtype, rd, ref, nrm, gf, minimizer, iters, 1)
    off = run_loop(monkeypatch, dtype, rd, ref, nrm, gf, minimizer, iters, 0)
    hits, misses = on["stats"]
    print(f"{case} {filt} {dn}: window verdicts {on['verdict'].tolist()}, kept {on['kept']}")
    assert on["it"] == off["it"] == iters and hits + misses == iters
    assert off["stats"] == (0, 0)
    assert np.array_equal(on["trace"], off["trace"])
    assert on["kept"] == off["kept"]
    if case in WINDOW_HOLDS:  # window keys in LDS (<= 4096) / in global memory
        assert (on["verdict"] == 1).any() and hits >= 1
    elif case in WINDOW_OVERFLOWS:  # more keys in the window than it holds: a miss every time
        assert not (on["verdict"][1:] == 1).any() and hits == 0
    cfg = oracle.make_cfg(filters=(of,), minimizer=minimizer, counter_max=iters, threads=8)
    rc, To, so, _ = oracle.icp(cfg, rd, ref, normals=nrm, trace=True)
    assert rc == 0 and so.iterations == on["it"]
    print(f"  |T - T_oracle| = {np.linalg.norm(on['T'] - To):.3e}, oracle kept {so.kept}")
    assert on["kept"] == so.kept
    assert np.linalg.norm(on["T"] - To) <= TOL[dtype]
    if case != "twin":  # every distance is exactly 0 at every iteration
        assert on["kept"] == len(rd) and np.array_equal(on["T"], np.eye(4, dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,filt", LOOP_CASES)
def test_window_loop_one_rank_comm(monkeypatch, case, filt, dtype):
    """The same loops through a one-rank communicator: the segment pack of
    counter_phase and spec_pick over the exchanged segment, 4096 keys a segment."""
    dn = np.dtype(dtype).name
    rd, ref, nrm, minimizer, iters = loop_case(case, dn)
    gf = LOOP_FILTERS[filt][0]
    on = run_loop(monkeypatch, dtype, rd, ref, nrm, gf, minimizer, iters, 1, sharded=True)
    off = run_loop(monkeypatch, dtype, rd, ref, nrm, gf, minimizer, iters, 0, sharded=True)
    hits, misses = on["stats"]
    print(f"{case} {filt} {dn} sharded: {hits} hits, {misses} misses")
    assert on["it"] == off["it"] == iters
    assert np.array_equal(on["trace"], off["trace"]) and on["kept"] == off["kept"]
    assert hits + misses == iters
    if case in SEGMENT_OVERFLOWS:  # beyond the segment cap: missed where the unsharded 10 000 hit
        assert hits == 0
    elif case in SEGMENT_HOLDS:
        assert hits >= 1

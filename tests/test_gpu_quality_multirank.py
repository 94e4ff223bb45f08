"""pmx_match_quality over two ranks on the one MI355X (the pattern of
test_gpu_similarity_multirank.py: one process per rank, the reading's
contiguous shards, host-staged collectives over torch.distributed gloo).

  * every count (links, overlap numerator and denominator, branch) equals the
    single-process value; the residual and the distance sum are fp64 sums of
    the same T terms in another order (per rank, then over the ranks), so
    they agree within 1e-12 relative in both dtypes;
  * one all-reduce per pass in pmx_comm_stats: two with an overlap branch,
    one without noise;
  * the density branch over two ranks returns PMX_E_BAD_PARAM and issues no
    collective.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import quality_cases as Q  # noqa: E402
from test_gpu_multirank import _free_port, shard_range  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KINDS = [Q.PLANE, Q.POINT, Q.SIM]
FIELDS = ("residual", "overlap_num", "overlap_den", "links", "dist_sum", "branch")


def setup(ctx, rd, ref, nrm, noise_rd, dtype):
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.set_reading_noise(noise_rd)
    ctx.set_reference_descriptors(Q.sensor_noise(ref, 2, dtype), None)
    ctx.match(np.asarray(Q.T_AT, dtype), knn=3)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    ctx.p2plane_system()


def figures(q):
    return np.array([float(getattr(q, f)) for f in FIELDS])


def _worker(rank, world, port, outdir):
    import torch  # noqa: F401  (first: its HIP runtime is the one the library binds to)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from libpointmatcher_amd import _capi

        comm = _capi.gloo_host_comm()
        res = {}
        for dtype in DTYPES:
            dn = np.dtype(dtype).name
            rd, ref, nrm = Q.clouds(130, dtype)
            lo, hi = shard_range(len(rd), world, rank)
            ctx = _capi.Context(0, dtype)
            ctx.comm_init_host(comm)
            setup(ctx, np.ascontiguousarray(rd[lo:hi]), ref, nrm, Q.sensor_noise(rd, 0, dtype)[lo:hi], dtype)
            for kind in KINDS:
                a0 = ctx.comm_stats()[0]
                q = ctx.match_quality(kind)
                res[f"{dn}_{kind}"] = np.concatenate([figures(q), [ctx.comm_stats()[0] - a0]])
            # no noise at all: one pass, one all-reduce
            ctx.set_reading_noise(None)
            ctx.set_reference_descriptors(None, None)
            a0 = ctx.comm_stats()[0]
            q = ctx.match_quality(Q.PLANE)
            res[f"{dn}_plain"] = np.concatenate([figures(q), [ctx.comm_stats()[0] - a0]])
            # the density branch: refused on every rank before any collective
            ctx.set_reading_noise(Q.sensor_noise(rd, 0, dtype)[lo:hi])
            ctx.set_reference_descriptors(Q.sensor_noise(ref, 2, dtype), np.ones(len(ref), dtype))
            a0 = ctx.comm_stats()[0]
            try:
                ctx.match_quality(Q.PLANE)
                refused = ""
            except _capi.InvalidParameter as e:
                refused = str(e)
            res[f"{dn}_refused"] = np.array([float("several ranks" in refused), ctx.comm_stats()[0] - a0])
            assert ctx.match_quality(Q.POINT).branch == Q.READING  # (point-to-point reads no density)
            ctx.close()
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mr_quality")
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
    rd, ref, nrm = Q.clouds(130, dtype)
    noise_rd = Q.sensor_noise(rd, 0, dtype)
    ctx = _capi.Context(0, dtype)
    setup(ctx, rd, ref, nrm, noise_rd, dtype)
    d, ids = ctx.get_matches()
    w = ctx.get_weights()
    p = Q.xform3(np.asarray(Q.T_AT, dtype), rd)
    one = {kind: figures(ctx.match_quality(kind)) for kind in KINDS}
    ctx.set_reading_noise(None)
    ctx.set_reference_descriptors(None, None)
    one["plain"] = figures(ctx.match_quality(Q.PLANE))
    ctx.close()
    # (the fixture keeps point-to-point's links away from the threshold the reduced sum forms)
    assert Q.restate(d, ids, w, p, ref, nrm, dtype, False, noise_rd=noise_rd)["margin"] >= 1e-6
    assert one[Q.PLANE][5] == Q.BOTH and one[Q.POINT][5] == Q.READING and one["plain"][5] == Q.NONE
    assert 0 < one[Q.PLANE][1] < one[Q.PLANE][2] and 0 < one[Q.POINT][1] < one[Q.POINT][2]
    for r in two_ranks:
        for key, passes in [(k, 2) for k in KINDS] + [("plain", 1)]:
            got, want = r[f"{dn}_{key}"], one[key]
            print(f"{dn} {key}: two ranks {got} one {want}")
            assert np.array_equal(got[[1, 2, 3, 5]], want[[1, 2, 3, 5]]), key
            assert Q.rel(got[0], want[0]) <= 1e-12 and Q.rel(got[4], want[4]) <= 1e-12, key
            assert int(got[6]) == passes, key
        assert list(r[f"{dn}_refused"]) == [1.0, 0.0]

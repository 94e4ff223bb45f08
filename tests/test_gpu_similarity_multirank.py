"""PointToPointSimilarityErrorMinimizer over two ranks on the one MI355X
(the pattern of test_gpu_multirank.py: one process per rank, the reading's
contiguous shards, the host-staged collectives over torch.distributed gloo).

  * the sharded similarity ICP equals the single-rank ICP on the whole
    reading: equal iteration counts, every rank the same transform, within
    1e-5 (f32) / 1e-12 (f64);
  * sigma rides in the exchange of the second pass's moments: on the same
    chain and the same number of iterations the similarity ICP issues exactly
    the collectives of PointToPoint's two-pass form (pmx_comm_stats).  The
    workers run with p2p_onepass=0, so that PointToPoint takes its two passes
    in double too (its one-pass form is an option of the rigid minimiser only
    and saves it a collective; similarity always takes two passes).
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from helpers import chain_yaml  # noqa: E402
from test_gpu_multirank import _free_port, shard_range  # noqa: E402
from test_gpu_similarity import BAR, P2P, SIM, TRIM75, clouds, rel, scale_of  # noqa: E402

pytestmark = pytest.mark.gpu

MAXDIST = (("MaxDistOutlierFilter", {"maxDist": 0.2}),)
ITERS = 12
RUNS = [("trim_sim", TRIM75, SIM), ("maxdist_sim", MAXDIST, SIM), ("maxdist_p2p", MAXDIST, P2P)]


def _run(icp_cls, dtype, rd, ref, filters, minimizer, comm=None):
    icp = icp_cls(dtype)
    if comm is not None:
        icp.comm_init_host(comm)
    icp.load_yaml(chain_yaml(filters=filters, minimizer=minimizer, maxit=ITERS))
    c0 = icp.comm_stats() if comm is not None else None
    T = icp.compute(rd, ref)
    s = icp.stats()
    c1 = icp.comm_stats() if comm is not None else None
    icp.close()
    coll = [c1[k] - c0[k] for k in ("allreduces", "allgathers")] if comm is not None else [0, 0]
    return np.concatenate([T.astype(np.float64).ravel(), [s.iterations, s.kept], coll])


def _worker(rank, world, port, outdir):
    os.environ["PMX_OPTS"] = "p2p_onepass=0"
    os.environ["PMX_DEVICE_LOOP"] = "1"
    import torch  # noqa: F401  (first: its bundled HIP runtime is then the one libpmx binds to)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from libpointmatcher_amd import _capi
        from libpointmatcher_amd.icp import ICP

        comm = _capi.gloo_host_comm()
        res = {}
        for dn in ("float32", "float64"):
            dtype = np.dtype(dn)
            rd, ref = clouds(300, dtype, 3)
            lo, hi = shard_range(rd.shape[0], world, rank)
            shard = np.ascontiguousarray(rd[lo:hi])
            for tag, filters, minimizer in RUNS:
                res[f"{dn}_{tag}"] = _run(ICP, dtype, shard, ref, filters, minimizer, comm)
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mr_similarity")
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


@pytest.mark.parametrize("dn", ["float32", "float64"])
def test_sharded_similarity_equals_single_rank(two_ranks, dn, monkeypatch):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    dtype = np.dtype(dn)
    rd, ref = clouds(300, dtype, 3)
    for tag, filters, minimizer in RUNS[:2]:
        a, b = two_ranks[0][f"{dn}_{tag}"], two_ranks[1][f"{dn}_{tag}"]
        np.testing.assert_array_equal(a[:18], b[:18])  # every rank ends with the same transform
        one = _run(ICP, dtype, rd, ref, filters, minimizer)
        err = rel(a[:16], one[:16])
        print(f"{dn} {tag}: iterations {int(a[16])}/{int(one[16])} kept {int(a[17])}/{int(one[17])} |dT|={err:.3g} "
              f"scale {scale_of(a[:16].reshape(4, 4)):.6f}")
        assert int(a[16]) == int(one[16]) == ITERS
        assert int(a[17]) == int(one[17])
        assert err <= BAR[dn]
        assert abs(scale_of(a[:16].reshape(4, 4)) - 1.04) < 0.01


@pytest.mark.parametrize("dn", ["float32", "float64"])
def test_similarity_adds_no_collective(two_ranks, dn):
    for r in two_ranks:
        s, p = r[f"{dn}_maxdist_sim"], r[f"{dn}_maxdist_p2p"]
        print(f"{dn}: similarity {s[18:]} PointToPoint {p[18:]} collectives over {int(s[16])} iterations")
        assert int(s[16]) == int(p[16]) == ITERS
        assert s[18] > 0 and np.array_equal(s[18:], p[18:])

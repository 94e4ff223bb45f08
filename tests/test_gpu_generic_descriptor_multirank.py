"""GenericDescriptorOutlierFilter over two ranks on the one MI355X (the
pattern of test_gpu_similarity_multirank.py: one process per rank, the
reading's contiguous shards, the host-staged collectives over gloo).

The soft form divides by the maximum over the entries of every rank.  The
reading is the reference moved by far less than the point spacing, so reading
point i matches reference point i, and the descriptor is below 0.4 on the
first half of the reference and up to 1 on the second: the global maximum is
matched by rank 1's shard alone, and a rank that divided by its own maximum
would scale rank 0's pairs by 2.5.

  * the sharded ICP equals the single-rank ICP on the whole reading: equal
    iteration counts and kept pairs, every rank the same transform, within
    1e-5 (f32) / 1e-12 (f64);
  * the soft chain issues exactly one more all-reduce per iteration than the
    same chain in hard mode (pmx_comm_stats): the maximum's.  Counted on the
    per-module path, which issues the collectives of the iterations that ran
    and no others; the device loop enqueues whole batches, the iterations past
    the stop included, and each enqueued iteration likewise carries one more.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from helpers import chain_yaml  # noqa: E402
from test_gpu_multirank import _free_port, shard_range  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3000
ITERS = 8
BAR = {"float32": 1e-5, "float64": 1e-12}
NAME = "GenericDescriptorOutlierFilter"
RUNS = {"soft": ((NAME, {"descName": "quality", "useSoftThreshold": 1}),),
        "hard": ((NAME, {"descName": "quality", "threshold": 0.3}),)}


def clouds(dtype):
    from libpointmatcher_amd.synth import reference_cloud
    ref, nrm = reference_cloud(N, dtype)
    c, s = np.cos(0.002), np.sin(0.002)
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [0.002, -0.001, 0.0015]
    rd = (ref.astype(np.float64) @ T.T).astype(dtype)
    rng = np.random.default_rng(5)
    u = rng.uniform(0, 1, N)
    desc = np.where(np.arange(N) < N // 2, 0.2 + 0.2 * u, 0.5 + 0.5 * u).astype(dtype)
    return rd, ref, nrm, desc


def _run(icp_cls, dtype, rd, ref, nrm, desc, filters, comm=None, loop="1"):
    os.environ["PMX_DEVICE_LOOP"] = loop
    icp = icp_cls(dtype)
    if comm is not None:
        icp.comm_init_host(comm)
    icp.load_yaml(chain_yaml(filters=filters, maxit=ITERS))
    icp.add_descriptor("reference", "quality", desc)
    c0 = icp.comm_stats() if comm is not None else None
    T = icp.compute(rd, ref, nrm)
    s = icp.stats()
    c1 = icp.comm_stats() if comm is not None else None
    icp.close()
    coll = [c1[k] - c0[k] for k in ("allreduces", "allgathers")] if comm is not None else [0, 0]
    return np.concatenate([T.astype(np.float64).ravel(), [s.iterations, s.kept], coll])


def _worker(rank, world, port, outdir):
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
            rd, ref, nrm, desc = clouds(np.dtype(dn).type)
            lo, hi = shard_range(rd.shape[0], world, rank)
            shard = np.ascontiguousarray(rd[lo:hi])
            for tag, filters in RUNS.items():
                res[f"{dn}_{tag}"] = _run(ICP, np.dtype(dn), shard, ref, nrm, desc, filters, comm)
                res[f"{dn}_{tag}_modules"] = _run(ICP, np.dtype(dn), shard, ref, nrm, desc, filters, comm, loop="0")
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mr_generic")
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
def test_sharded_soft_chain_equals_single_rank(two_ranks, dn, monkeypatch):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    rd, ref, nrm, desc = clouds(np.dtype(dn).type)
    # the arrangement: at the first match rank 0's pairs see no descriptor above 0.4
    assert desc[:N // 2].max() < 0.4 < 0.99 < desc[N // 2:].max()
    for tag in ("soft", "hard"):
        a, b = two_ranks[0][f"{dn}_{tag}"], two_ranks[1][f"{dn}_{tag}"]
        np.testing.assert_array_equal(a[:18], b[:18])  # every rank ends with the same transform
        one = _run(ICP, np.dtype(dn), rd, ref, nrm, desc, RUNS[tag])
        err = np.linalg.norm(a[:16] - one[:16])
        print(f"{dn} {tag}: iterations {int(a[16])}/{int(one[16])} kept {int(a[17])}/{int(one[17])} |dT|={err:.3g}")
        assert int(a[16]) == int(one[16]) == ITERS
        assert int(a[17]) == int(one[17])
        assert err <= BAR[dn]


@pytest.mark.parametrize("dn", ["float32", "float64"])
def test_soft_adds_one_allreduce_per_iteration(two_ranks, dn):
    for r in two_ranks:
        s, h = r[f"{dn}_soft_modules"], r[f"{dn}_hard_modules"]
        sl, hl = r[f"{dn}_soft"], r[f"{dn}_hard"]
        print(f"{dn}: modules soft {s[18:]} hard {h[18:]}, loop soft {sl[18:]} hard {hl[18:]} collectives over "
              f"{int(s[16])} iterations")
        assert int(s[16]) == int(h[16]) == int(sl[16]) == int(hl[16]) == ITERS
        assert s[18] - h[18] == ITERS and s[19] == h[19]
        # the device loop enqueues whole batches: the hard chain's all-reduces beyond the module
        # path's are its extra enqueued iterations (one system sum each), and each enqueued
        # iteration of the soft chain carries exactly one more
        enqueued = ITERS + (hl[18] - h[18])
        assert sl[18] - hl[18] == enqueued and sl[19] == hl[19]
        np.testing.assert_allclose(s[:16], sl[:16], rtol=0, atol=BAR[dn])

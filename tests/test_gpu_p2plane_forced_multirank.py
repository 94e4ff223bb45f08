"""PointToPlane's force2D / force4DOF over two ranks on the one MI355X (the
pattern of test_gpu_multirank.py: one process per rank, the reading's
contiguous shards, the host-staged collectives over torch.distributed gloo).
The packed forced sums are all-reduced as the unforced ones are: the sharded
ICP equals the single-process ICP on the whole reading, with equal iteration
counts, every rank the same transform, within 1e-5 (f32) / 1e-12 (f64).
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import force_cases as fc  # noqa: E402
import step_cases as sc  # noqa: E402
from helpers import chain_yaml  # noqa: E402
from test_gpu_multirank import _free_port, shard_range  # noqa: E402

pytestmark = pytest.mark.gpu

P2PL = "PointToPlaneErrorMinimizer"
MINIMIZER = {"4DOF": P2PL + ":\n    force4DOF: 1\n", "2D": P2PL + ":\n    force2D: 1\n"}
ITERS = 8


def _run(dtype, rd, ref, nrm, force, comm=None):
    from libpointmatcher_amd.icp import ICP
    icp = ICP(dtype)
    try:
        if comm is not None:
            icp.comm_init_host(comm)
        icp.load_yaml(chain_yaml(minimizer=MINIMIZER[force], maxit=ITERS))
        T = icp.compute(rd, ref, nrm)
        s = icp.stats()
        return np.concatenate([T.astype(np.float64).ravel(), [s.iterations, s.kept]])
    finally:
        icp.close()


def _worker(rank, world, port, outdir):
    os.environ["PMX_DEVICE_LOOP"] = "1"
    import torch  # noqa: F401  (first: its bundled HIP runtime is then the one libpmx binds to)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from libpointmatcher_amd import _capi

        comm = _capi.gloo_host_comm()
        res = {}
        for dn in ("float32", "float64"):
            dtype = np.dtype(dn)
            rd, ref, nrm = fc.scene(dtype)
            lo, hi = shard_range(rd.shape[0], world, rank)
            shard = np.ascontiguousarray(rd[lo:hi])
            for force in fc.FORCES:
                res[f"{dn}_{force}"] = _run(dtype, shard, ref, nrm, force, comm)
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mr_forced")
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
@pytest.mark.parametrize("force", fc.FORCES)
def test_sharded_forced_equals_single_process(two_ranks, monkeypatch, dn, force):
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    dtype = np.dtype(dn)
    rd, ref, nrm = fc.scene(dtype)
    a, b = two_ranks[0][f"{dn}_{force}"], two_ranks[1][f"{dn}_{force}"]
    np.testing.assert_array_equal(a, b)  # every rank ends with the same transform
    one = _run(dtype, rd, ref, nrm, force)
    err = np.linalg.norm(a[:16] - one[:16])
    print(f"{dn} {force}: iterations {int(a[16])}/{int(one[16])} kept {int(a[17])}/{int(one[17])} |dT| = {err:.3g}")
    assert int(a[16]) == int(one[16]) == ITERS
    assert int(a[17]) == int(one[17])
    assert err <= sc.BAR[dn]
    x = fc.step_vector(a[:16].reshape(4, 4), force)
    assert abs(x[0]) > 5e-4  # (the forced step moved)

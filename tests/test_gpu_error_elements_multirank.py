"""pmx_error_elements over two ranks on the one MI355X (the pattern of
test_gpu_quality_multirank.py: one process per rank, the reading's contiguous
shards, host-staged collectives over torch.distributed gloo).

The two shards' columns in rank order, with the shard's first index added to
reading_index, are the single-process columns, exactly; the prepare and the
fetch issue no collective.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import error_elements_cases as E  # noqa: E402
import quality_cases as Q  # noqa: E402
from test_gpu_multirank import _free_port, shard_range  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KEYS = E.FIELDS + ("ref_normals",)


def setup(ctx, rd, ref, nrm, dtype):
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.match(np.asarray(Q.T_AT, dtype), knn=3)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    ctx.p2plane_system()


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
            rd, ref, nrm = Q.clouds(257, dtype)
            lo, hi = shard_range(len(rd), world, rank)
            ctx = _capi.Context(0, dtype)
            ctx.comm_init_host(comm)
            setup(ctx, np.ascontiguousarray(rd[lo:hi]), ref, nrm, dtype)
            c0 = ctx.comm_stats()
            e = ctx.error_elements()
            assert ctx.comm_stats() == c0  # no collective
            for f in KEYS:
                res[f"{dn}_{f}"] = getattr(e, f)
            res[f"{dn}_counts"] = np.array([lo, e.rejected_matches, e.rejected_points])
            ctx.close()
        assert not comm.errors, comm.errors
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mr_elements")
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
def test_two_shards_concatenate_to_one(two_ranks, dtype):
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    rd, ref, nrm = Q.clouds(257, dtype)
    ctx = _capi.Context(0, dtype)
    setup(ctx, rd, ref, nrm, dtype)
    one = ctx.error_elements()
    ctx.close()
    assert 0 < one.columns < 3 * len(rd)
    for f in KEYS:
        parts = [r[f"{dn}_{f}"] + np.int32(r[f"{dn}_counts"][0]) if f == "reading_index" else r[f"{dn}_{f}"]
                 for r in two_ranks]
        got = np.concatenate(parts)
        assert got.dtype == getattr(one, f).dtype, f
        np.testing.assert_array_equal(got, getattr(one, f), err_msg=f)
    assert sum(int(r[f"{dn}_counts"][1]) for r in two_ranks) == one.rejected_matches
    assert sum(int(r[f"{dn}_counts"][2]) for r in two_ranks) == one.rejected_points

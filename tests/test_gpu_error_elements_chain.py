"""errorMinimizer->getErrorElements() through the whole chain on the GPU:
ICP.error_elements() / ICPSequence.error_elements() (pmx_icp_error_elements*).

The same ICP under PMX_DEVICE_LOOP 1 and 0 gives bit-identical columns, and
both equal error_elements_cases.restate applied to a Context driven to the
same last match (the trace's last transform but one).  The descriptors are the
numpy gathers of the test's own clouds by reading_index / ids, the reading's
normals rotated by the match's T_iter (T_refMean_dataIn is a pure translation
here: its rotation is the identity, exact).  All comparisons are exact.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import error_elements_cases as E  # noqa: E402
import quality_cases as Q  # noqa: E402
from helpers import chain_yaml  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DIFF = dict(minDiffRotErr=0.001, minDiffTransErr=0.01, smoothLength=2)
ARRAYS = ("reading", "reference", "dists", "ids", "weights", "reading_index")
N_RD = 1000


def seq_mean(ref, dtype):
    """The reference mean as ICP::compute forms it (ICP.cpp:291-292)."""
    t = np.dtype(dtype).type
    return np.array([np.cumsum(ref[:, r], dtype=dtype)[-1] / t(len(ref)) for r in range(3)], dtype)


def rotate(T, v):
    """The rotation block of T on the rows of v, each component (m0 n0 + m1 n1) + m2 n2 in T's dtype."""
    return np.stack([(T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2] for r in range(3)], 1)


def descriptors(dtype):
    rng = np.random.default_rng(17)
    dummy = rng.normal(0, 1, (N_RD, 2)).astype(dtype)
    v = rng.normal(0, 1, (N_RD, 3))
    rd_nrm = np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), dtype=dtype)
    dens = rng.uniform(1, 2, 1200).astype(dtype)
    return dummy, rd_nrm, dens


def run_icp(dtype, monkeypatch, device_loop):
    from libpointmatcher_amd.icp import ICP
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if device_loop else "0")
    rd, ref, nrm = Q.clouds(N_RD, dtype, centre=False)
    dummy, rd_nrm, dens = descriptors(dtype)
    icp = ICP(dtype)
    icp.load_yaml(chain_yaml(maxit=12, differential=DIFF))
    icp.keep_trace()
    icp.add_descriptor("reading", "dummy", dummy)
    icp.add_descriptor("reading", "normals", rd_nrm)
    icp.add_descriptor("reference", "densities", dens)
    icp.compute(rd, ref, nrm)
    e = icp.error_elements()
    out = dict(e=e, kept=icp.stats().kept, trace=icp.trace(),
               desc={(c, n): e.descriptor(c, n) for c, n in (("reading", "dummy"), ("reading", "normals"),
                                                              ("reference", "normals"), ("reference", "densities"),
                                                              ("reference", "absent"))})
    again = icp.error_elements()  # (cached: the same arrays)
    for f in ARRAYS:
        np.testing.assert_array_equal(getattr(again, f), getattr(e, f))
    icp.close()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_loop_and_modules_equal_restatement(dtype, monkeypatch):
    from libpointmatcher_amd import _capi
    loop = run_icp(dtype, monkeypatch, True)
    mod = run_icp(dtype, monkeypatch, False)
    assert len(loop["trace"]) == len(mod["trace"]) >= 2
    for f in ARRAYS:
        np.testing.assert_array_equal(getattr(loop["e"], f), getattr(mod["e"], f), err_msg=f)
    for k in loop["desc"]:
        np.testing.assert_array_equal(loop["desc"][k], mod["desc"][k], err_msg=str(k))
    # a Context driven to the same last match
    rd, ref, nrm = Q.clouds(N_RD, dtype, centre=False)
    dummy, rd_nrm, dens = descriptors(dtype)
    mean = seq_mean(ref, dtype)
    refc, rdc = ref.copy(), rd.copy()
    refc[:, :3] = ref[:, :3] - mean
    rdc[:, :3] = rd[:, :3] - mean
    T_at = loop["trace"][-2]
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(refc, nrm)
    ctx.set_reading(rdc)
    ctx.match(T_at, knn=1)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    d, ids = ctx.get_matches()
    w = ctx.get_weights()
    ctx.close()
    want = E.restate(d, ids, w, E.step_reading(T_at, rdc), refc, nrm)
    P = len(want["dists"])
    assert 0 < P < d.size
    for tag, r in (("loop", loop), ("modules", mod)):
        e = r["e"]
        assert r["kept"] == P == e.columns, tag
        for f in ARRAYS:
            assert getattr(e, f).dtype == want[f].dtype, (tag, f)
            np.testing.assert_array_equal(getattr(e, f), want[f], err_msg=f"{tag} {f}")
        assert (e.rejected_matches, e.rejected_points) == (want["rejected_matches"], want["rejected_points"]), tag
        assert (e.reading_desc_dim, e.reference_desc_dim) == (5, 4), tag
        ri, ii = want["reading_index"], want["ids"]
        np.testing.assert_array_equal(r["desc"]["reading", "dummy"], dummy[ri])
        np.testing.assert_array_equal(r["desc"]["reading", "normals"], rotate(T_at, rd_nrm)[ri])
        assert not np.array_equal(rotate(T_at, rd_nrm), rd_nrm)
        np.testing.assert_array_equal(r["desc"]["reference", "normals"], nrm[ii])
        np.testing.assert_array_equal(r["desc"]["reference", "densities"], dens[ii][:, None])
        assert r["desc"]["reference", "absent"] is None
        # demo 2 of the reference's advanced-API example: the mean distance of the kept pairs
        qi, s = np.nonzero((d != np.inf) & (w != 0))
        delta = E.step_reading(T_at, rdc)[qi, :3] - refc[ids[qi, s], :3]
        mean_mirrors = np.linalg.norm(delta, axis=1).sum() / len(qi)
        mean_elements = np.linalg.norm(e.reading[:, :3] - e.reference[:, :3], axis=1).sum() / e.columns
        assert mean_elements == mean_mirrors, tag


@pytest.mark.parametrize("dtype", DTYPES)
def test_sequence_and_second_compute(dtype):
    from libpointmatcher_amd.icp import ICPSequence
    rd, ref, nrm = Q.clouds(N_RD, dtype, centre=False)
    refc = ref.copy()
    refc[:, :3] = ref[:, :3] - seq_mean(ref, dtype)
    seq = ICPSequence(dtype)
    seq.load_yaml(chain_yaml(maxit=6, differential=DIFF))
    assert seq.set_map(ref, nrm)
    seq.compute(rd)
    e = seq.error_elements()
    assert e.columns == seq.stats().kept and 0 < e.columns < N_RD
    np.testing.assert_array_equal(e.reference, refc[e.ids])          # columns against the map
    np.testing.assert_array_equal(e.descriptor("reference", "normals"), nrm[e.ids])
    assert (np.diff(e.reading_index) > 0).all() and e.reading_index.max() >= 500
    # a second compute drops the cache
    seq.compute(np.ascontiguousarray(rd[:500]))
    e2 = seq.error_elements()
    assert e2.columns == seq.stats().kept and 0 < e2.columns < 500 and e2.reading_index.max() < 500
    np.testing.assert_array_equal(e2.reference, refc[e2.ids])
    seq.close()

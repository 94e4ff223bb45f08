"""getOverlap / getResidualError through the host chain, and
SimpleSensorNoiseDataPointsFilter (DataPointsFilters/SimpleSensorNoise.cpp:44-136).

CPU part: the filter is in the registry, its five models equal
quality_cases.sensor_noise bit for bit (max / multiply / add in T), the
reference's text for an unknown sensor, and the descriptor follows the points
through a later MaxDistDataPointsFilter.

GPU part: ICP.overlap() and ICP.residual_error() against quality_cases.restate
on the final match, rebuilt at the C ABI from the trace (the way
test_gpu_covariance.py rebuilds its match): the overlap equal to the
restatement's quotient in T, the residual within 1e-5 (f32) / 1e-12 (f64).
Paths: the icp_data config defaultSimpleSensorNoiseDataPointsFilter as it is
(device loop, and PMX_DEVICE_LOOP=0 in a child process), and on the box corner
with staged noise and densities the device loop, the module calls, a reading
step filter and ICPSequence with the noise on the map.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import quality_cases as Q  # noqa: E402
from helpers import chain_yaml, hom, rel_displacement  # noqa: E402
from libpointmatcher_amd.icp import ICP, ICPSequence  # noqa: E402

DTYPES = [np.float32, np.float64]
EMPTY = "Error, last error element empty. Error minimizer needs to be called at least once before using this method."
KAT = "defaultSimpleSensorNoiseDataPointsFilter"


def with_reading_filters(yaml, *filters):
    txt = "readingDataPointsFilters:\n"
    for name, params in filters:
        txt += f"  - {name}:\n" + "".join(f"      {k}: {v}\n" for k, v in params.items())
    return txt + yaml


def cloud100(dtype):
    """Half within 3 m, half within 40 m: every laser model has points on both sides of its floor."""
    rng = np.random.default_rng(11)
    return hom(np.concatenate([rng.uniform(-1.5, 1.5, (50, 3)), rng.uniform(-40, 40, (50, 3))]), dtype)


# ---------------------------------------------------------------- CPU part --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sensor_type", [0, 1, 2, 3, 4])
def test_five_models_equal_restatement(dtype, sensor_type):
    pts = cloud100(dtype)
    icp = ICP(dtype)
    icp.load_yaml(with_reading_filters(chain_yaml(), ("SimpleSensorNoiseDataPointsFilter",
                                                      {"sensorType": sensor_type, "gain": 2})))
    got = icp.filtered_descriptor("reading", pts, "simpleSensorNoise")
    icp.close()
    want = Q.sensor_noise(pts, sensor_type, dtype)
    assert got.shape == (100, 1) and got.dtype == np.dtype(dtype)
    if sensor_type != 3:  # (both arms of the max are taken)
        floor = np.dtype(dtype).type(Q.LASER[sensor_type][0])
        assert 5 < (want == floor).sum() < 95
    assert np.array_equal(got[:, 0], want)


def test_2d_cloud_uses_two_coordinates():
    rng = np.random.default_rng(12)
    pts = hom(rng.uniform(-8, 8, (100, 2)), np.float32)
    icp = ICP(np.float32)
    icp.load_yaml(with_reading_filters(chain_yaml(), ("SimpleSensorNoiseDataPointsFilter", {"sensorType": 0})))
    got = icp.filtered_descriptor("reading", pts, "simpleSensorNoise")
    icp.close()
    assert np.array_equal(got[:, 0], Q.sensor_noise(pts, 0, np.float32))


def test_unknown_sensor_type_has_the_reference_text():
    icp = ICP(np.float32)
    with pytest.raises(Exception) as e:
        icp.load_yaml(with_reading_filters(chain_yaml(), ("SimpleSensorNoiseDataPointsFilter", {"sensorType": 5})))
    assert "SimpleSensorNoiseDataPointsFilter: Error, sensorType id 5 does not exist." in str(e.value)
    with pytest.raises(Exception):  # gain's range is [1, inf)
        icp.load_yaml(with_reading_filters(chain_yaml(), ("SimpleSensorNoiseDataPointsFilter", {"gain": 0.5})))
    icp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_descriptor_survives_max_dist(dtype):
    pts = cloud100(dtype)
    icp = ICP(dtype)
    icp.load_yaml(with_reading_filters(chain_yaml(), ("SimpleSensorNoiseDataPointsFilter", {"sensorType": 2}),
                                       ("MaxDistDataPointsFilter", {"dim": 0, "maxDist": 1.0})))
    got = icp.filtered_descriptor("reading", pts, "simpleSensorNoise")
    assert icp.filtered_descriptor("reading", pts, "normals") is None
    icp.close()
    keep = pts[:, 0] < dtype(1.0)
    assert 10 < keep.sum() < 90
    assert np.array_equal(got[:, 0], Q.sensor_noise(pts, 2, dtype)[keep])


def test_overlap_before_any_compute_raises_the_reference_text():
    icp = ICP(np.float32)
    icp.load_yaml(chain_yaml())
    for call in (icp.overlap, icp.residual_error):
        with pytest.raises(RuntimeError) as e:
            call()
        assert EMPTY in str(e.value)
    icp.close()


# ---------------------------------------------------------------- GPU part --
def seq_mean(ref, dtype):
    """The reference mean as ICP::compute forms it (ICP.cpp:291-292)."""
    t = np.dtype(dtype).type
    return np.array([np.cumsum(ref[:, r], dtype=dtype)[-1] / t(len(ref)) for r in range(3)], dtype)


def restate_final(dtype, rd, ref, nrm, trace, ratio, plane, noise_rd=None, noise_ref=None, dens=None):
    """quality_cases.restate on the last iteration's match: the clouds centred as
    the chain centres them, the match at the trace's transform before the last."""
    from libpointmatcher_amd import _capi
    mean = seq_mean(ref, dtype)
    refc, rdc = ref.copy(), rd.copy()
    refc[:, :3] = ref[:, :3] - mean
    rdc[:, :3] = rd[:, :3] - mean
    T_at = trace[-2] if len(trace) > 1 else np.eye(4, dtype=dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(refc, nrm)
    ctx.set_reading(rdc)
    ctx.match(T_at, knn=1)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=ratio)
    d, ids = ctx.get_matches()
    w = ctx.get_weights()
    ctx.close()
    return Q.restate(d, ids, w, Q.xform3(T_at, rdc), refc, nrm, dtype, plane, noise_rd=noise_rd,
                     noise_ref=noise_ref, dens=dens)


def check(tag, dtype, overlap, residual, stats, want):
    t = np.dtype(dtype).type
    expect = float(t(want["num"]) / t(want["den"])) if want["branch"] else stats.overlap_ratio
    print(f"{tag}: overlap {overlap!r} want {expect!r} ({want['num']}/{want['den']}, branch {want['branch']}) "
          f"residual {residual!r} want {want['residual']!r} links {want['links']} margin {want['margin']:.3g}")
    assert want["margin"] >= 1e-6, tag  # (the fixture)
    assert stats.kept == want["links"], tag
    assert overlap == expect, tag
    assert Q.rel(residual, want["residual"]) <= Q.BAR[np.dtype(dtype).name], tag


def kat_run(golden):
    g, kat = golden
    rd, ref = hom(g["vtk1"], np.float32), hom(g["vtk0"], np.float32)
    icp = ICP(np.float32)
    icp.load_yaml(kat["icp_data_configs"][KAT])
    icp.keep_trace()
    T = icp.compute(rd, ref, None)
    out = dict(T=T, trace=icp.trace(), overlap=icp.overlap(), residual=icp.residual_error(), stats=icp.stats(),
               again=(icp.overlap(), icp.residual_error()),
               nrm=icp.filtered_descriptor("reference", ref, "normals"),
               noise=icp.filtered_descriptor("reading", rd, "simpleSensorNoise"))
    icp.close()
    return out


def _kat_child(q):
    import json
    os.environ["PMX_DEVICE_LOOP"] = "0"
    here = os.path.dirname(os.path.abspath(__file__))
    g = dict(np.load(os.path.join(here, "golden", "clouds.npz")))
    g.update(np.load(os.path.join(here, "golden", "clouds_vtk.npz")))
    with open(os.path.join(here, "golden", "kat.json")) as f:
        kat = json.load(f)
    r = kat_run((g, kat))
    q.put((r["T"], r["overlap"], r["residual"], r["stats"].iterations))


@pytest.mark.gpu
def test_icp_data_config_unchanged_with_overlap_and_residual(golden):
    """utest.cpp:81-160 with the config file as it is, then the two methods."""
    g, kat = golden
    rd, ref = hom(g["vtk1"], np.float32), hom(g["vtk0"], np.float32)
    r = kat_run(golden)
    err = rel_displacement(r["T"], np.array(kat["icp_data_ref_trans"][KAT]), g["vtk1"])
    print(f"{KAT}: rel err {err:.4f}, iterations {r['stats'].iterations}")
    assert err < kat["icp_data_rel_tol"]
    assert r["again"] == (r["overlap"], r["residual"])  # (cached)
    assert r["nrm"].shape == (len(ref), 3) and r["noise"].shape == (len(rd), 1)
    assert np.array_equal(r["noise"][:, 0], Q.sensor_noise(rd, 0, np.float32))
    # the reference carries no noise: point-to-plane's reading-noise branch
    want = restate_final(np.float32, rd, ref, r["nrm"], r["trace"], 0.75, True, noise_rd=r["noise"][:, 0])
    assert want["branch"] == Q.READING
    check(KAT, np.float32, r["overlap"], r["residual"], r["stats"], want)
    assert r["overlap"] != r["stats"].overlap_ratio  # (pmx_icp_stats keeps the weighted used ratio)
    # PMX_DEVICE_LOOP=0 in a child process: the module calls give the same answers
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_kat_child, args=(q,))
    p.start()
    T2, ov2, res2, it2 = q.get(timeout=300)
    p.join(60)
    assert p.exitcode == 0
    assert it2 == r["stats"].iterations and np.array_equal(T2, r["T"])
    assert ov2 == r["overlap"]
    assert Q.rel(res2, r["residual"]) <= Q.BAR["float32"]


STEP_FILTER = "readingStepDataPointsFilters:\n  - IdentityDataPointsFilter\n"
DIFF = dict(minDiffRotErr=0.001, minDiffTransErr=0.01, smoothLength=2)
TRIM = (("TrimmedDistOutlierFilter", {"ratio": 0.85}),)


@pytest.fixture(scope="module")
def box():
    """Per dtype name: the uncentred box-corner clouds with a noise for each
    and the reference's densities (pmx_surface_normals)."""
    from libpointmatcher_amd import _capi
    out = {}
    for dtype in DTYPES:
        rd, ref, nrm = Q.clouds(130, dtype, centre=False)
        dens = _capi.surface_normals(ref, knn=8)["densities"]
        out[np.dtype(dtype).name] = (rd, ref, nrm, Q.sensor_noise(rd, 0, dtype), Q.sensor_noise(ref, 2, dtype), dens)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("minimizer", [Q.PLANE, Q.COV, Q.POINT, Q.SIM])
def test_chain_paths_equal_restatement(box, dtype, minimizer, monkeypatch):
    dn = np.dtype(dtype).name
    rd, ref, nrm, n_rd, n_ref, dens = box[dn]
    plane = minimizer in (Q.PLANE, Q.COV)
    y = chain_yaml(filters=TRIM, minimizer=minimizer, maxit=12, differential=DIFF)
    got = {}
    for path, loop, step in (("loop", "1", False), ("modules", "0", False), ("step_filter", "1", True)):
        monkeypatch.setenv("PMX_DEVICE_LOOP", loop)
        icp = ICP(dtype)
        icp.load_yaml((STEP_FILTER if step else "") + y)
        icp.keep_trace()
        icp.add_descriptor("reading", "simpleSensorNoise", n_rd)
        icp.add_descriptor("reference", "simpleSensorNoise", n_ref)
        icp.add_descriptor("reference", "densities", dens)
        icp.compute(rd, ref, nrm)
        got[path] = dict(overlap=icp.overlap(), residual=icp.residual_error(), stats=icp.stats(), trace=icp.trace())
        icp.close()
    want = restate_final(dtype, rd, ref, nrm, got["loop"]["trace"], 0.85, plane, noise_rd=n_rd, noise_ref=n_ref,
                         dens=dens)
    assert want["branch"] == (Q.DENSITY if plane else Q.READING)
    for path, r in got.items():
        assert len(r["trace"]) == len(got["loop"]["trace"]) > 1
        check(f"{dn} {minimizer} {path}", dtype, r["overlap"], r["residual"], r["stats"], want)
    # without any noise: the weighted used ratio, exactly as before
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    icp = ICP(dtype)
    icp.load_yaml(y)
    icp.compute(rd, ref, nrm)
    assert icp.overlap() == icp.stats().overlap_ratio
    assert Q.rel(icp.residual_error(), want["residual"]) <= Q.BAR[dn]
    icp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_icp_sequence_noise_on_the_map(box, dtype):
    dn = np.dtype(dtype).name
    rd, ref, nrm, n_rd, n_ref, dens = box[dn]
    rd1, _, _ = Q.clouds(65, dtype, centre=False)
    seq = ICPSequence(dtype)
    seq.load_yaml(chain_yaml(filters=TRIM, minimizer=Q.PLANE, maxit=12, differential=DIFF))
    seq.keep_trace()
    seq.add_descriptor("reference", "simpleSensorNoise", n_ref)
    seq.add_descriptor("reference", "densities", dens)
    assert seq.set_map(ref, nrm)
    with pytest.raises(RuntimeError) as e:  # a new map: nothing to ask about yet
        seq.overlap()
    assert EMPTY in str(e.value)
    seq.compute(rd1)
    first = seq.overlap()  # (no reading noise: the reference-noise branch)
    seq.add_descriptor("reading", "simpleSensorNoise", n_rd)
    seq.compute(rd)
    ov, res, st, trace = seq.overlap(), seq.residual_error(), seq.stats(), seq.trace()
    seq.close()
    want = restate_final(dtype, rd, ref, nrm, trace, 0.85, True, noise_rd=n_rd, noise_ref=n_ref, dens=dens)
    assert want["branch"] == Q.DENSITY
    check(f"{dn} sequence", dtype, ov, res, st, want)
    assert 0 <= first <= 1

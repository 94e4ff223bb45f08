"""IncidenceAngle, RemoveSensorBias and Sphericality in the host chain: the
names load from YAML in every filter chain with the reference's parameters
(IncidenceAngle.h:57-59, RemoveSensorBias.h:67-73, Sphericality.h:72-78) and
raise the reference's InvalidField messages — without a GPU — and, on the GPU,
the reference's sensor-bias correction chain runs on a small cloud with the
values of the numpy references of sensor_cases.py.
"""
import numpy as np
import pytest

import sensor_cases as sc
from helpers import hom
from libpointmatcher_amd import icp as I
from libpointmatcher_amd.icp import ICP
from test_keep_filters_chain import TAIL, load, reading_chain

NAMES = [("IncidenceAngleDataPointsFilter", {}),
         ("RemoveSensorBiasDataPointsFilter", {"sensorType": 1, "angleThreshold": 80}),
         ("SphericalityDataPointsFilter", {"keepUnstructureness": 1, "keepStructureness": 1})]


@pytest.mark.parametrize("name,params", NAMES)
@pytest.mark.parametrize("key", ["readingDataPointsFilters", "referenceDataPointsFilters",
                                 "readingStepDataPointsFilters"])
def test_filter_loads_in_every_chain(name, params, key):
    load(reading_chain(name, params, key))
    load(reading_chain(name, params, key), np.float64)
    load(reading_chain(name, {}, key))  # defaults


@pytest.mark.parametrize("name,params,text", [
    ("RemoveSensorBiasDataPointsFilter", {"sensorType": 2}, "larger than maximum admissible value 1"),
    ("RemoveSensorBiasDataPointsFilter", {"sensorType": -1}, "smaller than minimum admissible value 0"),
    ("RemoveSensorBiasDataPointsFilter", {"angleThreshold": 90.5}, "larger than maximum admissible value 90."),
    ("RemoveSensorBiasDataPointsFilter", {"angleThreshold": -1}, "smaller than minimum admissible value 0."),
    ("RemoveSensorBiasDataPointsFilter", {"bogus": 1},
     "Parameter bogus for module RemoveSensorBiasDataPointsFilter was set but is not used"),
    ("SphericalityDataPointsFilter", {"bogus": 1},
     "Parameter bogus for module SphericalityDataPointsFilter was set but is not used"),
    ("IncidenceAngleDataPointsFilter", {"bogus": 1},
     "Parameter bogus was set but module IncidenceAngleDataPointsFilter dos not use any parameter"),
])
def test_parameters_are_the_references(name, params, text):
    with pytest.raises(I.InvalidParameter, match=text):
        load(reading_chain(name, params))


def chain_text(entries, key="readingDataPointsFilters", tail=TAIL):
    body = ""
    for name, params in entries:
        body += f"  - {name}:\n" + "".join(f"      {k}: {v}\n" for k, v in params.items())
    return f"{key}:\n{body}{tail}"


BIAS_CHAIN = [("ObservationDirectionDataPointsFilter", {}),
              ("SurfaceNormalDataPointsFilter", {"knn": 10, "keepEigenValues": 1}),
              ("OrientNormalsDataPointsFilter", {}),
              ("IncidenceAngleDataPointsFilter", {}),
              ("RemoveSensorBiasDataPointsFilter", {"sensorType": 1, "angleThreshold": 75}),
              ("SphericalityDataPointsFilter", {"keepUnstructureness": 1, "keepStructureness": 1})]


def test_bias_correction_chain_loads():
    load(chain_text(BIAS_CHAIN))
    load(chain_text(BIAS_CHAIN, "referenceDataPointsFilters"), np.float64)


def test_missing_descriptors_raise_invalid_field():
    """The checks come before any device work: no GPU needed."""
    pts = np.ones((5, 4), np.float32)
    obs = ("ObservationDirectionDataPointsFilter", {})
    inc = ("IncidenceAngleDataPointsFilter", {})
    for entries, staged, msg in [
        ([inc], {}, "IncidenceAngleDataPointsFilter: Error, cannot find normals in descriptors."),
        ([inc], {"normals": 3},
         "IncidenceAngleDataPointsFilter: Error, cannot find observation directions in descriptors."),
        ([("RemoveSensorBiasDataPointsFilter", {})], {},
         "RemoveSensorBiasDataPointsFilter: Error, cannot find incidence angles in descriptors."),
        ([("RemoveSensorBiasDataPointsFilter", {})], {"incidenceAngles": 1},
         "RemoveSensorBiasDataPointsFilter: Error, cannot find observationDirections in descriptors."),
        ([("SphericalityDataPointsFilter", {})], {},
         "SphericalityDataPointsFilter: Error, no eigValues found in descriptors."),
        ([("SphericalityDataPointsFilter", {})], {"eigValues": 2},
         "SphericalityDataPointsFilter: Error, the number of eigValues is not 3."),
        ([obs, ("SphericalityDataPointsFilter", {})], {"eigValues": 4},
         "SphericalityDataPointsFilter: Error, the number of eigValues is not 3."),
    ]:
        icp = ICP(np.float32)
        try:
            icp.load_yaml(chain_text(entries))
            for name, span in staged.items():
                icp.add_descriptor("reading", name, np.ones((5, span), np.float32))
            with pytest.raises(I.InvalidField) as e:
                icp.filtered_descriptor("reading", pts, "normals")
            assert str(e.value) == msg
        finally:
            icp.close()


# ------------------------------------------------------------ on the device --
def filtered(entries, pts, names, dtype):
    icp = ICP(dtype)
    try:
        icp.load_yaml(chain_text(entries))
        return {k: icp.filtered_descriptor("reading", pts, k) for k in names}
    finally:
        icp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_bias_correction_chain_values(golden, dtype):
    """ObservationDirection -> SurfaceNormal (eigenvalues) -> OrientNormals ->
    IncidenceAngle -> RemoveSensorBias -> Sphericality on 300 points of a
    scan.  Each new stage is compared with its numpy reference applied to the
    descriptors the stages before it left; the corrected points are read back
    through an ObservationDirection appended with the sensor at the origin
    (0 - p, exact).

    Measured on the MI355X: incidence angle 0.167 (float) / 0.125 (double) of
    its bar, corrected points 0.000 of theirs in both types."""
    g, _ = golden
    T = dtype
    pts = hom(g["car400"][::80][:300], T)
    n = len(pts)
    D = 3
    labels = ["observationDirections", "normals", "eigValues", "incidenceAngles", "sphericality", "unstructureness",
              "structureness", "densities", "eigVectors"]
    # up to IncidenceAngle: nothing dropped yet
    pre = filtered(BIAS_CHAIN[:4], pts, labels, T)
    assert [None if pre[k] is None else pre[k].shape for k in labels] == \
        [(n, 3), (n, 3), (n, 3), (n, 1), None, None, None, None, None]
    assert np.array_equal(pre["observationDirections"], -pts[:, :3])
    nrm, obs, inc = pre["normals"], pre["observationDirections"], pre["incidenceAngles"][:, 0]
    dot = sc.incidence_dot(nrm, obs)
    assert np.all(dot >= 0)  # OrientNormals turned them towards the sensor
    ok = np.abs(dot) <= 0.999  # (the bar's condition; the others are left to the unit tests)
    assert ok.sum() > n // 2
    frac = np.abs(inc - sc.incidence_angles(nrm, obs))[ok] / sc.incidence_bar(nrm, obs)[ok]
    print(f"{np.dtype(T).name}: incidence angle {frac.max():.3f} of the bar")
    assert np.all(frac <= 1)

    # the whole chain: labels and spans as the reference leaves them
    out = filtered(BIAS_CHAIN, pts, labels, T)
    thr = sc.angle_threshold(75., T)
    keep = sc.bias_keep(inc, thr)
    m = int(keep.sum())
    assert 0 < m < n
    assert [None if out[k] is None else out[k].shape for k in labels] == \
        [(m, 3), (m, 3), (m, 3), (m, 1), (m, 1), (m, 1), (m, 1), None, None]
    for k in ("observationDirections", "normals", "eigValues", "incidenceAngles"):  # compacted unchanged
        assert np.array_equal(out[k], pre[k][keep]), k
    sph, un, st = sc.sphericality(pre["eigValues"][keep])
    for k, want in (("sphericality", sph), ("unstructureness", un), ("structureness", st)):
        assert np.array_equal(out[k][:, 0], want, equal_nan=True), k

    # the corrected points
    moved = filtered(BIAS_CHAIN + [("ObservationDirectionDataPointsFilter", {})], pts, ["observationDirections"], T)
    got = -moved["observationDirections"]
    desc = np.ascontiguousarray(np.hstack([inc[:, None], obs]))
    want, _, wkeep = sc.remove_sensor_bias(pts, desc, 0, 1, 1, thr)
    assert np.array_equal(wkeep, keep) and got.shape == (m, 3)
    well = (inc[keep] >= 1e-3) & (inc[keep] <= float(thr) - 1e-3)
    assert well.sum() > m // 2
    bar = sc.bias_bar(pts[keep], desc[keep], 0, 1, 1)[:, :D]
    frac = (np.abs(got - want[:, :D]) / bar)[well]
    print(f"{np.dtype(T).name}: corrected points {frac.max():.3f} of the bar, "
          f"largest move {np.abs(want[:, :D] - pts[keep][:, :D]).max():.3g}")
    assert np.all(frac <= 1)
    assert np.abs(want[:, :D] - pts[keep][:, :D]).max() > 1e-4  # the correction is there


STEP_TAIL = """
matcher:
  KDTreeMatcher:
    knn: 1
errorMinimizer:
  PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 5
inspector:
  NullInspector
logger:
  NullLogger
"""


@pytest.mark.gpu
def test_sphericality_as_step_filter(golden, monkeypatch):
    """readingStepDataPointsFilters: Sphericality after a reading SurfaceNormal
    that keeps the eigenvalues: the ICP completes on the device-loop setting
    and with PMX_DEVICE_LOOP=0, with equal transforms."""
    g, _ = golden
    rd = hom(g["car401"][::25], np.float32)
    ref = hom(g["car400"][::25], np.float32)
    text = (chain_text([("SurfaceNormalDataPointsFilter", {"knn": 8, "keepEigenValues": 1})], tail="") +
            chain_text([("SphericalityDataPointsFilter", {"keepStructureness": 1})], "readingStepDataPointsFilters",
                       STEP_TAIL))
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PMX_DEVICE_LOOP", mode)
        icp = ICP(np.float32)
        try:
            icp.load_yaml(text)
            out[mode] = icp.compute(rd, ref)
            assert icp.stats().iterations == 5
        finally:
            icp.close()
    assert np.all(np.isfinite(out["1"])) and np.array_equal(out["1"], out["0"])
    assert not np.array_equal(out["1"], np.eye(4, dtype=np.float32))

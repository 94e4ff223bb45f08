"""NormalSpaceDataPointsFilter in the host chain: the registry knows the name
in each of the three filter lists, its parameters are documented and bounded
like the reference's (DataPointsFilters/NormalSpace.h:63-70), a cloud without
normals raises InvalidField with the reference's text, a 2-D cloud and
nbSample >= n pass through — all without a GPU.  On the GPU a YAML with
SurfaceNormal then NormalSpace as reading filters keeps the columns the literal
program of tests/normal_space_main.cpp keeps, and ICP gives the transform of
the same chain on the cloud subsampled beforehand.
"""
import numpy as np
import pytest

import keep_cases as kc
import normal_space_cases as nc
from libpointmatcher_amd import icp as I
from libpointmatcher_amd.icp import ICP
from libpointmatcher_amd.synth import reading_cloud, reference_cloud
from test_keep_filters_chain import TAIL, load, reading_chain

NAME = "NormalSpaceDataPointsFilter"


@pytest.mark.parametrize("params", [
    {},
    {"nbSample": 1, "seed": 0, "epsilon": 0.04908738521},
    {"nbSample": 4294967295, "seed": 4294967295, "epsilon": 3.14159265359},
])
@pytest.mark.parametrize("key", ["readingDataPointsFilters", "referenceDataPointsFilters",
                                 "readingStepDataPointsFilters"])
def test_filter_loads_in_every_chain(params, key):
    load(reading_chain(NAME, params, key))
    load(reading_chain(NAME, params, key), np.float64)


def test_loads_after_surface_normals():
    text = ("readingDataPointsFilters:\n"
            "  - SurfaceNormalDataPointsFilter:\n      knn: 8\n"
            f"  - {NAME}:\n      nbSample: 100\n" + TAIL)
    load(text)


@pytest.mark.parametrize("params,text", [
    ({"nbSample": 0}, "smaller than minimum admissible value 1"),
    ({"nbSample": 4294967296}, "larger than maximum admissible value 4294967295"),
    ({"seed": 4294967296}, "larger than maximum admissible value 4294967295"),
    ({"epsilon": 0.049}, "smaller than minimum admissible value 0.04908738521"),
    ({"epsilon": 3.1416}, "larger than maximum admissible value 3.14159265359"),
])
def test_parameter_bounds(params, text):
    for dtype in (np.float32, np.float64):
        with pytest.raises(I.InvalidParameter, match=text):
            load(reading_chain(NAME, params), dtype)


def test_unknown_parameter():
    with pytest.raises(I.InvalidParameter, match=f"Parameter bogus for module {NAME} was set but is not used"):
        load(reading_chain(NAME, {"bogus": 1}))


def test_docs_defaults_and_bounds():
    """NormalSpace.h:63-70, as Parametrizable dumps them (Parametrizable.cpp:51-74)."""
    want = ("- nbSample (default: 5000) - Number of point to select. - min: 1 - max: 4294967295\n"
            "- seed (default: 1) - Seed for the random generator. - min: 0 - max: 4294967295\n"
            "- epsilon (default: 0.09817477042) - Step of discretization for the angle spaces - min: 0.04908738521 - "
            "max: 3.14159265359\n")
    for dtype in (np.float32, np.float64):
        assert I.data_points_filter_doc(NAME, dtype) == want


def _filtered(text, pts, name, dtype=np.float32):
    icp = ICP(dtype)
    try:
        icp.load_yaml(text)
        return icp.filtered_descriptor("reading", pts, name)
    finally:
        icp.close()


def test_missing_normals_raise_invalid_field():
    pts = reading_cloud(50, np.float32)
    with pytest.raises(I.InvalidField, match="OrientNormalsDataPointsFilter: Error, cannot find normals in descriptors"):
        _filtered(reading_chain(NAME, {"nbSample": 10}), pts, "normals")


def test_early_exits_come_before_the_normals_check(capfd):
    """NormalSpace.cpp:73-86: a 2-D cloud (with a message) and nbSample >= n
    return before the filter looks for normals; neither draws."""
    kc.srand(3)
    first = kc._libc.rand()
    kc.srand(3)
    pts2 = np.ascontiguousarray(reading_cloud(50, np.float32)[:, [0, 1, 3]])
    assert _filtered(reading_chain(NAME, {"nbSample": 10}), pts2, "normals") is None
    assert "does not support 2D point cloud" in capfd.readouterr().err
    pts = reading_cloud(50, np.float32)
    assert _filtered(reading_chain(NAME, {"nbSample": 50}), pts, "normals") is None
    assert kc._libc.rand() == first


# ----------------------------------------------------------------------- GPU --
CHAIN = """
matcher:
  KDTreeMatcher:
    knn: 1
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.9
errorMinimizer:
  PointToPlaneErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 4
inspector:
  NullInspector
logger:
  NullLogger
"""
NORMALS = "  - SurfaceNormalDataPointsFilter:\n      knn: 8\n"
NSS = f"  - {NAME}:\n      nbSample: 600\n      seed: 5\n      epsilon: 0.19634954084936207\n"
REF = "referenceDataPointsFilters:\n" + NORMALS


@pytest.mark.gpu
def test_yaml_chain_keeps_the_literal_programs_columns(tmp_path):
    prog = nc.Programs(tmp_path, sanitize=False)
    ref, _ = reference_cloud(4000, np.float32)
    rd = reading_cloud(1500, np.float32)
    a, b = ICP(np.float32), ICP(np.float32)
    try:
        a.load_yaml("readingDataPointsFilters:\n" + NORMALS + NSS + REF + CHAIN)
        b.load_yaml("readingDataPointsFilters:\n" + NORMALS + REF + CHAIN)
        full = b.filtered_descriptor("reading", rd, "normals")
        cols, _, next_rand = prog.literal(np.ascontiguousarray(full), 600, 5, 42, 0.19634954084936207)
        kc.srand(42)
        kept = a.filtered_descriptor("reading", rd, "normals")
        assert kc._libc.rand() == next_rand
        assert kept.shape == (600, 3) and kept.tobytes() == full[cols].tobytes()
        kc.srand(42)
        Ta = a.compute(rd, ref)
        Tb = b.compute(np.ascontiguousarray(rd[cols]), ref)
    finally:
        a.close()
        b.close()
    assert np.isfinite(Ta).all() and np.array_equal(Ta, Tb)

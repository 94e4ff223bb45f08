"""The six keep-filters in the host chain, without a GPU: the five icp_data
configurations that name them load, their parameters are bounded like the
reference's (Shadow.h:60-65, MaxQuantileOnAxis.h:56-62, MaxDensity.h:57-62,
MaxPointCount.h:56-63, CutAtDescriptorThreshold.h:62-68; RemoveNaN has none),
they are accepted as step filters, and the two rand()-driven ones — host code
— match the numpy references of keep_cases.py, which a stand-alone C++ program
(keep_rand_main.cpp) pins on the same libc rand() sequence.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import keep_cases as kc
from helpers import TESTS
from libpointmatcher_amd import icp as I
from libpointmatcher_amd.icp import ICP

CONFIGS = ["defaultShadowDataPointsFilter", "defaultMaxDensityDataPointsFilter",
           "defaultMaxQuantileOnAxisDataPointsFilter", "defaultMaxPointCountDataPointsFilter",
           "defaultRemoveNaNDataPointsFilter"]

TAIL = """
matcher:
  KDTreeMatcher:
    knn: 1
errorMinimizer:
  PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 3
inspector:
  NullInspector
logger:
  NullLogger
"""


def reading_chain(name, params=None, key="readingDataPointsFilters"):
    body = f"  - {name}:\n" + "".join(f"      {k}: {v}\n" for k, v in (params or {}).items())
    return f"{key}:\n{body}{TAIL}"


def load(text, dtype=np.float32):
    icp = ICP(dtype)
    try:
        icp.load_yaml(text)
    finally:
        icp.close()


@pytest.mark.parametrize("name", CONFIGS)
def test_icp_data_config_loads(golden, name):
    _, kat = golden
    load(kat["icp_data_configs"][name])


@pytest.mark.parametrize("name,params", [
    ("ShadowDataPointsFilter", {"eps": 0.1}),
    ("MaxQuantileOnAxisDataPointsFilter", {"dim": 2, "ratio": 0.5}),
    ("RemoveNaNDataPointsFilter", {}),
    ("CutAtDescriptorThresholdDataPointsFilter", {"descName": "densities", "useLargerThan": 0, "threshold": -1.5}),
    ("MaxDensityDataPointsFilter", {"maxDensity": 10}),
    ("MaxPointCountDataPointsFilter", {"seed": 3, "maxCount": 100}),
])
@pytest.mark.parametrize("key", ["readingDataPointsFilters", "referenceDataPointsFilters",
                                 "readingStepDataPointsFilters"])
def test_filter_loads_in_every_chain(name, params, key):
    load(reading_chain(name, params, key))
    load(reading_chain(name, params, key), np.float64)


@pytest.mark.parametrize("name,params,text", [
    ("ShadowDataPointsFilter", {"eps": -0.1}, "smaller than minimum admissible value 0.0"),
    ("ShadowDataPointsFilter", {"eps": 3.2}, "larger than maximum admissible value 3.1416"),
    ("MaxQuantileOnAxisDataPointsFilter", {"dim": 3}, "larger than maximum admissible value 2"),
    ("MaxQuantileOnAxisDataPointsFilter", {"ratio": 0}, "smaller than minimum admissible value 0.0000001"),
    ("MaxQuantileOnAxisDataPointsFilter", {"ratio": 1}, "larger than maximum admissible value 0.9999999"),
    ("CutAtDescriptorThresholdDataPointsFilter", {"useLargerThan": 2}, None),
    ("MaxDensityDataPointsFilter", {"maxDensity": 0}, "smaller than minimum admissible value 0.0000001"),
    ("MaxPointCountDataPointsFilter", {"maxCount": 2147483648}, "larger than maximum admissible value 2147483647"),
    ("MaxPointCountDataPointsFilter", {"seed": 2147483648}, "larger than maximum admissible value 2147483647"),
])
def test_parameter_bounds(name, params, text):
    with pytest.raises(I.InvalidParameter, match=text):
        load(reading_chain(name, params))


@pytest.mark.parametrize("name", ["ShadowDataPointsFilter", "MaxQuantileOnAxisDataPointsFilter",
                                  "CutAtDescriptorThresholdDataPointsFilter", "MaxDensityDataPointsFilter",
                                  "MaxPointCountDataPointsFilter"])
def test_unknown_parameter(name):
    with pytest.raises(I.InvalidParameter, match=f"Parameter bogus for module {name} was set but is not used"):
        load(reading_chain(name, {"bogus": 1}))


def test_remove_nan_takes_no_parameter():
    with pytest.raises(I.InvalidParameter,
                       match="Parameter bogus was set but module RemoveNaNDataPointsFilter dos not use any parameter"):
        load(reading_chain("RemoveNaNDataPointsFilter", {"bogus": 1}))


def test_step_chain_of_three_parses():
    text = ("readingStepDataPointsFilters:\n"
            "  - ShadowDataPointsFilter:\n      eps: 0.2\n"
            "  - MaxPointCountDataPointsFilter:\n      maxCount: 50\n"
            "  - RemoveNaNDataPointsFilter:\n" + TAIL)
    load(text)


def test_minimizers_outside_the_scope_stay_unknown():
    for name in ("IdentityErrorMinimizer", "PointToPointWithCovErrorMinimizer"):
        with pytest.raises(I.InvalidElement):
            load(TAIL.replace("PointToPointErrorMinimizer", name))


# --------------------------------------------------------------- host loops --
@pytest.fixture(scope="module")
def keep_rand(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        raise FileNotFoundError("g++")
    exe = str(tmp_path_factory.mktemp("keep_rand") / "keep_rand")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(TESTS, "keep_rand_main.cpp"),
                           "-o", exe])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split()
    return run


def chain_sources(name, params, n, dtype=np.float32, dens=None):
    """Source index of every point the reading chain [name] keeps, read through
    a staged "tag" descriptor that holds each point's index."""
    pts = np.zeros((n, 4), dtype)
    pts[:, 0] = np.arange(n)
    pts[:, 3] = 1
    icp = ICP(dtype)
    try:
        icp.load_yaml(reading_chain(name, params))
        if dens is not None:
            icp.add_descriptor("reading", "densities", np.asarray(dens, dtype))
        icp.add_descriptor("reading", "tag", np.arange(n).astype(dtype))
        tag = icp.filtered_descriptor("reading", pts, "tag")
    finally:
        icp.close()
    return tag[:, 0].astype(int)


MPC_CASES = [(8, 3, 1), (12, 11, 7), (16, 8, 42), (16, 15, 2), (9, 0, 5), (10, 10, 1), (10, 11, 1), (1, 0, 1),
             (1, 1, 1)]


@pytest.mark.parametrize("n,max_count,seed", MPC_CASES)
def test_max_point_count_reference_is_pinned(keep_rand, n, max_count, seed):
    src = kc.max_point_count_sources(n, max_count, seed)
    out = keep_rand("maxpointcount", n, max_count, seed)
    if src is None:
        assert out == ["unchanged"] and max_count > n - 1
    else:
        assert [int(v) for v in out] == list(src)


def test_max_point_count_samples_with_repetition(keep_rand):
    """What the aliasing means: some source column appears twice for a seed
    where a true swap could not produce a repeat."""
    repeats = 0
    for seed in range(1, 20):
        src = kc.max_point_count_sources(16, 15, seed)
        repeats += len(set(src)) < len(src)
    assert repeats > 0


@pytest.mark.parametrize("n,max_count,seed", MPC_CASES)
def test_max_point_count_chain_equals_reference(n, max_count, seed):
    src = kc.max_point_count_sources(n, max_count, seed)
    got = chain_sources("MaxPointCountDataPointsFilter", {"maxCount": max_count, "seed": seed}, n)
    assert list(got) == (list(range(n)) if src is None else list(src))


DENSITY_CASES = [
    (1, 0.3, [0.1, 0.5, 0.2, 0.9, 0.9, 0.4, 0.31, 0.29, 2.0, 0.05]),   # one saturated point of 10: 1 / 10 = 0
    (5, 1.0, [3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0]),               # all saturated: 8 / 8 = 1, ratio 0
    (9, 0.5, [2.0, 0.1, 2.0, 0.7, 2.0, 0.6, 2.0, 0.2, 2.0, 2.0, 0.9, 0.55]),
    (3, 10.0, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]),              # nothing above the limit: no draw
    (11, 0.25, [0.5] * 16),
]


@pytest.mark.parametrize("seed,md,dens", DENSITY_CASES)
def test_max_density_reference_is_pinned(keep_rand, seed, md, dens):
    kc.srand(seed)
    keep = kc.max_density_keep(np.asarray(dens, np.float32), md)
    out = keep_rand("maxdensity", seed, md, *dens)
    assert [int(v) for v in out] == [int(k) for k in keep]


def test_max_density_all_saturated_keeps_none():
    kc.srand(5)
    assert not kc.max_density_keep(np.full(8, 3.0, np.float32), 1.0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("seed,md,dens", DENSITY_CASES)
def test_max_density_chain_equals_reference(seed, md, dens, dtype):
    kc.srand(seed)
    keep = kc.max_density_keep(np.asarray(dens, dtype), md)
    kc.srand(seed)
    got = chain_sources("MaxDensityDataPointsFilter", {"maxDensity": md}, len(dens), dtype, dens=dens)
    assert list(got) == list(np.nonzero(keep)[0])


def test_missing_descriptors_raise_invalid_field():
    pts = np.ones((5, 4), np.float32)
    for name, params, msg in [
        ("MaxDensityDataPointsFilter", {}, "MaxDensityDataPointsFilter: Error, no densities found in descriptors."),
        ("ShadowDataPointsFilter", {}, "ShadowDataPointsFilter, Error: cannot find normals in descriptors"),
        ("CutAtDescriptorThresholdDataPointsFilter", {"descName": "intensity"},
         "CutAtDescriptorThresholdDataPointsFilter: Error, field not found in descriptors."),
    ]:
        icp = ICP(np.float32)
        try:
            icp.load_yaml(reading_chain(name, params))
            with pytest.raises(I.InvalidField) as e:
                icp.filtered_descriptor("reading", pts, "normals")
            assert str(e.value) == msg
        finally:
            icp.close()


"""OctreeGridDataPointsFilter in the host chain, without a GPU: it loads in
each of the three filter lists, documents and bounds its parameters like the
reference (DataPointsFilters/OctreeGrid.h:80-83), and its host side — the
replay of the reference's column swaps and the random sampler's draws
(csrc/common/pmx_octree_replay.h) — built as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer equals the numpy restatement of
octree_cases.py.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import keep_cases as kc
import octree_cases as oc
from helpers import TESTS
from libpointmatcher_amd import icp as I
from test_keep_filters_chain import TAIL, load, reading_chain

ROOT = os.path.dirname(TESTS)
NAME = "OctreeGridDataPointsFilter"


@pytest.mark.parametrize("params", [
    {},
    {"buildParallel": 0, "maxPointByNode": 8, "maxSizeByNode": 0.5, "samplingMethod": 3},
    {"maxPointByNode": 4294967295, "maxSizeByNode": "inf", "samplingMethod": 1},
])
@pytest.mark.parametrize("key", ["readingDataPointsFilters", "referenceDataPointsFilters",
                                 "readingStepDataPointsFilters"])
def test_filter_loads_in_every_chain(params, key):
    load(reading_chain(NAME, params, key))
    load(reading_chain(NAME, params, key), np.float64)


def test_loads_next_to_other_filters():
    text = ("referenceDataPointsFilters:\n"
            f"  - {NAME}:\n      maxPointByNode: 4\n"
            "  - SurfaceNormalDataPointsFilter:\n      knn: 8\n" + TAIL)
    load(text)


@pytest.mark.parametrize("params,text", [
    ({"samplingMethod": 4}, "larger than maximum admissible value 3"),
    ({"samplingMethod": -1}, "smaller than minimum admissible value 0"),
    ({"maxPointByNode": 0}, "smaller than minimum admissible value 1"),
    ({"maxSizeByNode": -0.5}, "smaller than minimum admissible value 0"),
    ({"buildParallel": 2}, None),
])
def test_parameter_bounds(params, text):
    with pytest.raises(I.InvalidParameter, match=text):
        load(reading_chain(NAME, params))


def test_unknown_parameter():
    with pytest.raises(I.InvalidParameter, match=f"Parameter bogus for module {NAME} was set but is not used"):
        load(reading_chain(NAME, {"bogus": 1}))


def test_docs_defaults_and_bounds():
    """OctreeGrid.h:80-83, as Parametrizable dumps them (Parametrizable.cpp:51-74)."""
    want = (
        "- buildParallel (default: 1) - If 1 (true), use threads to build the octree. - min: 0 - max: 1\n"
        "- maxPointByNode (default: 1) - Number of point under which the octree stop dividing. - min: 1 - max: "
        "4294967295\n"
        "- maxSizeByNode (default: 0) - Size of the bounding box under which the octree stop dividing. - min: 0 - "
        "max: +inf\n"
        "- samplingMethod (default: 0) - Method to sample the Octree: First Point (0), Random (1), Centroid (2) (more "
        "accurate but costly), Medoid (3) (more accurate but costly) - min: 0 - max: 3\n")
    for dtype in (np.float32, np.float64):
        assert I.data_points_filter_doc(NAME, dtype) == want
    with pytest.raises(I.InvalidElement):
        I.data_points_filter_doc("NoSuchDataPointsFilter")


# ------------------------------------------------------- host side, sanitized --
@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        raise FileNotFoundError("g++")
    exe = str(tmp_path_factory.mktemp("octree_replay") / "octree_replay")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "libpointmatcher_amd", "csrc"),
                           os.path.join(TESTS, "octree_replay_main.cpp"), "-o", exe])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return [int(v) for v in out.stdout.split()]
    return run


@pytest.mark.parametrize("name,method", [("stale2000", oc.FIRST), ("stale2000", oc.RANDOM), ("presorted", oc.FIRST),
                                         ("tripled", oc.RANDOM), ("uniform1", oc.FIRST), ("lattice_p3", oc.RANDOM)])
def test_replay_under_sanitizers(replay, name, method):
    pts = oc.case(name, np.float32, 3)[0]
    pk = oc.picks(oc.case_leaves(name, "float32", 3), method)
    col, _ = oc.replay_columns(pk, len(pts))
    assert replay("replay", len(pts), *pk) == col


def test_rand_factors_under_sanitizers(replay):
    out = replay("rand", 40)
    kc.srand(1)
    want = [np.float32(np.float32(kc._libc.rand()) / np.float32(kc.RAND_MAX)) for _ in range(40)]
    kc.srand(1)
    first = kc._libc.rand()
    assert [struct.unpack("<f", struct.pack("<I", u))[0] for u in out[:40]] == [float(w) for w in want]
    assert out[40] == first  # srand(1) again at the end

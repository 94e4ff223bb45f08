"""OctreeGridDataPointsFilter on the GPU (pmx_octree_grid, csrc/pmx_octree.hip)
against the numpy restatement of octree_cases.py, bit for bit, on every case
there: float and double, octree and quadtree.

Bars:
  methods 0 (first) and 1 (random): features, descriptors (a 3-row "normals"
    and a 1-row one) and the column order identical to the literal reference —
    the recursion down to its own stop rule, the reference's swapCols / mapidx
    sequence with its stale lookups;
  methods 2 (centroid) and 3 (medoid): identical to the per-leaf form computed
    from the input cloud, and on the cloud already in visit order to the
    literal reference too (no lookup is stale there);
  a method-1 call leaves the process's rand() state as srand(1) does;
  an ICP whose reference filters are OctreeGrid then SurfaceNormal gives the
    normals and the transform of the same chain on the numpy-filtered cloud.
"""
import numpy as np
import pytest

import keep_cases as kc
import octree_cases as oc
from libpointmatcher_amd import _capi
from libpointmatcher_amd.icp import ICP
from libpointmatcher_amd.synth import reading_cloud, reference_cloud

pytestmark = pytest.mark.gpu

DIMS = [3, 2]


def run(name, dtype, dim, method):
    pts, desc, mp, ms = oc.case(name, dtype, dim)
    return _capi.octree_grid(pts, desc, mp, ms, method)


def expect(name, dtype, dim, method, literal):
    pts, desc, mp, ms = oc.case(name, dtype, dim)
    lv = oc.case_leaves(name, np.dtype(dtype).name, dim)
    if literal:
        f, d, _ = oc.literal(pts, desc, lv, method)
        return f, d
    return oc.from_input(pts, desc, lv, method)


def check(got, want, what):
    gf, gd = got
    ef, ed = want
    assert len(gf) == len(ef), f"{what}: {len(gf)} points, the reference keeps {len(ef)}"
    assert oc.same_bits(gf, ef), what + ": features"
    assert oc.same_bits(gd, ed), what + ": descriptors"


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
@pytest.mark.parametrize("method", [oc.FIRST, oc.RANDOM])
def test_first_and_random_equal_the_literal_reference(method, dtype, dim):
    for name in oc.case_names(dim):
        what = f"{name} {np.dtype(dtype).name} dim {dim} method {method}"
        check(run(name, dtype, dim, method), expect(name, dtype, dim, method, True), what)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
@pytest.mark.parametrize("method", [oc.CENTROID, oc.MEDOID])
def test_centroid_and_medoid_equal_the_per_leaf_form(method, dtype, dim):
    for name in oc.case_names(dim):
        what = f"{name} {np.dtype(dtype).name} dim {dim} method {method}"
        check(run(name, dtype, dim, method), expect(name, dtype, dim, method, False), what)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_presorted_cloud_equals_the_literal_reference_for_every_method(dtype, dim):
    for method in range(4):
        pts, desc, mp, ms = oc.case("presorted", dtype, dim)
        lv = oc.case_leaves("presorted", np.dtype(dtype).name, dim)
        f, d, stale = oc.literal(pts, desc, lv, method)
        if method != oc.RANDOM:  # (a random pick inside a leaf may lie below the leaf's number)
            assert stale == 0
        check(run("presorted", dtype, dim, method), (f, d), f"presorted method {method}")


def test_without_descriptors_and_empty():
    pts, _, mp, ms = oc.case("grid257_p3_s0", np.float32, 3)
    lv = oc.case_leaves("grid257_p3_s0", "float32", 3)
    for method in range(4):
        gf, gd = _capi.octree_grid(pts, None, mp, ms, method)
        ef = oc.literal(pts, None, lv, method)[0] if method < 2 else oc.from_input(pts, None, lv, method)[0]
        assert oc.same_bits(gf, ef) and gd.shape == (len(ef), 0)
        gf, gd = _capi.octree_grid(pts[:0], None, mp, ms, method)
        assert gf.shape == (0, 4) and gd.shape == (0, 0)


def test_random_sampler_resets_the_rand_state():
    kc.srand(1)
    first = kc._libc.rand()
    kc.srand(12345)
    kc._libc.rand()
    pts, desc, mp, ms = oc.case("grid257_p3_s0", np.float32, 3)
    _capi.octree_grid(pts, desc, mp, ms, oc.RANDOM)
    assert kc._libc.rand() == first


def test_bad_parameters():
    pts, desc, _, _ = oc.case("uniform63", np.float32, 3)
    for kw in (dict(sampling_method=4), dict(sampling_method=-1), dict(max_point_by_node=0),
               dict(max_size_by_node=-1.0)):
        with pytest.raises(_capi.InvalidParameter):
            _capi.octree_grid(pts, desc, **kw)
    with pytest.raises(_capi.InvalidParameter):
        _capi.octree_grid(np.ones((5, 5), np.float32), None)
    with pytest.raises(_capi.InvalidParameter):  # (the checks hold for an empty cloud too)
        _capi.octree_grid(pts[:0], None, sampling_method=7)


# --------------------------------------------------------------------- chain --
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
OCTREE = "  - OctreeGridDataPointsFilter:\n      maxPointByNode: 6\n      samplingMethod: {}\n"


@pytest.mark.parametrize("method", [oc.FIRST, oc.CENTROID])
def test_chain_equals_the_numpy_filtered_reference(method):
    ref, _ = reference_cloud(4000, np.float32)
    rd = reading_cloud(1500, np.float32)
    lv = oc.leaves(ref, 6, 0.0)
    pre = oc.literal(ref, None, lv, method)[0] if method == oc.FIRST else oc.from_input(ref, None, lv, method)[0]
    assert 0 < len(pre) < len(ref)
    a, b = ICP(np.float32), ICP(np.float32)
    try:
        a.load_yaml("referenceDataPointsFilters:\n" + OCTREE.format(method) + NORMALS + CHAIN)
        b.load_yaml("referenceDataPointsFilters:\n" + NORMALS + CHAIN)
        na = a.filtered_descriptor("reference", ref, "normals")
        nb = b.filtered_descriptor("reference", pre, "normals")
        assert na.shape == (len(pre), 3) and oc.same_bits(na, nb)
        Ta = a.compute(rd, ref)
        Tb = b.compute(rd, pre)
    finally:
        a.close()
        b.close()
    assert np.array_equal(Ta, Tb)

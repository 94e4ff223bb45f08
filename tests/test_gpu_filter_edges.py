"""SurfaceNormal, SamplingSurfaceNormal and VoxelGrid on the GPU
(pmx_normals.hip, pmx_ssn.hip, pmx_voxel.hip through the C ABI) against the
independent references of tests/filter_cases.py: float64 numpy with eigh, a
brute-force kNN judge, the recursive split and the voxel walk restated from
the reference's text.  The scenes, bars and constants are those of
tests/test_filter_reference.py, which runs the oracle through the same
assertions on a CPU, asserts every scene's preconditions and measures the
constants; nothing here depends on the oracle.
"""
import numpy as np
import pytest

import filter_cases as fc
from libpointmatcher_amd import _capi
from libpointmatcher_amd.synth import reference_cloud

pytestmark = pytest.mark.gpu

F = [np.float32, np.float64]
ALL = _capi.SSN_NORMALS | _capi.SSN_DENSITIES | _capi.SSN_EIGVALUES | _capi.SSN_EIGVECTORS


class DeviceBackend:
    def surface_normals(self, pts, k, max_dist):
        return _capi.surface_normals(pts, knn=k, max_dist=max_dist)

    def ssn(self, pts, desc, knn, method, ratio, max_box, average):
        return _capi.sampling_surface_normals(pts, desc, knn=knn, sampling_method=method, ratio=ratio,
                                              max_box_dim=max_box, flags=ALL | (_capi.SSN_AVERAGE if average else 0))

    def voxel(self, pts, desc, vsize, centroid, average):
        return _capi.voxel_grid(pts, desc, vsize, centroid, average)

    def srand(self, seed):
        fc._libc.srand(seed)   # (the library draws from the process's rand())


be = DeviceBackend()
_clouds = {}


def cloud(n, dtype):
    key = (n, np.dtype(dtype))
    if key not in _clouds:
        _clouds[key] = reference_cloud(n, dtype)[0]
        _clouds[key].setflags(write=False)
    return _clouds[key]


# ------------------------------------------------------------ SurfaceNormal --
@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("k", fc.SURFACE_K)
@pytest.mark.parametrize("n", [2000, 4000])
def test_surface(n, k, dtype):
    fc.run_surface(be, cloud(n, dtype), k, undecided_ok=(k == 3))


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plane_exact(axis, dtype):
    fc.run_plane_exact(be, axis, dtype)


@pytest.mark.parametrize("dtype", F)
def test_line_and_duplicates(dtype):
    fc.run_all_degenerate(be, fc.line_scene(300, dtype), 5)
    fc.run_all_degenerate(be, fc.duplicates_scene(dtype), 5)
    fc.run_all_degenerate(be, fc.duplicates_scene(dtype, D=2), 5)


@pytest.mark.parametrize("dtype", F)
def test_cube_lattice(dtype):
    fc.run_cube(be, dtype)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("D", [3, 2])
def test_radius(D, dtype):
    fc.run_radius(be, dtype, D)


@pytest.mark.parametrize("dtype", F)
def test_nan_point(dtype):
    fc.run_nan_point(be, cloud(2000, dtype), 6)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("k", [5, 17])
def test_offset(k, dtype):
    fc.run_surface(be, fc.offset_scene(cloud(2000, np.float64), dtype), k)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("n,k", [(n, 5) for n in fc.SIZES] + [(65, 64)])
def test_sizes(n, k, dtype):
    fc.run_surface(be, cloud(n, dtype), k)
    if k == 5:
        fc.run_all_degenerate(be, fc.line_scene(n, dtype), 5)   # the ballot's count over partly filled waves


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("k", [5, 17])
def test_permuted(k, dtype):
    fc.run_permuted(be, cloud(2000, dtype), k)


@pytest.mark.parametrize("dtype", F)
def test_2d(dtype):
    ring = fc.ring_scene(dtype)
    fc.check_surface_normals(be.surface_normals(ring, 6, np.inf), ring, 6)
    fc.run_wall(be, dtype)
    pts = fc.l_scene(dtype)
    fc.check_surface_normals(be.surface_normals(pts, 5, np.inf), pts, 5, expect="none")


# -------------------------------------------------- SamplingSurfaceNormal --
@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("method,average", [(1, True), (1, False), (0, True), (0, False)])
@pytest.mark.parametrize("tag", fc.SSN_SIZES)
def test_ssn_sizes(tag, method, average, D, dtype):
    n = fc.ssn_size(tag, 7)
    pts = fc.distinct_cloud(n, D, dtype, seed=3)
    desc = np.random.default_rng(9).normal(size=(n, 3)).astype(dtype)
    fc.run_ssn(be, pts, desc, 7, method, average=average, skip_cap=fc.SKIP_CAP)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("method", [0, 1])
def test_ssn_inherited_box(method, dtype):
    fc.run_ssn(be, fc.inherited_box_scene(dtype), None, 7, method)


@pytest.mark.parametrize("dtype", F)
def test_ssn_leaf_edges(dtype):
    for D in (3, 2):
        out, ref, _ = fc.run_ssn(be, fc.box_leaf_scene(16, dtype, D), None, 7, 1, max_box=16 * fc.LATTICE)
        assert len(out["features"]) == 1 and out["unfit"] == 0          # extent == maxBoxDim: kept
        out, ref, _ = fc.run_ssn(be, fc.box_leaf_scene(17, dtype, D), None, 7, 1, max_box=16 * fc.LATTICE)
        assert len(out["features"]) == 0 and out["unfit"] == 6          # one lattice step wider: dropped
        out, ref, _ = fc.run_ssn(be, fc.collinear_leaf_scene(dtype, D), None, 7, 1, fit_by={0: D == 2})
        assert out["unfit"] == (6 if D == 3 else 0)
    out, ref, _ = fc.run_ssn(be, fc.planar_leaf_scene(dtype), None, 7, 1, fit_by={0: True})
    assert len(out["features"]) == 1 and out["unfit"] == 0
    assert np.all(out["eig_values"][:, 0] == 0) and np.all(out["normals"] == np.array([0, 0, 1], dtype))


# ------------------------------------------------------------- VoxelGrid --
@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("centroid,average", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name", fc.VOXEL_NAMES)
def test_voxel(name, centroid, average, dtype):
    fc.run_voxel(be, name, dtype, centroid, average)


def test_zz_device_ratios():
    """(runs last in this file) the device's largest ratios, for the record;
    they set no bar"""
    print("\ndevice ratios vs tests/filter_cases.py:", {k: float(f"{v:.3g}") for k, v in fc.MEASURED.items()})

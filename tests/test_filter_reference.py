"""The oracle's SurfaceNormal, SamplingSurfaceNormal and VoxelGrid
(oracle/pmo_impl.inc) through the assertions of tests/filter_cases.py — the
same scenes and bars as tests/test_gpu_filter_edges.py, on a CPU — and every
scene's preconditions.  The last test prints the largest ratio reached for each
of the bars' constants: this file is where they are measured.
"""
import numpy as np
import pytest

import filter_cases as fc
from libpointmatcher_amd.synth import reference_cloud

F = [np.float32, np.float64]


class OracleBackend:
    def __init__(self, o):
        self.o = o

    def surface_normals(self, pts, k, max_dist):
        return self.o.surface_normals(pts, k=k, max_dist=max_dist, threads=4)

    def ssn(self, pts, desc, knn, method, ratio, max_box, average):
        flags = self.o.SSN_NORMALS | self.o.SSN_DENSITIES | self.o.SSN_EIGVALUES | self.o.SSN_EIGVECTORS
        return self.o.sampling_surface_normals(pts, desc, knn=knn, method=method, ratio=ratio, max_box=max_box,
                                               flags=flags | (self.o.SSN_AVERAGE if average else 0))

    def voxel(self, pts, desc, vsize, centroid, average):
        return self.o.voxel_grid(pts, desc, vsize, centroid, average)

    def srand(self, seed):
        fc._libc.srand(seed)


@pytest.fixture(scope="module")
def be(oracle):
    return OracleBackend(oracle)


def cloud(n, dtype):
    return reference_cloud(n, dtype)[0]


# ------------------------------------------------------------ the references --
def test_references_on_known_answers():
    # rank_ratio ~ l1 / l2 on a thin set, exactly 0 on a lattice line
    rng = np.random.default_rng(0)
    A = rng.normal(size=(9, 3)) * np.array([1.0, 1e-3, 0.0])
    w = np.linalg.eigvalsh(np.cov(A.T, bias=True) * 9)
    assert abs(fc.rank_ratio(A) / (w[1] * w[2] / (w[1] + w[2]) ** 2) - 1) < 1e-9
    for dt in F:
        assert fc.rank_ratio(fc.line_scene(7, dt)[:, :3].astype(np.float64)) == 0.0
        assert fc.degenerate_by_rule(fc.collinear_leaf_scene(dt)[:, :3].astype(np.float64), dt) == (True, True)
    # the kNN judge rejects a wrong row
    pts = cloud(300, np.float32)
    P = pts[:, :3].astype(np.float64)
    ids = np.argsort(((P[:, None] - P[None]) ** 2).sum(-1), axis=1, kind="stable")[:, :4].astype(np.float32)
    fc.knn_judge(pts, ids, 4)
    bad = ids.copy()
    bad[17, 3] = ids[17, 0] + 1 if ids[17, 0] + 1 not in ids[17] else ids[17, 0] + 2
    with pytest.raises(AssertionError):
        fc.knn_judge(pts, bad, 4)
    bad = ids.copy()
    bad[5, [1, 3]] = bad[5, [3, 1]]
    with pytest.raises(AssertionError):
        fc.knn_judge(pts, bad, 4)
    # sequential sums
    x = (np.arange(1, 2001, dtype=np.float32) * np.float32(0.1)).reshape(-1, 1)
    s = np.float32(0)
    for v in x[:, 0]:
        s = np.float32(s + v)
    assert fc.seq_sum(x)[0] == s


def test_scene_preconditions():
    for dt in F:
        for axis in range(3):
            pts = fc.plane_exact(axis, dt)
            others = [a for a in range(3) if a != axis]
            for a in others:
                assert len(np.unique(pts[:, a])) == len(pts), "coordinates distinct per axis"
            assert np.all(pts[:, axis] == pts[0, axis])
        for tag in fc.SSN_SIZES:
            for D in (2, 3):
                pts = fc.distinct_cloud(fc.ssn_size(tag, 7), D, dt, seed=3)
                for a in range(D):
                    assert len(np.unique(pts[:, a])) == len(pts), "coordinates distinct per axis"
        # inherited_box: the tight box would choose other axes
        pts = fc.inherited_box_scene(dt)
        for a in range(3):
            assert len(np.unique(pts[:, a])) == len(pts)
        a = fc.ssn_leaves(pts, 7)
        b = fc.ssn_leaves(pts, 7, tight_boxes=True)
        assert sorted(map(tuple, a)) != sorted(map(tuple, b)), "inherited and tight boxes give the same leaves"
        # the dense voxel: the sequential T sum is not the pairwise one
        pts, desc, vs = fc.voxel_scenes(dt)["dense"]
        inside = np.all((pts[:, :3] >= 0) & (pts[:, :3] < 1), axis=1)
        assert inside.sum() > 1000
        pair = np.array([np.ascontiguousarray(pts[inside][:, a]).sum(dtype=dt) for a in range(3)])  # numpy: pairwise
        assert np.any(fc.seq_sum(pts[inside][:, :3]) != pair)
        # lattice voxel scenes: points exactly on voxel faces
        pts, _, vs = fc.voxel_scenes(dt)["faces"]
        assert np.all(pts[:, :3] / dt(vs[0]) == np.round(pts[:, :3] / dt(vs[0])))
        pts, _, vs = fc.voxel_scenes(dt)["max_bound"]
        assert np.any(np.all(pts[:, :3] == pts[:, :3].max(axis=0), axis=1))


def test_inherited_box_first_cut_disagrees():
    """after the first cut (along x) the right child inherits y-bounds wider
    than its x-extent, while its own points are longer in x"""
    pts = fc.inherited_box_scene(np.float64)
    order = np.lexsort((np.arange(len(pts)), pts[:, 0]))
    right = pts[order[len(pts) - len(pts) // 2:]]
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    assert np.argmax(mx - mn) == 0
    inh = mx - mn
    inh[0] = mx[0] - right[:, 0].min()
    tight = right.max(axis=0) - right.min(axis=0)
    assert np.argmax(inh[:3]) == 1 and np.argmax(tight[:3]) == 0


# ------------------------------------------------------------ SurfaceNormal --
@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("k", fc.SURFACE_K)
@pytest.mark.parametrize("n", [2000, 4000])
def test_surface(be, n, k, dtype):
    fc.run_surface(be, cloud(n, dtype), k, undecided_ok=(k == 3))


@pytest.mark.parametrize("n", [2000, 4000])
def test_surface_skip_share_of_the_clouds(n):
    """the share the gap rule leaves out is a property of the clouds: float64,
    brute-force kNN, no filter in the loop"""
    pts = cloud(n, np.float64)
    P = pts[:, :3]
    order = np.argsort(((P[:, None] - P[None]) ** 2).sum(-1), axis=1, kind="stable")
    for k in fc.SURFACE_K:
        ids = order[:, :k]
        ref = fc.surface_normal_ref(pts, ids, np.ones_like(ids, bool))
        w, tr = ref["w"], ref["trace"]
        skipped = (np.minimum(w[:, 1] - w[:, 0], w[:, 2] - w[:, 1]) < fc.GAP_MIN * tr)
        print(f"N={n} k={k}: the gap rule leaves out {skipped.mean():.4f}")
        assert skipped.mean() <= fc.skip_cap_of(k)
        if k == 3:
            assert skipped.mean() > fc.SKIP_CAP, "k = 3 meets the common cap: drop SKIP_CAP_K3"
            for dt in F:  # sets near the rank threshold, where the filter's own word is taken
                und = sum(not fc.degenerate_by_rule(P[ids[i]].astype(dt).astype(np.float64), dt)[1] for i in range(n))
                print(f"N={n} k=3 {np.dtype(dt).name}: {und} sets within 64x of the rank threshold")
                assert und <= fc.UNDECIDED_CAP_K3 * n


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plane_exact(be, axis, dtype):
    pts = fc.plane_exact(axis, dtype)
    P = pts[:, :3].astype(np.float64)
    ids = np.argsort(((P[:, None] - P[None]) ** 2).sum(-1), axis=1, kind="stable")[:, :5]
    ref = fc.surface_normal_ref(pts, ids, np.ones_like(ids, bool))
    assert np.all(ref["C"][:, axis, :] == 0) and np.all(ref["C"][:, :, axis] == 0), "C's row and column exactly 0"
    fc.run_plane_exact(be, axis, dtype)


@pytest.mark.parametrize("dtype", F)
def test_line_and_duplicates(be, dtype):
    fc.run_all_degenerate(be, fc.line_scene(300, dtype), 5)
    fc.run_all_degenerate(be, fc.duplicates_scene(dtype), 5)
    fc.run_all_degenerate(be, fc.duplicates_scene(dtype, D=2), 5)


@pytest.mark.parametrize("dtype", F)
def test_cube_lattice(be, dtype):
    fc.run_cube(be, dtype)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("D", [3, 2])
def test_radius(be, D, dtype):
    fc.run_radius(be, dtype, D)


@pytest.mark.parametrize("dtype", F)
def test_nan_point(be, dtype):
    fc.run_nan_point(be, cloud(2000, dtype), 6)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("k", [5, 17])
def test_offset(be, k, dtype):
    fc.run_surface(be, fc.offset_scene(cloud(2000, np.float64), dtype), k)


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("n,k", [(n, 5) for n in fc.SIZES] + [(65, 64)])
def test_sizes(be, n, k, dtype):
    fc.run_surface(be, cloud(n, dtype), k)   # (no set near the rank threshold: the count is the reference's)
    if k == 5:
        fc.run_all_degenerate(be, fc.line_scene(n, dtype), 5)   # the count over partly filled waves


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("k", [5, 17])
def test_permuted(be, k, dtype):
    fc.run_permuted(be, cloud(2000, dtype), k)


@pytest.mark.parametrize("dtype", F)
def test_2d(be, dtype):
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
def test_ssn_sizes(be, tag, method, average, D, dtype):
    n = fc.ssn_size(tag, 7)
    pts = fc.distinct_cloud(n, D, dtype, seed=3)
    desc = np.random.default_rng(9).normal(size=(n, 3)).astype(dtype)
    out, ref, share = fc.run_ssn(be, pts, desc, 7, method, average=average, skip_cap=fc.SKIP_CAP)
    assert len(ref["kept"]) > 0


@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("method", [0, 1])
def test_ssn_inherited_box(be, method, dtype):
    pts = fc.inherited_box_scene(dtype)
    out, ref, _ = fc.run_ssn(be, pts, None, 7, method)
    fc._libc.srand(1234)
    tight = fc.ssn_ref(pts, None, 7, method, 0.6, np.inf, True, tight_boxes=True)
    assert not np.array_equal(tight["features"], ref["features"]), "the scene does not tell the boxes apart"
    for st in ref["stats"].values():   # a constructed scene: the gap rule leaves out no leaf
        w = st["w"]
        assert min(w[1] - w[0], w[2] - w[1]) >= fc.GAP_MIN * st["trace"]


@pytest.mark.parametrize("dtype", F)
def test_ssn_leaf_edges(be, dtype):
    for D in (3, 2):
        # extent == maxBoxDim: kept (the test is strict); one lattice step wider: dropped
        out, ref, _ = fc.run_ssn(be, fc.box_leaf_scene(16, dtype, D), None, 7, 1, max_box=16 * fc.LATTICE)
        assert len(ref["kept"]) == 1 and ref["unfit"] == 0
        out, ref, _ = fc.run_ssn(be, fc.box_leaf_scene(17, dtype, D), None, 7, 1, max_box=16 * fc.LATTICE)
        assert len(ref["kept"]) == 0 and ref["unfit"] == 6
        out, ref, _ = fc.run_ssn(be, fc.collinear_leaf_scene(dtype, D), None, 7, 1, fit_by={0: D == 2})
        assert ref["unfit"] == (6 if D == 3 else 0)
    out, ref, _ = fc.run_ssn(be, fc.planar_leaf_scene(dtype), None, 7, 1, fit_by={0: True})
    assert len(ref["kept"]) == 1 and ref["unfit"] == 0
    assert np.all(out["eig_values"][:, 0] == 0) and np.all(out["normals"] == np.array([0, 0, 1], dtype))


# ------------------------------------------------------------- VoxelGrid --
@pytest.mark.parametrize("dtype", F)
@pytest.mark.parametrize("centroid,average", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name", fc.VOXEL_NAMES)
def test_voxel(be, name, centroid, average, dtype):
    rf = fc.run_voxel(be, name, dtype, centroid, average)
    if name in ("one_voxel", "one_point"):
        assert len(rf) == 1


def test_zz_measured_ratios():
    """(runs last in this file) the largest ratios of the oracle against the
    references; the constants are 8x these, rounded up"""
    print("\nmeasured ratios (oracle vs tests/filter_cases.py):",
          {k: float(f"{v:.3g}") for k, v in fc.MEASURED.items()},
          "constants:", dict(K_lambda=fc.K_LAMBDA, K_v=fc.K_V, K_dens=fc.K_DENS, K_md=fc.K_MD))
    assert fc.MEASURED["skip"] <= fc.SKIP_CAP and fc.MEASURED["skip_k3"] <= fc.SKIP_CAP_K3 and \
        fc.MEASURED["skip_ssn"] <= fc.SKIP_CAP

"""The numpy restatement of OctreeGridDataPointsFilter (tests/octree_cases.py)
pinned on what the reference is known to do, without a GPU: its own utest's
expectation, the regular grid under the size limit, the stale column table,
the stalled centre, and the cloud in visit order on which the literal replay
and the per-leaf form agree bit for bit.
"""
import numpy as np
import pytest

import octree_cases as oc

DIMS = [3, 2]


def leaves(name, dtype, dim):
    return oc.case_leaves(name, np.dtype(dtype).name, dim)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_every_case_is_a_partition_in_rising_index(dtype, dim):
    for name in oc.case_names(dim):
        pts = oc.case(name, dtype, dim)[0]
        lv = leaves(name, dtype, dim)
        assert all(len(m) and np.all(np.diff(m) > 0) for m in lv), name
        assert np.array_equal(np.sort(np.concatenate(lv)), np.arange(len(pts))), name


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_distinct_points_are_all_kept(dtype, dim):
    """utest/ui/DataFilters.cpp:468 and following: maxPointByNode 1 and
    maxSizeByNode 0 on distinct points keep every point, whatever the sampler."""
    for name in ("uniform65", "uniform257", "grid5000_p1_s0", "lattice_p1", "collinear"):
        pts, desc, mp, ms = oc.case(name, dtype, dim)
        assert (mp, ms) == (1, 0.0) and len(np.unique(pts, axis=0)) == len(pts)
        lv = leaves(name, dtype, dim)
        assert len(lv) == len(pts), name
        for method in range(4):
            f, d, _ = oc.literal(pts, desc, lv, method)
            assert len(f) == len(pts)
            assert np.array_equal(np.unique(f, axis=0), np.unique(pts, axis=0)), (name, method)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_size_limit_gives_the_regular_grid(dtype, dim):
    """The box of these clouds is exactly [0, 1]^dim, so with maxSizeByNode
    0.25 the descent stops two levels down on cells of edge 1/4, and with
    maxPointByNode 1 every leaf above lies in one such cell: the leaves are
    the occupied cells.  `>` sends a point on a boundary to the lower cell."""
    for name in ("grid257_p1_squarter", "grid5000_p1_squarter", "lattice_quarter"):
        pts, _, mp, ms = oc.case(name, dtype, dim)
        assert (mp, ms) == (1, 0.25)
        cell = np.maximum(np.ceil(pts[:, :dim].astype(np.float64) * 4) - 1, 0).astype(int)
        assert len(leaves(name, dtype, dim)) == len(np.unique(cell, axis=0)), name
    for name in ("grid257_p3_sbox", "grid5000_p5000_sbox"):
        assert len(leaves(name, dtype, dim)) == 1


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_literal_replay_goes_stale(dtype, dim):
    """On the uniform 2 000-point cloud with maxPointByNode 3 the one-level
    table answers with columns that no longer hold the point asked for, and
    the kept columns are not the picks."""
    pts, desc, mp, ms = oc.case("stale2000", dtype, dim)
    lv = leaves("stale2000", dtype, dim)
    pk = oc.picks(lv, oc.FIRST)
    col, stale = oc.replay_columns(pk, len(pts))
    f, d, stale2 = oc.literal(pts, desc, lv, oc.FIRST)
    assert stale > 0 and stale2 == stale
    assert oc.same_bits(f, pts[col]) and oc.same_bits(d, desc[col])  # the integer replay is the literal one
    assert set(col) != set(pk)
    print(f"{np.dtype(dtype).name} dim {dim}: {len(lv)} leaves, {stale} stale lookups, "
          f"{len(set(col) - set(pk))} kept columns that are no leaf's pick")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_presorted_cloud_literal_equals_per_leaf_form(dtype, dim):
    pts, desc, mp, ms = oc.case("presorted", dtype, dim)
    lv = leaves("presorted", dtype, dim)
    assert all(int(m[0]) >= k for k, m in enumerate(lv))  # the table is never consulted
    assert np.array_equal(np.concatenate(lv), np.arange(len(pts)))
    for method in (oc.FIRST, oc.CENTROID, oc.MEDOID):
        f, d, stale = oc.literal(pts, desc, lv, method)
        assert stale == 0
        if method == oc.FIRST:
            ef, ed = pts[oc.picks(lv, method)], desc[oc.picks(lv, method)]
        else:
            ef, ed = oc.from_input(pts, desc, lv, method)
        assert oc.same_bits(f, ef) and oc.same_bits(d, ed), method
    # the random sampler picks inside a leaf, possibly below the leaf's number: literal only
    f, d, _ = oc.literal(pts, desc, lv, oc.RANDOM)
    col, _ = oc.replay_columns(oc.picks(lv, oc.RANDOM), len(pts))
    assert oc.same_bits(f, pts[col]) and oc.same_bits(d, desc[col])


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
def test_deep_cases(dtype, dim):
    eps = np.finfo(dtype).eps
    # more than one key of depth: the neighbours next to 1 separate, far below 21 (31) levels
    pts, _, mp, ms = oc.case("close_pair", dtype, dim)
    lv = leaves("close_pair", dtype, dim)
    assert len(lv) == len(pts)
    depth = oc.depth_reached(pts, mp, ms)
    assert depth > (31 if dtype == np.float32 else 60), depth
    # the stalled centre: distinct points the recursion never separates
    pts, _, mp, ms = oc.case("stalled", dtype, dim)
    lv = leaves("stalled", dtype, dim)
    assert len(np.unique(pts, axis=0)) == len(pts) and len(lv) < len(pts)
    together = [m for m in lv if len(m) > 1]
    assert len(together) == 1 and np.all(np.abs(pts[together[0], 0] - 1) <= 2 * eps)
    # two copies of the origin: down to the underflow of the radius
    pts, _, mp, ms = oc.case("origin_pair", dtype, dim)
    assert [list(m) for m in leaves("origin_pair", dtype, dim)] == [[0], [1, 2], [3]]
    assert oc.depth_reached(pts, mp, ms) > (140 if dtype == np.float32 else 1070)
    # duplicates never separate; an all-identical cloud is one leaf (root radius 0)
    assert sorted(len(m) for m in leaves("tripled", dtype, dim)) == [3] * 100
    assert len(leaves("identical", dtype, dim)) == 1


def test_random_ids_bracket_the_rand_state():
    import keep_cases as kc
    kc.srand(1)
    first = kc._libc.rand()
    kc.srand(77)
    ids = oc.random_ids([np.arange(5), np.arange(1), np.arange(1000)])
    assert kc._libc.rand() == first
    assert ids[1] == 0 and 0 <= ids[0] < 5 and 0 <= ids[2] < 1000

"""NormalSpaceDataPointsFilter without a GPU: the host side the library
compiles in (csrc/common/pmx_nss.h: the bucket of a normal, the shuffle, the
pick loop; csrc/common/pmx_octree_replay.h: the column replay) against the
literal program of tests/normal_space_main.cpp on every case of
normal_space_cases.py, both built as stand-alone programs under
AddressSanitizer and UndefinedBehaviorSanitizer.  The two share no code: the
shared header groups the points by a stable sort and picks over index ranges,
the literal program fills a vector of vectors and erases buckets.  What is left
to the GPU tests is the key kernel, the device sort and the gather.

Also here: std::mt19937's known answer, the reference utest's expectations
(utest/ui/DataFilters.cpp:493-556), and the device's certificate rule
evaluated in numpy fp64: the share of points it sends to the host on the
random-normals cases stays inside the caps the GPU test asserts (1 % float,
0.01 % double).
"""
import math

import numpy as np
import pytest

import keep_cases as kc
import normal_space_cases as nc


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return nc.Programs(tmp_path_factory.mktemp("normal_space"))


def test_mt19937_known_answer(prog):
    assert prog.mt_10000th() == 4123659995


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", list(nc.CASES))
def test_shared_header_equals_the_literal_program(prog, name, dtype):
    _, _, nrm, eps = nc.cloud(name, dtype)
    n = len(nrm)
    for nb in nc.nb_samples(name, n):
        for seed, srand in ((1, 1), (0, 7), (4294967295, 12345)):
            lit, _, lit_rand = prog.literal(nrm, nb, seed, srand, eps)
            sh, _, sh_rand = prog.shared(nrm, nb, seed, srand, eps)
            what = f"{name} {np.dtype(dtype).name} nbSample {nb} seed {seed} srand {srand}"
            assert len(lit) == nb, what
            assert np.array_equal(lit, sh), what
            assert lit_rand == sh_rand, what
            assert len(set(lit.tolist())) == nb and lit.min() >= 0 and lit.max() < n, what  # columns of the input, once
            # n - 1 draws from the process's state
            kc.srand(srand)
            for _ in range(n - 1):
                kc._libc.rand()
            assert kc._libc.rand() == lit_rand, what


def test_the_chosen_case_has_stale_lookups(prog):
    name, _ = nc.STALE_CASE
    for dtype in nc.DTYPES:
        _, _, nrm, eps = nc.cloud(name, dtype)
        _, stale, _ = prog.literal(nrm, len(nrm) - 1, 1, 1, eps)
        assert stale > 0


def test_seed_and_srand_both_matter(prog):
    _, _, nrm, eps = nc.cloud("n257", np.float32)
    a = prog.literal(nrm, 100, 1, 1, eps)[0]
    assert not np.array_equal(a, prog.literal(nrm, 100, 2, 1, eps)[0])
    assert not np.array_equal(a, prog.literal(nrm, 100, 1, 2, eps)[0])


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("eps", [nc.PI6, nc.PI32, nc.PI64])
def test_utest_expectations(prog, eps, dtype):
    """utest/ui/DataFilters.cpp:493-556: nbSample == n leaves the cloud as it
    is (and draws nothing), nbSample < n returns exactly nbSample points."""
    nrm = np.ascontiguousarray(nc.random_unit(400, 21), dtype=dtype)
    for which in ("literal", "shared"):
        cols, _, nxt = prog.filter(which, nrm, 400, 1, 5, eps)
        assert np.array_equal(cols, np.arange(400))
        kc.srand(5)
        assert kc._libc.rand() == nxt
        for nb in (1, 200, 399):
            assert len(prog.filter(which, nrm, nb, 1, 5, eps)[0]) == nb


def test_all_equal_is_the_tail_of_the_shuffle(prog):
    """One bucket: pick k is the k-th element from the end of the shuffle."""
    _, _, nrm, eps = nc.cloud("all_equal", np.float32)
    n = len(nrm)
    kc.srand(9)
    perm = list(range(n))
    for i in range(1, n):
        j = kc._libc.rand() % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    picks = perm[::-1][:100]
    col = list(range(n))
    table = {}
    for k, d in enumerate(picks):
        j = table[d] if d < k else d
        col[k], col[j] = col[j], col[k]
        table[k] = j
    assert prog.literal(nrm, 100, 1, 9, eps)[0].tolist() == col[:100]


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_bucket_grid_of_a_float_epsilon(prog, dtype):
    """The bucket counts come from the T value of epsilon: the keys of the
    literal program stay below cols * rows, and every bucket centre lands in
    its own bucket."""
    for eps in (nc.PI6, nc.PI32):
        cols, rows, nb = nc.bucket_grid(eps, dtype)
        assert cols >= round(2 * math.pi / eps) and rows >= round(math.pi / eps)
        nrm = np.ascontiguousarray(nc.bucket_centres(eps, dtype, 1), dtype=dtype)
        keys = prog.keys(nrm, eps)
        assert keys.max() < nb and len(set(keys.tolist())) == len(keys)
    pole = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]], dtype=dtype)
    assert prog.keys(pole, nc.PI32).tolist() == [0, 0]  # theta == T(pi) wraps to row 0


@pytest.mark.parametrize("dtype,cap", [(np.float32, 1e-2), (np.float64, 1e-4)])
@pytest.mark.parametrize("name", nc.RANDOM_CASES)
def test_certificate_share_on_random_normals(name, dtype, cap):
    _, _, nrm, eps = nc.cloud(name, dtype)
    flagged = nc.certificate(nrm, eps, dtype)
    assert flagged.sum() / len(nrm) <= cap
    # and on a million normals, where the share is a share and not a handful of points
    big = nc.random_unit(1_000_000, 99).astype(dtype)
    assert nc.certificate(big, eps, dtype).mean() <= cap


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_certified_points_agree_with_the_literal_keys(prog, dtype):
    """Where the rule certifies a point, the fp64 bucket is the literal T one
    (numpy's fp64 functions standing in for the device's)."""
    for name in ("n5000_pi64", "edges_pi64", "edges_pi6", "centres_pi32"):
        _, _, nrm, eps = nc.cloud(name, dtype)
        e = float(np.dtype(dtype).type(eps))
        cols, _, _ = nc.bucket_grid(eps, dtype)
        ok = ~nc.certificate(nrm, eps, dtype)
        v = nrm.astype(np.float64)
        theta = np.arccos(v[:, 2])
        phi = np.fmod(np.arctan2(v[:, 1], v[:, 0]) + 2 * math.pi, 2 * math.pi)
        fp64 = (np.floor(theta / e) * cols + np.floor(phi / e)).astype(np.int64)
        lit = prog.keys(nrm, eps)
        assert np.array_equal(fp64[ok], lit[ok]), name
        if name.startswith("edges"):
            assert (~ok).sum() > 0


def test_out_of_range_bucket_search(prog):
    """The theta route the reference's assert guards is closed in both types;
    the search may still find an input through the azimuth.  Whatever it finds
    must be what the literal program calls undefined."""
    for dtype in nc.DTYPES:
        found = nc.find_out_of_range(dtype)
        if found is None:
            continue
        nrm, eps = found
        cloud = np.ascontiguousarray(np.stack([nrm, nrm]), dtype=dtype)
        with pytest.raises(nc.Undefined):
            prog.keys(cloud, eps)

"""NormalSpaceDataPointsFilter on the GPU (pmx_normal_space, csrc/pmx_nss.hip)
against the literal program of tests/normal_space_main.cpp, bit for bit, on
the cases of normal_space_cases.py, float and double.

Bars:
  features, descriptors and n_out identical to the literal program's columns
    on the same input and the same srand state: the buckets, the shuffle, the
    picks, the bucket-erase order, the swap sequence with its stale lookups;
  after the call the process's next rand() is that of a host that drew n - 1
    times;
  on the random-normals cases at most 1 % (float) / 0.01 % (double) of the
    points are evaluated on the host — a condition, so that the test cannot
    pass with every point sent there — and on the edge cases some are;
  the early exits copy the cloud and draw nothing; every documented
    PMX_E_BAD_PARAM is raised.
"""
import ctypes as C

import numpy as np
import pytest

import keep_cases as kc
import normal_space_cases as nc
from libpointmatcher_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return nc.Programs(tmp_path_factory.mktemp("normal_space_gpu"), sanitize=False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(prog, name, dtype, nb, seed=1, srand=1, normals_row=0, extra_after=0):
    pts, desc, nrm, eps = nc.cloud(name, dtype, normals_row, extra_after)
    cols, stale, next_rand = prog.literal(nrm, nb, seed, srand, eps)
    kc.srand(srand)
    gf, gd, rechecked = _capi.normal_space(pts, desc, normals_row, nb, seed, eps)
    after = kc._libc.rand()
    what = f"{name} {np.dtype(dtype).name} nbSample {nb} seed {seed} srand {srand}"
    assert len(gf) == len(cols) == min(nb, len(pts)), what
    assert same_bits(gf, pts[cols]), what + ": features"
    assert same_bits(gd, desc[cols]), what + ": descriptors"
    assert after == next_rand, what + ": the rand() state"
    return rechecked, stale


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", [c for c in nc.CASES if c not in nc.RANDOM_CASES and not c.startswith("edges")])
def test_equals_the_literal_program(prog, name, dtype):
    n = len(nc.cloud(name, dtype)[0])
    for nb in nc.nb_samples(name, n):
        _, stale = check(prog, name, dtype, nb)
        if (name, -1) == nc.STALE_CASE and nb == n - 1:
            assert stale > 0


@pytest.mark.parametrize("dtype,cap", [(np.float32, 1e-2), (np.float64, 1e-4)])
@pytest.mark.parametrize("name", nc.RANDOM_CASES)
def test_random_normals_and_the_recheck_share(prog, name, dtype, cap):
    n = len(nc.cloud(name, dtype)[0])
    for nb in nc.nb_samples(name, n):
        rechecked, _ = check(prog, name, dtype, nb)
        assert rechecked / n <= cap


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", [c for c in nc.CASES if c.startswith("edges")])
def test_edge_normals_are_rechecked_and_still_equal(prog, name, dtype):
    n = len(nc.cloud(name, dtype)[0])
    for nb in nc.nb_samples(name, n):
        rechecked, _ = check(prog, name, dtype, nb)
        assert rechecked > 0


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_seeds_and_srand_states(prog, dtype):
    for seed in (0, 1, 4294967295):
        for srand in (1, 7, 12345):
            check(prog, "n257", dtype, 100, seed, srand)


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_normals_between_other_descriptor_rows(prog, dtype):
    check(prog, "n257", dtype, 128, normals_row=2, extra_after=1)
    check(prog, "edges_pi32", dtype, 150, normals_row=1, extra_after=2)


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_early_exits_copy_the_cloud_and_draw_nothing(dtype):
    pts, desc, _, eps = nc.cloud("n65", dtype)
    kc.srand(3)
    first = kc._libc.rand()
    for p, d, nb in ((pts, desc, 65), (pts, desc, 1000), (pts[:, [0, 1, 3]], desc, 5), (pts[:0], desc[:0], 5)):
        kc.srand(3)
        gf, gd, rechecked = _capi.normal_space(p, d, 0, nb, 1, eps)
        assert kc._libc.rand() == first
        assert same_bits(gf, np.ascontiguousarray(p)) and same_bits(gd, d) and rechecked == 0


def test_bad_parameters():
    pts, desc, _, eps = nc.cloud("n65", np.float32, normals_row=1)
    ok = dict(normals_row=1, nb_sample=10, seed=1, epsilon=eps)
    for kw in (dict(nb_sample=0), dict(nb_sample=-1), dict(epsilon=0.049), dict(epsilon=3.1416), dict(epsilon=0.0),
               dict(epsilon=float("nan")), dict(normals_row=2), dict(normals_row=-1)):
        with pytest.raises(_capi.InvalidParameter):
            _capi.normal_space(pts, desc, **{**ok, **kw})
    with pytest.raises(_capi.InvalidParameter):
        _capi.normal_space(np.ones((5, 5), np.float32), np.ones((5, 3), np.float32), 0, 2)
    # the bounds themselves are admissible, compared in the cloud's type
    for e in (nc.EPS_MIN, nc.EPS_MAX):
        assert len(_capi.normal_space(pts, desc, 1, 10, 1, e)[0]) == 10


def test_more_than_2_31_points_is_refused_before_anything_is_read():
    l = _capi.lib()
    buf = np.zeros(16, np.float32)
    no = C.c_int64(0)
    rc = l.pmx_normal_space(0, _capi.PMX_F32, _capi._ptr(buf), 4, 2 ** 31, _capi._ptr(buf), 3, 0, 1, 1,
                            nc.PI32, _capi._ptr(buf), _capi._ptr(buf), C.byref(no), None)
    assert rc == _capi.PMX_E_BAD_PARAM and b"2^31" in l.pmx_last_error(None)


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_undefined_normals_name_the_first_offending_point(dtype):
    pts, desc, _, eps = nc.cloud("n257", dtype)
    for bad in ([np.nan, 0.0, 0.5], [0.0, np.nan, 0.5], [0.0, 0.0, np.nan], [0.0, 0.0, 1.5], [0.0, 0.0, -1.0000002]):
        d = desc.copy()
        d[200] = bad
        d[77] = bad
        kc.srand(3)
        first = kc._libc.rand()
        kc.srand(3)
        with pytest.raises(_capi.InvalidParameter, match="point 77 "):
            _capi.normal_space(pts, d, 0, 10, 1, eps)
        assert kc._libc.rand() == first  # an error return draws nothing


def test_out_of_range_bucket(prog):
    """A bucket index >= nbBucket, found by the CPU search of
    normal_space_cases.find_out_of_range (float: through the azimuth; double:
    none exists, and the case is dropped there)."""
    found = nc.find_out_of_range(np.float32)
    assert found is not None
    nrm, eps = found
    pts, desc, _, _ = nc.cloud("n257", np.float32)
    d = desc.copy()
    d[123] = nrm
    with pytest.raises(nc.Undefined) as lit:
        prog.literal(np.ascontiguousarray(d), 10, 1, 1, eps)
    assert lit.value.args[0] == 123
    with pytest.raises(_capi.InvalidParameter, match="point 123 .*bucket"):
        _capi.normal_space(pts, d, 0, 10, 1, eps)
    assert nc.find_out_of_range(np.float64) is None

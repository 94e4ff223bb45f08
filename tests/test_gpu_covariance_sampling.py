"""CovarianceSamplingDataPointsFilter on the GPU (pmx_covariance_sampling,
csrc/pmx_covs.hip) on the cases of covariance_sampling_cases.py, float and
double, all three torque norms.

Bars:
  features, descriptors and n_out bit-identical to the columns of the literal
    program (tests/covariance_sampling_main.cpp) when that program is given the
    report's own centre, L and eigvec; the same with a caller-supplied identity
    basis and a random orthonormal basis, whose report's eigvec is that basis
    rounded to T;
  the report's centre and torqueNorm-1 L equal the exact value (the sum taken
    with math.fsum and its exact residual) up to the bound of an fp64 sum of n
    terms in any order, (n - 1) 2^-53 sum|x| / n, plus half an ulp of T for the
    rounding to T; torqueNorm-2 L exactly; cov the exact sum of the same T
    products up to (n - 1) 2^-53 sum|product|;
  in double before rounding, ||cov X - X Lambda||_F <= 1e-12 ||cov||_F and
    ||X^T X - I||_F <= 1e-12 (the project's fp64 bar); the eigenvalues ascend
    and match numpy.linalg.eigvalsh to 1e-12 ||cov||_F.  The vectors are not
    compared with numpy's: the plane case has repeated eigenvalues;
  depth <= nbSample; two calls give identical bytes; the process's next rand()
    after a call is that of a host that drew nothing; the early exits copy the
    cloud even without normals; every documented PMX_E_BAD_PARAM is raised with
    its message;
  one chain run as the reference's utest does (utest/ui/DataFilters.cpp:558-609):
    SurfaceNormal then CovarianceSampling as reading filters, nbSample points
    kept and the final transform within the reference's 3-D tolerance of 0.1
    (utest/utest.h:64-85).
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import covariance_sampling_cases as cc
import keep_cases as kc
from libpointmatcher_amd import _capi
from libpointmatcher_amd.icp import ICP
from libpointmatcher_amd.synth import reading_cloud, reference_cloud, t_gt

pytestmark = pytest.mark.gpu
U = Fraction(1, 2 ** 53)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return cc.Programs(tmp_path_factory.mktemp("covariance_sampling_gpu"), sanitize=False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def exact_sum(x):
    """The sum of the doubles x as a Fraction: fsum is the correctly rounded
    sum, and the fsum of the terms with it subtracted is its residual (exact
    to a further 2^-53 of that residual)."""
    x = [float(a) for a in x]
    s = math.fsum(x)
    return Fraction(s) + Fraction(math.fsum(x + [-s]))


def sum_bound(x, n):
    return (n - 1) * U * exact_sum(np.abs(np.asarray(x, np.float64)))


def half_ulp(value, dtype):
    return Fraction(float(np.spacing(np.dtype(dtype).type(abs(value))))) / 2


def check(prog, name, dtype, tn, nb, basis=None, normals_row=0, extra_after=0):
    pts, desc, nrm = cc.cloud(name, dtype, normals_row, extra_after)
    n = len(pts)
    what = f"{name} {np.dtype(dtype).name} torqueNorm {tn} nbSample {nb}"
    gf, gd, rep = _capi.covariance_sampling(pts, desc, normals_row, nb, tn, basis)
    path = prog.write(pts, nrm, rep["center"], rep["lnorm"], rep["eigvec"])
    cols, depth, stale = prog.literal(path, dtype, n, nb)
    assert len(gf) == len(cols) == nb, what
    assert same_bits(gf, pts[cols]), what + ": features"
    assert same_bits(gd, desc[cols]), what + ": descriptors"
    assert rep["depth"] == depth and 1 <= depth <= nb, what + ": depth"
    return rep, stale


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_equals_the_literal_program_on_its_own_basis(prog, name, dtype):
    n = len(cc.cloud(name, dtype)[0])
    for tn in cc.TORQUE_NORMS:
        for nb in cc.nb_samples(n):
            _, stale = check(prog, name, dtype, tn, nb)
            if name == cc.STALE_CASE and tn == 1 and nb == n - 1:
                assert stale > 0


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_supplied_bases_are_used_as_given(prog, name, dtype):
    n = len(cc.cloud(name, dtype)[0])
    q, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((6, 6)))
    for basis in (np.eye(6), q):
        for tn in cc.TORQUE_NORMS:
            for nb in cc.nb_samples(n):
                rep, _ = check(prog, name, dtype, tn, nb, basis=basis)
                assert same_bits(rep["eigvec"], basis.astype(dtype).astype(np.float64))


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_normals_between_other_descriptor_rows(prog, dtype):
    for tn in cc.TORQUE_NORMS:
        for nb in cc.nb_samples(257):
            check(prog, "n257", dtype, tn, nb, normals_row=2, extra_after=1)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_report_centre_l_and_covariance(name, dtype):
    pts, desc, nrm = cc.cloud(name, dtype)
    n = len(pts)
    dt = np.dtype(dtype).type
    for tn in cc.TORQUE_NORMS:
        rep = _capi.covariance_sampling(pts, desc, 0, 1, tn)[2]
        c = rep["center"]
        for a in range(3):
            x = pts[:, a].astype(np.float64)
            err = abs(Fraction(float(c[a])) - exact_sum(x) / n)
            assert err <= sum_bound(x, n) / n + half_ulp(c[a], dtype), f"{name} centre {a}"
            assert float(dt(c[a])) == c[a]  # a T value
        L = rep["lnorm"]
        if tn == 0:
            assert L == 1.0
        elif tn == 1:
            d = pts[:, :3] - c.astype(dtype)  # in T, as the library forms the terms
            dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)
            err = abs(Fraction(L) - exact_sum(dist) / n)
            assert err <= sum_bound(dist, n) / n + half_ulp(L, dtype), f"{name} Lavg"
        else:
            ext = pts[:, :3].max(axis=0) - pts[:, :3].min(axis=0)  # in T
            assert L == float(ext.max() / dt(2)), f"{name} Lmax"
        v = cc.v_rows(pts, nrm, c, L)
        cov = rep["cov"]
        assert np.array_equal(cov, cov.T)
        for r in range(6):
            for k in range(r, 6):
                prod = (v[:, r] * v[:, k]).astype(np.float64)  # each product in T
                err = abs(Fraction(float(cov[r, k])) - exact_sum(prod))
                assert err <= sum_bound(prod, n), f"{name} cov[{r}, {k}]"


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_defined_basis(prog, name, dtype):
    pts, desc, _ = cc.cloud(name, dtype)
    for tn in cc.TORQUE_NORMS:
        rep = _capi.covariance_sampling(pts, desc, 0, 1, tn)[2]
        cov, w = rep["cov"], rep["eigval"]
        scale = np.linalg.norm(cov)
        assert np.all(np.diff(w) >= 0)
        assert np.abs(w - np.linalg.eigvalsh(cov)).max() <= 1e-12 * scale
        # The report holds the basis after rounding to T.  The basis before
        # rounding is the header's solve of the reported cov, run as a stand-alone
        # program: the fp64 bar is held on it, for float clouds too, and the report
        # must be exactly its rounding.
        pw, X = prog.eigen(cov)
        assert same_bits(pw, w)
        assert same_bits(rep["eigvec"], X.astype(dtype).astype(np.float64))
        assert np.linalg.norm(cov @ X - X * w) <= 1e-12 * scale
        assert np.linalg.norm(X.T @ X - np.eye(6)) <= 1e-12
        for k in range(6):  # the largest component of every vector is positive
            assert X[:, k].max() >= -X[:, k].min() and X[:, k].max() > 0


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_two_calls_give_identical_bytes_and_draw_nothing(dtype):
    pts, desc, _ = cc.cloud("n4099", dtype)
    kc.srand(3)
    first = kc._libc.rand()
    outs = []
    for _ in range(2):
        kc.srand(3)
        gf, gd, rep = _capi.covariance_sampling(pts, desc, 0, 2000, 1)
        assert kc._libc.rand() == first
        outs.append(gf.tobytes() + gd.tobytes() + b"".join(np.asarray(rep[k]).tobytes() for k in sorted(rep)))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_early_exits_copy_the_cloud_even_without_normals(dtype):
    pts, desc, _ = cc.cloud("n65", dtype)
    for p, d, nb in ((pts, desc, 65), (pts, desc, 1000), (pts, None, 65), (pts, desc[:, :2], 70),
                     (pts[:0], desc[:0], 5)):
        gf, gd, rep = _capi.covariance_sampling(p, d, 0, nb, 1)
        assert same_bits(gf, p) and rep["depth"] == 0
        assert gd.shape == (len(p), 0 if d is None else d.shape[1]) and (d is None or same_bits(gd, d))


def test_bad_parameters():
    pts, desc, _ = cc.cloud("n65", np.float32, normals_row=1)
    ok = dict(normals_row=1, nb_sample=10, torque_norm=1)
    for kw, text in ((dict(nb_sample=0), "nbSample must be >= 1"), (dict(nb_sample=-1), "nbSample must be >= 1"),
                     (dict(torque_norm=3), "torqueNorm must be 0"), (dict(torque_norm=-1), "torqueNorm must be 0"),
                     (dict(normals_row=2), "not rows of the descriptors"),
                     (dict(normals_row=-1), "not rows of the descriptors"),
                     (dict(basis=np.full((6, 6), np.nan)), "basis has a non-finite entry"),
                     (dict(basis=np.eye(6) * 1e300), "basis has a non-finite entry")):
        with pytest.raises(_capi.InvalidParameter, match=text):
            _capi.covariance_sampling(pts, desc, **{**ok, **kw})
    with pytest.raises(_capi.InvalidParameter, match="3-D clouds only"):
        _capi.covariance_sampling(np.ascontiguousarray(pts[:, [0, 1, 3]]), desc, **ok)
    with pytest.raises(_capi.InvalidParameter, match="3-D clouds only"):  # before the early exit
        _capi.covariance_sampling(np.ascontiguousarray(pts[:, [0, 1, 3]]), desc, 1, 1000, 1)
    same = np.tile(pts[:1], (65, 1))
    for tn in (1, 2):
        with pytest.raises(_capi.InvalidParameter, match="L = 0"):
            _capi.covariance_sampling(same, desc, 1, 10, tn)
    assert len(_capi.covariance_sampling(same, desc, 1, 10, 0)[0]) == 10


def test_more_than_2_31_points_is_refused_before_anything_is_read():
    l = _capi.lib()
    buf = np.zeros(16, np.float32)
    no = C.c_int64(0)
    rc = l.pmx_covariance_sampling(0, _capi.PMX_F32, _capi._ptr(buf), 4, 2 ** 31, _capi._ptr(buf), 3, 0, 1, 1, None,
                                   _capi._ptr(buf), _capi._ptr(buf), C.byref(no), None)
    assert rc == _capi.PMX_E_BAD_PARAM and b"2^31" in l.pmx_last_error(None)


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_non_finite_points_name_the_first_one(dtype):
    pts, desc, _ = cc.cloud("n4099", dtype)
    for where, bad in (("p", np.nan), ("p", np.inf), ("n", np.nan), ("n", -np.inf)):
        p, d = pts.copy(), desc.copy()
        for i in (3000, 77):
            (p if where == "p" else d)[i, 1] = bad
        with pytest.raises(_capi.InvalidParameter, match="point 77 has a non-finite"):
            _capi.covariance_sampling(p, d, 0, 10, 1)


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
      maxIterationCount: 10
inspector:
  NullInspector
logger:
  NullLogger
"""
NORMALS = "  - SurfaceNormalDataPointsFilter:\n      knn: 5\n"


def test_yaml_chain_as_the_reference_utest_runs_it():
    ref, _ = reference_cloud(4000, np.float32)
    rd = reading_cloud(1500, np.float32)
    for tn in cc.TORQUE_NORMS:
        covs = f"  - CovarianceSamplingDataPointsFilter:\n      nbSample: 500\n      torqueNorm: {tn}\n"
        icp = ICP(np.float32)
        try:
            icp.load_yaml("readingDataPointsFilters:\n" + NORMALS + covs + "referenceDataPointsFilters:\n" + NORMALS +
                          CHAIN)
            kept = icp.filtered_descriptor("reading", rd, "normals")
            T = np.asarray(icp.compute(rd, ref), np.float64)
        finally:
            icp.close()
        assert kept.shape == (500, 3)
        want = t_gt()
        assert abs(np.linalg.norm(want[:3, 3]) - np.linalg.norm(T[:3, 3])) <= 0.1
        cos = (np.trace(want[:3, :3].T @ T[:3, :3]) - 1) / 2
        assert math.acos(min(1.0, max(-1.0, cos))) <= 0.1
        # (the identity is inside that tolerance too: the sampled points must also
        # have moved the reading towards the truth)
        print(f"torqueNorm {tn}: |T - T_gt| {np.linalg.norm(T - want):.3e}, |I - T_gt| "
              f"{np.linalg.norm(np.eye(4) - want):.3e}")
        assert np.linalg.norm(T - want) < np.linalg.norm(np.eye(4) - want)

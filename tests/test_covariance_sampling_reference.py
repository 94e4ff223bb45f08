"""The host side of CovarianceSamplingDataPointsFilter (csrc/common/pmx_covs.h:
the per-point expressions and the pick loop, with pmx_octree_replay.h) against
the literal program of tests/covariance_sampling_main.cpp, on the CPU.  Both
run as stand-alone programs under ASan / UBSan on every case of
covariance_sampling_cases.py, float and double, all three torque norms, with
the centre, L and basis computed in numpy; the identity basis and a permuted
basis are included.

Bars:
  the shared header's kept columns and its depth equal the literal program's;
  depth <= nbSample everywhere (so min(n, nbSample) entries of each list are
    all the picks can reach);
  with the identity basis the columns also equal a numpy / Python restatement
    that shares no code with either program;
  one case is asserted to have stale lookups in the column table;
  the basis the library defines (covs_sym_eigen, in double before any rounding
    to T) meets the project's fp64 bar on the covariance of every case.
"""
import numpy as np
import pytest

import covariance_sampling_cases as cc


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return cc.Programs(tmp_path_factory.mktemp("covariance_sampling"), sanitize=True)


def both(prog, pts, nrm, c, L, X, what):
    n = len(pts)
    path = prog.write(pts, nrm, c, L, X)
    out = {}
    for nb in cc.nb_samples(n):
        cols, depth, stale = prog.literal(path, pts.dtype, n, nb)
        scols, sdepth = prog.shared(path, pts.dtype, n, nb)
        assert len(cols) == nb and len(set(cols.tolist())) == nb, what
        assert np.array_equal(cols, scols), f"{what} nbSample {nb}: columns"
        assert depth == sdepth, f"{what} nbSample {nb}: depth"
        assert 1 <= depth <= nb, f"{what} nbSample {nb}: depth {depth}"
        out[nb] = (cols, depth, stale)
    return out


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_shared_header_equals_the_literal_program(prog, name, dtype):
    pts, _, nrm = cc.cloud(name, dtype)
    n = len(pts)
    for tn in cc.TORQUE_NORMS:
        c, L, X = cc.centre_l_basis(pts, nrm, tn)
        out = both(prog, pts, nrm, c, L, X, f"{name} {np.dtype(dtype).name} torqueNorm {tn}")
        if name == cc.STALE_CASE and tn == 1:
            assert out[n - 1][2] > 0


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_defined_basis_meets_the_fp64_bar(prog, name, dtype):
    """covs_sym_eigen in double, before any rounding to T, on the covariance of
    a float and of a double cloud: ||cov X - X L||_F <= 1e-12 ||cov||_F,
    ||X^T X - I||_F <= 1e-12, eigenvalues ascending and numpy's to the same
    bar, every vector's largest component positive."""
    pts, _, nrm = cc.cloud(name, dtype)
    for tn in cc.TORQUE_NORMS:
        c, L, _ = cc.centre_l_basis(pts, nrm, tn)
        v = cc.v_rows(pts, nrm, c, L).astype(np.float64)
        cov = v.T @ v
        cov = (cov + cov.T) / 2
        w, X = prog.eigen(cov)
        scale = np.linalg.norm(cov)
        assert np.all(np.diff(w) >= 0)
        assert np.abs(w - np.linalg.eigvalsh(cov)).max() <= 1e-12 * scale
        assert np.linalg.norm(cov @ X - X * w) <= 1e-12 * scale
        assert np.linalg.norm(X.T @ X - np.eye(6)) <= 1e-12
        for k in range(6):
            assert X[:, k].max() >= -X[:, k].min() and X[:, k].max() > 0


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_identity_and_permuted_basis(prog, name, dtype):
    pts, _, nrm = cc.cloud(name, dtype)
    n = len(pts)
    c, L, X = cc.centre_l_basis(pts, nrm, 1)
    eye = np.eye(6, dtype=dtype)
    out = both(prog, pts, nrm, c, L, eye, f"{name} {np.dtype(dtype).name} identity")
    for nb, (cols, depth, _) in out.items():
        want, wdepth = cc.numpy_columns(pts, nrm, c, L, nb)
        assert np.array_equal(cols, want), f"{name} nbSample {nb}: numpy"
        assert depth == wdepth
    perm = [3, 0, 5, 1, 4, 2]
    both(prog, pts, nrm, c, L, np.ascontiguousarray(X[:, perm]), f"{name} {np.dtype(dtype).name} permuted")

"""The Transformation modules' parameter functions, which run without a GPU:
checkParameters and correctParameters of RigidTransformation,
SimilarityTransformation and PureTranslation (TransformationsImpl.cpp:89-151,
197-210, 233-269) through icp.Transformation.

The first test is the reference's own (utest/ui/Transformations.cpp:80-131) with
its matrices as data.  correct_parameters is then compared bit for bit with a
numpy restatement in the module's dtype, every operation rounded on its own in
the reference's order.  PureTranslation's check is Eigen's isApprox:
||A - I||_F^2 <= p^2 min(||A||_F^2, ||I||_F^2), p = 1e-5 (float) / 1e-12
(double); it is tested a factor 4 inside and a factor 4 outside the bound, far
from where the order of the norm's sum could matter.
"""
import numpy as np
import pytest

from libpointmatcher_amd import icp as I

DTYPES = [np.float32, np.float64]

# utest/ui/Transformations.cpp:90-93
T_3D_NON_ORTHO = [[0.99935116, 0.13669771, 0.03436585, 1.71138524],
                  [-0.02633967, 0.99326295, -0.04907545, -0.10860933],
                  [-0.03615132, 0.04400287, 0.99820427, -0.04454497],
                  [0., 0., 0., 1.]]
# :108-112
T_2D_NON_ORTHO = [[0.8, -0.5, 0.], [0.5, 0.8, 0.], [0., 0., 1.]]
# :127-128
T_2D_REFLECTION = [[1., 0., 0.], [0., -1., 0.], [0., 0., 1.]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                          b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_unit_test_rigid(dtype):
    rigid = I.Transformation("RigidTransformation", dtype)
    T3 = np.array(T_3D_NON_ORTHO, dtype)
    assert not rigid.check_parameters(T3)
    for _ in range(10):  # stability over iterations
        T3 = rigid.correct_parameters(T3)
        assert rigid.check_parameters(T3)
    T2 = np.array(T_2D_NON_ORTHO, dtype)
    assert not rigid.check_parameters(T2)
    for _ in range(10):
        T2 = rigid.correct_parameters(T2)
        assert rigid.check_parameters(T2)
    with pytest.raises(I.TransformationError, match="only proper rigid transformations are supported"):
        rigid.correct_parameters(np.array(T_2D_REFLECTION, dtype))


# ---- numpy restatements, every operation a scalar of the dtype ----
def normalized(v):
    z = v[0] * v[0]
    z = z + v[1] * v[1]
    z = z + v[2] * v[2]
    if z > 0:
        s = np.sqrt(z)
        return [v[0] / s, v[1] / s, v[2] / s]
    return list(v)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def correct_rigid(P):
    dt = P.dtype.type
    out = P.copy()
    if P.shape[0] == 4:
        c1 = normalized([P[r, 1] for r in range(3)])
        c2 = normalized([P[r, 2] for r in range(3)])
        n0 = cross(c1, c2)
        n1 = cross(c2, n0)
        for r in range(3):
            out[r, 0], out[r, 1], out[r, 2] = n0[r], n1[r], c2[r]
    else:
        a = (P[0, 0] + P[1, 1]) / dt(2)
        b = (-P[1, 0] + P[0, 1]) / dt(2)
        s = np.sqrt(a * a + b * b)
        a, b = a / s, b / s
        out[0, 0], out[0, 1], out[1, 0], out[1, 1] = a, b, -b, a
    return out


def near_rotation(rows, seed, dtype):
    """A rotation (with translation) disturbed by a few 1e-4: inside the 2-D
    form's 0.001 tests, not orthogonal to the last bits."""
    rng = np.random.default_rng(seed)
    T = np.eye(rows)
    if rows == 4:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        T[:3, :3] = q
    else:
        a = rng.uniform(-np.pi, np.pi)
        T[:2, :2] = [[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]  # the reference's [a b; -b a]
    T[:rows - 1, :rows - 1] += rng.uniform(-2e-4, 2e-4, size=(rows - 1, rows - 1))
    T[:rows - 1, rows - 1] = rng.uniform(-5, 5, size=rows - 1)
    return T.astype(dtype)


@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_parameters_bit_equal_to_restatement(dtype, rows):
    rigid = I.Transformation("RigidTransformation", dtype)
    for seed in range(6):
        P = near_rotation(rows, seed, dtype)
        got = rigid.correct_parameters(P)
        want = correct_rigid(P)
        assert got.dtype == np.dtype(dtype)
        assert same_bits(got, want), (seed, got - want)
        assert not same_bits(got, P)  # (the correction did something)
        assert rigid.check_parameters(got)
        # the translation column and the bottom row are the input's
        assert same_bits(got[:, rows - 1], P[:, rows - 1]) and same_bits(got[rows - 1], P[rows - 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_rigid_check_is_the_determinant_bound(dtype):
    rigid = I.Transformation("RigidTransformation", dtype)
    for rows in (3, 4):
        for s, ok in ((1.0, True), (1.0004, True), (1.002, False), (0.998, False)):
            T = np.eye(rows, dtype=dtype)
            T[0, 0] = s  # det R = s
            T[0, rows - 1] = 3
            assert rigid.check_parameters(T) == ok, (rows, s)
    # a reflection has det -1
    assert not rigid.check_parameters(np.diag([1, -1, 1, 1]).astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_similarity_checks_and_corrects_nothing(dtype):
    sim = I.Transformation("SimilarityTransformation", dtype)
    T = (np.arange(16).reshape(4, 4) * 0.37 - 2).astype(dtype)
    assert sim.check_parameters(T)
    assert same_bits(sim.correct_parameters(T), T)
    assert sim.check_parameters(np.array(T_2D_REFLECTION, dtype))


@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pure_translation_check_both_sides_of_isapprox(dtype, rows):
    pt = I.Transformation("PureTranslation", dtype)
    p = 1e-5 if dtype == np.float32 else 1e-12
    T = np.eye(rows, dtype=dtype)
    T[:rows - 1, rows - 1] = [7.5, -3.25, 100.0][:rows - 1]  # (the translation is zeroed before the test)
    assert pt.check_parameters(T)
    # one off-diagonal entry e: ||A - I||_F = e, the bound p sqrt(min(rows + e^2, rows))
    bound = p * np.sqrt(rows)
    for where in ((0, 1), (rows - 1, 0)):  # the left block and the bottom row both count
        inside, outside = T.copy(), T.copy()
        inside[where] = bound / 4
        outside[where] = bound * 4
        assert pt.check_parameters(inside), where
        assert not pt.check_parameters(outside), where
    # a diagonal entry off by e likewise (1 + e is exact enough in both types at 4 x the bound)
    outside = T.copy()
    outside[0, 0] = dtype(1) + dtype(bound * 4)
    assert not pt.check_parameters(outside)
    rot = T.copy()
    rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1] = 0.8, 0.6, -0.6, 0.8
    assert not pt.check_parameters(rot)


@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pure_translation_correct(dtype, rows):
    pt = I.Transformation("PureTranslation", dtype)
    rng = np.random.default_rng(5)
    T = rng.normal(size=(rows, rows)).astype(dtype)
    assert not pt.check_parameters(T)
    got = pt.correct_parameters(T)
    want = np.eye(rows, dtype=dtype)
    want[:rows - 1, rows - 1] = T[:rows - 1, rows - 1]
    assert same_bits(got, want)
    assert pt.check_parameters(got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_registrar_names(dtype):
    for name in ("RigidTransformation", "SimilarityTransformation", "PureTranslation"):
        t = I.Transformation(name, dtype)
        assert t.check_parameters(np.eye(4, dtype=dtype)) and t.check_parameters(np.eye(3, dtype=dtype))
        t.close()
    with pytest.raises(I.InvalidElement, match="NoSuchTransformation"):
        I.Transformation("NoSuchTransformation", dtype)


def test_non_square_parameters_are_invalid():
    rigid = I.Transformation("RigidTransformation")
    with pytest.raises(I.InvalidParameter):
        rigid.check_parameters(np.zeros((3, 4), np.float32))
    with pytest.raises(I.InvalidParameter):
        rigid.correct_parameters(np.eye(5, dtype=np.float32))


def test_compute_without_gpu_fails_loudly():
    from libpointmatcher_amd import _capi
    if _capi.device_count() > 0:
        pytest.skip("GPU present")
    rigid = I.Transformation("RigidTransformation")
    with pytest.raises(RuntimeError, match="no HIP device"):
        rigid.compute(np.ones((5, 4), np.float32), np.eye(4, dtype=np.float32))

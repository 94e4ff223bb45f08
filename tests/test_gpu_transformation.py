"""Transformation::compute on the GPU (pmx_transform_cloud, csrc/pmx_transform.hip)
through icp.Transformation and _capi.transform_cloud.

The bar is bit equality with a numpy restatement of the contract in np.float32 /
np.float64: every feature row r is ((P_r0 x + P_r1 y) + P_r2 z) + P_r3 h (2-D:
(P_r0 x + P_r1 y) + P_r2 h), every rotated span row the same sequential sum over
the rotation block, each multiply and add a separate numpy operation (numpy
fuses nothing), no `@`.  Descriptor rows outside the rotated spans must come out
with the input's bits.  NaNs compare by position, everything else by bit pattern
(so the sign of a zero counts).

Sizes: 0 (empty), 1, 63 / 64 / 65 (the wave edge), 257 (one block and a tail of
one), 4099 (17 blocks, odd).
"""
import numpy as np
import pytest

from helpers import chain_yaml
from libpointmatcher_amd import _capi
from libpointmatcher_amd import icp as I
from libpointmatcher_amd.synth import reading_cloud, reference_cloud

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SIZES = [0, 1, 63, 64, 65, 257, 4099]

# utest/ui/Transformations.cpp:90-93
T_3D_NON_ORTHO = [[0.99935116, 0.13669771, 0.03436585, 1.71138524],
                  [-0.02633967, 0.99326295, -0.04907545, -0.10860933],
                  [-0.03615132, 0.04400287, 0.99820427, -0.04454497],
                  [0., 0., 0., 1.]]


def same_values(a, b):
    """Equal bit for bit (signed zeros included), any NaN for a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(u), np.where(nb, 0, b).view(u))


# ---- the contract restated ----
def features_ref(F, P):
    rows = F.shape[1]
    out = np.empty_like(F)
    with np.errstate(all="ignore"):
        for r in range(rows):
            acc = P[r, 0] * F[:, 0]
            for c in range(1, rows):
                acc = acc + P[r, c] * F[:, c]
            out[:, r] = acc
    return out


def descriptors_ref(Dsc, P, labels, rotate=True):
    D = P.shape[0] - 1
    out = Dsc.copy()
    off = 0
    with np.errstate(all="ignore"):
        for name, span in labels:
            if rotate and name in ("normals", "observationDirections"):
                for r in range(D):
                    acc = P[r, 0] * Dsc[:, off]
                    for c in range(1, D):
                        acc = acc + P[r, c] * Dsc[:, off + c]
                    out[:, off + r] = acc
            off += span
    return out


# ---- parameters ----
def rotation(D, seed):
    rng = np.random.default_rng(seed)
    if D == 3:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        return q
    a = rng.uniform(-np.pi, np.pi)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def params(kind, D, dtype):
    """(transformation name, rows x rows parameters)"""
    rows = D + 1
    T = np.eye(rows)
    rng = np.random.default_rng(40 + D)
    if kind == "rigid":  # a rotation with translation
        T[:D, :D] = rotation(D, 7)
        T[:D, D] = rng.uniform(-3, 3, size=D)
        return "RigidTransformation", T.astype(dtype)
    if kind == "similarity":  # scale 1.04
        T[:D, :D] = 1.04 * rotation(D, 8)
        T[:D, D] = rng.uniform(-3, 3, size=D)
        return "SimilarityTransformation", T.astype(dtype)
    # a general affine matrix: the bottom row is not 0 .. 0 1, so the homogeneous output row is computed
    T = rng.uniform(-1.5, 1.5, size=(rows, rows))
    return "SimilarityTransformation", T.astype(dtype)


KINDS = ["rigid", "similarity", "affine"]


# ---- clouds ----
def layouts(D):
    return {
        "none": [],
        "normals": [("normals", D)],
        "mixed": [("intensity", 1), ("normals", D), ("extra", 4), ("observationDirections", D), ("tail", 2)],
        "wide": [("filler", 40 - D), ("normals", D)],  # a 40-row descriptor, the span last
    }


def cloud(n, D, dtype, labels, seed=0):
    rng = np.random.default_rng(1000 * D + n + seed)
    F = np.hstack([rng.uniform(-20, 20, size=(n, D)), np.ones((n, 1))]).astype(dtype)
    dd = sum(span for _, span in labels)
    Dsc = rng.normal(size=(n, dd)).astype(dtype) if dd else None
    return F, Dsc


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_bit_equal_to_restatement(dtype, D, n):
    for kind in KINDS:
        name, P = params(kind, D, dtype)
        tr = I.Transformation(name, dtype)
        for lname, labels in layouts(D).items():
            F, Dsc = cloud(n, D, dtype, labels)
            F0, D0 = F.copy(), None if Dsc is None else Dsc.copy()
            of, od = tr.compute(F, P, Dsc, labels)
            assert of.shape == F.shape and of.dtype == np.dtype(dtype)
            assert same_values(of, features_ref(F0, P)), (kind, lname)
            if Dsc is None:
                assert od is None
            else:
                want = descriptors_ref(D0, P, labels)
                assert same_values(od, want), (kind, lname)
                # stated on its own: the pass-through rows have the input's bits, the spans were rotated
                off = 0
                for label, span in labels:
                    if label in ("normals", "observationDirections"):
                        if n:
                            assert not same_values(od[:, off:off + span], D0[:, off:off + span]), (kind, lname, label)
                    else:
                        assert same_values(od[:, off:off + span], D0[:, off:off + span]), (kind, lname, label)
                    off += span
            # the inputs are left as they were
            assert same_values(F, F0) and (Dsc is None or same_values(Dsc, D0))
        tr.close()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cloud_in_cloud_out(dtype, D):
    labels = layouts(D)["mixed"]
    F, Dsc = cloud(257, D, dtype, labels)
    fl = [(c, 1) for c in "xyz"[:D]] + [("pad", 1)]
    c = I.Cloud(F.copy(), fl, Dsc.copy(), list(labels))
    name, P = params("rigid", D, dtype)
    out = I.Transformation(name, dtype).compute(c, P)
    assert isinstance(out, I.Cloud) and out is not c
    assert out.feature_labels == fl and out.descriptor_labels == list(labels)
    assert same_values(out.features, features_ref(F, P))
    assert same_values(out.descriptors, descriptors_ref(Dsc, P, labels))
    assert same_values(out.descriptor("normals"), descriptors_ref(Dsc, P, labels)[:, 1:1 + D])
    assert same_values(c.features, F) and same_values(c.descriptors, Dsc)
    # a cloud without descriptors
    bare = I.Transformation(name, dtype).compute(I.Cloud(F.copy(), fl, np.empty((257, 0), dtype), []), P)
    assert bare.descriptors.shape == (257, 0) and same_values(bare.features, features_ref(F, P))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_and_signed_zero_points(dtype, D):
    """NaN, +-inf and -0.0 go through the expression like any other value:
    inf * 0 and inf - inf give NaN where the restatement gives it, and a sum of
    negative zeros stays negative."""
    labels = layouts(D)["mixed"]
    F, Dsc = cloud(65, D, dtype, labels, seed=3)
    nan, inf = np.nan, np.inf
    specials = [nan, inf, -inf, -0.0, 0.0]
    for i, v in enumerate(specials):
        F[i, i % D] = v                      # one special coordinate
        F[10 + i, :D] = v                    # every coordinate
        Dsc[i, 1 + i % D] = v                # inside "normals"
        Dsc[10 + i, 1:1 + D] = v
        Dsc[20 + i, 0] = v                   # pass-through rows
        Dsc[20 + i, 1 + D + 4 + D] = v
    F[30] = -0.0                             # the homogeneous entry too: every term is a signed zero
    F[31] = 0.0
    F[32, D] = nan
    F[33, D] = inf
    for kind in KINDS:
        name, P = params(kind, D, dtype)
        of, od = I.Transformation(name, dtype).compute(F, P, Dsc, labels)
        wf, wd = features_ref(F, P), descriptors_ref(Dsc, P, labels)
        assert np.isnan(wf).any() and np.isinf(wf).any() and np.isnan(wd).any()
        assert np.array_equal(of, wf, equal_nan=True) and np.array_equal(od, wd, equal_nan=True)
        for got, want in ((of, wf), (od, wd)):  # the sign of every zero
            z = want == 0
            assert np.array_equal(np.signbit(got[z]), np.signbit(want[z]))
        assert same_values(of, wf), kind
        assert same_values(od, wd), kind
    # a matrix with zero and negative entries: outputs that are exactly -0.0 and +0.0
    P = np.zeros((D + 1, D + 1), dtype)
    P[0, 0], P[1, 1], P[D, D] = 1, -1, 1
    of, od = _capi.transform_cloud(F, P, Dsc, spans=(1,))
    wf = features_ref(F, P)
    assert (np.signbit(wf) & (wf == 0)).any() and (~np.signbit(wf) & (wf == 0)).any()
    assert same_values(of, wf)
    assert same_values(od, descriptors_ref(Dsc, P, [("intensity", 1), ("normals", D), ("rest", 6 + D)]))


@pytest.mark.parametrize("n", [0, 1, 65, 4099])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_aliased_output_equals_separate_output(dtype, D, n):
    _, P = params("affine", D, dtype)
    for lname, labels in layouts(D).items():
        F, Dsc = cloud(n, D, dtype, labels, seed=9)
        spans, off = [], 0
        for label, span in labels:
            if label in ("normals", "observationDirections"):
                spans.append(off)
            off += span
        of, od = _capi.transform_cloud(F, P, Dsc, spans)
        assert same_values(of, features_ref(F, P))
        if Dsc is not None:
            assert same_values(od, descriptors_ref(Dsc, P, labels))
        Fa, Da = F.copy(), None if Dsc is None else Dsc.copy()
        rf, rd = _capi.transform_cloud(Fa, P, Da, spans, in_place=True)
        assert rf is Fa and rd is Da
        assert same_values(Fa, of), lname
        assert Dsc is None or same_values(Da, od), lname


def test_span_order_and_full_tiling():
    """Spans given out of order, and spans that tile the whole descriptor (the
    form uploaded as it is, without packing)."""
    D, dtype = 3, np.float32
    _, P = params("similarity", D, dtype)
    labels = [("normals", 3), ("observationDirections", 3)]
    F, Dsc = cloud(257, D, dtype, labels)
    want = descriptors_ref(Dsc, P, labels)
    for spans in ((0, 3), (3, 0)):
        _, od = _capi.transform_cloud(F, P, Dsc, spans)
        assert same_values(od, want)
    labels8 = [("normals", 3)] * 8  # the cap itself
    F, Dsc = cloud(65, D, dtype, labels8 + [("tail", 1)])
    _, od = _capi.transform_cloud(F, P, Dsc, [3 * k for k in range(8)])
    assert same_values(od, descriptors_ref(Dsc, P, labels8 + [("tail", 1)]))
    assert _capi.TRANSFORM_MAX_SPANS == 8


# ---------------------------------------------------------------- errors --
@pytest.mark.parametrize("dtype", DTYPES)
def test_rigid_refuses_non_orthogonal_and_leaves_the_cloud(dtype):
    labels = [("normals", 3)]
    F, Dsc = cloud(65, 3, dtype, labels)
    F0, D0 = F.copy(), Dsc.copy()
    rigid = I.Transformation("RigidTransformation", dtype)
    with pytest.raises(I.TransformationError, match="rotation matrix is not orthogonal"):
        rigid.compute(F, np.array(T_3D_NON_ORTHO, dtype), Dsc, labels)
    assert same_values(F, F0) and same_values(Dsc, D0)
    c = I.Cloud(F, [("x", 1), ("y", 1), ("z", 1), ("pad", 1)], Dsc, labels)
    with pytest.raises(I.TransformationError):
        rigid.compute(c, np.array(T_3D_NON_ORTHO, dtype))
    assert same_values(c.features, F0) and same_values(c.descriptors, D0)
    # the same matrix is a similarity's to apply
    of, _ = I.Transformation("SimilarityTransformation", dtype).compute(F, np.array(T_3D_NON_ORTHO, dtype))
    assert same_values(of, features_ref(F0, np.array(T_3D_NON_ORTHO, dtype)))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pure_translation(dtype, D):
    labels = layouts(D)["mixed"]
    F, Dsc = cloud(257, D, dtype, labels)
    pt = I.Transformation("PureTranslation", dtype)
    _, R = params("rigid", D, dtype)
    with pytest.raises(I.TransformationError, match="PureTranslation: Error, left part  not identity."):
        pt.compute(F, R, Dsc, labels)
    T = np.eye(D + 1, dtype=dtype)
    T[:D, D] = [1.5, -2.25, 0.125][:D]
    of, od = pt.compute(F, T, Dsc, labels)
    assert same_values(of, features_ref(F, T))
    assert not same_values(of, F)
    assert same_values(od, Dsc)  # normals and observationDirections included: nothing is rotated


def test_wrong_span_width_is_invalid_field():
    F, Dsc = cloud(65, 3, np.float32, [("normals", 2), ("other", 1)])
    _, P = params("rigid", 3, np.float32)
    with pytest.raises(I.InvalidField, match="normals"):
        I.Transformation("RigidTransformation").compute(F, P, Dsc, [("normals", 2), ("other", 1)])
    with pytest.raises(I.InvalidField, match="observationDirections"):
        I.Transformation("SimilarityTransformation").compute(F, P, Dsc, [("other", 1), ("observationDirections", 2)])
    # PureTranslation rotates nothing, so the width does not matter to it
    T = np.eye(4, dtype=np.float32)
    _, od = I.Transformation("PureTranslation").compute(F, T, Dsc, [("normals", 2), ("other", 1)])
    assert same_values(od, Dsc)


def test_wrong_parameter_size_is_invalid_parameter():
    F, _ = cloud(65, 3, np.float32, [])
    for name in ("RigidTransformation", "SimilarityTransformation", "PureTranslation"):
        with pytest.raises(I.InvalidParameter):
            I.Transformation(name).compute(F, np.eye(3, dtype=np.float32))
    with pytest.raises(I.InvalidParameter):  # labels that do not add up to the descriptor rows
        I.Transformation("RigidTransformation").compute(F, np.eye(4, dtype=np.float32),
                                                        np.zeros((65, 4), np.float32), [("normals", 3)])


@pytest.mark.parametrize("n", [0, 65])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_param_cases(dtype, n):
    """Every PMX_E_BAD_PARAM of pmx_transform_cloud, for an empty cloud too."""
    # rows outside {3, 4}
    for rows in (2, 5):
        with pytest.raises(_capi.InvalidParameter, match="2-D or 3-D"):
            _capi.transform_cloud(np.ones((n, rows), dtype), np.eye(rows, dtype=dtype))
    for D in (2, 3):
        F = np.ones((n, D + 1), dtype)
        P = np.eye(D + 1, dtype=dtype)
        Dsc = np.ones((n, 9 * D), dtype)
        # a span that leaves desc: past the end by one row, and before the start
        for off in (9 * D - D + 1, 9 * D, -1):
            with pytest.raises(_capi.InvalidParameter, match="leaves"):
                _capi.transform_cloud(F, P, Dsc, spans=(0, off))
        # spans without desc
        with pytest.raises(_capi.InvalidParameter, match="without descriptors"):
            _capi.transform_cloud(F, P, None, spans=(0,))
        # more spans than the cap (each of them valid)
        with pytest.raises(_capi.InvalidParameter, match="more than 8 spans"):
            _capi.transform_cloud(F, P, Dsc, spans=[k * D for k in range(9)])
        # overlapping spans
        with pytest.raises(_capi.InvalidParameter, match="overlap"):
            _capi.transform_cloud(F, P, Dsc, spans=(0, D - 1))
        # and the last valid offset is one
        of, od = _capi.transform_cloud(F, P, Dsc, spans=(9 * D - D,))
        assert of.shape == F.shape and od.shape == Dsc.shape


# ------------------------------------------------------- a tie to the loop --
def test_transformed_reading_is_nearer_the_reference():
    """A sanity check, not a tolerance: the reading moved by the ICP's result
    lies nearer the reference than the reading as it came."""
    dtype = np.float32
    ref, nrm = reference_cloud(4000, dtype)
    rd = reading_cloud(2000, dtype)
    icp = I.ICP(dtype)
    icp.load_yaml(chain_yaml(maxit=15))
    T = icp.compute(rd, ref, nrm)
    icp.close()
    rigid = I.Transformation("RigidTransformation", dtype)
    assert rigid.check_parameters(T)
    moved, _ = rigid.compute(rd, T)
    assert same_values(moved, features_ref(rd, T))

    def mean_nn(a):
        a3, r3 = a[:, :3].astype(np.float64), ref[:, :3].astype(np.float64)
        d2 = (a3 * a3).sum(1)[:, None] - 2.0 * (a3 @ r3.T) + (r3 * r3).sum(1)[None, :]
        return float(np.sqrt(np.maximum(d2.min(1), 0)).mean())

    before, after = mean_nn(rd), mean_nn(moved)
    print(f"mean nearest-neighbour distance: {before:.5f} before, {after:.5f} after")
    assert after < before

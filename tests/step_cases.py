"""Hand-built degenerate scenes for one ICP step and the independent
references they are judged by (test infrastructure; shared by
tests/test_dense_kit.py, CPU, and tests/test_gpu_step_degenerate.py, GPU).

Scenes: the reading is the reference moved by a small rigid motion
(rotations ~1e-3 rad, translations ~1e-3, the point spacing is 0.05 - 0.1, so
every point's nearest reference point is its own image).  Where the structure
of a case needs a coordinate to be exactly zero in the reading too (p x n must
hold exact zeros), that coordinate is `pinned`: put back to the reference's
value after the motion.  The motion's other components lie partly inside the
null space of the case (an in-plane slide of a floor, a slide along a
corridor): the minimal-norm step leaves them alone, exactly.

References (none of them shares code with csrc/common/pmx_dense.h or
oracle/pmo_dense.inc):
  * exact_min_norm: for a system whose zero rows / columns are exactly zero the
    minimal-norm solution is the solution of the full-rank sub-system on the
    other rows / columns and zero elsewhere; the sub-system is solved by
    Gaussian elimination over fractions.Fraction on the T-valued entries (no
    rank tolerance, no rounding);
  * increment64: PointToPlane's rigid increment (Rodrigues; the 2-D form) in
    float64;
  * kabsch / kabsch_similarity: numpy.linalg.svd in float64 with
    d = sign(det(U V^T)) on the last singular direction.
"""
from fractions import Fraction

import numpy as np

EPS = {"float32": float(np.finfo(np.float32).eps), "float64": float(np.finfo(np.float64).eps)}
BAR = {"float32": 1e-5, "float64": 1e-12}  # the project's parity bar on ||dT||_F


# ------------------------------------------------------------------ scenes --
def rot3(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def hom(p, dtype):
    return np.ascontiguousarray(np.c_[p, np.ones(len(p))], dtype=dtype)


ROT = (0.8e-3, -1.1e-3, 1.3e-3)
TRANS = (1.2e-3, -0.9e-3, 0.7e-3)


def move(p, D, rot=ROT, trans=TRANS):
    """p (n, D) float64 under the small rigid motion."""
    if D == 3:
        return p @ rot3(*rot).T + np.asarray(trans)
    c, s = np.cos(rot[2]), np.sin(rot[2])
    return p @ np.array([[c, -s], [s, c]]).T + np.asarray(trans[:2])


def floor_grid():
    x = (np.arange(12) - 5.5) * 0.1
    y = (np.arange(11) - 5.0) * 0.1
    a, b = [v.ravel() for v in np.meshgrid(x, y, indexing="ij")]
    return np.stack([a, b, np.zeros_like(a)], 1)  # 132 points on z = 0


def _wall(axis, c):
    """A wall on the plane coord[axis] = c above the floor: 11 x 8 points."""
    u = (np.arange(11) - 5.0) * 0.1
    z = (np.arange(8) + 1) * 0.1
    a, b = [v.ravel() for v in np.meshgrid(u, z, indexing="ij")]
    p = np.zeros((len(a), 3))
    p[:, axis] = c
    p[:, 1 - axis] = a
    p[:, 2] = b
    return p


def _axis_normals(n, axis, D=3):
    out = np.zeros((n, D))
    out[:, axis] = 1.0
    return out


def _scene(ref, nrm, dtype, pinned=None, rot=ROT, trans=TRANS):
    """(reading, reference, normals) in dtype; pinned: boolean (n, D) mask of
    the reading coordinates kept at the reference's value."""
    D = ref.shape[1]
    refT = np.ascontiguousarray(ref, dtype=dtype)
    rd = move(refT.astype(np.float64), D, rot, trans).astype(dtype)
    if pinned is not None:
        rd[pinned] = refT[pinned]
    return hom(rd, dtype), hom(refT, dtype), np.ascontiguousarray(nrm, dtype=dtype)


def plane3d_case(rank, dtype):
    """(reading, reference, normals, zero rows / columns of A): the issue's
    exact-structural-rank table; F = (p x n, n)."""
    fl = floor_grid()
    if rank == 1:    # points on the z axis, n = e_z: F = (0, 0, 0, 0, 0, 1)
        ref = np.zeros((100, 3))
        ref[:, 2] = (np.arange(100) - 49.5) * 0.05
        nrm = _axis_normals(100, 2)
        pin = np.zeros((100, 3), bool)
        pin[:, :2] = True
        zero = [0, 1, 2, 3, 4]
    elif rank == 2:  # points on the x axis, n = e_z: F = (0, -x, 0, 0, 0, 1)
        ref = np.zeros((120, 3))
        ref[:, 0] = (np.arange(120) - 59.5) * 0.05
        nrm = _axis_normals(120, 2)
        pin = np.zeros((120, 3), bool)
        pin[:, 1] = True
        zero = [0, 2, 3, 4]
    elif rank == 3:  # a floor: F = (y, -x, 0, 0, 0, 1)
        ref, nrm, pin, zero = fl, _axis_normals(len(fl), 2), None, [2, 3, 4]
    elif rank == 4:  # floor + a vertical line at y = 0 exactly, n = e_x: F = (0, z, 0, 1, 0, 0)
        line = np.zeros((20, 3))
        line[:, 0] = 0.65
        line[:, 2] = (np.arange(20) + 1) * 0.05
        ref = np.vstack([fl, line])
        nrm = np.vstack([_axis_normals(len(fl), 2), _axis_normals(20, 0)])
        pin = np.zeros(ref.shape, bool)
        pin[len(fl):, 1] = True
        zero = [2, 4]
    elif rank == 5:  # floor + the wall x = c (a corridor: t_y free): wall F = (0, z, -y, 1, 0, 0)
        w = _wall(0, 0.65)
        ref = np.vstack([fl, w])
        nrm = np.vstack([_axis_normals(len(fl), 2), _axis_normals(len(w), 0)])
        pin, zero = None, [4]
    elif rank == 6:  # floor + walls x = c and y = c
        w0, w1 = _wall(0, 0.65), _wall(1, 0.6)
        ref = np.vstack([fl, w0, w1])
        nrm = np.vstack([_axis_normals(len(fl), 2), _axis_normals(len(w0), 0), _axis_normals(len(w1), 1)])
        pin, zero = None, []
    else:
        raise ValueError(rank)
    return _scene(ref, nrm, dtype, pin) + (zero,)


def plane2d_case(rank, dtype):
    """2-D: F = (p_x n_y - p_y n_x, n_x, n_y)."""
    u = (np.arange(100) - 49.5) * 0.05
    if rank == 1:    # points at x = 0, n = e_y: F = (0, 0, 1)
        ref = np.stack([np.zeros_like(u), u], 1)
        nrm = _axis_normals(100, 1, 2)
        pin = np.zeros((100, 2), bool)
        pin[:, 0] = True
        zero = [0, 1]
    elif rank == 2:  # the wall y = 0, n = e_y: F = (x, 0, 1)
        ref = np.stack([u, np.zeros_like(u)], 1)
        nrm, pin, zero = _axis_normals(100, 1, 2), None, [1]
    elif rank == 3:  # an L: the wall y = 0 and the wall x = -2.6, n = e_x: F = (-y, 1, 0)
        v = (np.arange(60) + 1) * 0.05
        ref = np.vstack([np.stack([u, np.zeros_like(u)], 1), np.stack([np.full_like(v, -2.6), v], 1)])
        nrm = np.vstack([_axis_normals(100, 1, 2), _axis_normals(60, 0, 2)])
        pin, zero = None, []
    else:
        raise ValueError(rank)
    return _scene(ref, nrm, dtype, pin) + (zero,)


# the well_conditioned switch (pmx_step.h): lambda_min(A) / ||A||_F targets
SWITCH_TARGETS = {"float32": [1e-5, 1e-4, 5e-4, 2e-3, 1e-2],
                  "float64": [1e-13, 1e-11, 5e-10, 2e-9, 1e-8, 1e-6]}


def tilted_floor(a, dtype):
    """A 20 x 20 floor whose normals are normalize(a g_x, a g_y, 1), g a fixed
    +-1 pattern per point: lambda_min(A) / ||A||_F scales like a^2."""
    x = (np.arange(20) - 9.5) * 0.1
    p, q = [v.ravel() for v in np.meshgrid(x, x, indexing="ij")]
    ref = np.stack([p, q, np.zeros_like(p)], 1)
    g = np.random.default_rng(3).choice([-1.0, 1.0], size=(len(ref), 2))
    nrm = np.c_[a * g, np.ones(len(ref))]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return _scene(ref, nrm, dtype)


def conditioning_ratio(A):
    """lambda_min(A) / ||A||_F in float64 (A symmetric positive definite)."""
    A = np.asarray(A, np.float64)
    return float(np.linalg.eigvalsh(0.5 * (A + A.T))[0] / np.linalg.norm(A))


def _ratio_of_tilt(a):
    rd, ref, nrm = tilted_floor(a, np.float64)
    P3, N3 = rd[:, :3], nrm
    F = np.hstack([np.cross(P3, N3), N3])
    return conditioning_ratio(F.T @ F)


_tilts = {}


def tilt_for(target):
    """The tilt a whose float64 system has lambda_min / ||A||_F = target
    (bisection on the monotone branch a in (1e-9, 0.5))."""
    if target not in _tilts:
        lo, hi = 1e-9, 0.5
        for _ in range(80):
            mid = np.sqrt(lo * hi)
            if _ratio_of_tilt(mid) < target:
                lo = mid
            else:
                hi = mid
        _tilts[target] = float(np.sqrt(lo * hi))
    return _tilts[target]


def switch_case(target, dtype):
    return tilted_floor(tilt_for(target), dtype)


# point-to-point scenes: (reading, reference), kept-pair centroids near the origin
def p2p_case(name, dtype):
    if name == "coplanar":    # a flat grid slid in its plane and tilted slightly: m has an exactly zero row
        return _scene(floor_grid(), np.zeros((132, 3)), dtype, rot=(2.0e-3, -1.5e-3, 1.3e-3),
                      trans=(1.2e-3, -0.9e-3, 0.7e-3))[:2]
    if name == "reflection":  # a thin slab z = +-0.01, the reading's z negated, a small in-plane rotation
        ref = floor_grid()
        ref[:, 2] = 0.01 * np.random.default_rng(5).choice([-1.0, 1.0], size=len(ref))
        rd, refT, _ = _scene(ref, np.zeros_like(ref), dtype, rot=(0.0, 0.0, 1.3e-3), trans=(1.2e-3, -0.9e-3, 0.0))
        rd[:, 2] = -refT[:, 2]
        return rd, refT
    if name == "collinear":   # points on the x axis, turned about z and slid: m has one non-zero row
        ref = np.zeros((120, 3))
        ref[:, 0] = (np.arange(120) - 59.5) * 0.05
        return _scene(ref, np.zeros_like(ref), dtype, rot=(0.0, 0.0, 1.3e-3), trans=(1.2e-3, -0.9e-3, 0.0))[:2]
    if name == "reflection2d":  # points near the line y = 0 (+-0.02), mirrored across it and turned slightly
        u = (np.arange(100) - 49.5) * 0.05
        ref = np.stack([u, 0.02 * np.random.default_rng(6).choice([-1.0, 1.0], size=100)], 1)
        rd, refT, _ = _scene(ref, np.zeros_like(ref), dtype, rot=(0.0, 0.0, 0.4e-3), trans=(1.2e-3, 0.0, 0.0))
        # (the mirror image of the turned line: y negated)
        rd[:, 1] = -rd[:, 1]
        return rd, refT
    raise ValueError(name)


def identity_match(rd, ref):
    """Brute-force nearest neighbour in float64: every reading point's nearest
    reference point is its own index, strictly."""
    D = ref.shape[1] - 1
    d = ((rd[:, None, :D].astype(np.float64) - ref[None, :, :D].astype(np.float64)) ** 2).sum(-1)
    own = np.diag(d).copy()
    np.fill_diagonal(d, np.inf)
    return bool((own < d.min(axis=1)).all())


# -------------------------------------------------------------- references --
def exact_min_norm(A, b):
    """(x float64, live indices): the minimal-norm solution of A x = b for A
    whose zero rows / columns are exactly zero, the live sub-system solved over
    the rationals.  Raises ArithmeticError if the sub-system is singular."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    n = len(b)
    live = [i for i in range(n) if A[i].any() or A[:, i].any()]
    dead = [i for i in range(n) if i not in live]
    assert not b[dead].any(), "inconsistent system: b is non-zero on a zero row"
    r = len(live)
    M = [[Fraction(float(A[i, j])) for j in live] + [Fraction(float(b[i]))] for i in live]
    for k in range(r):
        piv = next((i for i in range(k, r) if M[i][k] != 0), None)
        if piv is None:
            raise ArithmeticError(f"sub-system of rank < {r}")
        M[k], M[piv] = M[piv], M[k]
        for i in range(r):
            if i != k and M[i][k] != 0:
                f = M[i][k] / M[k][k]
                M[i] = [a - f * c for a, c in zip(M[i], M[k])]
    x = np.zeros(n)
    for k, i in enumerate(live):
        x[i] = float(M[k][r] / M[k][k])
    return x, live


def cond2(A, live):
    s = np.linalg.svd(np.asarray(A, np.float64)[np.ix_(live, live)], compute_uv=False)
    return float(s[0] / s[-1])


def increment64(x, rows):
    """PointToPlane.cpp:245-312 in float64."""
    x = np.asarray(x, np.float64)
    out = np.eye(rows)
    if rows == 4:
        th = np.linalg.norm(x[:3])
        if th > 0:
            k = x[:3] / th
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            out[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        out[:3, 3] = x[3:]
    else:
        c, s = np.cos(x[0]), np.sin(x[0])
        out[:2, :2] = [[c, -s], [s, c]]
        out[:2, 2] = x[1:]
    return out


def step_vector(dT):
    """The x of a point-to-plane increment read back out of the matrix, in
    float64: the rotation vector from the skew part (its entries are sums of a
    small and a tiny term: relative error ~ eps_T, no absolute floor), the
    translation as stored."""
    dT = np.asarray(dT, np.float64)
    if dT.shape[0] == 4:
        R = dT[:3, :3]
        s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin(th) axis
        n = np.linalg.norm(s)
        r = s * (np.arcsin(n) / n) if n > 0 else s
        return np.r_[r, dT[:3, 3]]
    return np.r_[np.arctan2(dT[1, 0], dT[0, 0]), dT[:2, 2]]


def solve_ratio(x, x_exact, A, live, dtype):
    """||x - x_exact|| / (n eps_T cond2(A_r) ||x_exact||), the K of the bound."""
    n = np.asarray(A).shape[0]
    den = n * EPS[np.dtype(dtype).name] * cond2(A, live) * np.linalg.norm(x_exact)
    return float(np.linalg.norm(np.asarray(x, np.float64) - x_exact) / den)


def p2point_sums(rd, ref, dtype):
    """PointToPoint.cpp:61-80 for the identity match with unit weights: the
    means in T, the centred products in T summed in float64: (mp, mq, m, sigma)."""
    t = np.dtype(dtype).type
    D = ref.shape[1] - 1
    p, q = rd[:, :D], ref[:, :D]
    winv = t(1) / t(len(p))
    mp = p.astype(np.float64).sum(0).astype(dtype) * winv
    mq = q.astype(np.float64).sum(0).astype(dtype) * winv
    pc, qc = p - mp, q - mq
    m = (qc[:, :, None] * pc[:, None, :]).astype(np.float64).sum(0)
    sq = pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]
    if D == 3:
        sq = sq + pc[:, 2] * pc[:, 2]
    assert m.dtype == np.float64 and pc.dtype == np.dtype(dtype)
    return mp, mq, m, float(sq.astype(np.float64).sum())


def kabsch(m, mp, mq, sigma=None):
    """(T, d, singular values) in float64: R = U diag(1, .., d) V^T of m = sum
    qc pc^T, d = sign(det(U V^T)), t = mq - s R mp; s = 1, or with sigma the
    similarity's (sum of the signed singular values) / sigma."""
    m = np.asarray(m, np.float64)
    D = m.shape[0]
    U, S, Vt = np.linalg.svd(m)
    d = 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0
    E = np.eye(D)
    E[D - 1, D - 1] = d
    R = U @ E @ Vt
    s = 1.0
    if sigma is not None:
        s = (S[:-1].sum() + d * S[-1]) / float(sigma)
    out = np.eye(D + 1)
    out[:D, :D] = s * R
    out[:D, D] = np.asarray(mq, np.float64) - s * R @ np.asarray(mp, np.float64)
    return out, d, S


# ------------------------------------------------------------------- bounds --
# Measured on the CPU over every case of tests/test_dense_kit.py (its docstring
# holds the figures): 8 x the largest ratio of the host kit and the oracle.
K_SOLVE = 1.8   # ||x - x_exact|| <= K_SOLVE n eps_T cond2(A_r) ||x_exact||
K_P2P = 34.0    # ||T - T_kabsch||_F <= K_P2P eps_T


def check_structure(A, b, zero, dtype):
    """The preconditions of an exact-rank case on a (float64) system: the rows
    and columns `zero` are exactly zero, every other is live and the live
    sub-system is non-singular over the rationals.  Returns the T-valued
    system, the exact minimal-norm solution and the live indices."""
    n = len(b)
    live_want = [i for i in range(n) if i not in zero]
    assert not A[zero].any() and not A[:, zero].any() and not b[zero].any()
    At, bt = A.astype(dtype), b.astype(dtype)
    x_exact, live = exact_min_norm(At, bt)  # (raises if the sub-system is singular)
    assert live == live_want
    assert np.linalg.norm(x_exact) > 0
    return At, bt, x_exact, live

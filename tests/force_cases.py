"""PointToPlaneErrorMinimizer's force2D / force4DOF restated in numpy (test
infrastructure, no GPU; ErrorMinimizers/PointToPlane.cpp:171-312), the
yardstick of tests/test_gpu_p2plane_forced*.py.

With p the transformed reading point, q the matched reference point, n its
normal and w the pair's weight, over the ErrorElements columns (dist != inf and
w != 0):
  force4DOF  cross = (Gamma p) . n = -p_y n_x + p_x n_y,  F = [cross; n_x; n_y; n_z],
             dot = ((p - q) . n) in 3-D,  x = [yaw, t_x, t_y, t_z],
             T = [AngleAxis(yaw, unitZ), t]
  force2D    cross = p_x n_y - p_y n_x,  F = [cross; n_x; n_y],
             dot = (p_x - q_x) n_x + (p_y - q_y) n_y  (no z term),  x = [angle, t_x, t_y],
             T = I_4 with Rotation2D(angle) top-left and (t_x, t_y) top-right
  none       F = [p x n; n], the 3-D dot, x = [rotation vector, t]
A = sum (w F) F^T and b = -sum (w F) dot.  Every product is formed in T (the
cloud's dtype) in the reference's order and summed in float64; the system is
cast to T as the minimiser holds it and solved in float64 (numpy lstsq: the
minimal-norm solution where the system is rank-deficient); the transform is
built in float64.

Scenes come from tests/step_cases.py (its motion, normals and `_scene`): a
floor and two walls, the reading the reference under the small rigid motion
with roll, pitch and z components.
"""
import numpy as np

import oracle_py as O
import step_cases as sc

FORCES = ("4DOF", "2D")
NF = {None: 6, "4DOF": 4, "2D": 3}


# ------------------------------------------------------------------ scenes --
def _grid(nu, nv, du, u0, v0):
    u = u0 + np.arange(nu) * du
    v = v0 + np.arange(nv) * du
    a, b = [x.ravel() for x in np.meshgrid(u, v, indexing="ij")]
    return a, b


def _floor(nx, ny):
    a, b = _grid(nx, ny, 0.05, -0.05 * (nx - 1) / 2, -0.05 * (ny - 1) / 2)
    return np.stack([a, b, np.zeros_like(a)], 1)


def _wall(axis, c, nu, nz):
    a, b = _grid(nu, nz, 0.05, -0.05 * (nu - 1) / 2, 0.05)
    p = np.zeros((len(a), 3))
    p[:, axis] = c
    p[:, 1 - axis] = a
    p[:, 2] = b
    return p


def scene(dtype, parts="floor+walls"):
    """(reading, reference, normals): (n, 4), (n, 4), (n, 3) in dtype.
    floor+walls: 40 x 35 floor, walls x = c (30 x 20) and y = c (27 x 20): 2540
    points, not a multiple of 4 x 256; full rank in every mode.
    floor: rank 1 under force4DOF (yaw, x, y free), 1404 points.
    wall: the wall x = c alone, rank 2 under force2D (t_y free), 600 points."""
    fl, w0, w1 = _floor(40, 35), _wall(0, 1.05, 30, 20), _wall(1, 0.95, 27, 20)
    if parts == "floor+walls":
        ref = np.vstack([fl, w0, w1])
        nrm = np.vstack([sc._axis_normals(len(fl), 2), sc._axis_normals(len(w0), 0), sc._axis_normals(len(w1), 1)])
    elif parts == "floor":
        ref, nrm = _floor(39, 36), sc._axis_normals(39 * 36, 2)
    elif parts == "wall":
        ref, nrm = w0, sc._axis_normals(len(w0), 0)
    else:
        raise ValueError(parts)
    return sc._scene(ref, nrm, dtype)


def scene2d(dtype):
    """A 2-D L (step_cases' rank-3 case): force2D changes nothing on it."""
    return sc.plane2d_case(3, dtype)[:3]


# ------------------------------------------------------------------ system --
def forced_system(step, ref, nrm, ids, dists, w, force):
    """(A, b, kept): the normal equations of `force` (None, "4DOF", "2D") in
    float64 from T products, for the (N, k) match (ids, dists) with weights w;
    step is the transformed reading (N, 4), ref (M, 4), nrm (M, 3)."""
    dt = step.dtype
    assert ref.dtype == dt and nrm.dtype == dt and w.dtype == dt and dists.dtype == dt
    N, k = ids.shape
    keep = (dists != np.inf) & (w != 0)
    ii, ss = np.nonzero(keep)
    p = step[ii, :3]
    j = ids[ii, ss]
    q, n, ww = ref[j, :3], nrm[j], w[ii, ss]
    d = p - q
    if force == "4DOF":
        cross = ((-p[:, 1]) * n[:, 0] + p[:, 0] * n[:, 1])[:, None]
        F = np.hstack([cross, n])
        dot = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    elif force == "2D":
        cross = (p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0])[:, None]
        F = np.hstack([cross, n[:, :2]])
        dot = d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]
    else:
        cross = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                          p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], 1)
        F = np.hstack([cross, n])
        dot = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    wF = ww[:, None] * F
    assert F.dtype == dt and wF.dtype == dt and dot.dtype == dt
    A = (wF[:, :, None] * F[:, None, :]).astype(np.float64).sum(0)
    b = -(wF * dot[:, None]).astype(np.float64).sum(0)
    return A, b, len(ii)


def solve64(A, b, dtype):
    """The system as the minimiser holds it (T), solved in float64; minimal norm
    where it is rank-deficient."""
    A64 = np.asarray(A).astype(dtype).astype(np.float64)
    b64 = np.asarray(b).astype(dtype).astype(np.float64)
    return np.linalg.lstsq(A64, b64, rcond=None)[0]


def transform64(x, force):
    """PointToPlane.cpp:245-312 in float64, 4 x 4."""
    x = np.asarray(x, np.float64)
    if force is None:
        return sc.increment64(x, 4)
    out = np.eye(4)
    c, s = np.cos(x[0]), np.sin(x[0])
    out[:2, :2] = [[c, -s], [s, c]]
    if force == "4DOF":
        out[:3, 3] = x[1:4]
    else:
        out[:2, 3] = x[1:3]
    return out


def step64(A, b, force, dtype):
    return transform64(solve64(A, b, dtype), force)


def step_vector(dT, force):
    """The x of a forced increment read back out of the matrix in float64
    (step_cases.step_vector for the unforced one)."""
    dT = np.asarray(dT, np.float64)
    if force is None:
        return sc.step_vector(dT)
    ang = np.arctan2(dT[1, 0], dT[0, 0])
    return np.r_[ang, dT[:3, 3]] if force == "4DOF" else np.r_[ang, dT[:2, 3]]


# --------------------------------------------------------------------- ICP --
def matmul_seq(A, B):
    """A B in float64 with every product and every sum rounded once, the inner
    sums sequential (Eigen's scalar product, ICP.cpp:419, 437-441; what the
    library builds with -ffp-contract=off).  numpy's `@` goes through BLAS,
    whose fused multiply-adds round the rotation's entries next to 1
    differently: one unit in the last place, 1.1e-16, per composition."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    n = A.shape[0]
    C = np.zeros((n, n))
    for r in range(n):
        for c in range(n):
            s = A[r, 0] * B[0, c]
            for k in range(1, n):
                s = s + A[r, k] * B[k, c]
            C[r, c] = s
    return C


def icp(rd, ref, nrm, force, iters, knn=1, filters=(("TrimmedDistOutlierFilter", {"ratio": 0.85}),), centre=True):
    """A plain ICP loop with a Counter checker only (exactly `iters` iterations,
    identity T_init): oracle_py.knn, oracle_py.outlier_chain, the minimiser
    above.  As ICP::compute does (ICP.cpp:291-312, 437-441) the loop runs in the
    frame of the reference's mean (formed in T, sequential sums): the forced
    minimisations do not reach a zero residual on a motion with roll and pitch,
    so their iterates, unlike the unforced ones, depend on the frame they are
    linearised in.  T_iter is kept in float64, composed by matmul_seq, and
    handed to the transform in T."""
    dt = rd.dtype
    t = dt.type
    mean = np.zeros(3, dt)
    if centre:
        mean = np.array([np.cumsum(ref[:, r], dtype=dt)[-1] / t(len(ref)) for r in range(3)], dt)
    Tm = np.eye(4)
    Tm[:3, 3] = mean.astype(np.float64)
    Tmi = np.eye(4)
    Tmi[:3, 3] = -mean.astype(np.float64)
    refc = ref.copy()
    refc[:, :3] = ref[:, :3] - mean
    rdc = O.transform(Tmi.astype(dt), rd)
    T = np.eye(4)
    for _ in range(iters):
        step = O.transform(T.astype(dt), rdc)
        d, ids, _ = O.knn(refc, step, k=knn)
        rc, w = O.outlier_chain(list(filters), d)
        assert rc == 0
        A, b, kept = forced_system(step, refc, nrm, ids, d, w, force)
        assert kept > 0
        T = matmul_seq(step64(A, b, force, dt), T)
    return matmul_seq(matmul_seq(Tm, T), Tmi)

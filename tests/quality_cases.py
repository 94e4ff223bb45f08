"""The yardstick of ErrorMinimizer::getResidualError / getOverlap and of
SimpleSensorNoiseDataPointsFilter: the reference's lines restated in numpy
(ErrorMinimizers/PointToPlane.cpp:338-350 and :387-464, PointToPoint.cpp:139-164,
DataPointsFilters/SimpleSensorNoise.cpp:85-136).  Per-link terms in the ICP's
dtype in the reference's order, sums in float64.  Used by test_gpu_quality.py.

The fixture is test_gpu_covariance.py's box corner: three mutually orthogonal
unit squares with exact axis normals, the reading its points plus 0.01 noise
under a small pose offset.
"""
import math

import numpy as np

BAR = {"float32": 1e-5, "float64": 1e-12}
PLANE, POINT, COV, SIM = ("PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer",
                          "PointToPlaneWithCovErrorMinimizer", "PointToPointSimilarityErrorMinimizer")
# pmx_quality.branch (include/pmx.h)
NONE, DENSITY, BOTH, READING, REFERENCE = range(5)


# ------------------------------------------------------------------ fixture --
def box_corner(n_side=20):
    """Three unit squares on the planes x = 0, y = 0, z = 0: points and normals."""
    g = (np.arange(n_side) + 0.5) / n_side
    a, b = [v.ravel() for v in np.meshgrid(g, g, indexing="ij")]
    z = np.zeros_like(a)
    pts = np.concatenate([np.stack([z, a, b], 1), np.stack([a, z, b], 1), np.stack([a, b, z], 1)])
    nrm = np.concatenate([np.tile(e, (a.size, 1)) for e in np.eye(3)])
    return pts, nrm


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rigid(rx, ry, rz, t):
    T = np.eye(4)
    T[:3, :3] = rot(rx, ry, rz)
    T[:3, 3] = t
    return T


def clouds(n_rd, dtype, seed=3, centre=True):
    """(reading n_rd x 4, reference M x 4, normals M x 3): the reference centred
    on its mean when `centre` (what a context is given), the reading the box's
    points plus noise under the inverse of a small pose about that centre."""
    rng = np.random.default_rng(seed + n_rd)
    ref, nrm = box_corner()
    faces = rng.integers(0, 3, n_rd)
    uv = rng.uniform(0.05, 0.95, (n_rd, 2))
    rd = np.zeros((n_rd, 3))
    for f in range(3):
        m = faces == f
        rd[np.ix_(m, [c for c in range(3) if c != f])] = uv[m]
    rd += rng.normal(0, 0.01, rd.shape)
    off = ref.mean(0)
    ref = ref - off
    rd = rd - off
    pose = rigid(0.02, -0.015, 0.025, [0.01, -0.008, 0.012])
    rd = (np.linalg.inv(pose) @ np.c_[rd, np.ones(n_rd)].T).T[:, :3]
    if not centre:  # (the same geometry away from the origin: what an ICP is given)
        ref = ref + off
        rd = rd + off
    hom = lambda p: np.ascontiguousarray(np.c_[p, np.ones(len(p))], dtype=dtype)  # noqa: E731
    return hom(rd), hom(ref), np.ascontiguousarray(nrm, dtype=dtype)


T_AT = rigid(0.004, -0.003, 0.005, [0.002, -0.001, 0.003])  # the match's transform


def xform3(T, p):
    """The device's transform of the reading (pmx_p2plane.h xform3), in T's dtype."""
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] * p[:, 3]
                     for r in range(3)], 1)


# ------------------------------------------------------------- sensor noise --
LASER = {0: (0.012, 0.0068, 0.0008), 1: (0.028, 0.0013, 0.0001), 2: (0.018, 0.0006, 0.0015),
         4: (0.004, 0.0053, -0.0092)}


def sensor_noise(feat, sensor_type, dtype):
    """SimpleSensorNoiseDataPointsFilter::inPlaceFilter (SimpleSensorNoise.cpp:85-136)
    for feat (n x rows, homogeneous row last), every operation in dtype."""
    t = np.dtype(dtype).type
    f = np.asarray(feat, dtype)[:, :-1]
    sq = f[:, 0] * f[:, 0]
    for c in range(1, f.shape[1]):
        sq = sq + f[:, c] * f[:, c]
    norm = np.sqrt(sq)
    if sensor_type == 3:  # Kinect / Xtion: norm^2 * (0.5 * 0.00285)
        return (norm * norm) * t(0.5 * 0.00285)
    min_radius, beam_angle, beam_const = (t(v) for v in LASER[sensor_type])
    out = np.maximum(min_radius, beam_angle * norm + beam_const)
    assert out.dtype == np.dtype(dtype)
    return out


# -------------------------------------------------------------- restatement --
def branch_of(plane, noise_rd, noise_ref, dens):
    if not plane:
        return READING if noise_rd is not None else NONE
    if noise_rd is not None and noise_ref is not None:
        return DENSITY if dens is not None else BOTH
    if noise_rd is not None:
        return READING
    return REFERENCE if noise_ref is not None else NONE


def restate(d, ids, w, p, ref, nrm, dtype, plane, noise_rd=None, noise_ref=None, dens=None):
    """getResidualError and getOverlap over the ErrorElements columns of a
    match: d, ids, w (N x k, the mirrors), p (N x 3, the step reading in dtype),
    ref / nrm the reference.  Returns a dict with residual, links, dist_sum,
    points, rejected, branch, num, den, median_density and margin (the smallest
    relative distance of a point-to-point link from its threshold)."""
    t = np.dtype(dtype).type
    d, w = np.asarray(d, dtype), np.asarray(w, dtype)
    kept = (d != np.inf) & (w != 0)
    qi, s = np.nonzero(kept)  # (reading point, then link rank: the ErrorElements column order)
    r = np.sqrt(d[qi, s])
    assert r.dtype == np.dtype(dtype)
    out = dict(links=int(kept.sum()), dist_sum=float(r.astype(np.float64).sum()),
               points=int(kept.any(1).sum()), num=0, den=0, median_density=0.0, margin=np.inf)
    out["rejected"] = len(d) - out["points"]
    if plane:
        q, n = np.asarray(ref, dtype)[ids[qi, s], :3], np.asarray(nrm, dtype)[ids[qi, s]]
        dl = np.asarray(p, dtype)[qi] - q
        e = ((dl[:, 0] * n[:, 0]) + (dl[:, 1] * n[:, 1])) + (dl[:, 2] * n[:, 2])
        term = w[qi, s] * (e * e)
        assert term.dtype == np.dtype(dtype)
        out["residual"] = float(term.astype(np.float64).sum())
    else:
        out["residual"] = out["dist_sum"]
    b = out["branch"] = branch_of(plane, noise_rd, noise_ref, dens)
    if b == NONE:
        return out
    if plane:
        if b == DENSITY:
            vals = np.asarray(dens, dtype)[ids[qi, s]]
            at = int(len(vals) * 0.5)
            med = np.partition(vals, at)[at]
            out["median_density"] = float(med)
            radius = t(1.0 / math.pow(float(med), 1 / 3.0))
            u = (radius + np.asarray(noise_rd, dtype)[qi]) + np.asarray(noise_ref, dtype)[ids[qi, s]]
        elif b == BOTH:
            u = np.asarray(noise_rd, dtype)[qi] + np.asarray(noise_ref, dtype)[ids[qi, s]]
        elif b == READING:
            u = np.asarray(noise_rd, dtype)[qi]
        else:
            u = np.asarray(noise_ref, dtype)[ids[qi, s]]
        assert u.dtype == np.dtype(dtype)
        hit = np.zeros(len(d), bool)
        hit[qi[r < u]] = True  # (a point is hit when any of its kept links is inside)
        out["num"], out["den"] = int(hit.sum()), out["points"] + out["rejected"]
    else:
        mean = t(out["dist_sum"] / out["links"])
        thr = mean + np.asarray(noise_rd, dtype)[qi]
        assert thr.dtype == np.dtype(dtype)
        out["num"], out["den"] = int((r < thr).sum()), out["links"]
        out["margin"] = float(np.min(np.abs(r.astype(np.float64) - thr) / thr))
    return out


def rel(a, b):
    return abs(a - b) / abs(b)

"""The clouds CovarianceSamplingDataPointsFilter (device, csrc/pmx_covs.hip) is
tested on, and the two stand-alone programs they are checked against.

Nothing here imports the library.  The expectation of every case comes from
tests/covariance_sampling_main.cpp, a literal restatement of
DataPointsFilters/CovarianceSampling.cpp:136-249 that takes the centre, L and
the basis as inputs and prints, per output column, the input column it holds;
the filter moves whole columns, so the expected cloud is the input's columns
in that order.  tests/covariance_sampling_shared_main.cpp runs the host side
the library compiles in (csrc/common/pmx_covs.h) the same way.

  cloud(name, dtype)        points (n, 4), descriptors (n, dd), normals (n, 3)
  CASES                     name -> builder of (points (n, 3), normals (n, 3))
  nb_samples(n)             1, n // 2, n - 1
  Programs(tmp)             builds both programs; .literal / .shared run a case
  centre_l_basis(...)       the three inputs in numpy (any sound values do:
                            both programs take them as given)
  numpy_columns(...)        the selection for the identity basis in numpy and
                            plain Python, sharing no code with either program
"""
import os
import shutil
import subprocess

import numpy as np

from helpers import TESTS

ROOT = os.path.dirname(TESTS)
DTYPES = [np.float32, np.float64]
TORQUE_NORMS = [0, 1, 2]


def random_unit(n, rng):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ellipsoid(n, seed):
    """Points on an off-centre ellipsoid (semi-axes 3, 2, 1) with its outward
    unit normals: every one of the six directions is constrained."""
    rng = np.random.default_rng(seed)
    u = random_unit(n, rng)
    axes = np.array([3.0, 2.0, 1.0])
    g = u / axes
    return u * axes + np.array([5.0, -2.0, 1.0]), g / np.linalg.norm(g, axis=1, keepdims=True)


def plane(n, seed):
    """A plane with identical normals: v = [inv (dy, -dx, 0); 0, 0, 1], a
    covariance of rank 3, and long runs of zero magnitudes tied by index."""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-4.0, 4.0, (n, 2)), np.full((n, 1), 0.75)], axis=1)
    return p, np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1))


def doubled(n, seed):
    """Every point twice (the copies half a cloud apart): exact ties in every list."""
    p, nr = ellipsoid(n // 2, seed)
    return np.concatenate([p, p]), np.concatenate([nr, nr])


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 6.0, (n, 3)), random_unit(n, rng)


CASES = {
    "n2": lambda: ellipsoid(2, 1),
    "n7": lambda: ellipsoid(7, 2),
    "n63": lambda: ellipsoid(63, 3),
    "n64": lambda: ellipsoid(64, 4),
    "n65": lambda: ellipsoid(65, 5),
    "n255": lambda: ellipsoid(255, 6),
    "n256": lambda: ellipsoid(256, 7),
    "n257": lambda: ellipsoid(257, 8),
    "n4099": lambda: ellipsoid(4099, 9),
    "n20011": lambda: ellipsoid(20011, 10),
    "plane": lambda: plane(300, 11),
    "doubled": lambda: doubled(400, 12),
    "random": lambda: random_cloud(1000, 13),
}
STALE_CASE = "n257"  # with nbSample = n - 1 picks below the running column number must occur


def nb_samples(n):
    return sorted({1, max(1, n // 2), n - 1})


_cache = {}


def cloud(name, dtype, normals_row=0, extra_after=0):
    """points (n, 4), descriptors (n, normals_row + 3 + extra_after) with the
    normals at normals_row, and the normals (n, 3) on their own.  The other
    descriptor rows are distinct per column, so a wrong column cannot pass for
    the right one (the doubled case repeats points and normals on purpose)."""
    key = (name, np.dtype(dtype).name, normals_row, extra_after)
    if key not in _cache:
        p, nr = CASES[name]()
        n = len(p)
        nrm = np.ascontiguousarray(nr, dtype=dtype)
        pts = np.ascontiguousarray(np.concatenate([p, np.ones((n, 1))], axis=1), dtype=dtype)
        i = np.arange(n, dtype=np.float64)
        before = np.stack([1000.0 + i + r for r in range(normals_row)], axis=1) if normals_row else np.empty((n, 0))
        after = np.stack([-2000.0 - i - r for r in range(extra_after)], axis=1) if extra_after else np.empty((n, 0))
        desc = np.ascontiguousarray(np.concatenate([before.astype(dtype), nrm, after.astype(dtype)], axis=1))
        for a in (pts, desc, nrm):
            a.setflags(write=False)
        _cache[key] = (pts, desc, nrm)
    return _cache[key]


def v_rows(pts, nrm, centre, L):
    """v_i = [inv * ((p - c) x n); n] in the cloud's type, one operation at a
    time (numpy rounds each), as include/pmx.h defines it: (n, 6)."""
    dt = pts.dtype.type
    c = np.asarray(centre, dtype=dt)
    inv = dt(1.0 / float(dt(L)))
    d = pts[:, :3] - c
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return np.stack([inv * (dy * nz - dz * ny), inv * (dz * nx - dx * nz), inv * (dx * ny - dy * nx), nx, ny, nz],
                    axis=1)


def centre_l_basis(pts, nrm, torque_norm):
    """A centre, an L and an orthonormal basis in numpy, in the cloud's type."""
    dt = pts.dtype.type
    c = pts[:, :3].astype(np.float64).mean(axis=0).astype(dt)
    if torque_norm == 0:
        L = dt(1)
    elif torque_norm == 1:
        L = dt(np.linalg.norm(pts[:, :3].astype(np.float64) - c.astype(np.float64), axis=1).mean())
    else:
        L = dt((pts[:, :3].max(axis=0) - pts[:, :3].min(axis=0)).max() / dt(2))
    v = v_rows(pts, nrm, c, L).astype(np.float64)
    _, X = np.linalg.eigh(v.T @ v)
    return c, L, X.astype(dt)


class Programs:
    """The literal program and the shared-header program, built once."""

    def __init__(self, tmp, sanitize=True):
        cxx = shutil.which("g++")
        if cxx is None:
            raise FileNotFoundError("g++")
        self.tmp = str(tmp)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        self.exe = {}
        for which, src in (("literal", "covariance_sampling_main.cpp"),
                           ("shared", "covariance_sampling_shared_main.cpp")):
            exe = os.path.join(self.tmp, which)
            subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off"] + flags +
                                  ["-I", os.path.join(ROOT, "libpointmatcher_amd", "csrc"), os.path.join(TESTS, src),
                                   "-o", exe])
            self.exe[which] = exe
        self._count = 0

    def write(self, pts, nrm, centre, L, basis):
        """The input file of both programs: points, normals, centre, L, basis in T."""
        dt = pts.dtype
        path = os.path.join(self.tmp, f"case_{self._count}.bin")
        self._count += 1
        with open(path, "wb") as f:
            for a in (pts[:, :3], nrm, centre, [L], basis):
                f.write(np.ascontiguousarray(np.asarray(a), dtype=dt).tobytes())  # (T values: exact)
        return path

    def run(self, which, path, dtype, n, nb_sample):
        t = "d" if np.dtype(dtype) == np.float64 else "f"
        out = subprocess.run([self.exe[which], "filter", t, path, str(n), str(nb_sample)], capture_output=True,
                             text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.split("\n")
        cols = np.array(lines[0].split(), dtype=np.int64)
        return (cols, int(lines[1])) + ((int(lines[2]),) if which == "literal" else ())

    def eigen(self, cov):
        """(eigenvalues (6,), basis (6, 6)) of covs_sym_eigen on cov, in double,
        before any rounding to the cloud's type."""
        path = os.path.join(self.tmp, f"cov_{self._count}.bin")
        self._count += 1
        np.ascontiguousarray(cov, dtype=np.float64).tofile(path)
        out = subprocess.run([self.exe["shared"], "eigen", path], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.split("\n")
        return np.array(lines[0].split(), dtype=np.float64), np.array(lines[1].split(), dtype=np.float64).reshape(6, 6)

    def literal(self, path, dtype, n, nb_sample):
        """(kept columns, deepest list position read, stale lookups)."""
        return self.run("literal", path, dtype, n, nb_sample)

    def shared(self, path, dtype, n, nb_sample):
        """(kept columns, deepest list position read)."""
        return self.run("shared", path, dtype, n, nb_sample)


def numpy_columns(pts, nrm, centre, L, nb_sample):
    """The kept columns for the identity basis (m_k = v_k), restated in numpy
    and plain Python: stable argsort by falling |v_k|, the pick loop with t in
    the cloud's type, the swap sequence with its one-level lookup table."""
    dt = pts.dtype.type
    v = v_rows(pts, nrm, centre, L)
    n = len(v)
    lists = [list(np.argsort(-np.abs(v[:, k]), kind="stable")) for k in range(6)]
    at, t, taken, picks = [0] * 6, [dt(0)] * 6, np.zeros(n, bool), []
    for _ in range(nb_sample):
        k = min(range(6), key=lambda j: (t[j], j))
        while taken[lists[k][at[k]]]:
            at[k] += 1
        i = lists[k][at[k]]
        at[k] += 1
        taken[i] = True
        t = [dt(t[j] + dt(v[i, j] * v[i, j])) for j in range(6)]
        picks.append(int(i))
    col, table = list(range(n)), {}
    for k, d in enumerate(picks):
        j = table[d] if d < k else d
        col[k], col[j] = col[j], col[k]
        table[k] = j
    return np.array(col[:nb_sample], dtype=np.int64), max(at)

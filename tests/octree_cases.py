"""Independent numpy reference for OctreeGridDataPointsFilter (device,
csrc/pmx_octree.hip) and the clouds the tests run it on.

Nothing here is imported from the package under test or from the oracle
wrapper.  The functions restate DataPointsFilters/OctreeGrid.cpp and
utils/octree.hpp with file:line notes, every operation in the arrays' own type
and in the reference's order (numpy rounds each elementwise multiply and add
on its own: no fused multiply-add).

  leaves()            the literal recursion (octree.hpp:229-368), iterative: it
                      follows the radius down to the stop rule, ~150 levels in
                      float and ~2100 in double when points never separate;
                      non-empty leaves in visit order (octree.hpp:373-385)
  literal()           the four samplers as the reference runs them, column
                      contents included: swapCols, the one-level mapidx table
                      and every read and write through it (OctreeGrid.cpp:48-282)
  from_input()        centroid and medoid of each leaf from the input cloud's
                      own columns: what the device builds for methods 2 and 3
"""
import functools

import numpy as np

import keep_cases as kc  # glibc rand() / srand() through ctypes

FIRST, RANDOM, CENTROID, MEDOID = range(4)
DTYPES = [np.float32, np.float64]


# --------------------------------------------------------------------- tree --
def root_box(pts):
    """octree.hpp:238-251, in T: (center, radius)."""
    T = pts.dtype.type
    dim = pts.shape[1] - 1
    mn = pts[:, :dim].min(axis=0)
    mx = pts[:, :dim].max(axis=0)
    radii = mx - mn
    center = mn + radii * T(0.5)
    radius = radii.max() * T(0.5)
    return center, radius


def leaves(pts, max_pts, max_size):
    """Non-empty leaves in visit order, each an array of rising input indices."""
    T = pts.dtype.type
    dim = pts.shape[1] - 1
    n = len(pts)
    if n == 0:
        return []
    P = np.ascontiguousarray(pts[:, :dim])
    limit = float(T(max_size))  # maxSizeByNode is a T
    center, radius = root_box(pts)
    out = []
    stack = [(center, radius, np.arange(n))]
    weights = (1 << np.arange(dim)).astype(np.int64)
    with np.errstate(under="ignore"):
        while stack:
            c, r, ids = stack.pop()
            if float(r) * 2.0 <= limit or len(ids) <= max_pts:  # octree.hpp:312
                if len(ids):
                    out.append(ids)
                continue
            child = ((P[ids] > c).astype(np.int64) * weights).sum(axis=1)  # octree.hpp:181-189
            half = r * T(0.5)
            for i in range((1 << dim) - 1, -1, -1):  # pushed backwards: child 0 is visited first
                sub = ids[child == i]
                if len(sub) == 0:
                    continue  # (an empty leaf: skipped by every sampler, OctreeGrid.cpp:50)
                sign = np.array([T(0.5) if (i >> a) & 1 else T(-0.5) for a in range(dim)], dtype=pts.dtype)
                stack.append((c + sign * r, half, sub))  # octree.hpp:335-341
    return out


def depth_reached(pts, max_pts, max_size):
    """The depth of the deepest leaf (for the tests' own assertions)."""
    T = pts.dtype.type
    dim = pts.shape[1] - 1
    P = np.ascontiguousarray(pts[:, :dim])
    limit = float(T(max_size))
    center, radius = root_box(pts)
    deepest = 0
    stack = [(center, radius, np.arange(len(pts)), 0)]
    weights = (1 << np.arange(dim)).astype(np.int64)
    with np.errstate(under="ignore"):
        while stack:
            c, r, ids, d = stack.pop()
            if float(r) * 2.0 <= limit or len(ids) <= max_pts:
                deepest = max(deepest, d)
                continue
            child = ((P[ids] > c).astype(np.int64) * weights).sum(axis=1)
            for i in range(1 << dim):
                sub = ids[child == i]
                if len(sub):
                    sign = np.array([T(0.5) if (i >> a) & 1 else T(-0.5) for a in range(dim)], dtype=pts.dtype)
                    stack.append((c + sign * r, r * T(0.5), sub, d + 1))
    return deepest


# ----------------------------------------------------------------- samplers --
def random_ids(lv):
    """RandomPtsSampler's member number per leaf (OctreeGrid.cpp:85-109, 130-137):
    srand(1), one rand() per leaf, srand(1)."""
    kc.srand(1)
    ids = []
    for m in lv:
        r = np.float32(np.float32(kc._libc.rand()) / np.float32(kc.RAND_MAX))
        ids.append(int(np.float32(len(m) - 1) * r))
    kc.srand(1)
    return ids


def picks(lv, method):
    if method == FIRST:
        return [int(m[0]) for m in lv]
    return [int(m[i]) for m, i in zip(lv, random_ids(lv))]


def replay_columns(pk, n):
    """FirstPtsSampler's swapCols / mapidx sequence (OctreeGrid.cpp:55-67) on
    column numbers alone: the input column each of the kept columns holds, and
    how many lookups were stale."""
    col = list(range(n))
    mapidx = {}
    stale = 0
    for k, d in enumerate(pk):
        j = d
        if d < k:
            j = mapidx[d]
            stale += int(col[j] != d)
        col[k], col[j] = col[j], col[k]
        mapidx[k] = j
    return col[:len(pk)], stale


def _dist(p, c):
    e = p - c
    z = e[0] * e[0] + e[1] * e[1]
    if len(e) == 3:
        z = z + e[2] * e[2]
    return np.sqrt(z)


def literal(pts, desc, lv, method):
    """The reference's visit (OctreeGrid.cpp:48-282) on copies of the columns.
    Returns (features, descriptors, stale) — stale: the lookups mapidx answered
    with a column that no longer holds the point asked for."""
    T = pts.dtype.type
    D = pts.shape[1] - 1
    F = pts.copy()
    S = desc.copy() if desc is not None else None
    where = np.arange(len(pts))  # where[i]: the column that holds input point i now
    mapidx = {}
    stale = 0
    idx = 0
    rid = random_ids(lv) if method == RANDOM else None

    def look(d):
        nonlocal stale
        if d < idx:
            j = mapidx[d]
            stale += int(where[d] != j)
            return j
        return d

    def swap(a, b):
        if a == b:
            return
        F[[a, b]] = F[[b, a]]
        if S is not None:
            S[[a, b]] = S[[b, a]]
        ia, ib = np.nonzero(where == a)[0], np.nonzero(where == b)[0]
        where[ia], where[ib] = b, a

    with np.errstate(all="ignore"):
        for k, m in enumerate(lv):
            n = len(m)
            if method == FIRST:
                j = look(int(m[0]))
            elif method == RANDOM:
                j = look(int(m[rid[k]]))
            elif method == CENTROID:
                j = look(int(m[0]))
                for cur in m[1:]:
                    i = look(int(cur))
                    F[j, :D] = F[j, :D] + F[i, :D]
                    if S is not None:
                        S[j] = S[j] + S[i]
                F[j, :D] = F[j, :D] / T(n)
                if S is not None:
                    S[j] = S[j] / T(n)
            else:
                c = np.zeros(D, pts.dtype)
                real = [look(int(cur)) for cur in m]
                for i in real:
                    c = c + F[i, :D]
                c = c / T(n)
                best, j = np.finfo(pts.dtype).max, 0
                for i in real:
                    d = _dist(F[i, :D], c)
                    if d < best:
                        best, j = d, i
            swap(idx, j)
            mapidx[idx] = j
            idx += 1
    return F[:idx], (S[:idx] if S is not None else None), stale


def from_input(pts, desc, lv, method):
    """Column k = the centroid / medoid of leaf k from the input's own columns."""
    T = pts.dtype.type
    D = pts.shape[1] - 1
    F = np.empty((len(lv), pts.shape[1]), pts.dtype)
    S = np.empty((len(lv), desc.shape[1]), desc.dtype) if desc is not None else None
    with np.errstate(all="ignore"):
        for k, m in enumerate(lv):
            n = len(m)
            if method == CENTROID:
                s = pts[m[0]].copy()
                for i in m[1:]:
                    s[:D] = s[:D] + pts[i, :D]
                s[:D] = s[:D] / T(n)
                F[k] = s
                if S is not None:
                    t = desc[m[0]].copy()
                    for i in m[1:]:
                        t = t + desc[i]
                    S[k] = t / T(n)
            else:
                c = np.zeros(D, pts.dtype)
                for i in m:
                    c = c + pts[i, :D]
                c = c / T(n)
                best, j = np.finfo(pts.dtype).max, 0
                for i in m:
                    d = _dist(pts[i, :D], c)
                    if d < best:
                        best, j = d, int(i)
                F[k] = pts[j]
                if S is not None:
                    S[k] = desc[j]
    return F, S


# -------------------------------------------------------------------- clouds --
def hom(xyz, dtype):
    xyz = np.asarray(xyz, np.float64)
    return np.hstack([xyz, np.ones((len(xyz), 1))]).astype(dtype)


def descriptors(n, dtype, seed=0):
    """A 3-row "normals" and a 1-row descriptor, every value distinct enough
    that a misplaced column shows."""
    rng = np.random.default_rng(1000 + seed + n)
    return rng.normal(0, 1, (n, 4)).astype(dtype)


def uniform(n, dim, dtype, seed=0, corners=True):
    """Uniform in the unit box; from two points on, two opposite corners are in
    it (unless corners is off), so the root box is exactly [0, 1]^dim and every
    centre a dyadic number."""
    rng = np.random.default_rng(seed + 31 * n + dim)
    xyz = rng.random((n, dim))
    if n >= 2 and corners:
        xyz[n // 3] = 0.0
        xyz[(2 * n) // 3] = 1.0
    return hom(xyz, dtype)


def lattice(dim, dtype, k=3):
    """Every point of the 2^-k lattice of the unit box, in a scrambled order:
    each lies exactly on cell boundaries (`>` sends it to the lower child)."""
    g = np.arange((1 << k) + 1) / float(1 << k)
    xyz = np.stack(np.meshgrid(*([g] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    rng = np.random.default_rng(5)
    return hom(xyz[rng.permutation(len(xyz))], dtype)


def collinear(dim, dtype, n=40):
    xyz = np.zeros((n, dim))
    xyz[:, 0] = np.random.default_rng(6).permutation(n) / 16.0
    return hom(xyz, dtype)


def close_pair(dim, dtype, far, origin=False):
    """Neighbouring numbers next to 1 on the first axis and one point far away.
    With far = 1024 and a point at the origin the box is [0, 1024]: every
    centre is a dyadic number, one of them falls exactly on each of the
    neighbours, and the last two separate ~34 (float) or ~63 (double) levels
    down — more than one key of depth."""
    eps = np.finfo(dtype).eps
    xs = [1.0, 1.0 + eps, 1.0 + 2 * eps]
    xs = xs + [far] + ([0.0] if origin else [])
    xyz = np.zeros((len(xs), dim))
    xyz[:, 0] = xs
    return hom(xyz, dtype)


def origin_pair(dim, dtype):
    """Two copies of the origin between two opposite corners: the centre walks
    towards 0 as -radius and stops moving only when the radius underflows, so
    the descent is the longest there is (~150 levels in float, ~1075 in double)."""
    xyz = np.zeros((4, dim))
    xyz[0] = -1.0
    xyz[3] = 1.0
    return hom(xyz, dtype)


@functools.lru_cache(maxsize=None)
def _cases(dtype_name, dim):
    dtype = np.dtype(dtype_name).type
    out = {}

    def add(name, pts, max_pts, max_size):
        out[name] = (pts, descriptors(len(pts), dtype), int(max_pts), float(max_size))

    for n in (1, 2, 63, 64, 65, 257):
        add(f"uniform{n}", uniform(n, dim, dtype), 1, 0.0)
    for n in (257, 5000):
        u = uniform(n, dim, dtype)
        for mp in (1, 3, n):
            for ms, tag in ((0.0, "0"), (0.25, "quarter"), (1.0, "box")):
                add(f"grid{n}_p{mp}_s{tag}", u, mp, ms)
    u = uniform(100, dim, dtype, seed=3, corners=False)  # (a copy of the origin would walk down to the underflow)
    add("tripled", np.vstack([u, u, u]), 1, 0.0)
    add("identical", np.repeat(uniform(1, dim, dtype, seed=4), 50, axis=0), 1, 0.0)
    add("collinear", collinear(dim, dtype), 1, 0.0)
    add("lattice_p1", lattice(dim, dtype), 1, 0.0)
    add("lattice_p3", lattice(dim, dtype), 3, 0.0)
    add("lattice_quarter", lattice(dim, dtype), 1, 0.25)
    add("close_pair", close_pair(dim, dtype, 1024.0, origin=True), 1, 0.0)
    add("stalled", close_pair(dim, dtype, STALL_FAR), 1, 0.0)
    add("origin_pair", origin_pair(dim, dtype), 1, 0.0)
    add("stale2000", uniform(2000, dim, dtype, seed=9), 3, 0.0)
    pts, desc, mp, ms = out["stale2000"]
    order = np.concatenate(leaves(pts, mp, ms))
    out["presorted"] = (np.ascontiguousarray(pts[order]), np.ascontiguousarray(desc[order]), mp, ms)
    return out


# With this far point the box is [1, 1000] and its centres are 1 + 999 * 2^-l,
# rounded: they close in on 1 from above and stop moving before one of them
# falls between every pair of neighbours, so the recursion never separates
# them all (tests/test_octree_reference.py asserts it).
STALL_FAR = 1000.0


def case_names(dim=3):
    return list(_cases("float32", dim).keys())


def case(name, dtype, dim):
    """(points, descriptors, maxPointByNode, maxSizeByNode)"""
    return _cases(np.dtype(dtype).name, dim)[name]


@functools.lru_cache(maxsize=None)
def case_leaves(name, dtype_name, dim):
    pts, _, mp, ms = case(name, dtype_name, dim)
    return leaves(pts, mp, ms)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(a.view(u), b.view(u))

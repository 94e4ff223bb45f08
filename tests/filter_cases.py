"""Independent references, scenes and shared assertions for the three device
data filters: SurfaceNormal, SamplingSurfaceNormal and VoxelGrid.

Everything here is plain numpy, in float64 unless a T-valued sequential sum
is part of the definition.  Nothing is imported from the package under test
or from the oracle wrapper, and there is no Jacobi: eigen pairs come from
numpy.linalg.eigh.  The functions restate the reference files with file:line
notes; where the reference leaves a choice open they follow DESIGN.md §4
"Deliberate definitions" (sorted k-columns, a leaf's points in index order,
sequential sums, ascending eigen pairs compared up to sign).

Both tests/test_filter_reference.py (the oracle, on a CPU) and
tests/test_gpu_filter_edges.py (the HIP kernels) run the `run_*` functions
below; a backend is any object with
    surface_normals(pts, k, max_dist) -> dict      (normals, densities, eig_values,
                                                    eig_vectors, matched_ids, mean_dists, degenerate)
    ssn(pts, desc, knn, method, ratio, max_box, average) -> dict
    voxel(pts, desc, vsize, centroid, average) -> (features, descriptors)
    srand(seed)
"""
import ctypes
import math

import numpy as np

EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
LATTICE = 2.0 ** -6  # lattice scenes: coordinates m * 2^-6, |m| < 2^12

# The bars' constants: 8x the largest ratio the oracle reached against these
# references over every scene (tests/test_filter_reference.py prints them;
# DESIGN.md §4 records them).  The device's ratios never set them.
K_LAMBDA = 8.2   # 8 x 1.02
K_V = 5.2        # 8 x 0.649
K_DENS = 103.0   # 8 x 12.8   (the table's K_d, measured apart for its two quantities:
K_MD = 32.0      # 8 x 3.94    never above the one shared constant, 8 x 12.8)
GAP_MIN = 1e-2       # eigenvectors are compared where gap >= GAP_MIN * trace
SKIP_CAP = 0.02      # share of a surface scene's points the gap rule may leave out
# k = 3: a point and its two nearest span a triangle, l0 is 0 by construction and
# l1 < GAP_MIN * trace for every thin triangle: 18.5 % of these very clouds'
# points in float64 with a brute-force kNN (test_filter_reference.py asserts
# it, with no filter in the loop).  No implementation can meet 2 % there.
SKIP_CAP_K3 = 0.20
# k = 3 again: a thin triangle can lie within 64x of the rank threshold, where
# the side it falls on is the filter's own word (undecided_ok).  At most this
# share of a surface scene's points may be such: 0.8 % (16 of 2000) in float,
# none in double, counted with a brute-force kNN and no filter in the loop.
UNDECIDED_CAP_K3 = 0.01

# largest ratios seen in this process, by constant (the CPU file prints them)
MEASURED = {"K_lambda": 0.0, "K_v": 0.0, "K_dens": 0.0, "K_md": 0.0, "skip": 0.0, "skip_k3": 0.0, "skip_ssn": 0.0,
            "undecided_k3": 0.0}

_libc = ctypes.CDLL(None)
_libc.rand.restype = ctypes.c_int
RAND_MAX = 2147483647


def eps_of(a):
    return EPS[np.dtype(a.dtype)]


def hom(p, dtype):
    p = np.asarray(p, dtype=np.float64)
    return np.ascontiguousarray(np.hstack([p, np.ones((len(p), 1))]).astype(dtype))


def _note(name, value):
    if value > MEASURED[name]:
        MEASURED[name] = float(value)


# ---------------------------------------------------------------------------
# kNN judge (float64 brute force; no tie rule on either side)
# ---------------------------------------------------------------------------
def knn_judge(pts, ids, k, max_dist=np.inf):
    """Asserts that `ids` (n, k; -1 = invalid) are k nearest neighbours of every
    point in its own cloud (KDTreeMatcher with self-match, MatchersImpl.cpp:85-101,
    radius inclusive), to 4 eps_T relative on the float64 squared distances."""
    eps = eps_of(pts)
    n, rows = pts.shape
    P = pts[:, :rows - 1].astype(np.float64)
    ids = np.asarray(ids)
    assert ids.shape == (n, k)
    I = ids.astype(np.int64)
    assert np.array_equal(I.astype(ids.dtype), ids), "ids are integers"
    assert np.all((I >= -1) & (I < n))
    valid = I >= 0
    # valid entries first (the padding comes last, PointMatcher.h:377-378)
    assert np.all(valid[:, :-1] >= valid[:, 1:]), "a valid id after an invalid one"
    r2 = float(pts.dtype.type(max_dist)) ** 2 if np.isfinite(max_dist) else np.inf
    lo, hi = 1 - 4 * eps, 1 + 4 * eps
    for a in range(0, n, 512):
        b = min(n, a + 512)
        with np.errstate(invalid="ignore"):
            D2 = ((P[a:b, None, :] - P[None, :, :]) ** 2).sum(axis=2)  # NaN rows / columns: non-finite points
        Ic, vc = I[a:b], valid[a:b]
        d = np.take_along_axis(D2, np.where(vc, Ic, 0), axis=1)
        assert np.all(np.isfinite(d[vc])), "a non-finite point listed as a neighbour"
        assert np.all(d[vc] <= r2 * hi), "a neighbour beyond max_dist"
        srt = np.sort(np.where(vc, Ic, -1 - np.arange(k)[None, :]), axis=1)
        assert np.all(srt[:, 1:] != srt[:, :-1]), "an id twice in a row"
        dd = np.where(vc, d, np.inf)
        assert np.all(dd[:, 1:] >= dd[:, :-1] * lo), "distances decrease along a row"
        # completeness: everything clearly closer than the k-th returned distance
        # (max_dist where the row is not full) is in the row
        kth = np.where(vc[:, -1], dd[:, -1], r2)
        closer = D2 < (kth * lo)[:, None]
        rowsel = np.repeat(np.arange(b - a), k)[vc.ravel()]
        closer[rowsel, Ic.ravel()[vc.ravel()]] = False
        assert not closer.any(), "a closer point is missing from a row"
    return valid


# ---------------------------------------------------------------------------
# SurfaceNormal (SurfaceNormal.cpp:164-250, utils.h:89-139)
# ---------------------------------------------------------------------------
def rank_ratio(A):
    """A (m, D) float64 coordinates.  For D = 3: e2(S) / trace(S)^2 of the centred
    scatter S (e2 = the sum of the principal 2x2 minors = l0 l1 + l0 l2 + l1 l2;
    ~ l1 / l2 where the set is nearly collinear); for D = 2: 1 if trace(S) > 0
    else 0.  SurfaceNormal.cpp:193's `rank + 1 >= D` asks for rank >= D - 1: the
    set is degenerate where this ratio is negligible.  Evaluated in long double
    on m S = m sum(a a^T) - s s^T with a centred on the first point, so that an
    exactly collinear lattice set gives (nearly) exactly zero."""
    L = np.longdouble
    a = (A - A[0]).astype(L)
    m = L(len(a))
    s = a.sum(axis=0)
    S = m * (a.T @ a) - np.outer(s, s)
    tr = np.trace(S)
    if not tr > 0:
        return 0.0
    if A.shape[1] == 2:
        return 1.0
    e2 = (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) + (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) + \
         (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1])
    return float(abs(e2) / (tr * tr))


def degenerate_by_rule(A, dtype):
    """The independent reading of `C.fullPivHouseholderQr().rank() + 1 < D`
    (Eigen's threshold: eps_T * D relative to the largest pivot).  Returns
    (degenerate, decided): `decided` is False where the ratio lies within 64x
    of the threshold — no scene may contain such a set."""
    tol = A.shape[1] * EPS[np.dtype(dtype)]
    r = rank_ratio(A)
    return r <= tol, not (tol / 64 <= r <= tol * 64)


def surface_normal_ref(pts, ids, valid):
    """Per point: the float64 mean, C = NN NN^T, eigh(C), density
    real / (4/3 pi max|NN_j|^3), mean distance |p - mean| over the given
    neighbours (ids (n, k), valid (n, k) bool), on the T-valued coordinates."""
    n, rows = pts.shape
    D = rows - 1
    P = pts[:, :D].astype(np.float64)
    real = valid.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # (n, k, D) :173-181, relative to the point itself: exact in float64 for T-valued near
        # neighbours, so the judge has no cancellation of its own far from the origin
        Q = np.where(valid[:, :, None], P[np.where(valid, ids, 0)] - P[:, None, :], 0.0)
        mean = Q.sum(axis=1) / real[:, None]                                    # :184
        NN = np.where(valid[:, :, None], Q - mean[:, None, :], 0.0)             # :185
        C = np.einsum("nka,nkb->nab", NN, NN)                                   # :187
        ok = np.isfinite(C).all(axis=(1, 2))
        w, V = np.linalg.eigh(np.where(ok[:, None, None], C, 0.0))              # ascending (sortEigen, :199-210)
        maxn = np.sqrt((NN ** 2).sum(axis=2)).max(axis=1)
        dens = real / ((4.0 / 3.0) * math.pi * maxn ** 3)                       # utils.h:106-120
        mdist = np.sqrt((mean ** 2).sum(axis=1))                                # :247-248 (|p - mean|)
    return dict(real=real, mean=mean, C=C, w=w, V=V, trace=np.trace(C, axis1=1, axis2=2), dens=dens, mdist=mdist,
                finite=ok)


def _eig_check(lam, vec, C, w, V, tr, cnt, eps, gap_rule=True):
    """lam (m, D), vec (m, D, D) (eigenvectors in columns) in T against
    eigh's (w, V) of C in float64; cnt = the set's size (the bars' k).  Returns
    the share of points at which the gap rule left an eigenvector out."""
    lam = lam.astype(np.float64)
    vec = vec.astype(np.float64)
    m, D = lam.shape
    if m == 0:
        return 0.0
    unit = (cnt + 3) * eps * tr
    assert np.all(tr > 0)
    assert np.all(lam[:, 1:] >= lam[:, :-1]), "eigenvalues ascending"
    r = np.abs(lam - w).max(axis=1) / unit
    _note("K_lambda", r.max())
    assert r.max() <= K_LAMBDA, f"eigenvalues: ratio {r.max():.3g} > K_lambda {K_LAMBDA}"
    G = np.einsum("nab,nac->nbc", vec, vec) - np.eye(D)
    assert np.abs(G).max() <= 8 * eps, f"|V^T V - I| = {np.abs(G).max():.3g} > 8 eps"
    res = np.einsum("nab,nbj->naj", C, vec) - vec * lam[:, None, :]
    rr = np.sqrt((res ** 2).sum(axis=1)).max(axis=1) / unit
    _note("K_lambda", rr.max())
    assert rr.max() <= K_LAMBDA, f"|C v - l v|: ratio {rr.max():.3g} > K_lambda {K_LAMBDA}"
    skipped = np.zeros(m, bool)
    if gap_rule:
        for j in range(D):
            others = np.delete(w, j, axis=1)
            gap = np.abs(others - w[:, j:j + 1]).min(axis=1)
            use = gap >= GAP_MIN * tr
            skipped |= ~use
            v, u = vec[:, :, j], V[:, :, j]
            s = np.where((v * u).sum(axis=1) < 0, -1.0, 1.0)
            sin = np.sqrt(((v / np.sqrt((v * v).sum(axis=1))[:, None] - s[:, None] * u) ** 2).sum(axis=1))
            if use.any():
                q = (sin[use] * gap[use] / unit[use]).max()
                _note("K_v", q)
                assert q <= K_V, f"eigenvector {j}: ratio {q:.3g} > K_v {K_V}"
    return float(skipped.mean())


def check_surface_normals(out, pts, k, max_dist=np.inf, expect=None, skip_cap=0.0, eig_rows=None, gap_rule=True,
                          undecided_ok=False):
    """Every assertion on one SurfaceNormal result.  expect: None (the rank rule
    decides), "all" or "none" (by construction).  undecided_ok: sets within 64x
    of the rank threshold may fall on either side (their outputs must still be
    those of the side they fell on); otherwise no set may be that close.
    eig_rows: restrict the eigen-pair assertions to these points.  Returns
    the reference dict."""
    dt = pts.dtype
    eps = eps_of(pts)
    n, rows = pts.shape
    D = rows - 1
    for name, shape in (("normals", (n, D)), ("densities", (n,)), ("eig_values", (n, D)),
                        ("eig_vectors", (n, D * D)), ("matched_ids", (n, k)), ("mean_dists", (n,))):
        assert out[name].shape == shape and out[name].dtype == dt, name
    valid = knn_judge(pts, out["matched_ids"], k, max_dist)
    ids = out["matched_ids"].astype(np.int64)
    ref = surface_normal_ref(pts, ids, valid)
    P = pts[:, :D].astype(np.float64)
    if expect == "all":
        deg = np.ones(n, bool)
    elif expect == "none":
        deg = np.zeros(n, bool)
    else:
        deg = np.zeros(n, bool)
        undecided = 0
        for i in range(n):
            if ref["real"][i] == 0 or not np.isfinite(P[i]).all():
                deg[i] = True
                continue
            deg[i], decided = degenerate_by_rule(P[ids[i][valid[i]]], dt)
            if not decided:
                assert undecided_ok, f"point {i}: the rank test is not clear-cut on this scene"
                deg[i] = out["mean_dists"][i] == dt.type(18446744073709551615.0)
                undecided += 1
        _note("undecided_k3", undecided / n)
        assert undecided <= UNDECIDED_CAP_K3 * n, f"{undecided} of {n} sets lie near the rank threshold"
    assert out["degenerate"] == int(deg.sum()), (out["degenerate"], int(deg.sum()))
    # degenerate points: zero eigen pairs, density 0, mean distance (T)SIZE_MAX (:213-216, 232-236, 244)
    assert np.all(out["eig_values"][deg] == 0) and np.all(out["eig_vectors"][deg] == 0)
    assert np.all(out["normals"][deg] == 0) and np.all(out["densities"][deg] == 0)
    assert np.all(out["mean_dists"][deg] == dt.type(18446744073709551615.0))
    g = ~deg
    if eig_rows is not None:
        sel = np.zeros(n, bool)
        sel[eig_rows] = True
        g &= sel
    if g.any():
        vec = out["eig_vectors"][g].reshape(-1, D, D)   # serializeEigVec: row k of eigenVe at k*D (utils.h:93-100)
        share = _eig_check(out["eig_values"][g], vec, ref["C"][g], ref["w"][g], ref["V"][g], ref["trace"][g],
                           ref["real"][g].astype(np.float64), eps, gap_rule)
        _note("skip_k3" if skip_cap == SKIP_CAP_K3 else "skip", share)
        assert share <= skip_cap, f"the gap rule leaves out {share:.4f} of the points (cap {skip_cap})"
        # the normal is the smallest eigenvalue's vector, clamped to [-1, 1] (:222-228)
        assert np.array_equal(out["normals"][g], np.clip(vec[:, :, 0], -1, 1))
        rd = np.abs(out["densities"][g].astype(np.float64) / ref["dens"][g] - 1) / ((ref["real"][g] + 3) * eps)
        _note("K_dens", rd.max())
        assert rd.max() <= K_DENS, f"density: ratio {rd.max():.3g} > K_dens {K_DENS}"
        md = ref["mdist"][g]
        got = out["mean_dists"][g].astype(np.float64)
        assert np.all(got[md == 0] == 0)
        rm = np.where(md > 0, np.abs(got - md) / np.where(md > 0, md, 1.0), 0.0) / ((ref["real"][g] + 3) * eps)
        _note("K_md", rm.max())
        assert rm.max() <= K_MD, f"mean distance: ratio {rm.max():.3g} > K_md {K_MD}"
    return ref


# ---------------------------------------------------------------------------
# SamplingSurfaceNormal (SamplingSurfaceNormal.cpp:170-342)
# ---------------------------------------------------------------------------
def ssn_leaves(pts, knn, tight_boxes=False):
    """buildNew (:171-221) exactly as written: the leaves (index-sorted arrays)
    in depth-first, left-first order.  tight_boxes: take the split axis from the
    box's own bounding box instead of the inherited bounds (only to prove that a
    scene tells the two apart)."""
    n, rows = pts.shape
    leaves = []

    def build(idx, mn, mx):
        count = len(idx)
        if count <= knn:                                   # :179
            leaves.append(np.sort(idx))
            return
        if tight_boxes:
            ext = pts[idx].max(axis=0) - pts[idx].min(axis=0)
        else:
            ext = mx - mn                                  # :190, in T
        cut, best = 0, pts.dtype.type(0)                   # argMax, utils.h:141-157: strict >, first maximum
        for r in range(rows):
            if ext[r] > best:
                best, cut = ext[r], r
        right = count // 2                                 # :193-194
        left = count - right
        order = idx[np.lexsort((idx, pts[idx, cut]))]      # nth_element's partition; ties by index
        cutval = pts[order[left], cut]                     # :206-207
        lmx, rmn = mx.copy(), mn.copy()
        lmx[cut] = cutval                                  # :210-214
        rmn[cut] = cutval
        build(order[:left], mn, lmx)                       # :217-220
        build(order[left:], rmn, mx)

    build(np.arange(n), pts.min(axis=0), pts.max(axis=0))  # :139-140 (every row, the homogeneous one too)
    return leaves


def seq_sum(x):
    """the sequential sum of x's rows in x's own type, first row first"""
    return np.add.accumulate(x, axis=0, dtype=x.dtype)[-1]


def ssn_ref(pts, desc, knn, method, ratio, max_box, average, tight_boxes=False, fit_by=None):
    """fuseRange (:223-342) over the leaves of ssn_leaves.  Returns the kept
    points in index order: features and descriptors in T (bit-exact bars), the
    float64 eigen reference of each kept point's leaf, the unfit count and the
    leaves.  The rand() draws of method 0 come from the process's libc, in leaf
    order.  fit_by: {leaf number: bool} overrides the rank rule where a scene
    fixes the answer by construction."""
    dt = pts.dtype
    T = dt.type
    n, rows = pts.shape
    D = rows - 1
    leaves = ssn_leaves(pts, knn, tight_boxes)
    keep = {}      # point index -> leaf number
    feat = pts.copy()
    dsc = None if desc is None else desc.copy()
    unfit = 0
    stats = {}
    for l, idx in enumerate(leaves):
        d = pts[idx, :D]                                                    # :233-235
        box = (d.max(axis=0) - d.min(axis=0)).max()                         # :236-237, in T
        if box > T(max_box):                                                # :239, strict
            unfit += len(idx)
            continue
        A = d.astype(np.float64)
        if fit_by is not None and l in fit_by:
            fit = fit_by[l]
        else:
            degen, decided = degenerate_by_rule(A, dt)                      # :254
            assert decided, f"leaf {l}: the rank test is not clear-cut on this scene"
            fit = not degen
        if not fit:
            unfit += len(idx)                                               # :262
            continue
        mean = A.mean(axis=0)
        NN = A - mean
        C = NN.T @ NN
        w, V = np.linalg.eigh(C)
        maxn = np.sqrt((NN ** 2).sum(axis=1)).max()
        stats[l] = dict(C=C, w=w, V=V, trace=np.trace(C), cnt=len(idx),
                        dens=len(idx) / ((4.0 / 3.0) * math.pi * maxn ** 3))
        if method == 0:                                                     # :286-309
            for i in idx:
                r = np.float32(_libc.rand()) / np.float32(RAND_MAX)
                if r < T(ratio):
                    keep[int(i)] = l
        else:                                                               # :312-340
            k = int(idx[0])
            keep[k] = l
            feat[k, :D] = seq_sum(d) / T(len(idx))                          # :244, :315 (sequential, index order)
            feat[k, D] = 1
            if dsc is not None and average:
                dsc[k] = seq_sum(desc[idx]) / T(len(idx))                   # :323-327
    kept = np.array(sorted(keep), dtype=np.int64)                           # :145
    return dict(kept=kept, features=feat[kept], descriptors=None if dsc is None else dsc[kept],
                leaf_of=[keep[int(i)] for i in kept], stats=stats, unfit=unfit, leaves=leaves)


def check_ssn(out, ref, pts, has_desc, skip_cap=0.0):
    """out: the filter's dict; ref: ssn_ref's.  skip_cap: the share of the kept
    points whose eigenvectors the gap rule may leave out (0 in a constructed
    scene).  Returns that share."""
    eps = eps_of(pts)
    D = pts.shape[1] - 1
    m = len(ref["kept"])
    assert out["unfit"] == ref["unfit"], (out["unfit"], ref["unfit"])
    assert len(out["features"]) == m
    assert np.array_equal(out["features"], ref["features"]), "features (kept set / T-valued means)"
    if has_desc:
        assert np.array_equal(out["descriptors"], ref["descriptors"]), "descriptors"
    if m == 0:
        return 0.0
    st = [ref["stats"][l] for l in ref["leaf_of"]]
    C = np.array([s["C"] for s in st])
    w = np.array([s["w"] for s in st])
    V = np.array([s["V"] for s in st])
    tr = np.array([s["trace"] for s in st])
    cnt = np.array([s["cnt"] for s in st], dtype=np.float64)
    vec = out["eig_vectors"].reshape(-1, D, D)
    share = _eig_check(out["eig_values"], vec, C, w, V, tr, cnt, eps)
    _note("skip_ssn", share)
    assert share <= skip_cap, f"the gap rule leaves out {share:.4f} of the kept points (cap {skip_cap})"
    assert np.array_equal(out["normals"], vec[:, :, 0])    # computeNormal: the smallest eigenvalue's column
    dens = np.array([s["dens"] for s in st])
    rd = np.abs(out["densities"].astype(np.float64) / dens - 1) / ((cnt + 3) * eps)
    _note("K_dens", rd.max())
    assert rd.max() <= K_DENS, f"density: ratio {rd.max():.3g} > K_dens {K_DENS}"
    return share


# ---------------------------------------------------------------------------
# VoxelGrid (VoxelGrid.cpp:60-343), point by point in T
# ---------------------------------------------------------------------------
def voxel_ref(pts, desc, vsize, centroid, average):
    dt = pts.dtype
    T = dt.type
    n, rows = pts.shape
    D = rows - 1
    vs = [T(v) for v in vsize]                                   # Parametrizable::get<T> (:53-55)
    mn, mx = pts.min(axis=0), pts.max(axis=0)                    # :97-98
    minB = [mn[a] / vs[a] if a < D else T(0) for a in range(3)]  # :100-111
    maxB = [mx[a] / vs[a] if a < D else T(0) for a in range(3)]
    nd = [int(np.uint32((T(1) + maxB[a]) - minB[a])) if a < D else 0 for a in range(3)]  # :115-121
    ndx, ndy, ndz = nd
    M = 1 << 32
    numvox = (ndx * ndy * (ndz if D == 3 else 1)) % M
    assert numvox > 0
    members = {}                                                 # voxel -> its points, in point order (:155-182)
    for p in range(n):
        i = int(np.floor(pts[p, 0] / vs[0] - minB[0]))
        j = int(np.floor(pts[p, 1] / vs[1] - minB[1]))
        assert i >= 0 and j >= 0
        if D == 3:
            k = int(np.floor(pts[p, 2] / vs[2] - minB[2]))
            assert k >= 0
            idx = (i + j * ndx + k * ndx * ndy) % M
        else:
            idx = (i + j * ndx) % M
        assert idx < numvox
        members.setdefault(idx, []).append(p)
    feat = pts.copy()
    dsc = None if desc is None else desc.copy()
    keep = []
    for idx, mem in members.items():
        first = mem[0]
        cnt = T(len(mem))                                        # `/= numPoints` (unsigned -> T)
        if centroid:
            feat[first, :D] = seq_sum(pts[mem][:, :D]) / cnt     # :192-232
        else:                                                    # :272-304: rows 1..3 receive the centres (sic)
            k = 0
            if D == 3:
                k = idx // (ndx * ndy)
                if k == ndz:
                    feat[first, 3] = mx[2] - T(k - 1) * vs[2] / T(2)
                else:
                    feat[first, 3] = T(k) * vs[2] + vs[2] / T(2)
            j = (idx - k * ndx * ndy) // ndx
            if j == ndy:
                feat[first, 2] = mx[1] - T(j - 1) * vs[1] / T(2)
            else:
                feat[first, 2] = T(j) * vs[1] + vs[1] / T(2)
            i = idx - k * ndx * ndy - j * ndx
            if i == ndx:
                feat[first, 1] = mx[0] - T(i - 1) * vs[0] / T(2)
            else:
                feat[first, 1] = T(i) * vs[0] + vs[0] / T(2)
        if dsc is not None and average:
            dsc[first] = seq_sum(desc[mem]) / cnt                # :208-213, 234-238, 248-270, 307-311
        keep.append(first)
    keep = np.array(sorted(keep), dtype=np.int64)                # :322
    return feat[keep], (np.zeros((len(keep), 0), dt) if dsc is None else dsc[keep])


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def lattice(m, dtype):
    m = np.asarray(m, dtype=np.int64)
    assert np.all(np.abs(m) < 2 ** 12)
    return hom(m * LATTICE, dtype)


def ribbons_2d():
    """(960, 2) integer lattice points, every x and every y distinct: 15 zigzag
    ribbons, 512 apart in y; along a ribbon x steps by 64 and y alternates by
    70.  The 5 nearest of a point are its own ribbon's c-2 .. c+2: a clearly
    two-dimensional, clearly anisotropic set."""
    out = []
    for r in range(-7, 8):
        for c in range(-32, 32):
            out.append((64 * c + (r + 7), 512 * r + (c + 32) + 70 * (c & 1)))
    return np.array(out, dtype=np.int64)


def plane_exact(axis, dtype):
    xy = ribbons_2d()
    m = np.insert(xy, axis, 37, axis=1)  # the constant coordinate
    return lattice(m, dtype)


def line_scene(n, dtype, D=3):
    v = np.array([1, 2, -1][:D])
    return lattice(np.arange(n)[:, None] * v[None, :], dtype)


def duplicates_scene(dtype, D=3):
    rng = np.random.default_rng(11)
    sites = rng.permutation(8000)[:40 * D].reshape(40, D) - 4000
    return lattice(np.repeat(sites, 8, axis=0)[rng.permutation(320)], dtype)


def cube_scene(dtype):
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    interior = np.flatnonzero(np.all((g > 0) & (g < 9), axis=1))
    return lattice(g * 16 - 72, dtype), interior


def pairs_scene(dtype, D):
    """100 isolated pairs: partners (3, 1, 2) lattice steps apart, pairs 64 apart"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * 64 - 128
    off = np.array([3, 1, 2])
    m = np.concatenate([g, g + off])[:, :D]
    if D == 2:
        m = np.unique(m, axis=0)
    return lattice(m, dtype)


PAIR_SELF_ONLY = 1 * LATTICE      # < |(3, 1)| lattice steps
PAIR_BOTH = 8 * LATTICE           # > |(3, 1, 2)|, < 64 - 3


def ring_scene(dtype):
    rng = np.random.default_rng(7)
    t = rng.uniform(0, 2 * np.pi, 1500)
    return hom(np.column_stack([np.cos(t), np.sin(t)]) * (1 + rng.normal(0, 0.01, (1500, 1))), dtype)


def wall_scene(dtype):
    """2-D, x constant: rank 1 — degenerate geometry that passes the rank test in
    2-D (1 + 1 >= 2): l0 exactly 0, the normal exactly (1, 0)."""
    y = np.cumsum(1 + (np.arange(300) * 7) % 5)  # uneven steps: no equidistant pairs
    return lattice(np.column_stack([np.full(300, 21), y - 450]), dtype)


def l_scene(dtype):
    """2-D: a wall along y and one along x, different uneven spacings, meeting in a corner"""
    a = np.cumsum(2 + (np.arange(150) * 3) % 4)
    b = np.cumsum(5 + (np.arange(150) * 5) % 3)
    m = np.concatenate([np.column_stack([np.zeros(150, int), a]), np.column_stack([b, np.zeros(150, int)]),
                        [[0, 0]]])
    return lattice(m, dtype)


def offset_scene(cloud, dtype):
    """the surface cloud at millimetre spread, moved to (1000, -2000, 500)"""
    p = cloud[:, :3].astype(np.float64) * 1e-3 + np.array([1000.0, -2000.0, 500.0])
    return hom(p, dtype)


# --- SSN
def distinct_cloud(n, D, dtype, seed):
    """n points, every coordinate distinct along every axis (after the cast to T)"""
    rng = np.random.default_rng(seed)
    p = np.column_stack([rng.permutation(4 * n)[:n] for _ in range(D)]).astype(np.float64)
    p = (p - 2 * n) * (np.array([1.0, 0.6, 0.3])[:D] / n)   # a 4 x 2.4 x 1.2 slab
    p += rng.uniform(-0.01, 0.01, p.shape) / n
    return hom(p, dtype)


def inherited_box_scene(dtype):
    """An L in the x-y plane, half a unit thick in z: the long arm along x
    (x in [0, 10], y in [0, 1]) holds more than half of the points' x-order, the
    short arm rises along y at small x (x in [0, 1], y in [1, 9]).  The first
    cut is along x; the right child (large x) inherits y-bounds [0, 9] although
    its points span only [0, 1] in y, so the inherited box cuts y where the
    tight box would cut x.  80 points, 16 leaves; the seed is the one of 0..3999
    whose leaves' eigenvalues lie furthest apart (smallest gap 1.9 % of the
    trace), so that the gap rule leaves out none of them: the CPU file asserts
    that and the disagreement of the boxes."""
    rng = np.random.default_rng(2488)
    n1, n2 = 52, 28
    arm_x = np.column_stack([rng.uniform(0, 10, n1), rng.uniform(0, 1, n1)])
    arm_y = np.column_stack([rng.uniform(0, 1, n2), rng.uniform(1, 9, n2)])
    p = np.concatenate([arm_x, arm_y])[rng.permutation(n1 + n2)]
    return hom(np.column_stack([p, rng.uniform(0, 0.5, n1 + n2)]), dtype)


def box_leaf_scene(width, dtype, D=3):
    """one leaf of 6 lattice points whose largest extent is `width` lattice steps"""
    m = np.array([[0, 0, 0], [width, 3, 1], [5, 9, 2], [11, 4, 7], [2, 13, 5], [7, 1, 11]])[:, :D]
    return lattice(m, dtype)


def planar_leaf_scene(dtype):
    m = np.array([[0, 0, 5], [16, 3, 5], [5, 9, 5], [11, 4, 5], [2, 13, 5], [7, 1, 5]])
    return lattice(m, dtype)


def collinear_leaf_scene(dtype, D=3):
    t = np.array([0, 1, 3, 4, 7, 9])
    return lattice(t[:, None] * np.array([2, 1, 3][:D])[None, :], dtype)


# --- voxels
def voxel_scenes(dtype):
    """name -> (pts, desc, vsize).  Lattice scenes: vsize a power of two, points
    exactly on voxel faces."""
    rng = np.random.default_rng(31)
    sc = {}
    m = rng.integers(-16, 17, (600, 3)) * 32             # multiples of 0.5 in [-8, 8]: all on faces of 0.5-voxels
    sc["faces"] = (lattice(m, dtype), rng.normal(size=(600, 3)).astype(dtype), (0.5, 0.5, 0.5))
    sc["faces_aniso"] = (lattice(m, dtype), rng.normal(size=(600, 2)).astype(dtype), (0.5, 1.0, 2.0))
    sc["negative"] = (lattice(-np.abs(rng.integers(1, 4000, (500, 3))), dtype), None, (4.0, 8.0, 2.0))
    sc["one_voxel"] = (lattice(rng.integers(0, 63, (300, 3)), dtype), rng.normal(size=(300, 1)).astype(dtype),
                       (64.0, 64.0, 64.0))
    sc["one_point"] = (lattice([[5, -7, 9]], dtype), np.ones((1, 2), dtype), (0.25, 0.25, 0.25))
    top = np.concatenate([rng.integers(0, 257, (200, 3)), [[256, 256, 256], [0, 0, 0], [256, 0, 256]]]) * 8
    sc["max_bound"] = (lattice(top, dtype), None, (4.0, 4.0, 4.0))      # the maximum lies on the last face
    sc["2d"] = (lattice(rng.integers(-2000, 2000, (700, 2)), dtype), rng.normal(size=(700, 2)).astype(dtype),
                (2.0, 4.0, 1.0))
    dense = np.concatenate([rng.uniform(0.0, 0.999, (1500, 3)), rng.uniform(-3, 3, (300, 3))])
    sc["dense"] = (hom(dense[rng.permutation(1800)], dtype), rng.normal(1.0, 0.5, (1800, 2)).astype(dtype),
                   (1.0, 1.0, 1.0))
    return sc


VOXEL_NAMES = ["faces", "faces_aniso", "negative", "one_voxel", "one_point", "max_bound", "2d", "dense"]


# ---------------------------------------------------------------------------
# the cases, shared by the CPU (oracle) and the GPU files
# ---------------------------------------------------------------------------
SURFACE_K = [3, 5, 10, 16, 17, 64]
SIZES = [6, 63, 64, 65, 255, 256, 257, 1025]


def skip_cap_of(k):
    return SKIP_CAP_K3 if k == 3 else SKIP_CAP


def run_surface(be, cloud, k, undecided_ok=False):
    out = be.surface_normals(cloud, k, np.inf)
    check_surface_normals(out, cloud, k, skip_cap=skip_cap_of(k), undecided_ok=undecided_ok)


def run_plane_exact(be, axis, dtype):
    pts = plane_exact(axis, dtype)
    out = be.surface_normals(pts, 5, np.inf)
    check_surface_normals(out, pts, 5, expect="none")
    e = np.zeros(3, dtype)
    e[axis] = 1
    assert np.all(out["eig_values"][:, 0] == 0), "l0 exactly 0"
    assert np.all(out["normals"] == e[None, :]), "the normal exactly the plane's axis"
    assert not np.signbit(out["normals"][:, axis]).any()


def run_all_degenerate(be, pts, k, max_dist=np.inf):
    out = be.surface_normals(pts, k, max_dist)
    check_surface_normals(out, pts, k, max_dist, expect="all")
    assert out["degenerate"] == len(pts)
    return out


def run_cube(be, dtype):
    pts, interior = cube_scene(dtype)
    out = be.surface_normals(pts, 7, np.inf)
    knn_judge(pts, out["matched_ids"], 7)
    # boundary points: the 7 nearest are not unique (lattice ties); interior points: C = 2 h^2 I
    ids = out["matched_ids"].astype(np.int64)
    ref = surface_normal_ref(pts, ids, ids >= 0)
    g = interior
    h2 = (16 * LATTICE) ** 2
    assert np.all(ref["C"][g] == 2 * h2 * np.eye(3)), "precondition: a triple eigenvalue"
    vec = out["eig_vectors"][g].reshape(-1, 3, 3)
    _eig_check(out["eig_values"][g], vec, ref["C"][g], ref["w"][g], ref["V"][g], ref["trace"][g],
               np.full(len(g), 7.0), eps_of(pts), gap_rule=False)
    assert np.all(out["eig_values"][g] == dtype(2 * h2)), "lattice scene: bit-exact"


def run_radius(be, dtype, D):
    pts = pairs_scene(dtype, D)
    out = run_all_degenerate(be, pts, 5, PAIR_SELF_ONLY)
    ids = out["matched_ids"].astype(np.int64)
    assert np.array_equal(ids[:, 0], np.arange(len(pts))) and np.all(ids[:, 1:] == -1), "real = 1"
    out = be.surface_normals(pts, 5, PAIR_BOTH)
    assert np.all((out["matched_ids"] >= 0).sum(axis=1) == 2), "real = 2"
    check_surface_normals(out, pts, 5, PAIR_BOTH, expect="all" if D == 3 else "none")


def run_nan_point(be, cloud, k, at=777):
    bad = np.insert(cloud, at, np.array([np.nan, 0.5, -0.25, 1.0], cloud.dtype), axis=0)
    a = be.surface_normals(cloud, k, np.inf)
    b = be.surface_normals(bad, k, np.inf)
    ids = b["matched_ids"].astype(np.int64)
    assert np.all(ids[at] == -1), "a non-finite query matches nothing"
    assert not np.any(ids == at), "the non-finite point is nobody's neighbour"
    assert b["degenerate"] == a["degenerate"] + 1
    assert np.all(b["eig_values"][at] == 0) and np.all(b["eig_vectors"][at] == 0) and b["densities"][at] == 0
    assert np.all(b["normals"][at] == 0) and b["mean_dists"][at] == cloud.dtype.type(18446744073709551615.0)
    rest = np.delete(np.arange(len(bad)), at)
    back = np.where(ids > at, ids - 1, ids)[rest]
    assert np.array_equal(back, a["matched_ids"].astype(np.int64))
    for name in ("normals", "densities", "eig_values", "eig_vectors", "mean_dists"):
        assert np.array_equal(b[name][rest], a[name]), name
    check_surface_normals(a, cloud, k, skip_cap=SKIP_CAP)


def run_permuted(be, cloud, k):
    perm = np.random.default_rng(5).permutation(len(cloud))
    a = be.surface_normals(cloud, k, np.inf)
    b = be.surface_normals(np.ascontiguousarray(cloud[perm]), k, np.inf)  # b's point j is a's point perm[j]
    assert b["degenerate"] == a["degenerate"]
    assert np.array_equal(perm[b["matched_ids"].astype(np.int64)], a["matched_ids"].astype(np.int64)[perm])
    for name in ("normals", "densities", "eig_values", "eig_vectors", "mean_dists"):
        assert np.array_equal(b[name], a[name][perm]), name
    check_surface_normals(a, cloud, k, skip_cap=SKIP_CAP)


def run_wall(be, dtype):
    pts = wall_scene(dtype)
    out = be.surface_normals(pts, 5, np.inf)
    check_surface_normals(out, pts, 5, expect="none")
    assert np.all(out["eig_values"][:, 0] == 0) and np.all(out["normals"] == np.array([1, 0], dtype))


SSN_SIZES = ["knn", "knn+1", "2knn+1", 1000, 3001]


def ssn_size(tag, knn):
    return {"knn": knn, "knn+1": knn + 1, "2knn+1": 2 * knn + 1}.get(tag, tag)


def run_ssn(be, pts, desc, knn, method, ratio=0.6, max_box=np.inf, average=True, fit_by=None, seed=1234,
            skip_cap=0.0):
    be.srand(seed)
    out = be.ssn(pts, desc, knn, method, ratio, max_box, average)
    _libc.srand(seed)
    ref = ssn_ref(pts, desc, knn, method, ratio, max_box, average, fit_by=fit_by)
    share = check_ssn(out, ref, pts, desc is not None, skip_cap)
    return out, ref, share


def run_voxel(be, name, dtype, centroid, average):
    pts, desc, vs = voxel_scenes(dtype)[name]
    gf, gd = be.voxel(pts, desc, vs, centroid, average)
    rf, rd = voxel_ref(pts, desc, vs, centroid, average)
    assert gf.shape == rf.shape and np.array_equal(gf, rf), "features"
    if desc is not None:
        assert gd.shape == rd.shape and np.array_equal(gd, rd), "descriptors"
    return rf

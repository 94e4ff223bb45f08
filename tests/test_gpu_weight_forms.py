"""A reduction's inline weight is the materialised weight.

The chain's weight of one match entry (distance predicates x robust value x
the SurfaceNormal 0/1) is evaluated inline by every minimiser reduction and
by the covariance, and written out as an array only for get_weights().  This
pins that the two agree: the ErrorElements counts each system reports are the
counts of the array get_weights() returns, and the weight sum is the array's
sum over the kept entries.

Only the public context is used.  Every system is called before
get_weights() (inline evaluation everywhere but the point-to-point kernels
under a robust point-to-plane distance, which always read the array) and
after it (the array is resident).

Bars: the counts are integers and equal.  sum_w and fsum(w[kept]) are fp64
sums of the same N k values of T in different orders, each within
N k 2^-53 fsum of the exact sum, hence within N k 2^-52 fsum of each other.

Shapes: 3-D, M = 6000 with normals; N = 4099 (no multiple of 256, so the
k = 1 unrolled rounds end in a partial one); k = 1, 3, 5, one per code path
of the point-to-plane reduction and the covariance; max_dist = 0.5, which
leaves entries at (inf, -1), and three reading points moved about 3 units off
every surface, whose entries are all invalid whatever the chain.
"""
import math

import numpy as np
import pytest

from libpointmatcher_amd import _capi
from libpointmatcher_amd.synth import reading_cloud, reference_cloud, surface, t_gt

pytestmark = pytest.mark.gpu

M, N, MAX_DIST = 6000, 4099, 0.5
TRIM = ("TrimmedDistOutlierFilter", {"ratio": 0.8})
MAXD = ("MaxDistOutlierFilter", {"maxDist": 0.4})
MIND = ("MinDistOutlierFilter", {"minDist": 0.1})
ROBUST, ROBUST_P2PL, SN = ("robust", {}), ("robust", {"point2plane": True}), ("normal", {})
CHAINS = {
    "trimmed": [TRIM],
    "maxdist+mindist": [MAXD, MIND],
    "robust": [ROBUST],
    "trimmed+robust": [TRIM, ROBUST],
    "robust_p2pl": [ROBUST_P2PL],
    "normal": [SN],
    "normal+trimmed": [SN, TRIM],
    "normal+robust": [SN, ROBUST],
}

_CACHE = {}


def clouds():
    """Reference with normals, reading, the reading's normals (float64; cast per
    test): the analytic normal of each reading point in the reading's frame, a
    fixed 30 % of them turned by a seeded angle in [0.3, 1.5] rad."""
    if not _CACHE:
        ref, nrm = reference_cloud(M, np.float64)
        rd = reading_cloud(N, np.float64)
        rd[-3:, :3] = [[-6.0, 0.0, 0.0], [-6.1, 0.2, -0.1], [-5.9, -0.3, 0.2]]  # (3 units from every face)
        _, n = surface(N, 2)  # (the reading's seed: the normals reading_cloud drops)
        rn = n @ t_gt()[:3, :3]  # (R_gt^T n per point)
        rng = np.random.default_rng(77)
        turn = rng.permutation(N)[: (3 * N) // 10]
        for j, a, x in zip(turn, rng.uniform(0.3, 1.5, turn.size), rng.normal(size=(turn.size, 3))):
            x = x / np.linalg.norm(x)
            K = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
            rn[j] = (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K) @ rn[j]
        _CACHE["c"] = (ref, nrm, rd, rn)
    return _CACHE["c"]


def small_step(dtype):
    """A solved increment for the covariance: 0.01 rad about z, a small translation."""
    T = np.eye(4)
    c, s = np.cos(0.01), np.sin(0.01)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [0.01, -0.02, 0.005]
    return T.astype(dtype)


def apply_chain(ctx, chain):
    for pos, (name, p) in enumerate(chain):
        if name == "robust":
            ctx.outlier_robust(pos, "cauchy", 1.0, np.inf, _capi.RS_MAD, 0.0, point2plane=p.get("point2plane", False))
        elif name == "normal":
            ctx.outlier_surface_normal(pos, max_angle=0.6)
        else:
            ctx.outlier(name, pos, **p)


def systems(ctx):
    """(name, Stats) of the three minimisers' systems for the resident match."""
    return [("p2plane", ctx.p2plane_system()[-1]), ("p2point", ctx.p2point_system()[-1]),
            ("similarity", ctx.p2point_similarity_system()[-1])]


@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_inline_weight_is_materialised_weight(dtype, k, chain):
    ref, nrm, rd, rn = (a.astype(dtype) for a in clouds())
    ctx = _capi.Context(0, dtype)
    try:
        ctx.set_reference(ref, nrm)
        ctx.set_reading(rd)
        ctx.set_reading_normals(rn)
        ctx.match(np.eye(4, dtype=dtype), knn=k, max_dist=MAX_DIST)
        apply_chain(ctx, CHAINS[chain])
        d, ids = ctx.get_matches()
        before = systems(ctx)
        pairs_before = ctx.p2plane_covariance(small_step(dtype))[2]
        w = ctx.get_weights()
        after = systems(ctx)
        pairs_after = ctx.p2plane_covariance(small_step(dtype))[2]
    finally:
        ctx.close()

    finite = np.isfinite(d)
    nz = w != 0
    kept = finite & nz
    want = dict(nonzero_weights=int(nz.sum()), kept=int(kept.sum()), rejected_matches=int((finite & ~nz).sum()),
                rejected_points=int((~kept.any(axis=1)).sum()))
    fsum = math.fsum(w[kept].astype(np.float64))
    bound = N * k * 2.0 ** -52 * fsum
    print(f"entries {d.size}: invalid {int((~finite).sum())}, " + ", ".join(f"{a} {b}" for a, b in want.items())
          + f", fsum(w[kept]) {fsum!r}, bound {bound:.3e}")

    # the inputs hold what the comparison is about
    assert np.array_equal(ids < 0, ~finite)
    assert (~finite).any() and kept.any()
    assert want["rejected_points"] >= 1

    for when, stats in (("before", before), ("after", after)):
        for name, st in stats:
            got = {f: getattr(st, f) for f in want}
            print(f"  {when} get_weights, {name}: {got}, sum_w {st.sum_w!r} (diff {st.sum_w - fsum:.3e})")
            assert got == want, (when, name)
            assert abs(st.sum_w - fsum) <= bound, (when, name)
    assert pairs_before == want["kept"] and pairs_after == want["kept"]

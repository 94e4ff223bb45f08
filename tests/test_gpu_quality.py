"""ErrorMinimizer::getResidualError and getOverlap on the GPU, at the C ABI:
pmx_match_quality / pmx_loop_quality with pmx_set_reading_noise and
pmx_set_reference_descriptors.

The yardstick is quality_cases.restate: the reference's lines in numpy, fed
with the matches and weights read back through pmx_get_matches /
pmx_get_weights and the match's transform.  65 and 130 reading points (one
wave plus a tail; past one block's first round), k = 1 (the neighbour records,
and the id gather with nbr_cache = 0) and k = 3 (id gather, the any-link rule).

Bars: the residual's relative error 1e-5 (f32) / 1e-12 (f64), the project's
parity bars (every term is non-negative: no cancellation).  Every count and
the median density are equal to the restatement's: the comparisons are on the
resident distances in fixed-order T arithmetic.  Point-to-point's threshold
holds a float64 sum whose order differs from numpy's, so the fixture is first
checked to keep every link at least 1e-6 relative away from it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import quality_cases as Q  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KINDS = [Q.PLANE, Q.POINT, Q.SIM]
CHAINS = ["trim", "robust", "maxdist"]
MAX_DIST = 0.03  # about a fifth of the reading points have no reference point this near


def run_chain(ctx, chain, knn, dtype):
    from libpointmatcher_amd import _capi
    ctx.match(np.asarray(Q.T_AT, dtype), knn=knn, max_dist=MAX_DIST if chain == "maxdist" else np.inf)
    if chain == "trim":
        ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    elif chain == "robust":  # real weights; the approximation zeroes the far pairs
        ctx.outlier_robust(0, "cauchy", 0.5, 1.5, _capi.RS_MAD, 0.0)
    # ("maxdist": the empty chain, w = dist != inf)


@pytest.fixture(scope="module")
def descriptors():
    """Per (dtype name, n_rd): the clouds, the reading's noise (sensor model 0),
    the reference's (model 2) and its densities (pmx_surface_normals)."""
    from libpointmatcher_amd import _capi
    out = {}
    for dtype in DTYPES:
        for n_rd in (65, 130):
            rd, ref, nrm = Q.clouds(n_rd, dtype)
            dens = _capi.surface_normals(ref, knn=8)["densities"]
            assert np.isfinite(dens).all() and (dens > 0).all()
            out[np.dtype(dtype).name, n_rd] = (rd, ref, nrm, Q.sensor_noise(rd, 0, dtype),
                                               Q.sensor_noise(ref, 2, dtype), dens)
    return out


def check(tag, got, want, dn):
    print(f"{tag}: residual {got.residual:.9g}/{want['residual']:.9g} links {got.links}/{want['links']} "
          f"overlap {got.overlap_num}/{got.overlap_den} want {want['num']}/{want['den']} branch {got.branch} "
          f"median {got.median_density!r}/{want['median_density']!r} margin {want['margin']:.3g}")
    assert got.branch == want["branch"], tag
    assert got.links == want["links"], tag
    assert Q.rel(got.residual, want["residual"]) <= Q.BAR[dn], tag
    assert Q.rel(got.dist_sum, want["dist_sum"]) <= Q.BAR[dn], tag
    assert want["margin"] >= 1e-6, tag  # (the fixture, not the code under test)
    assert (got.overlap_num, got.overlap_den) == (want["num"], want["den"]), tag
    assert got.median_density == want["median_density"], tag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rd", [65, 130])
@pytest.mark.parametrize("chain", CHAINS)
def test_module_path_matches_restatement(descriptors, dtype, n_rd, chain):
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    rd, ref, nrm, n_rd_noise, n_ref_noise, dens = descriptors[dn, n_rd]
    p = Q.xform3(np.asarray(Q.T_AT, dtype), rd)
    for knn, nbr_cache in ((1, 1), (1, 0), (3, 1)):
        ctx = _capi.Context(0, dtype)
        ctx.set_option("nbr_cache", nbr_cache)
        ctx.set_reference(ref, nrm)
        ctx.set_reading(rd)
        run_chain(ctx, chain, knn, dtype)
        kept = ctx.p2plane_system()[2].kept  # (the minimiser's own inline kept rule, pmx_stats)
        d, ids = ctx.get_matches()
        w = ctx.get_weights()
        base = f"{dn} n={n_rd} {chain} knn={knn} nbr={nbr_cache}"
        plain = Q.restate(d, ids, w, p, ref, nrm, dtype, True)
        assert 6 < plain["links"] < d.size, base  # (the chain rejects something and keeps enough)
        if chain == "maxdist":
            assert plain["rejected"] > 0, base
        if chain == "robust":
            assert ((w != 0) & (w != 1)).any(), base
        # the four point-to-plane branches, then no noise at all
        for rn, fn, fd in ((1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 1)):
            ctx.set_reading_noise(n_rd_noise if rn else None)
            ctx.set_reference_descriptors(n_ref_noise if fn else None, dens if fd else None)
            kw = dict(noise_rd=n_rd_noise if rn else None, noise_ref=n_ref_noise if fn else None,
                      dens=dens if fd else None)
            for kind in KINDS:
                plane = kind == Q.PLANE
                want = Q.restate(d, ids, w, p, ref, nrm, dtype, plane, **kw)
                got = ctx.match_quality(kind)
                check(f"{base} {kind} noise={rn}{fn}{fd}", got, want, dn)
                assert got.links == kept, base  # (the materialised weights keep what the reduction keeps)
                if not (rn or fn):
                    assert got.branch == 0 and got.overlap_num == 0 and got.overlap_den == 0
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_explicit_step_transform_and_cov_kind(descriptors, dtype):
    """T_step given explicitly equals the match's own; WithCov is PointToPlane."""
    from libpointmatcher_amd import _capi
    rd, ref, nrm, n_rd_noise, n_ref_noise, dens = descriptors[np.dtype(dtype).name, 130]
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.set_reading_noise(n_rd_noise)
    ctx.set_reference_descriptors(n_ref_noise, dens)
    run_chain(ctx, "trim", 1, dtype)
    a = ctx.match_quality(Q.PLANE)
    b = ctx.match_quality(Q.COV, T_step=np.asarray(Q.T_AT, dtype))
    for f, _ in a._fields_:
        assert getattr(a, f) == getattr(b, f), f
    # a new reading clears its noise; a new reference its descriptors
    ctx.set_reading(rd)
    run_chain(ctx, "trim", 1, dtype)
    assert ctx.match_quality(Q.PLANE).branch == Q.REFERENCE
    assert ctx.match_quality(Q.POINT).branch == Q.NONE
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    run_chain(ctx, "trim", 1, dtype)
    assert ctx.match_quality(Q.PLANE).branch == Q.NONE
    ctx.close()


def test_errors_are_statuses():
    from libpointmatcher_amd import _capi
    rd, ref, nrm = Q.clouds(65, np.float32)
    ctx = _capi.Context(0, np.float32)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    with pytest.raises(_capi.PmxError):  # PMX_E_STATE: no match yet
        ctx.match_quality(Q.PLANE)
    with pytest.raises(_capi.PmxError):  # PMX_E_STATE: no loop has run
        ctx.loop_quality(Q.PLANE)
    ctx.loop_begin(filters=[("TrimmedDistOutlierFilter", 0.85)], checkers=[("CounterTransformationChecker", 4)])
    with pytest.raises(_capi.PmxError):  # begun, not finished
        ctx.loop_quality(Q.PLANE)
    ctx.close()
    # point-to-plane's residual needs the reference normals
    ctx = _capi.Context(0, np.float32)
    ctx.set_reference(ref)
    ctx.set_reading(rd)
    ctx.match(np.eye(4, dtype=np.float32), knn=1)
    with pytest.raises(_capi.InvalidParameter):
        ctx.match_quality(Q.PLANE)
    assert ctx.match_quality(Q.POINT).links == 65
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_device_loop_equals_module_path(descriptors, dtype, kind):
    from libpointmatcher_amd import _capi
    dn = np.dtype(dtype).name
    rd, ref, nrm, n_rd_noise, n_ref_noise, dens = descriptors[dn, 130]
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    ctx.set_reading_noise(n_rd_noise)
    ctx.set_reference_descriptors(n_ref_noise, dens)
    ctx.loop_begin(filters=[("TrimmedDistOutlierFilter", 0.85)], minimizer=kind,
                   checkers=[("CounterTransformationChecker", 4)], keep_trace=True)
    st = ctx.loop_run(10)
    assert st.done and st.iterations == 4
    loop = ctx.loop_quality(kind)
    tr = ctx.loop_trace(0, 4)
    # the module path: the fourth iteration's match ran at the third's transform
    ctx.set_reading(rd)
    ctx.set_reading_noise(n_rd_noise)
    ctx.match(tr[2], knn=1)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    mod = ctx.match_quality(kind)
    d, ids = ctx.get_matches()
    want = Q.restate(d, ids, ctx.get_weights(), Q.xform3(tr[2], rd), ref, nrm, dtype, kind == Q.PLANE,
                     noise_rd=n_rd_noise, noise_ref=n_ref_noise, dens=dens)
    ctx.close()
    check(f"{dn} {kind} module", mod, want, dn)
    check(f"{dn} {kind} loop", loop, want, dn)
    for f in ("overlap_num", "overlap_den", "links", "branch", "median_density"):
        assert getattr(loop, f) == getattr(mod, f), f
    assert Q.rel(loop.residual, mod.residual) <= Q.BAR[dn]

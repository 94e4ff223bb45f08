"""plan_grid_match (csrc/pmx_match_plan.h): which form of the grid match runs,
with which list size, reuse mode, neighbour records, window and counter sum.

The table below was written by hand from the rules as they stood spread over
match_impl, launch_grid_match, launch_kt and the kernels before the plan
existed; it is not produced by the function under test.  No GPU: the header
is plain C++, built into a shim with g++ (helpers.match_plan).
"""
import itertools
import shutil

import pytest

from helpers import match_plan

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ builds tests/match_plan_shim.cpp")

WIDE, TABLE, COLD, LANE, BOTH = range(5)  # MatchForm

# a warm k = 1 match: per-lane mode, reuse on, the previous match of this
# reading at this level with this k, which wrote its neighbour records
BASE = dict(grid_mode=1, knn=1, N=1000, reuse_on=1, nbr_on=1, safe_valid=1, have_match=1, ids_grid=1, prev_knn=1,
            same_level=1, nbr_prev=1, level_normals=1, loop_on=0, tile_dispatch=0, window_on=0, step_counters=0,
            have_counters=1)
BASE_PLAN = dict(form=LANE, run=1, reuse=2, kt=2, nbr=1, nbr_normals=1, window=0, counter_sum=1, safe_valid=1,
                 nbr_prev=1)
NO_NBR = dict(nbr=0, nbr_normals=0, nbr_prev=0)
NO_REUSE = dict(reuse=0, safe_valid=0, **NO_NBR)
NO_PREV = dict(have_match=0)


def warm(k):
    return dict(knn=k, prev_knn=k)


# (facts that differ from BASE, plan fields that differ from BASE_PLAN)
TABLE_ROWS = [
    ({}, {}),
    # k against the list size: with reuse the list keeps the (k+1)-th entry, up to 16
    (warm(2), dict(kt=4, **NO_NBR)),
    (warm(3), dict(kt=4, **NO_NBR)),
    (warm(4), dict(kt=5, **NO_NBR)),
    (warm(5), dict(kt=8, **NO_NBR)),
    (warm(7), dict(kt=8, **NO_NBR)),
    (warm(8), dict(kt=16, **NO_NBR)),
    (warm(15), dict(kt=16, **NO_NBR)),
    (warm(16), dict(kt=16, **NO_NBR)),  # (no room for the 17th: never certifies)
    (warm(17), dict(form=WIDE, kt=0, **NO_REUSE)),
    # ... the cold tile keeps k entries
    (dict(**NO_PREV), dict(form=COLD, reuse=1, kt=1)),
    (dict(**warm(3), **NO_PREV), dict(form=COLD, reuse=1, kt=4, **NO_NBR)),
    (dict(**warm(4), **NO_PREV), dict(form=COLD, reuse=1, kt=4, **NO_NBR)),
    (dict(**warm(15), **NO_PREV), dict(form=COLD, reuse=1, kt=16, **NO_NBR)),
    (dict(**warm(16), **NO_PREV), dict(form=COLD, reuse=1, kt=16, **NO_NBR)),
    (dict(**warm(17), **NO_PREV), dict(form=WIDE, kt=0, **NO_REUSE)),
    # ... and so does a match without reuse (never cold: nothing is stored)
    (dict(reuse_on=0), dict(kt=1, **NO_REUSE)),
    (dict(reuse_on=0, **NO_PREV), dict(kt=1, **NO_REUSE)),
    (dict(reuse_on=0, **warm(3)), dict(kt=4, **NO_REUSE)),
    (dict(reuse_on=0, **warm(4)), dict(kt=4, **NO_REUSE)),
    (dict(reuse_on=0, **warm(5)), dict(kt=5, **NO_REUSE)),
    (dict(reuse_on=0, **warm(15)), dict(kt=16, **NO_REUSE)),
    (dict(reuse_on=0, **warm(16)), dict(kt=16, **NO_REUSE)),
    (dict(reuse_on=0, **warm(17)), dict(form=WIDE, kt=0, **NO_REUSE)),
    # grid_mode 0: the table's tiles, no reuse, never cold; the wide search all the same
    (dict(grid_mode=0), dict(form=TABLE, kt=1, **NO_REUSE)),
    (dict(grid_mode=0, **NO_PREV), dict(form=TABLE, kt=1, **NO_REUSE)),
    (dict(grid_mode=0, **warm(3)), dict(form=TABLE, kt=4, **NO_REUSE)),
    (dict(grid_mode=0, **warm(4)), dict(form=TABLE, kt=4, **NO_REUSE)),
    (dict(grid_mode=0, **warm(15)), dict(form=TABLE, kt=16, **NO_REUSE)),
    (dict(grid_mode=0, **warm(17)), dict(form=WIDE, kt=0, **NO_REUSE)),
    # the previous match: none (above), unusable, with another k, at another level
    (dict(safe_valid=0), dict(form=COLD, reuse=1, kt=1)),
    (dict(ids_grid=0), dict(form=COLD, reuse=1, kt=1)),
    (dict(prev_knn=3), dict(form=COLD, reuse=1, kt=1)),
    (dict(knn=3, prev_knn=1), dict(form=COLD, reuse=1, kt=4, **NO_NBR)),
    (dict(same_level=0), dict(reuse=1)),
    (dict(same_level=0, **warm(3)), dict(reuse=1, kt=4, **NO_NBR)),
    # neighbour records (k = 1): read by a certifying match only if the last match wrote them ...
    (dict(nbr_on=0), NO_NBR),
    (dict(nbr_prev=0), NO_NBR),
    (dict(nbr_prev=0, same_level=0), dict(reuse=1)),  # (nothing is read: written for the next match)
    (dict(nbr_prev=0, **NO_PREV), dict(form=COLD, reuse=1, kt=1)),
    # ... except in the device loop, where every match writes them; not under tile dispatch
    (dict(loop_on=1), {}),
    (dict(loop_on=1, nbr_prev=0), {}),
    (dict(loop_on=1, nbr_on=0), NO_NBR),
    (dict(loop_on=1, tile_dispatch=1), dict(form=BOTH, **NO_NBR)),
    (dict(loop_on=1, tile_dispatch=1, nbr_prev=0), dict(form=BOTH, **NO_NBR)),
    (dict(loop_on=1, tile_dispatch=1, same_level=0), dict(form=BOTH, reuse=1, **NO_NBR)),
    (dict(loop_on=1, tile_dispatch=1, **warm(3)), dict(form=BOTH, kt=4, **NO_NBR)),
    (dict(loop_on=1, tile_dispatch=1, **NO_PREV), dict(form=COLD, reuse=1, kt=1, **NO_NBR)),
    (dict(loop_on=1, tile_dispatch=1, reuse_on=0), dict(kt=1, **NO_REUSE)),
    (dict(loop_on=1, tile_dispatch=1, **warm(17)), dict(form=WIDE, kt=0, **NO_REUSE)),
    (dict(loop_on=0, tile_dispatch=1), {}),  # (the loop's setting means nothing outside it)
    # a level without normals: the records carry the points only
    (dict(level_normals=0), dict(nbr_normals=0)),
    (dict(level_normals=0, **NO_PREV), dict(form=COLD, reuse=1, kt=1, nbr_normals=0)),
    (dict(level_normals=0, nbr_on=0), NO_NBR),
    # the window needs the per-lane mode and the counters
    (dict(window_on=1), dict(window=1)),
    (dict(window_on=1, **NO_PREV), dict(form=COLD, reuse=1, kt=1, window=1)),
    (dict(window_on=1, **warm(17)), dict(form=WIDE, kt=0, window=1, **NO_REUSE)),
    (dict(window_on=1, have_counters=0), dict(window=0, counter_sum=0)),
    (dict(window_on=1, grid_mode=0), dict(form=TABLE, kt=1, window=0, **NO_REUSE)),
    (dict(have_counters=0), dict(counter_sum=0)),
    # merge_counter / step_counter: a later launch folds the counters
    (dict(step_counters=1), dict(counter_sum=0)),
    (dict(step_counters=1, window_on=1), dict(window=1, counter_sum=0)),
    # an empty reading launches nothing; the bookkeeping is the same
    (dict(N=0), dict(run=0, counter_sum=0)),
]


@pytest.mark.parametrize("row", range(len(TABLE_ROWS)))
def test_truth_table(row):
    facts, want = TABLE_ROWS[row]
    got = match_plan()({**BASE, **facts})
    assert got == {**BASE_PLAN, **want}, facts


def test_invariants():
    """Every combination of the boolean facts, knn in the table's set, the
    previous k equal or not.  The list-size invariants speak of the forms that
    keep a per-lane list: the wide search (knn > 16) has none (kt = 0)."""
    plan = match_plan()
    bools = ["reuse_on", "nbr_on", "safe_valid", "have_match", "ids_grid", "same_level", "nbr_prev", "level_normals",
             "loop_on", "tile_dispatch", "window_on", "step_counters", "have_counters"]
    n = 0
    for grid_mode, knn, same_k in itertools.product((0, 1), (1, 3, 4, 15, 16, 17), (0, 1)):
        for bits in itertools.product((0, 1), repeat=len(bools)):
            f = dict(zip(bools, bits), grid_mode=grid_mode, knn=knn, prev_knn=knn if same_k else knn + 1, N=5)
            p = plan(f)
            n += 1
            usable = f["safe_valid"] and f["have_match"] and f["ids_grid"] and same_k
            cold = p["form"] == COLD
            assert p["form"] in (WIDE, TABLE, COLD, LANE, BOTH)
            assert (p["form"] == WIDE) == (knn > 16), f
            if p["form"] in (COLD, BOTH):
                assert grid_mode >= 1, f
            if p["form"] == TABLE:
                assert grid_mode == 0, f
            if p["reuse"] == 2:
                assert usable and f["same_level"], f
            assert p["reuse"] in (0, 1, 2)
            if p["nbr"]:
                assert knn == 1 and p["reuse"] != 0, f
            if p["nbr_normals"]:
                assert p["nbr"] and f["level_normals"], f
            if p["form"] != WIDE:
                assert p["kt"] in (1, 2, 4, 5, 8, 16) and p["kt"] >= knn, f
                if p["reuse"] != 0 and not cold and knn < 16:
                    assert p["kt"] > knn, f
            if p["window"]:
                assert f["have_counters"] and grid_mode >= 1, f
            if p["counter_sum"]:
                assert f["have_counters"] and not f["step_counters"], f
            assert p["safe_valid"] == (p["reuse"] != 0) and p["nbr_prev"] == p["nbr"], f
    assert n == 2 * 6 * 2 * 2 ** len(bools)

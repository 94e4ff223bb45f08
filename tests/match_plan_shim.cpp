// Test-only shim: plan_grid_match (csrc/pmx_match_plan.h) behind a flat C
// function, for tests/test_match_plan.py.  helpers.match_plan() builds it on
// demand with g++ and loads it with ctypes; the product never links it.
#include "pmx_match_plan.h"

// facts: grid_mode, knn, N, reuse_on, nbr_on, safe_valid, have_match, ids_grid,
//        prev_knn, same_level, nbr_prev, level_normals, loop_on, tile_dispatch,
//        window_on, step_counters, have_counters
// plan:  form, run, reuse, kt, nbr, nbr_normals, window, counter_sum,
//        safe_valid, nbr_prev
extern "C" void pmx_plan_grid_match(const long long* in, int* out) {
    pmx::MatchFacts f;
    f.grid_mode = (int)in[0];
    f.knn = (int)in[1];
    f.N = in[2];
    f.reuse_on = in[3] != 0;
    f.nbr_on = in[4] != 0;
    f.safe_valid = in[5] != 0;
    f.have_match = in[6] != 0;
    f.ids_grid = in[7] != 0;
    f.prev_knn = (int)in[8];
    f.same_level = in[9] != 0;
    f.nbr_prev = in[10] != 0;
    f.level_normals = in[11] != 0;
    f.loop_on = in[12] != 0;
    f.tile_dispatch = in[13] != 0;
    f.window_on = in[14] != 0;
    f.step_counters = in[15] != 0;
    f.have_counters = in[16] != 0;
    const pmx::GridMatchPlan p = pmx::plan_grid_match(f);
    out[0] = (int)p.form;
    out[1] = p.run;
    out[2] = p.reuse;
    out[3] = p.kt;
    out[4] = p.nbr;
    out[5] = p.nbr_normals;
    out[6] = p.window;
    out[7] = p.counter_sum;
    out[8] = p.safe_valid;
    out[9] = p.nbr_prev;
}

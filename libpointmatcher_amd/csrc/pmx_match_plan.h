// pmx_match_plan.h — which form of the grid match runs, and with what.
//
// Plain C++ (no HIP): plan_grid_match is the one place the host's rules are
// written.  match_grid (pmx_chain.hip) reads the facts off the context and
// takes its bookkeeping from the plan, launch_grid_match (pmx_grid.hip)
// launches what the plan says ("The grid match's plan").  Where the
// device takes over (LoopCtl::use_tile, level, prev_level) is noted at the field.
#pragma once

#include <cstdint>

namespace pmx {

constexpr int kLaneMaxK = 16;  // the per-lane searches' largest k-list (wider: the wave-per-query search)

// what match_grid knows before the match
struct MatchFacts {
    int grid_mode = 1;  // option grid_mode: 0 the wave table's tiles, >= 1 the per-lane search
    int knn = 1;
    int64_t N = 0;                           // queries of this rank
    bool reuse_on = false, nbr_on = false;   // options grid_reuse, nbr_records
    // the previous match of this reading, as the output buffers hold it
    bool safe_valid = false, have_match = false, ids_grid = false;
    int prev_knn = 0;
    bool same_level = false;  // it ran on the level this match runs on
    bool nbr_prev = false;    // it wrote the neighbour records
    bool level_normals = false;  // the level has interleaved point / normal records
    bool loop_on = false;        // device loop: the kernels read LoopCtl
    bool tile_dispatch = false;  // the loop's LoopCfg.tile_dispatch
    bool window_on = false;      // a quantile window is on (pmx_spec.h)
    bool step_counters = false;  // merge_counter || step_counter: a later launch folds the counters
    bool have_counters = false;  // the spread counters exist
};

enum class MatchForm {
    Wide,             // k > kLaneMaxK: a wave per query (pmx_knn_wide.hip), no reuse
    TableTile,        // grid_mode 0: the tile kernel over the reading's wave table
    ColdTile,         // a reading's first match under reuse: the tile kernel's cold form
    Lane,             // the per-lane shell search, with the reuse certificate in mode 2
    LaneAndWarmTile,  // tile dispatch: both enqueued, LoopCtl::use_tile picks one on the device
};

struct GridMatchPlan {
    MatchForm form = MatchForm::Lane;
    bool run = false;  // N > 0: anything is launched at all
    // 0 off, 1 store the safe radii, 2 and certify from the previous match
    int reuse = 0;     // (device loop: 1 / 2 from LoopCtl::prev_level == level)
    int kt = 0;        // the k-list's size, one of {1, 2, 4, 5, 8, 16} (Wide: 0, no per-lane list)
    bool nbr = false;  // k = 1 neighbour records are written (and read by the certificate)
    bool nbr_normals = false;  // ... with the neighbour's normal behind them
    bool window = false;       // the quantile window classifies the distances written
    bool counter_sum = false;  // the counter-sum kernel follows the match
    bool safe_valid = false, nbr_prev = false;  // what the context remembers of this match
};

inline GridMatchPlan plan_grid_match(const MatchFacts& f) {
    GridMatchPlan p;
    p.run = f.N > 0;
    // the output buffers hold the previous match of the same reading (same k) with its safe radii
    const bool no_prev = !(f.safe_valid && f.have_match && f.ids_grid && f.prev_knn == f.knn);
    if (f.reuse_on && f.grid_mode >= 1 && f.knn <= kLaneMaxK)  // (the wide search keeps no safe radii)
        p.reuse = !no_prev && f.same_level ? 2 : 1;
    // (a reuse match reads the records only if the last match wrote them; a
    // device-loop match decides reuse on the device, where every match of the
    // loop writes them.  Not for dense readings, tile dispatch: most queries
    // miss there, and the records' writes cost more than the certificate
    // saves, C5 1.51 vs 1.47 ms/iteration)
    p.nbr = p.reuse != 0 && f.knn == 1 && f.nbr_on && (p.reuse != 2 || f.nbr_prev || f.loop_on) &&
            !(f.loop_on && f.tile_dispatch);
    p.nbr_normals = p.nbr && f.level_normals;
    const bool cold = no_prev && f.reuse_on && f.grid_mode >= 1;  // a new reading's first match
    if (f.knn > kLaneMaxK)
        p.form = MatchForm::Wide;
    else if (cold)
        p.form = MatchForm::ColdTile;
    else if (f.grid_mode >= 1)  // (device loop: the step picks one of the two forms)
        p.form = f.loop_on && f.tile_dispatch && p.reuse ? MatchForm::LaneAndWarmTile : MatchForm::Lane;
    else
        p.form = MatchForm::TableTile;
    if (p.form != MatchForm::Wide) {
        // with reuse the list keeps room for the (k+1)-th point (the safe radius;
        // the cold tile writes radius 0 and keeps k entries)
        const int kl = p.reuse && f.grid_mode >= 1 && f.knn < 16 && !cold ? f.knn + 1 : f.knn;
        // (5: k = 4 with the (k+1)-th entry: 5 fit the 128-VGPR budget, 8 spilled)
        p.kt = kl == 1 ? 1 : kl <= 2 ? 2 : kl <= 4 ? 4 : kl <= 5 ? 5 : kl <= 8 ? 8 : 16;
    }
    // (the window needs the per-lane kernel and the counters)
    p.window = f.window_on && f.grid_mode >= 1 && f.have_counters;
    // (off: the counter phase is merged into the launch that follows the match)
    p.counter_sum = p.run && f.have_counters && !f.step_counters;
    p.safe_valid = p.reuse != 0;
    p.nbr_prev = p.nbr;
    return p;
}

}  // namespace pmx

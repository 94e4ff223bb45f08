// pmx_elements.h — ErrorMinimizer::getErrorElements of the last match
// (ErrorMinimizer.cpp:58-193): the kept pairs themselves, compacted on the
// device (pmx_elements.hip).
//
// A column is an entry (i, s) with dist != inf && w != 0, i the reading INDEX
// (not the slot) rising and s the link rank rising within i: the loop of
// ErrorMinimizer.cpp:98-135.  w is the chain's materialised weight (the
// mirror's array, pmx_weight.h), so a negative weight is a column and a zero
// one is not.
//
// The match and its weights live in slot order; the columns come out in index
// order through the inverse map index -> slot, built once per prepare
// (launch_elements_inverse; none when the reading is in index order).  Entry
// e' = i * k + s of the index order is decided by thread e' of blocks of
// kKeepBlock, reading slot entry inv[i] * k + s; the ballots, the block scan
// and the lane prefix are pmx_keep.hip's (keep_block_ballot, launch_keep_scan),
// so the compaction is stable, deterministic and free of float atomics.
#pragma once

#include "pmx_internal.h"

namespace pmx {

// the counters launch_elements_flag adds to (zeroed by the caller)
enum ElementsCounter { kElRejMatches = 0, kElRejPoints = 1, kElBadOrder = 2, kElCounters = 3 };

template <typename T>
struct ElementsIn {
    MatchView<T> m;
    const T* w;          // [N * k] slot order
    const int32_t* inv;  // [N] reading index -> slot (null: identity)
    int64_t ref_count;   // records m.ref / m.pn hold (ids beyond it are not gathered)
};

// the columns (device, capacity P each; any may be null)
template <typename T>
struct ElementsOut {
    T* reading;      // rows x P point-major: the step reading point
    T* reference;    // rows x P: the matched record
    T* ref_normals;  // D x P: its normal record
    T* dists;
    int32_t* ids;    // original reference indices
    T* weights;
    int32_t* reading_index;
    int32_t* link_rank;
};

// inv[order[s]] = s; entries of order outside [0, N) are counted in counters[kElBadOrder]
void launch_elements_inverse(const int32_t* order, int64_t N, int32_t* inv, unsigned long long* counters,
                             hipStream_t s);
// the ballots and block counts of the N * k entries in index order (sc sized
// for N * k), rejected matches and rejected points added to counters
template <typename T>
void launch_elements_flag(const ElementsIn<T>& in, const KeepScratch& sc, unsigned long long* counters, hipStream_t s);
// after launch_keep_scan(sc): the kept entries' columns; rows 3 (x, y, h) or 4
template <typename T>
void launch_elements_scatter(const ElementsIn<T>& in, const Mat4<T>& Tm, int rows, const KeepScratch& sc,
                             const ElementsOut<T>& out, hipStream_t s);

}  // namespace pmx

// pmx_octree_replay.h — the host side of OctreeGridDataPointsFilter's samplers
// (DataPointsFilters/OctreeGrid.cpp:48-137): plain C++, no device code, so a
// stand-alone program can include it.
//
// The reference moves the pick of leaf k (visit order) to column k with
// swapCols(k, j) and remembers in mapidx[k] the column it exchanged with; a
// pick d < k is looked up as mapidx[d].  That table is one level deep: a
// column displaced at step a to column c is displaced again at step c, and a
// later lookup of a still answers c.  The kept columns are therefore not always
// the picks.  octree_replay_columns restates the sequence on column numbers
// alone, stale lookups included.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

namespace pmx {

// picks[k] (< n): the input column the sampler chose for leaf k.  Returns, for
// each of the L kept columns, the input column it holds after the reference's
// swaps (OctreeGrid.cpp:55-67) and its conservativeResize(L).
inline std::vector<int32_t> octree_replay_columns(const int32_t* picks, int64_t L, int64_t n) {
    std::vector<int32_t> col((size_t)n), mapidx((size_t)L);
    for (int64_t i = 0; i < n; ++i) col[(size_t)i] = (int32_t)i;
    for (int64_t k = 0; k < L; ++k) {
        const int32_t d = picks[k];
        const int32_t j = d < k ? mapidx[(size_t)d] : d;
        std::swap(col[(size_t)k], col[(size_t)j]);
        mapidx[(size_t)k] = j;
    }
    col.resize((size_t)L);
    return col;
}

// RandomPtsSampler's draws (OctreeGrid.cpp:85-137): srand(1) when the sampler
// is built, one rand() per non-empty leaf in visit order, the factor
// float(rand() / float(RAND_MAX)), and srand(1) again in finalize — every call
// leaves the process's rand() state as srand(1) does.
inline void octree_rand_factors(int64_t L, float* out) {
    std::srand(1);
    for (int64_t k = 0; k < L; ++k) out[k] = (float)(std::rand() / (float)RAND_MAX);
    std::srand(1);
}

}  // namespace pmx

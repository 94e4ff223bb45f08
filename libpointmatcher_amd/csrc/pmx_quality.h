// pmx_quality.h — ErrorMinimizer::getResidualError and getOverlap of the last
// match (ErrorMinimizers/PointToPlane.cpp:316-465, PointToPoint.cpp:104-164,
// PointToPointSimilarity.cpp:101-150) as reductions over the resident match
// (pmx_quality.hip); values: QualitySums of pmx_sums.h.
//
// A link (slot i, rank s) is a column of ErrorElements when dist != inf and
// w != 0 (ErrorMinimizer.cpp:75-131), w the chain's materialised weight (the
// mirror's array: entry_weight of every entry, pmx_weight.h).  Per kept link, every product and sum in T,
// separately rounded, in the reference's order, widened to double and added
// in fp64:
//   point-to-plane residual  w * (e * e), e = ((d0 n0) + (d1 n1)) + (d2 n2),
//                            d = p - q, p the step reading point (xform3);
//                            2-D clouds in the embedded form (the z terms are
//                            exactly 0)
//   point-to-point residual  sqrt(dist): the match's own squared distance (the
//                            homogeneous row adds (1 - 1)^2 = 0), unweighted
//   links, sum sqrt(dist), reading points with / without a kept link
// The second pass counts, against an uncertainty in T:
//   point-to-plane  the reading points with a kept link whose
//                   sqrt(dist) < u, u by QualityBranch
//   point-to-point  the kept links with sqrt(dist) < mean + noise_rd[i]
#pragma once

#include "pmx_internal.h"

namespace pmx {

// the branch of getOverlap the descriptors present select (PointToPlane.cpp:
// 390-425); point-to-point knows kQBNone and kQBReading only (PointToPoint.cpp:131)
enum QualityBranch {
    kQBNone = 0,     // no noise: the caller falls back to the weighted used ratio
    kQBDensity = 1,  // u = (medianRadius + noise_rd[i]) + noise_ref[id]
    kQBBoth = 2,     // u = noise_rd[i] + noise_ref[id]
    kQBReading = 3,  // u = noise_rd[i]
    kQBReference = 4 // u = noise_ref[id]
};

// The resident match (m; point-to-plane reads m.pn / m.nrm, or m.nbr at
// k = 1), its materialised weights and the descriptors the reductions read;
// m.gidx maps the ids to the original reference ids the descriptors are in.
template <typename T>
struct QualityIn {
    MatchView<T> m;
    const T* w;
    const T* noise_rd;     // [N] slot order, or null
    const T* noise_ref;    // [M] original id order, or null
    const T* dens_ref;     // [M] original id order, or null
};

// First pass: QualitySums::kPass1NV per-block partials.  plane: the
// point-to-plane residual (needs the normals), else point-to-point's.  keys
// (may be null): [N * k], the reference density of every kept link, +inf for
// the others (the median's input).
template <typename T>
void launch_match_quality(const QualityIn<T>& in, const Mat4<T>& Tm, bool plane, T* keys, double* partials,
                          hipStream_t s);
// Second pass: one value (QualitySums::kHits).  base: medianRadius
// (kQBDensity) or point-to-point's mean distance.
template <typename T>
void launch_match_overlap(const QualityIn<T>& in, bool plane, int branch, T base, double* partials, hipStream_t s);
// keys[(size_t)(P * 0.5)] of the ascending order of keys[0, n) (nth_element's
// element, PointToPlane.cpp:398-401), P <= n the number of finite-ranked
// entries the caller counted.  Allocates and frees its scratch; synchronises s.
template <typename T>
hipError_t quality_median(const T* keys, int64_t n, int64_t P, T* median, hipStream_t s);

}  // namespace pmx

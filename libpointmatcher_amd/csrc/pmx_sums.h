// pmx_sums.h — the layout of the error minimisers' sums, once, for host and
// device: the reduction kernels' accumulators (pmx_reduce.hip, pmx_p2plane.h,
// pmx_cov.hip, pmx_quality.hip), the result area they are finalized into
// (pmx_ctx.d_result) and its readers, the device step (pmx_step.h) and the host
// readback (pmx_chain.hip).
// Accumulator v lands at result[base + v]; base is 0, kPass2At, kCovAt or QualitySums::kAt.
#pragma once

#if defined(__HIPCC__)
#define PMX_SUMS_HD __host__ __device__ __forceinline__
#else
#define PMX_SUMS_HD inline
#endif

namespace pmx {

constexpr int kNVMax = 48;           // accumulators of one reduction at most (d_partials: kRedBlocks x kNVMax)
constexpr int kStepRes = kNVMax;     // doubles of the result area the device step reads, from 0
constexpr int kResultDoubles = 128;  // the result area: the doubles ahead of the select state (kBlkSel)

// The ErrorElements block (ErrorMinimizer.cpp:133-192), at a form's kStats
// (point-to-point's ends at kRejPoints: its sum of the weights is kSw).
enum { kKept, kNonzero, kRejMatches, kRejPoints, kSumW };
struct SumStats {
    double kept, nz, rejM, rejP, sw;
};

// Point-to-plane: A row-major (FULL: the NF x NF product of a robust chain's
// real weights; otherwise the upper triangle, r <= c), b, the ErrorElements block.
template <int DIM, bool FULL>
struct P2PlaneSums {
    static constexpr int NF = DIM == 3 ? 6 : 3;
    static constexpr int NS = FULL ? NF * NF : NF * (NF + 1) / 2;
    static constexpr int kB = NS, kStats = NS + NF, NV = kStats + kSumW + 1;
};
constexpr int p2plane_nv(int dim, bool full) {
    return dim == 3 ? (full ? P2PlaneSums<3, true>::NV : P2PlaneSums<3, false>::NV)
                    : (full ? P2PlaneSums<2, true>::NV : P2PlaneSums<2, false>::NV);
}

// Point-to-point.  Pass 1: sum w, sum w p, sum w q, the ErrorElements counts.
// Two passes: the centred moments sum (w qc_r) pc_c from kPass2At, the
// similarity minimiser's sigma behind them.  One pass (device loop, double):
// pass 1's sums and the raw moments sum (w q_r) p_c from kRaw.
struct P2PointSums {
    static constexpr int kSw = 0, kSp = 1, kSq = 4, kStats = 7;
    static constexpr int kPass1NV = kStats + kRejPoints + 1;
    static constexpr int kRaw = kPass1NV, kMomentsNV = kRaw + 9;
    static constexpr int kPass2At = 16, kPass2NV = 9, kPass2SimNV = kPass2NV + 1;
    static constexpr int kSigma = kPass2At + kPass2NV;
    static constexpr int moment(int r, int c) { return r * 3 + c; }  // (2-D: the top-left 2 x 2)
};

// PointToPlaneWithCov's estimate, behind what the step reads (the system and
// the statistics stay as the minimiser left them): the upper triangle of H
// (row-major, r <= c), the kept-pair count, the upper triangle of Q.
constexpr int kCovAt = 64;
constexpr int kCovTri = 21;
constexpr int kCovCount = kCovTri;
constexpr int kCovQ = kCovTri + 1;
constexpr int kCovNV = 2 * kCovTri + 1;

// getResidualError / getOverlap of the last match (pmx_quality.hip), behind the
// covariance: the first pass's sums over the kept links, then the second
// pass's count (the reading points hit, or point-to-point's links inside).
struct QualitySums {
    static constexpr int kAt = 112;
    enum { kResidual, kLinks, kSqrtSum, kPoints, kRejPoints, kPass1NV, kHits = kPass1NV, kNV };
};

static_assert(P2PointSums::kPass1NV == 11 && P2PointSums::kMomentsNV == 20 && P2PointSums::kSigma == 25, "layout");
static_assert(P2PlaneSums<3, true>::NV <= kNVMax && P2PlaneSums<3, false>::NV <= kNVMax &&
                  P2PlaneSums<2, true>::NV <= kNVMax && P2PlaneSums<2, false>::NV <= kNVMax &&
                  P2PointSums::kMomentsNV <= kNVMax && kCovNV <= kNVMax,
              "a reduction's partials hold kNVMax values");
static_assert(kStepRes == 48 && P2PlaneSums<3, true>::NV <= kStepRes && P2PointSums::kMomentsNV <= kStepRes &&
                  P2PointSums::kSigma < kStepRes,
              "the step reads the first kStepRes doubles");
static_assert(P2PointSums::kPass1NV <= P2PointSums::kPass2At, "pass 1 ends before the second pass's sums");
static_assert(kStepRes <= kCovAt && kCovAt + kCovNV <= kResultDoubles, "the covariance behind the step's area");
static_assert(kCovAt + kCovNV <= QualitySums::kAt && QualitySums::kAt + QualitySums::kNV <= kResultDoubles &&
                  QualitySums::kNV <= kNVMax,
              "the quality sums behind the covariance");

// The five statistics of a form's sums.
template <int DIM>
PMX_SUMS_HD SumStats p2plane_stats(const double* r, bool full) {
    const double* s = r + (full ? P2PlaneSums<DIM, true>::kStats : P2PlaneSums<DIM, false>::kStats);
    return {s[kKept], s[kNonzero], s[kRejMatches], s[kRejPoints], s[kSumW]};
}
PMX_SUMS_HD SumStats p2point_stats(const double* r) {
    const double* s = r + P2PointSums::kStats;
    return {s[kKept], s[kNonzero], s[kRejMatches], s[kRejPoints], r[P2PointSums::kSw]};
}

// The normal equations as T (PointToPlane.cpp:230, 243): A (NF x NF; the triangle
// mirrored: exactly symmetric with 0/1 weights), b = -(the sums' b).  Moves and casts only.
template <typename T, int DIM, bool FULL>
PMX_SUMS_HD void p2plane_unpack(const double* __restrict__ r, T* A, T* b) {
    using L = P2PlaneSums<DIM, FULL>;
    constexpr int NF = L::NF;
    if constexpr (FULL) {
#pragma unroll
        for (int i = 0; i < NF * NF; ++i) A[i] = (T)r[i];
    } else {
        int a = 0;
        for (int i = 0; i < NF; ++i)
            for (int j = i; j < NF; ++j, ++a) A[i * NF + j] = A[j * NF + i] = (T)r[a];
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) b[i] = (T)(-r[L::kB + i]);
}

}  // namespace pmx

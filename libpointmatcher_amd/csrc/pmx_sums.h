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

// PointToPlane's force2D / force4DOF (PointToPlane.cpp:177-210; the values of
// PMX_FORCE_*, pmx.h).
enum { kForceNone = 0, kForce2D = 1, kForce4DOF = 2 };
// force2D on a 3-D context: the 2-D form over the x, y rows of the transformed
// reading point, of the matched point and of its normal (dot has no z term), so
// the sums are P2PlaneSums<2, FULL> from the 2-D accumulation run on the 3-D
// records.  On a 2-D context it changes nothing.  This is the form (the DIM of
// P2PlaneSums and of the reduction) a context's dimension and the force select.
constexpr int p2plane_sums_dim(int dim, int force) { return force == kForce2D ? 2 : dim; }
// force4DOF (3-D only): F = [p_x n_y - p_y n_x; n], the rows F[2..5] of the 3-D
// form with the same dot, so x = (yaw, t) solves rows and columns kFirst.. of
// P2PlaneSums<3, FULL>; nothing else is accumulated.
struct P2Plane4DofSums {
    static constexpr int NF = 4, kFirst = 2;
};
// the unknowns of the step's system
constexpr int p2plane_nf(int dim, int force) {
    return force == kForce4DOF                  ? P2Plane4DofSums::NF
           : p2plane_sums_dim(dim, force) == 3 ? P2PlaneSums<3, false>::NF
                                               : P2PlaneSums<2, false>::NF;
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
static_assert(P2PlaneSums<3, true>::NV == 47 && P2PlaneSums<3, false>::NV == 32,
              "the 3-D triangle fills a 32-value transpose (block_store): a forced mode adds nothing to it");
static_assert(P2PlaneSums<2, true>::NV == 17 && P2PlaneSums<2, false>::NV == 14 && p2plane_sums_dim(3, kForce2D) == 2 &&
                  p2plane_sums_dim(3, kForce4DOF) == 3 && p2plane_sums_dim(2, kForce2D) == 2,
              "force2D reduces a 3-D context into the 2-D form");
static_assert(P2Plane4DofSums::kFirst + P2Plane4DofSums::NF == P2PlaneSums<3, false>::NF && p2plane_nf(3, kForce4DOF) == 4 &&
                  p2plane_nf(3, kForce2D) == 3 && p2plane_nf(3, kForceNone) == 6 && p2plane_nf(2, kForceNone) == 3,
              "the 4-DOF system is the trailing block of the 3-D one");
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

// force4DOF's normal equations from the 3-D form's sums: rows and columns
// P2Plane4DofSums::kFirst.. of p2plane_unpack<T, 3, FULL>'s A and b, the same
// values cast the same way (moves and casts only).
template <typename T, bool FULL>
PMX_SUMS_HD void p2plane_unpack_4dof(const double* __restrict__ r, T* A, T* b) {
    using L = P2PlaneSums<3, FULL>;
    constexpr int NF = L::NF, N4 = P2Plane4DofSums::NF, K = P2Plane4DofSums::kFirst;
    if constexpr (FULL) {
#pragma unroll
        for (int i = 0; i < N4; ++i)
#pragma unroll
            for (int j = 0; j < N4; ++j) A[i * N4 + j] = (T)r[(K + i) * NF + K + j];
    } else {
        int a = 0;  // (the triangle's index, walked as p2plane_unpack walks it)
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = i; j < NF; ++j, ++a)
                if (i >= K) A[(i - K) * N4 + (j - K)] = A[(j - K) * N4 + (i - K)] = (T)r[a];
    }
#pragma unroll
    for (int i = 0; i < N4; ++i) b[i] = (T)(-r[L::kB + K + i]);
}

}  // namespace pmx

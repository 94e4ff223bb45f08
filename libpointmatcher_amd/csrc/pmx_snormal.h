// pmx_snormal.h — the SurfaceNormalOutlierFilter's per-pair predicate
// (pointmatcher/OutlierFiltersImpl.cpp:225-285), shared by the weight kernel
// of the module path (pmx_snormal.hip) and the reductions (pmx_reduce.hip).
//
// The filter sees the step reading (ICP.cpp:381-390), whose normals are
// R_iter (R_0 n): R_0 n is resident (SNPred::rn, rounded to T at upload) and
// R_iter is applied here from the iteration's step transform, so no second
// copy of the normals exists.  Every product and sum is rounded to T
// separately and summed left to right, as the reference's dense products:
//   r_c   = (m_c0 n_0 + m_c1 n_1) + m_c2 n_2        (2-D: no third term)
//   |v|   = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2),  v^ = v / |v|
//   w     = |(a^_0 b^_0 + a^_1 b^_1) + a^_2 b^_2| < eps ? 0 : 1
// A zero normal normalises to NaN and `NaN < eps` is false: the pair is kept.
#pragma once

#include "pmx_internal.h"

namespace pmx {

// device loop: the reference normal records of this iteration's grid level
template <typename T>
__device__ __forceinline__ void sn_bind(SNPred<T>& p, const LoopCtl* ctl, const GridDesc<T>* gd) {
    if (ctl) {
        p.nrm = gd[ctl->level].gpn + 1;
        p.rs = 2;
    }
}

// rn: the reading point's resident normal; qn: the matched reference point's
// normal record; Tm: the step transform (embedded 4x4)
template <typename T>
__device__ __forceinline__ bool sn_pass(const SNPred<T>& p, const Mat4<T>& Tm, const P4<T>& rn, const P4<T>& qn) {
    T dot;
    if (p.dim == 3) {
        const T ax = (Tm.m[0] * rn.x + Tm.m[1] * rn.y) + Tm.m[2] * rn.z;
        const T ay = (Tm.m[4] * rn.x + Tm.m[5] * rn.y) + Tm.m[6] * rn.z;
        const T az = (Tm.m[8] * rn.x + Tm.m[9] * rn.y) + Tm.m[10] * rn.z;
        const T na = sqrt((ax * ax + ay * ay) + az * az);
        const T nb = sqrt((qn.x * qn.x + qn.y * qn.y) + qn.z * qn.z);
        dot = ((ax / na) * (qn.x / nb) + (ay / na) * (qn.y / nb)) + (az / na) * (qn.z / nb);
    } else {
        const T ax = Tm.m[0] * rn.x + Tm.m[1] * rn.y;
        const T ay = Tm.m[4] * rn.x + Tm.m[5] * rn.y;
        const T na = sqrt(ax * ax + ay * ay);
        const T nb = sqrt(qn.x * qn.x + qn.y * qn.y);
        dot = (ax / na) * (qn.x / nb) + (ay / na) * (qn.y / nb);
    }
    const T a = dot < (T)0 ? -dot : dot;
    return !(a < p.eps);
}

// the filter's weight of match entry (slot i, id): 0 for an invalid id
template <typename T>
__device__ __forceinline__ bool sn_entry(const SNPred<T>& p, const Mat4<T>& Tm, int64_t i, int32_t id) {
    if (id < 0) return false;
    return sn_pass(p, Tm, gld(p.rn, i), gld(p.nrm, (int64_t)id * p.rs));
}

}  // namespace pmx

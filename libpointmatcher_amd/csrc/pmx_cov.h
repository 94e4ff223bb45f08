// pmx_cov.h — the per-pair terms of PointToPlaneWithCovErrorMinimizer's
// covariance estimate (ErrorMinimizers/PointToPlaneWithCov.cpp:106-150) and
// the launch of its reduction (pmx_cov.hip).
//
// For every column of ErrorElements (the kept pairs of the last match, the
// rule of p2plane_body in pmx_p2plane.h) the reference forms three 6-vectors
//   a = (n, r_p n_alpha, r_p n_beta, r_p n_gamma)            -> J_hessian += a a^T
//   u = (n N_reading, (n_alpha, n_beta, n_gamma) (E + r_p N_reading))
//   v = (n N_reference, r_q (n_alpha, n_beta, n_gamma) N_reference)
// and the estimate is sigma^2 H^-1 Q H^-1 with H = sum a a^T and
// Q = d2J_dZdX d2J_dZdX^T = sum (u u^T + v v^T).  The kernel returns the two
// sums; the 6x6 inverse and products stay on the host (pm_icp.cpp).
//
// The "ranges" r_p, r_q are what the reference computes: the norms of the step
// reading point and of the matched reference point in the frame ICP minimises
// in, i.e. relative to the reference's mean (ICP.cpp:291-299), not distances
// to the sensor.  A zero range divides by zero and the pair's terms are NaN,
// as in the reference; there is no guard.
#pragma once

#include "pmx_internal.h"

namespace pmx {

// (values of the reduction: kCovCount, kCovQ, kCovNV of pmx_sums.h)

// alpha, beta, gamma, t_x, t_y, t_z of the solved increment, in T
// (PointToPlaneWithCov.cpp:94-99)
template <typename T>
struct CovParams {
    T alpha, beta, gamma, tx, ty, tz;
};

// one kept pair: p the step reading point, q the centred reference point, n
// its normal.  Every product and sum rounded to T separately, left to right as
// the reference's expressions (:116-146); the products of the upper triangles
// widened to double and added in fp64.  H first, Q from QO, kCovTri values each.
template <typename T, bool WITH_H, bool WITH_Q, int QO, int NV>
__device__ __forceinline__ void cov_add(double (&acc)[NV], T px, T py, T pz, const P4<T>& q, const P4<T>& n,
                                        const CovParams<T>& c) {
    const T rp = sqrt((px * px + py * py) + pz * pz);
    const T dpx = px / rp, dpy = py / rp, dpz = pz / rp;
    const T na = n.z * dpy - n.y * dpz;
    const T nb = n.x * dpz - n.z * dpx;
    const T ng = n.y * dpx - n.x * dpy;
    if (WITH_H) {
        const T a[6] = {n.x, n.y, n.z, rp * na, rp * nb, rp * ng};
        int o = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = r; cc < 6; ++cc) acc[o++] += (double)(a[r] * a[cc]);
    }
    if (WITH_Q) {
        const T rq = sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
        const T dqx = q.x / rq, dqy = q.y / rq, dqz = q.z / rq;
        T E = n.x * ((((px - c.gamma * py) + c.beta * pz) + c.tx) - q.x);
        E = E + n.y * ((((c.gamma * px + py) - c.alpha * pz) + c.ty) - q.y);
        E = E + n.z * (((((-c.beta) * px + c.alpha * py) + pz) + c.tz) - q.z);
        T Nr = n.x * ((dpx - c.gamma * dpy) + c.beta * dpz);
        Nr = Nr + n.y * ((c.gamma * dpx + dpy) - c.alpha * dpz);
        Nr = Nr + n.z * (((-c.beta) * dpx + c.alpha * dpy) + dpz);
        const T Nf = -((n.x * dqx + n.y * dqy) + n.z * dqz);
        const T er = E + rp * Nr;
        const T u[6] = {n.x * Nr, n.y * Nr, n.z * Nr, na * er, nb * er, ng * er};
        const T v[6] = {n.x * Nf, n.y * Nf, n.z * Nf, (rq * na) * Nf, (rq * nb) * Nf, (rq * ng) * Nf};
        int o = QO;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = r; cc < 6; ++cc) {
                acc[o] += (double)(u[r] * u[cc]);
                acc[o] += (double)(v[r] * v[cc]);
                ++o;
            }
    }
}

// The reduction over the kept pairs of a 3-D match: per-block partials of the
// kCovNV values into partials[v * kRedBlocks + block] (launch_finalize sums
// them).  m / Tm / chain as launch_p2plane_partial; never part of a
// device-loop iteration (no LoopCtl).
template <typename T>
void launch_p2plane_cov(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, const CovParams<T>& cp,
                        double* partials, hipStream_t s);

}  // namespace pmx

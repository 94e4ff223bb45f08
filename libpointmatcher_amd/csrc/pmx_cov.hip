// pmx_cov.hip — the reduction behind PointToPlaneWithCovErrorMinimizer's
// covariance (ErrorMinimizers/PointToPlaneWithCov.cpp:72-162): H = sum a a^T
// and Q = sum (u u^T + v v^T) over the ErrorElements columns of the last
// match (pmx_cov.h has the per-pair terms).
//
// One launch per ICP, after the loop stopped: it walks the match arrays the
// last point-to-plane reduction walked, with the same kept rule (dist != inf
// and a non-zero chain weight, the SurfaceNormal and GenericDescriptor
// factors included; a real-valued weight only decides kept / not kept, the reference's estimate reads
// no weight), the same id source and, at k = 1, the match's neighbour records.
// Bytes per pair as p2plane_partial: reading 16, dist 4, point and normal
// record 32 in slot order (or id 4 and two 16-byte gathers) in float.  The T
// products go to fp64 accumulators, 21 + 1 + 21 per lane; the block and
// finalize sums are the fixed-order ones of the other reductions
// (block_store, launch_finalize), so the result is deterministic.
#include "pmx_cov.h"
#include "pmx_p2plane.h"

namespace pmx {

// entry (slot i, distance dv, id) is a column of ErrorElements: dist != inf
// and w != 0 (ErrorMinimizer.cpp:75-131) for the chain's weight w (entry_weight,
// pmx_weight.h; q, n: the matched records as loaded, rn: the reading's normal)
template <typename T, bool SN, bool GD>
__device__ __forceinline__ bool cov_kept(const WChain<T>& chain, const WRange<T>& wr, const Mat4<T>& Tm, T dv,
                                         int32_t id, const P4<T>& rn, T px, T py, T pz, const P4<T>& q,
                                         const P4<T>& n) {
    if (dv == (T)__builtin_huge_val()) return false;
    return entry_weight<T, SN, true, GD>(chain, chain.sn, wr, Tm, dv, id, px, py, pz, q, loaded(n), loaded(rn),
                                         chain.gd) != (T)0;
}

template <typename T, bool SN, bool GD>
__global__ __launch_bounds__(256) void p2plane_cov_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                          const P4<T>* __restrict__ ref,
                                                          const P4<T>* __restrict__ nrm, int rs,
                                                          const T* __restrict__ d, const int32_t* __restrict__ ids,
                                                          WChain<T> chain, int k, int64_t N, T alpha, T beta, T gamma,
                                                          T t_x, T t_y, T t_z, double* __restrict__ partials,
                                                          const P4<T>* __restrict__ nbr) {
    constexpr int NV = kCovNV;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const CovParams<T> cp{alpha, beta, gamma, t_x, t_y, t_z};
    const WRange<T> wr = chain_resolve(chain);
    const T inf = (T)__builtin_huge_val();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // whether an entry's records are worth gathering: without the robust
    // filter a rejecting predicate makes the weight 0 (with it, 0 * NaN is not)
    const auto may_keep = [&](T dv) { return dv != inf && ((GD ? chain.real() : chain.robust != 0) || chain_keep(wr, dv)); };
    int64_t i0 = (int64_t)xcd_block() * blockDim.x + threadIdx.x;
    if (k == 1) {
        // k = 1: U slots per round, every load that needs no id issued up
        // front (the neighbour records come in slot order with the query)
        constexpr int U = 2;
        for (; i0 < N; i0 += U * stride) {
            P4<T> r[U], q[U], n[U];
            P4<T> rn[SN ? U : 1];
            T dv[U];
            int32_t id[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t ii = i0 + u * stride;
                const int64_t jj = ii < N ? ii : i0;
                r[u] = rd[jj];
                dv[u] = d[jj];
                id[u] = 0;
                if (nbr) {
                    q[u] = nbr[jj];
                    n[u] = nbr[N + jj];
                    if (SN || GD) id[u] = ids[jj];
                } else {
                    id[u] = ids[jj];
                }
                if (SN) rn[u] = gld(chain.sn.rn, jj);
            }
            if (!nbr) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool gat = i0 + u * stride < N && id[u] >= 0 && may_keep(dv[u]);
                    const int64_t g = (int64_t)(gat ? id[u] : 0) * rs;  // (position 0 always exists)
                    q[u] = gld(ref, g);
                    n[u] = gld(nrm, g);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (i0 + u * stride >= N) continue;
                T px, py, pz;
                xform3(Tm, r[u], px, py, pz);
                if (!cov_kept<T, SN, GD>(chain, wr, Tm, dv[u], id[u], rn[SN ? u : 0], px, py, pz, q[u], n[u])) continue;
                acc[kCovCount] += 1.0;
                cov_add<T, true, true, kCovQ, NV>(acc, px, py, pz, q[u], n[u], cp);
            }
        }
    }
    for (int64_t i = i0; k != 1 && i < N; i += stride) {
        T px, py, pz;
        xform3(Tm, rd[i], px, py, pz);
        P4<T> rn{};
        if (SN) rn = gld(chain.sn.rn, i);
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = d[e];
            if (!may_keep(dv)) continue;
            const int32_t id = ids[e];
            const int64_t g = (int64_t)(id >= 0 ? id : 0) * rs;
            const P4<T> q = gld(ref, g), n = gld(nrm, g);
            if (!cov_kept<T, SN, GD>(chain, wr, Tm, dv, id, rn, px, py, pz, q, n)) continue;
            acc[kCovCount] += 1.0;
            cov_add<T, true, true, kCovQ, NV>(acc, px, py, pz, q, n, cp);
        }
    }
    block_store<NV>(acc, partials);
}

template <typename T>
void launch_p2plane_cov(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, const CovParams<T>& cp,
                        double* partials, hipStream_t s) {
    const bool gd = chain.gd.desc != nullptr;
    auto* const kern = gd ? (chain.sn.rn ? p2plane_cov_kernel<T, true, true> : p2plane_cov_kernel<T, false, true>)
                          : (chain.sn.rn ? p2plane_cov_kernel<T, true, false> : p2plane_cov_kernel<T, false, false>);
    // (the neighbour records where the last point-to-plane reduction read them: k = 1, no real-valued weights)
    const P4<T>* nbr = m.k == 1 && !chain.real() ? m.nbr : nullptr;
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, m.rd, Tm, m.pn, m.nrm, m.rs, m.d, m.ids, chain, m.k, m.N,
                       cp.alpha, cp.beta, cp.gamma, cp.tx, cp.ty, cp.tz, partials, nbr);
}

template void launch_p2plane_cov<float>(const MatchView<float>&, const Mat4<float>&, const WChain<float>&,
                                        const CovParams<float>&, double*, hipStream_t);
template void launch_p2plane_cov<double>(const MatchView<double>&, const Mat4<double>&, const WChain<double>&,
                                         const CovParams<double>&, double*, hipStream_t);

}  // namespace pmx

// pmx_p2plane.h — the point-to-plane accumulation of the reduction kernel
// (pmx_reduce.hip).
#pragma once

#include "pmx_internal.h"

namespace pmx {

template <typename T>
__device__ __forceinline__ void xform3(const Mat4<T>& M, const P4<T>& p, T& x, T& y, T& z) {
    x = ((M.m[0] * p.x + M.m[1] * p.y) + M.m[2] * p.z) + M.m[3] * p.w;
    y = ((M.m[4] * p.x + M.m[5] * p.y) + M.m[6] * p.z) + M.m[7] * p.w;
    z = ((M.m[8] * p.x + M.m[9] * p.y) + M.m[10] * p.z) + M.m[11] * p.w;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The wave sums of V per-lane values (V a power of two, <= 64) by a
// butterfly that halves the values at every step: V - 1 + log2(64 / V)
// shuffles instead of V * 6 for V separate wave_sums.  On return lane L holds
// the sum of value idx = (L >> log2(64 / V)) ... in a fixed order (every
// lane of a group of 64 / V lanes holds the same sum); deterministic.
template <int V>
__device__ __forceinline__ double wave_transpose_sum(double (&v)[V], int& idx) {
    static_assert(V >= 1 && V <= 64 && (V & (V - 1)) == 0, "power of two <= 64");
    const int lane = threadIdx.x & 63;
    idx = 0;
    int d = 32;
#pragma unroll
    for (int h = V / 2; h >= 1; h >>= 1, d >>= 1) {
        const bool up = (lane & d) != 0;
        // (the halves are exchanged with bit masks: a select between two
        // elements would become a dynamically indexed load of the array,
        // which moves the whole array to scratch)
        const long long m = up ? -1ll : 0ll;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const long long a = __double_as_longlong(v[i]), b = __double_as_longlong(v[i + h]);
            const double send = __longlong_as_double((a & m) | (b & ~m));
            const double keep = __longlong_as_double((b & m) | (a & ~m));
            v[i] = keep + __shfl_xor(send, d);
        }
        idx += up ? h : 0;
    }
    double s = v[0];
#pragma unroll
    for (; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}
// the lane that writes value idx of a wave_transpose_sum<V>
template <int V>
__device__ __forceinline__ bool transpose_writer() {
    return ((threadIdx.x & 63) & (64 / V - 1)) == 0;
}

// block reduction of NV accumulators; writes partials[v * gridDim.x + blockIdx.x]
// (value-major: the finalize reads each value's block partials contiguously)
template <int NV>
__device__ __forceinline__ void block_store(double (&acc)[NV], double* __restrict__ partials) {
    // (the power of two the transposed wave sum takes)
    constexpr int V = NV <= 8 ? 8 : NV <= 16 ? 16 : NV <= 32 ? 32 : 64;
    static_assert(NV <= 64, "block_store: at most 64 values");
    __shared__ double red[4][V];
    const int wave = threadIdx.x >> 6;
    double x[V];
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = v < NV ? acc[v] : 0.0;
    int idx;
    const double s = wave_transpose_sum<V>(x, idx);
    if (transpose_writer<V>()) red[wave][idx] = s;
    __syncthreads();
    for (int v = threadIdx.x; v < NV; v += blockDim.x) {
        const double r = ((red[0][v] + red[1][v]) + red[2][v]) + red[3][v];
        partials[(int64_t)v * gridDim.x + blockIdx.x] = r;
    }
}

// One match entry in the ErrorElements counts from acc[S] (ErrorMinimizer.cpp:
// 75-131); true for a kept pair.  A query with none is a rejected point (the
// caller's count).  (p2plane_body keeps the rule written out: through this helper
// its 2-D float form took 106 VGPRs instead of 92, 4 waves per SIMD instead of 5.)
template <int S, int NV>
__device__ __forceinline__ bool count_entry(double (&acc)[NV], bool nonzero, bool finite) {
    if (nonzero) acc[S + kNonzero] += 1.0;  // (w != 0).count()
    if (!finite) return false;
    if (!nonzero) {
        acc[S + kRejMatches] += 1.0;
        return false;
    }
    acc[S + kKept] += 1.0;
    return true;
}

// one kept pair: F and dot in T exactly as PointToPlane.cpp:171-243, the
// upper triangle of F F^T and F dot added in fp64
template <typename T, int DIM, int NV>
__device__ __forceinline__ void p2plane_add(double (&acc)[NV], T px, T py, T pz, const P4<T>& q, const P4<T>& n,
                                            T w = (T)1) {
    constexpr int NF = P2PlaneSums<DIM, false>::NF;
    T F[NF];
    T dot;
    if (DIM == 3) {
        F[0] = py * n.z - pz * n.y;
        F[1] = pz * n.x - px * n.z;
        F[2] = px * n.y - py * n.x;
        F[3] = n.x;
        F[4] = n.y;
        F[5] = n.z;
        dot = ((px - q.x) * n.x + (py - q.y) * n.y) + (pz - q.z) * n.z;
    } else {
        F[0] = px * n.y - py * n.x;
        F[1] = n.x;
        F[2] = n.y;
        dot = (px - q.x) * n.x + (py - q.y) * n.y;
    }
    // wF = w * F (PointToPlane.cpp:218-227); with the 0/1 weights w = 1 and
    // wF is F exactly
    int a = 0;
#pragma unroll
    for (int r = 0; r < NF; ++r) {
        const T wF = w * F[r];
#pragma unroll
        for (int c = r; c < NF; ++c) acc[a++] += (double)(wF * F[c]);
        acc[P2PlaneSums<DIM, false>::kB + r] += (double)(wF * dot);
    }
}

// values: P2PlaneSums<DIM, false> (pmx_sums.h); one block's sums to
// partials[v * gridDim.x + blockIdx.x]
// k up to this: the reduction issues a query's k gathers together
constexpr int kGatherK = 4;
// SN: the chain holds the SurfaceNormalOutlierFilter (chain.sn, pmx_weight.h):
// every entry's id and the reading's normal are loaded as well, the gathered
// reference normal serves both the predicate and F, and a pair counts as kept
// only when both predicates pass (the product of the weights)
// GD: the chain holds a hard GenericDescriptorOutlierFilter (gdp: chain.gd, or
// its copy bound to the device loop's level): every entry's id is loaded as
// well, and the pair's descriptor value is gathered by it.
// The keep test below is entry_weight<T, SN, true, GD>(...) != 0 (pmx_weight.h,
// the definition) for a chain of 0/1 factors, which is all this body is
// launched for: pair_keep (pmx_weight.h), called once per k range around each
// range's own order of loads.
template <typename T, int DIM, bool SN = false, bool GD = false>
__device__ __forceinline__ void p2plane_body(const P4<T>* __restrict__ rd, const Mat4<T>& Tm,
                                             const P4<T>* __restrict__ ref, const P4<T>* __restrict__ nrm, int rs,
                                             const T* __restrict__ d, const int32_t* __restrict__ ids,
                                             const WChain<T>& chain, int k, int64_t N,
                                             double* __restrict__ partials, const P4<T>* __restrict__ nbr = nullptr,
                                             const GDPred<T>& gdp = GDPred<T>{}) {
    constexpr int ST = P2PlaneSums<DIM, false>::kStats;  // (kSumW is the kept count with 0/1 weights)
    constexpr int NV = P2PlaneSums<DIM, false>::NV;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const WRange<T> wr = chain_resolve(chain);
    const T inf = (T)__builtin_huge_val();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // XCD-aware block order (pmx_internal.h): the blocks of one XCD take
    // adjacent slot ranges, so the gathered point/normal records of
    // neighbouring queries meet in one L2 (the partial slot stays blockIdx.x)
    int64_t i0 = (int64_t)xcd_block() * blockDim.x + threadIdx.x;
    if (k == 1) {
        // k = 1: U slots per round with every load issued up front (the
        // reduction is latency-bound: slot -> id -> gathered point / normal;
        // with the match's neighbour records, nbr, the point and the normal
        // come in slot order with the query, no dependent gather)
        constexpr int U = 4;
        for (; i0 < N; i0 += U * stride) {
            P4<T> r[U];
            T dv[U];
            int32_t id[U];
            P4<T> q[U], n[U];
            P4<T> rn[SN ? U : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t ii = i0 + u * stride;
                const int64_t jj = ii < N ? ii : i0;
                r[u] = rd[jj];
                dv[u] = d[jj];
                if (nbr) {
                    q[u] = nbr[jj];
                    n[u] = nbr[N + jj];
                    if (SN || GD) id[u] = ids[jj];
                } else {
                    id[u] = ids[jj];
                }
                if (SN) rn[u] = gld(chain.sn.rn, jj);
            }
            bool kp[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                kp[u] = i0 + u * stride < N && dv[u] != inf && chain_keep(wr, dv[u]);
                if (!nbr) {
                    // (SN: the normal of every valid entry the distances keep, also at an infinite distance)
                    const bool gat = SN ? i0 + u * stride < N && id[u] >= 0 && chain_keep(wr, dv[u]) : kp[u];
                    const int64_t g = (int64_t)(gat ? id[u] : 0) * rs;  // (position 0 always exists)
                    q[u] = gld(ref, g);
                    n[u] = gld(nrm, g);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (i0 + u * stride >= N) continue;
                const bool keep = pair_keep<T, SN, GD>(chain, gdp, wr, Tm, dv[u], id[u], rn[SN ? u : 0], n[u]);
                if (SN || GD) kp[u] = kp[u] && keep;
                if (keep) acc[ST + kNonzero] += 1.0;
                if (dv[u] != inf && !keep) acc[ST + kRejMatches] += 1.0;
                if (!kp[u]) {
                    acc[ST + kRejPoints] += 1.0;
                    continue;
                }
                acc[ST + kKept] += 1.0;
                acc[ST + kSumW] += 1.0;
                T px, py, pz;
                xform3(Tm, r[u], px, py, pz);
                p2plane_add<T, DIM, NV>(acc, px, py, pz, q[u], n[u]);
            }
        }
    }
    if (k > 1 && k <= kGatherK) {
        // 1 < k <= kGatherK: the query's k distances and ids first, then every
        // kept entry's point and normal gathers in flight together, then the
        // sums in rank order (the loop below, one dependent gather at a time,
        // took 45 us for C4's 4 M pairs)
        for (; i0 < N; i0 += stride) {
            const int64_t i = i0;
            const P4<T> rp = rd[i];
            T dv[kGatherK];
            int32_t id[kGatherK];
#pragma unroll
            for (int s = 0; s < kGatherK; ++s) {
                dv[s] = s < k ? d[i * k + s] : inf;
                id[s] = s < k ? ids[i * k + s] : -1;
            }
            P4<T> q[kGatherK], n[kGatherK];
#pragma unroll
            for (int s = 0; s < kGatherK; ++s) {
                const bool kp = SN ? s < k && id[s] >= 0 && chain_keep(wr, dv[s])
                                   : s < k && dv[s] != inf && chain_keep(wr, dv[s]);
                const int64_t g = (int64_t)(kp ? id[s] : 0) * rs;  // (position 0 always exists)
                q[s] = gld(ref, g);
                n[s] = gld(nrm, g);
            }
            T px, py, pz;
            xform3(Tm, rp, px, py, pz);
            P4<T> rn{};
            if (SN) rn = gld(chain.sn.rn, i);
            bool exist = false;
#pragma unroll
            for (int s = 0; s < kGatherK; ++s) {
                if (s >= k) continue;
                const bool keep = pair_keep<T, SN, GD>(chain, gdp, wr, Tm, dv[s], id[s], rn, n[s]);
                if (keep) acc[ST + kNonzero] += 1.0;
                if (dv[s] == inf) continue;
                if (!keep) {
                    acc[ST + kRejMatches] += 1.0;
                    continue;
                }
                exist = true;
                acc[ST + kKept] += 1.0;
                acc[ST + kSumW] += 1.0;  // (the 0/1 weights)
                p2plane_add<T, DIM, NV>(acc, px, py, pz, q[s], n[s]);
            }
            if (!exist) acc[ST + kRejPoints] += 1.0;
        }
    }
    for (int64_t i = i0; k != 1 && i < N; i += stride) {
        T px, py, pz;
        xform3(Tm, rd[i], px, py, pz);
        bool exist = false;
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = d[e];
            bool keep = chain_keep(wr, dv);
            if (SN || GD) {  // (the id and the records only for an entry the distances keep)
                const int32_t id = ids[e];
                if (keep && id >= 0)
                    keep = pair_keep<T, SN, GD>(chain, gdp, wr, Tm, dv, id, SN ? gld(chain.sn.rn, i) : P4<T>{},
                                                SN ? gld(nrm, (int64_t)id * rs) : P4<T>{});
                else
                    keep = false;
            }
            if (keep) acc[ST + kNonzero] += 1.0;
            if (dv == inf) continue;
            if (!keep) {
                acc[ST + kRejMatches] += 1.0;
                continue;
            }
            exist = true;
            acc[ST + kKept] += 1.0;
            acc[ST + kSumW] += 1.0;  // (the 0/1 weights)
            const int32_t id = ids[e];
            p2plane_add<T, DIM, NV>(acc, px, py, pz, gld(ref, (int64_t)id * rs), gld(nrm, (int64_t)id * rs));
        }
        if (!exist) acc[ST + kRejPoints] += 1.0;
    }
    block_store<NV>(acc, partials);
}

}  // namespace pmx

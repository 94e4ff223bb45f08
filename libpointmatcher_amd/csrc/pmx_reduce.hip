// pmx_reduce.hip — error-minimiser reductions (normal equations) on the device.
//
// Replaces ErrorElements (pointmatcher/ErrorMinimizer.cpp:58-193: compaction
// of the kept pairs + gather of the matched reference points) and the dense
// parts of PointToPlaneErrorMinimizer::compute_in_place
// (ErrorMinimizers/PointToPlane.cpp:171-243, crossProduct
// ErrorMinimizer.cpp:281-315) and PointToPointErrorMinimizer::compute_in_place
// (ErrorMinimizers/PointToPoint.cpp:61-81).  Nothing is compacted: each lane
// walks its slots, evaluates the outlier chain on the distance (weights are
// 0/1, see WChain), skips dist == inf, counts weight 0 as a rejected match,
// and for kept pairs gathers q = ref[id], n = normal[id] (grid order after a
// grid match: coherent) and adds the T-precision products of the reference's
// formulas into fp64 accumulators:
//   F = [p x n ; n]  (3-D),  F = [p_x n_y - p_y n_x ; n]  (2-D)
//   A_rc += (w F_r) F_c,   b_r += (w F_r) dot,   dot = ((dx n_x + dy n_y) + dz n_z)
// With w = 1, (w F_r) F_c == F_r F_c == F_c F_r bit for bit, so Eigen's
// wF * F^T is exactly symmetric: only the upper triangle (21 / 6 terms) is
// accumulated and the host mirrors it.  Per-block partials (fixed 1024-block
// grid, fixed lane order) are summed by finalize_kernel in block order, so
// results are deterministic.  ~56 B per pair (reading 16, dist 4, id 4,
// gathered point 16, gathered normal 16).
#include "pmx_internal.h"
#include "pmx_p2plane.h"
#include "pmx_spec.h"

namespace pmx {

// The chain's weight of entry e (slot i, step point p) in the point-to-point
// reductions: entry_weight (pmx_weight.h) with the matched normal gathered
// only where the SurfaceNormal factor needs it (these kernels carry none
// otherwise).  A robust point-to-plane distance is not evaluated here: its
// weights come materialised (w_arr, every factor in them).
template <typename T, bool SN, bool GD = false>
__device__ __forceinline__ T p2point_weight(const WChain<T>& chain, const SNPred<T>& sn, const WRange<T>& wr,
                                            const Mat4<T>& Tm, T dv, const T (&p)[3], int64_t i, int64_t e,
                                            const int32_t* __restrict__ ids, const GDPred<T>& gdp = GDPred<T>{}) {
    const auto inline_weight = [&]() {
        const int32_t id = SN || GD ? ids[e] : 0;
        return entry_weight<T, SN, false, GD>(
            chain, sn, wr, Tm, dv, id, p[0], p[1], p[2], P4<T>{}, [&]() { return gld(sn.nrm, (int64_t)id * sn.rs); },
            [&]() { return gld(sn.rn, i); }, gdp);
    };
    // (the test of the array sits inside the robust side, where it was when the
    // SN = false kernels were tuned: they compile to the same instructions)
    const auto robust_side = [&]() {
        if (chain.w_arr) return chain.w_arr[e];
        return inline_weight();
    };
    return chain.robust ? robust_side() : inline_weight();
}
// the launchers' choice among a kernel's instantiations (sn, gd: the chain
// holds the SurfaceNormal / GenericDescriptor filter); chains without the
// GenericDescriptor filter launch the GD = false ones, as before it existed
#define PMX_PICK(sn, gd, K, ...)                                                         \
    ((gd) ? ((sn) ? K<__VA_ARGS__, true, true> : K<__VA_ARGS__, false, true>) \
          : ((sn) ? K<__VA_ARGS__, true, false> : K<__VA_ARGS__, false, false>))

// (values: P2PlaneSums<DIM, false>, pmx_sums.h)
template <typename T, int DIM, bool SN, bool GD>
__global__ __launch_bounds__(256) void p2plane_partial_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                              const P4<T>* __restrict__ ref,
                                                              const P4<T>* __restrict__ nrm, int rs,
                                                              const T* __restrict__ d,
                                                              const int32_t* __restrict__ ids, WChain<T> chain,
                                                              int k, int64_t N, double* __restrict__ partials,
                                                              const LoopCtl* __restrict__ ctl,
                                                              const GridDesc<T>* __restrict__ gd,
                                                              unsigned long long* __restrict__ vzero,
                                                              const P4<T>* __restrict__ nbr) {
    if (ctl) {  // device loop
        if (ctl->done) return;
        ctl_transform(ctl, Tm);
        ref = gd[ctl->level].gpn;
        nrm = ref + 1;
        rs = 2;
    }
    if (vzero && blockIdx.x == 0)  // (the spread counters the merged counter phase read, for the next match)
        for (int c = 0; c < 4; ++c) vzero[(size_t)(c * kVSlots + threadIdx.x) * kVStride] = 0ull;
    GDPred<T> gdp = chain.gd;  // (a copy: writing the kernel argument would move the chain to scratch)
    if (GD) gd_bind(gdp, ctl, gd);
    p2plane_body<T, DIM, SN, GD>(rd, Tm, ref, nrm, rs, d, ids, chain, k, N, partials, nbr, gdp);
}

// Real-valued weights (a RobustOutlierFilter in the chain; per-module path):
// the ErrorElements counts on w != 0, sum of w in the fifth counter.  A is
// accumulated in full: (w F_r) F_c and (w F_c) F_r round differently, and the
// reference's wF * F^T keeps that asymmetry (PointToPlane.cpp:218-227).
// (values: P2PlaneSums<DIM, true>, pmx_sums.h)
template <typename T, int DIM, int NV>
__device__ __forceinline__ void p2plane_add_full(double (&acc)[NV], T px, T py, T pz, const P4<T>& q,
                                                 const P4<T>& n, T w) {
    using L = P2PlaneSums<DIM, true>;
    constexpr int NF = L::NF;
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
#pragma unroll
    for (int r = 0; r < NF; ++r) {
        const T wF = w * F[r];
#pragma unroll
        for (int c = 0; c < NF; ++c) acc[r * NF + c] += (double)(wF * F[c]);
        acc[L::kB + r] += (double)(wF * dot);
    }
}
template <typename T, int DIM, bool SN, bool GD>
__global__ __launch_bounds__(256) void p2plane_weighted_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                               const P4<T>* __restrict__ ref,
                                                               const P4<T>* __restrict__ nrm, int rs,
                                                               const T* __restrict__ d,
                                                               const int32_t* __restrict__ ids, WChain<T> chain,
                                                               int k, int64_t N, double* __restrict__ partials,
                                                               const LoopCtl* __restrict__ ctl,
                                                               const GridDesc<T>* __restrict__ gd) {
    if (ctl) {  // device loop (a robust chain): transform and level from the device
        if (ctl->done) return;
        ctl_transform(ctl, Tm);
        ref = gd[ctl->level].gpn;
        nrm = ref + 1;
        rs = 2;
    }
    using L = P2PlaneSums<DIM, true>;
    constexpr int NV = L::NV;
    GDPred<T> gdp = chain.gd;
    if (GD) gd_bind(gdp, ctl, gd);
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const WRange<T> wr = chain_resolve(chain);
    const T inf = (T)__builtin_huge_val();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        T px, py, pz;
        xform3(Tm, rd[i], px, py, pz);
        bool exist = false;
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = d[e];
            const int32_t id = ids[e];
            P4<T> q{}, n{};
            if (id >= 0) {
                q = gld(ref, (int64_t)id * rs);
                n = gld(nrm, (int64_t)id * rs);
            }
            const T w = entry_weight<T, SN, true, GD>(chain, chain.sn, wr, Tm, dv, id, px, py, pz, q, loaded(n),
                                                      [&]() { return gld(chain.sn.rn, i); }, gdp);
            if (!count_entry<L::kStats>(acc, w != (T)0, dv != inf)) continue;
            exist = true;
            acc[L::kStats + kSumW] += (double)w;
            p2plane_add_full<T, DIM, NV>(acc, px, py, pz, q, n, w);
        }
        if (!exist) acc[L::kStats + kRejPoints] += 1.0;
    }
    block_store<NV>(acc, partials);
}

// dim: the sums' form (p2plane_sums_dim, pmx_sums.h), not the context's
// dimension.  Every instantiation transforms, loads and gathers whole 3-D
// records (a 2-D context's z is 0) and DIM selects the accumulation alone, so
// force2D on a 3-D context is the DIM = 2 instantiation as it stands: the 3-D
// step transform (xform3), the 3-D records, the chain's 3-D predicates and
// weights, and p2plane_add<T, 2> on the x, y of p, q and n.
template <typename T>
void launch_p2plane_partial(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, int dim,
                            double* partials, const LoopCtl* ctl, const GridDesc<T>* gd, unsigned long long* vzero,
                            hipStream_t s) {
    const bool sn = chain.sn.rn != nullptr;  // (the instantiations with the normal predicate)
    const bool gdf = chain.gd.desc != nullptr;  // (and with the descriptor factor)
    if (chain.real()) {  // real-valued weights: the full asymmetric A (this kernel has no neighbour-record path)
        auto* const kern = dim == 3 ? PMX_PICK(sn, gdf, p2plane_weighted_kernel, T, 3)
                                    : PMX_PICK(sn, gdf, p2plane_weighted_kernel, T, 2);
        hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, m.rd, Tm, m.pn, m.nrm, m.rs, m.d, m.ids, chain, m.k,
                           m.N, partials, ctl, gd);
        return;
    }
    // (m.nbr, k = 1: the kernel reads the records in slot order instead of gathering by id)
    auto* const kern = dim == 3 ? PMX_PICK(sn, gdf, p2plane_partial_kernel, T, 3)
                                : PMX_PICK(sn, gdf, p2plane_partial_kernel, T, 2);
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, m.rd, Tm, m.pn, m.nrm, m.rs, m.d, m.ids, chain, m.k, m.N,
                       partials, ctl, gd, vzero, m.nbr);
}

// Sum the per-block partials: one block per accumulator, each thread adds a
// fixed strided subset in order, then a fixed-shape tree — the summation
// order never changes, so results are bitwise reproducible.
__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ partials, int nblocks, int nv,
                                                       double* __restrict__ out, const LoopCtl* __restrict__ ctl) {
    __shared__ double red[4];
    if (ctl && ctl->done) return;
    const int v = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += partials[(int64_t)v * nblocks + b];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[v] = (red[0] + red[1]) + (red[2] + red[3]);
}

void launch_finalize(const double* partials, int nblocks, int nv, double* out, const LoopCtl* ctl, hipStream_t s) {
    hipLaunchKernelGGL(finalize_kernel, dim3(nv), dim3(256), 0, s, partials, nblocks, nv, out, ctl);
}

// ------------------------------------------------------------ point-to-point --
// (values: P2PointSums, pmx_sums.h)
// What the three kernels do first: in the device loop (ctl) the step transform,
// the level's points and normals from the device.  sn: the caller's copy of chain.sn
// (writing the kernel argument would move the chain to scratch).  False: the loop is done.
template <typename T, bool SN, bool GD>
__device__ __forceinline__ bool p2point_begin(const LoopCtl* __restrict__ ctl, const GridDesc<T>* __restrict__ gd,
                                              Mat4<T>& Tm, const P4<T>* __restrict__& ref, SNPred<T>& sn,
                                              GDPred<T>& gdp) {
    if (ctl) {
        if (ctl->done) return false;
        ctl_transform(ctl, Tm);
        ref = gd[ctl->level].gpts;
    }
    if (SN) sn_bind(sn, ctl, gd);
    if (GD) gd_bind(gdp, ctl, gd);
    return true;
}

// pass 1: sum w, sum p*w, sum q*w (PointToPoint.cpp:67-72; with w = 1,
// p * w == p exactly) + ErrorElements counts; RAW: the one-pass form's raw
// moments sum (w q_r) p_c as well.  block: this block's place in the walk.
template <typename T, bool SN, bool RAW, bool GD>
__device__ __forceinline__ void p2point_sums_body(const P4<T>* __restrict__ rd, const Mat4<T>& Tm,
                                                  const P4<T>* __restrict__ ref, const T* __restrict__ d,
                                                  const int32_t* __restrict__ ids, const WChain<T>& chain,
                                                  const SNPred<T>& sn, const GDPred<T>& gdp, int k, int64_t N,
                                                  uint32_t block, double* __restrict__ partials) {
    using L = P2PointSums;
    constexpr int NV = RAW ? L::kMomentsNV : L::kPass1NV;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const WRange<T> wr = chain_resolve(chain);
    const T inf = (T)__builtin_huge_val();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)block * blockDim.x + threadIdx.x; i < N; i += stride) {
        T p[3];
        xform3(Tm, rd[i], p[0], p[1], p[2]);
        bool exist = false;
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = d[e];
            // 0/1 weights, or a robust chain's real weight (point2point distance)
            const T w = p2point_weight<T, SN, GD>(chain, sn, wr, Tm, dv, p, i, e, ids, gdp);
            if (!count_entry<L::kStats>(acc, w != (T)0, dv != inf)) continue;
            exist = true;
            const P4<T> q = gld(ref, ids[e]);
            const T wq[3] = {q.x * w, q.y * w, q.z * w};
            acc[L::kSw] += (double)w;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                acc[L::kSp + r] += (double)(p[r] * w);
                acc[L::kSq + r] += (double)wq[r];
#pragma unroll
                for (int c = 0; RAW && c < 3; ++c) acc[L::kRaw + L::moment(r, c)] += (double)wq[r] * (double)p[c];
            }
        }
        if (!exist) acc[L::kStats + kRejPoints] += 1.0;
    }
    block_store<NV>(acc, partials);
}

template <typename T, bool SN, bool GD>
__global__ __launch_bounds__(256) void p2point_pass1_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                            const P4<T>* __restrict__ ref, const T* __restrict__ d,
                                                            const int32_t* __restrict__ ids, WChain<T> chain, int k,
                                                            int64_t N, double* __restrict__ partials,
                                                            const LoopCtl* __restrict__ ctl,
                                                            const GridDesc<T>* __restrict__ gd) {
    SNPred<T> sn = chain.sn;
    GDPred<T> gdp = chain.gd;
    if (!p2point_begin<T, SN, GD>(ctl, gd, Tm, ref, sn, gdp)) return;
    p2point_sums_body<T, SN, false, GD>(rd, Tm, ref, d, ids, chain, sn, gdp, k, N, blockIdx.x, partials);
}

template <typename T>
void launch_p2point_pass1(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, double* partials,
                          const LoopCtl* ctl, const GridDesc<T>* gd, hipStream_t s) {
    auto* const kern = PMX_PICK(chain.sn.rn, chain.gd.desc, p2point_pass1_kernel, T);
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, m.rd, Tm, m.ref, m.d, m.ids, chain, m.k, m.N, partials,
                       ctl, gd);
}

// means in T: w_sum_inv = 1 / w.sum(); mean = sum * w_sum_inv (PointToPoint.cpp:67-72)
template <typename T>
__global__ void p2point_means_kernel(const double* __restrict__ sums, T* __restrict__ means, int dim,
                                     const LoopCtl* __restrict__ ctl) {
    if (threadIdx.x != 0 || (ctl && ctl->done)) return;
    const T winv = (T)1 / (T)sums[P2PointSums::kSw];
    for (int r = 0; r < 3; ++r) {
        means[r] = r < dim ? (T)sums[P2PointSums::kSp + r] * winv : (T)0;
        means[3 + r] = r < dim ? (T)sums[P2PointSums::kSq + r] * winv : (T)0;
    }
}

template <typename T>
void launch_p2point_means(const double* sums, T* means_dev, int dim, const LoopCtl* ctl, hipStream_t s) {
    hipLaunchKernelGGL(p2point_means_kernel<T>, dim3(1), dim3(64), 0, s, sums, means_dev, dim, ctl);
}

// pass 2: m = sum (qc * w) pc^T  (PointToPoint.cpp:76-81), 3x3 (2-D uses the
// top-left 2x2; z terms are exactly zero).  SIM (PointToPointSimilarity): a
// tenth sum, sigma = sum ||pc||^2 w (PointToPointSimilarity.cpp:69): each
// pair's squared norm in T, (pcx pcx + pcy pcy) + pcz pcz, times w, added in
// fp64.  The rigid minimiser's instantiations (SIM false) hold nine sums as before.
template <typename T, bool SIM, bool SN, bool GD>
__global__ __launch_bounds__(256) void p2point_pass2_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                            const P4<T>* __restrict__ ref, const T* __restrict__ d,
                                                            const int32_t* __restrict__ ids, WChain<T> chain, int k,
                                                            int64_t N, const T* __restrict__ means,
                                                            double* __restrict__ partials,
                                                            const LoopCtl* __restrict__ ctl,
                                                            const GridDesc<T>* __restrict__ gd) {
    using L = P2PointSums;
    constexpr int NV = SIM ? L::kPass2SimNV : L::kPass2NV;
    SNPred<T> sn = chain.sn;
    GDPred<T> gdp = chain.gd;
    if (!p2point_begin<T, SN, GD>(ctl, gd, Tm, ref, sn, gdp)) return;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const WRange<T> wr = chain_resolve(chain);
    const T inf = (T)__builtin_huge_val();
    const T mp[3] = {means[0], means[1], means[2]};
    const T mq[3] = {means[3], means[4], means[5]};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        T p[3];
        xform3(Tm, rd[i], p[0], p[1], p[2]);
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = d[e];
            const T w = p2point_weight<T, SN, GD>(chain, sn, wr, Tm, dv, p, i, e, ids, gdp);
            if (dv == inf || w == (T)0) continue;
            const P4<T> q4 = gld(ref, ids[e]);
            const T q[3] = {q4.x, q4.y, q4.z};
            T pc[3], qc[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                pc[r] = p[r] - mp[r];
                qc[r] = q[r] - mq[r];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[L::moment(r, c)] += (double)((qc[r] * w) * pc[c]);  // (qc * w) pc
            }
            if constexpr (SIM)  // (sigma behind the moments: kSigma of the result area)
                acc[L::kPass2NV] += (double)(((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]) * w);
        }
    }
    block_store<NV>(acc, partials);
}

template <typename T>
void launch_p2point_pass2(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, const T* means_dev,
                          bool similarity, double* partials, const LoopCtl* ctl, const GridDesc<T>* gd,
                          hipStream_t s) {
    auto* const kern = similarity ? PMX_PICK(chain.sn.rn, chain.gd.desc, p2point_pass2_kernel, T, true)
                                  : PMX_PICK(chain.sn.rn, chain.gd.desc, p2point_pass2_kernel, T, false);
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, m.rd, Tm, m.ref, m.d, m.ids, chain, m.k, m.N, means_dev,
                       partials, ctl, gd);
}

// Point-to-point in one pass (device loop): the sums both of the reference's
// passes need — sum w, sum w p, sum w q, the ErrorElements counters and the
// raw moments sum (w q) p^T — in one read of the matches.  The step forms the
// weighted means in T as p2point_means_kernel does and centres the moments in
// fp64: sum w (q - mq)(p - mp)^T = sum (w q) p^T - mq (sum w p)^T
// - (sum w q) mp^T + (sum w) mq mp^T (PointToPoint.cpp:67-81 by the same
// identity; the two-pass kernels above are the per-module path's).
template <typename T, bool SN, bool GD>
__global__ __launch_bounds__(256) void p2point_moments_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                              const P4<T>* __restrict__ ref, const T* __restrict__ d,
                                                              const int32_t* __restrict__ ids, WChain<T> chain, int k,
                                                              int64_t N, double* __restrict__ partials,
                                                              const LoopCtl* __restrict__ ctl,
                                                              const GridDesc<T>* __restrict__ gd) {
    SNPred<T> sn = chain.sn;
    GDPred<T> gdp = chain.gd;
    if (!p2point_begin<T, SN, GD>(ctl, gd, Tm, ref, sn, gdp)) return;
    p2point_sums_body<T, SN, true, GD>(rd, Tm, ref, d, ids, chain, sn, gdp, k, N, xcd_block(), partials);
}

template <typename T>
void launch_p2point_moments(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, double* partials,
                            const LoopCtl* ctl, const GridDesc<T>* gd, hipStream_t s) {
    auto* const kern = PMX_PICK(chain.sn.rn, chain.gd.desc, p2point_moments_kernel, T);
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, m.rd, Tm, m.ref, m.d, m.ids, chain, m.k, m.N, partials,
                       ctl, gd);
}

// Materialise the chain's weight of every entry e = slot * k + rank (the host
// mirror and what reads it; never on the hot path): entry_weight with what
// this chain's factors need loaded first.  A robust point-to-plane distance
// needs the step reading and the matched point and normal; the SurfaceNormal
// factor the matched normal, which at k = 1 comes from the match's neighbour
// record when there is one (nbr_n, slot order, no dependent gather).
template <typename T, bool SN, bool GD>
__global__ __launch_bounds__(256) void weights_chain_kernel(const P4<T>* __restrict__ rd, Mat4<T> Tm,
                                                            const P4<T>* __restrict__ ref,
                                                            const P4<T>* __restrict__ nrm, int rs,
                                                            const T* __restrict__ d, const int32_t* __restrict__ ids,
                                                            WChain<T> chain, int k, int64_t n,
                                                            const P4<T>* __restrict__ nbr_n, T* __restrict__ w) {
    const WRange<T> wr = chain_resolve(chain);
    const bool p2pl = chain.robust && chain.rb_p2pl;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t i = k == 1 ? e : e / k;
        const int32_t id = SN || GD || p2pl ? ids[e] : -1;
        T px = 0, py = 0, pz = 0;
        P4<T> q{}, qn{};
        if (id >= 0 && (!GD || SN || p2pl)) {  // (the descriptor factor alone reads no record)
            const int64_t g = (int64_t)id * rs;
            qn = nbr_n ? gld(nbr_n, i) : gld(nrm, g);
            if (p2pl) {
                q = gld(ref, g);
                xform3(Tm, rd[i], px, py, pz);
            }
        }
        w[e] = entry_weight<T, SN, true, GD>(chain, chain.sn, wr, Tm, d[e], id, px, py, pz, q, loaded(qn),
                                             [&]() { return gld(chain.sn.rn, i); }, chain.gd);
    }
}
template <typename T>
void launch_weights_chain(const MatchView<T>& m, const Mat4<T>& Tm, const WChain<T>& chain, T* w, hipStream_t s) {
    const int64_t n = m.N * m.k;
    if (n <= 0) return;
    int64_t g = (n + 1023) / 1024;
    if (g > 4096) g = 4096;
    auto* const kern = PMX_PICK(chain.sn.rn, chain.gd.desc, weights_chain_kernel, T);
    hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(256), 0, s, m.rd, Tm, m.pn, m.nrm, m.rs, m.d, m.ids, chain, m.k, n,
                       m.nbr ? m.nbr + m.N : nullptr, w);
}

#define PMX_INST(T)                                                                                                \
    template void launch_p2plane_partial<T>(const MatchView<T>&, const Mat4<T>&, const WChain<T>&, int, double*,  \
                                            const LoopCtl*, const GridDesc<T>*, unsigned long long*, hipStream_t); \
    template void launch_p2point_pass1<T>(const MatchView<T>&, const Mat4<T>&, const WChain<T>&, double*,         \
                                          const LoopCtl*, const GridDesc<T>*, hipStream_t);                        \
    template void launch_p2point_means<T>(const double*, T*, int, const LoopCtl*, hipStream_t);                    \
    template void launch_p2point_moments<T>(const MatchView<T>&, const Mat4<T>&, const WChain<T>&, double*,       \
                                            const LoopCtl*, const GridDesc<T>*, hipStream_t);                      \
    template void launch_p2point_pass2<T>(const MatchView<T>&, const Mat4<T>&, const WChain<T>&, const T*, bool,  \
                                          double*, const LoopCtl*, const GridDesc<T>*, hipStream_t);               \
    template void launch_weights_chain<T>(const MatchView<T>&, const Mat4<T>&, const WChain<T>&, T*, hipStream_t);
PMX_INST(float)
PMX_INST(double)
#undef PMX_INST


// Load this translation unit's code object now (pmx_ctx_create): HIP loads a
// module at the first launch of any of its kernels, and that host-side stall
// (milliseconds for the large grid module) would otherwise land inside the
// first ICP iteration.
void preload_reduce() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&finalize_kernel));
}

}  // namespace pmx

// pmx_quality.hip — the reductions behind ErrorMinimizer::getResidualError and
// getOverlap (pmx_quality.h has the per-link terms).
//
// Asked for at most once per ICP, after the loop stopped, never inside an
// iteration (no LoopCtl): two launches of 512 x 256 over the match arrays the
// last minimiser walked.  Bytes per link in float, first pass: dist 4,
// weight 4, and point-to-plane's reading 16 (per point) plus the point and
// normal records 32 in slot order (k = 1) or id 4 and two 16-byte gathers;
// with densities the id 4, the original id 4, the density 4 and the key 4
// written.  Second pass: dist 4, weight 4, the reading noise 4 per point, and
// with reference noise id 4, original id 4, noise 4.  The T terms go to fp64
// accumulators per lane; the block and finalize sums are the fixed-order ones
// of the other reductions (block_store, launch_finalize): deterministic.
#include "pmx_quality.h"
#include "pmx_p2plane.h"
#include "pmx_sort.h"

namespace pmx {

// the correctly rounded square root, whatever the build's flags say
__device__ __forceinline__ float sqrt_rn(float x) { return __fsqrt_rn(x); }
__device__ __forceinline__ double sqrt_rn(double x) { return __dsqrt_rn(x); }

template <typename T>
__device__ __forceinline__ bool quality_kept(const QualityIn<T>& in, int64_t e, T dv) {
    return dv != (T)__builtin_huge_val() && in.w[e] != (T)0;
}
// the original reference id of a kept link's match
template <typename T>
__device__ __forceinline__ int32_t quality_orig(const QualityIn<T>& in, int64_t e) {
    const int32_t id = in.m.ids[e];
    return in.m.gidx ? gld(in.m.gidx, id) : id;
}

template <typename T, bool PLANE>
__global__ __launch_bounds__(256) void match_quality_kernel(QualityIn<T> in, Mat4<T> Tm, T* __restrict__ keys,
                                                            double* __restrict__ partials) {
    using L = QualitySums;
    constexpr int NV = L::kPass1NV;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const int k = in.m.k;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)xcd_block() * blockDim.x + threadIdx.x; i < in.m.N; i += stride) {
        T px = 0, py = 0, pz = 0;
        if (PLANE) xform3(Tm, in.m.rd[i], px, py, pz);
        bool any = false;
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = in.m.d[e];
            const bool kept = quality_kept(in, e, dv);
            if (keys) keys[e] = kept ? in.dens_ref[quality_orig(in, e)] : (T)__builtin_huge_val();
            if (!kept) continue;
            any = true;
            const T r = sqrt_rn(dv);
            acc[L::kLinks] += 1.0;
            acc[L::kSqrtSum] += (double)r;
            if (PLANE) {
                P4<T> q, n;
                if (in.m.nbr) {  // (k = 1: the records in slot order)
                    q = in.m.nbr[i];
                    n = in.m.nbr[in.m.N + i];
                } else {
                    const int64_t g = (int64_t)in.m.ids[e] * in.m.rs;
                    q = gld(in.m.pn, g);
                    n = gld(in.m.nrm, g);
                }
                const T dx = px - q.x, dy = py - q.y, dz = pz - q.z;
                const T dot = ((dx * n.x) + (dy * n.y)) + (dz * n.z);  // PointToPlane.cpp:341-345
                acc[L::kResidual] += (double)(in.w[e] * (dot * dot));  // :347
            } else {
                acc[L::kResidual] += (double)r;  // PointToPoint.cpp:162-163
            }
        }
        if (any)
            acc[L::kPoints] += 1.0;
        else
            acc[L::kRejPoints] += 1.0;
    }
    block_store<NV>(acc, partials);
}

template <typename T, bool PLANE>
__global__ __launch_bounds__(256) void match_overlap_kernel(QualityIn<T> in, int branch, T base,
                                                            double* __restrict__ partials) {
    double acc[1] = {0.0};
    const int k = in.m.k;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)xcd_block() * blockDim.x + threadIdx.x; i < in.m.N; i += stride) {
        const T nr = branch != kQBReference ? in.noise_rd[i] : (T)0;
        bool hit = false;
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            const T dv = in.m.d[e];
            if (!quality_kept(in, e, dv)) continue;
            const T r = sqrt_rn(dv);
            if (PLANE) {
                T u = nr;  // PointToPlane.cpp:404-419
                if (branch == kQBDensity) u = (base + nr) + in.noise_ref[quality_orig(in, e)];
                if (branch == kQBBoth) u = nr + in.noise_ref[quality_orig(in, e)];
                if (branch == kQBReference) u = in.noise_ref[quality_orig(in, e)];
                hit = hit || r < u;
            } else if (r < base + nr) {  // PointToPoint.cpp:145
                acc[0] += 1.0;
            }
        }
        if (PLANE && hit) acc[0] += 1.0;
    }
    block_store<1>(acc, partials);
}

template <typename T>
void launch_match_quality(const QualityIn<T>& in, const Mat4<T>& Tm, bool plane, T* keys, double* partials,
                          hipStream_t s) {
    auto* const kern = plane ? match_quality_kernel<T, true> : match_quality_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, in, Tm, keys, partials);
}

template <typename T>
void launch_match_overlap(const QualityIn<T>& in, bool plane, int branch, T base, double* partials, hipStream_t s) {
    auto* const kern = plane ? match_overlap_kernel<T, true> : match_overlap_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(kRedBlocks), dim3(256), 0, s, in, branch, base, partials);
}

template <typename T>
hipError_t quality_median(const T* keys, int64_t n, int64_t P, T* median, hipStream_t s) {
    if (n <= 0 || P <= 0 || P > n || n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    T* sorted = nullptr;
    void* temp = nullptr;
    size_t bytes = 0;
    hipError_t e = pmx_sort_keys<T>(nullptr, bytes, keys, sorted, (int)n, 0, 8 * (int)sizeof(T), s);
    if (e == hipSuccess) e = hipMalloc((void**)&sorted, sizeof(T) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&temp, bytes > 0 ? bytes : 16);
    if (e == hipSuccess) e = pmx_sort_keys<T>(temp, bytes, keys, sorted, (int)n, 0, 8 * (int)sizeof(T), s);
    const size_t at = (size_t)((double)P * 0.5);  // values.size() * 0.5, PointToPlane.cpp:398
    if (e == hipSuccess) e = hipMemcpyAsync(median, sorted + at, sizeof(T), hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (sorted) (void)hipFree(sorted);
    if (temp) (void)hipFree(temp);
    return e;
}

#define PMX_INST(T)                                                                                              \
    template void launch_match_quality<T>(const QualityIn<T>&, const Mat4<T>&, bool, T*, double*, hipStream_t); \
    template void launch_match_overlap<T>(const QualityIn<T>&, bool, int, T, double*, hipStream_t);            \
    template hipError_t quality_median<T>(const T*, int64_t, int64_t, T*, hipStream_t);
PMX_INST(float)
PMX_INST(double)
#undef PMX_INST

}  // namespace pmx

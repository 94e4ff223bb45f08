// pmx_snormal.hip — SurfaceNormalOutlierFilter (pointmatcher/
// OutlierFiltersImpl.cpp:225-285) on the device: the reading's normals made
// resident (pmx_set_reading_normals) and the filter's weights on the module
// path (pmx_outlier_surface_normal, materialised for the host mirror).  The
// reductions evaluate the same predicate inline (pmx_snormal.h,
// pmx_reduce.hip).
#include "pmx_internal.h"
#include "pmx_snormal.h"

namespace pmx {

// out[s] = R_0 n[order[s]] as a 16-byte (f32) / 32-byte (f64) record
// (nx, ny, nz, 0): the rotation block of T_refMean_dataIn applied once
// (ICP.cpp:345-347 transforms the descriptors with the points), each
// component (m0 n0 + m1 n1) + m2 n2 in T.  order == null: identity.
template <typename T>
__global__ __launch_bounds__(256) void reading_normals_kernel(const T* __restrict__ raw, int D,
                                                              const int32_t* __restrict__ order, int64_t n,
                                                              Mat4<T> M0, P4<T>* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t q = order ? (int64_t)order[s] : s;
    const T* v = raw + q * D;
    P4<T> o{};
    if (D == 3) {
        const T x = v[0], y = v[1], z = v[2];
        o.x = (M0.m[0] * x + M0.m[1] * y) + M0.m[2] * z;
        o.y = (M0.m[4] * x + M0.m[5] * y) + M0.m[6] * z;
        o.z = (M0.m[8] * x + M0.m[9] * y) + M0.m[10] * z;
    } else {
        const T x = v[0], y = v[1];
        o.x = M0.m[0] * x + M0.m[1] * y;
        o.y = M0.m[4] * x + M0.m[5] * y;
    }
    out[s] = o;
}

template <typename T>
void launch_reading_normals(const T* raw, int D, const int32_t* order, int64_t n, const Mat4<T>& M0, P4<T>* out,
                            hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(reading_normals_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw, D, order,
                       n, M0, out);
}

// The filter's factor of the materialised weights: one thread per match
// entry e = slot * k + rank, w[e] *= 0/1.  The reading normal is one
// dwordx4 (f32) record per entry; the reference normal comes from the match's
// neighbour record (nbr_n: k = 1, slot order, no dependent gather) or from
// the records the ids index.  16 B reading normal + 4 B id + 16 B reference
// normal + 8 B weight per entry (f32).
template <typename T>
__global__ __launch_bounds__(256) void sn_weights_kernel(T* __restrict__ w, int64_t n, int k, SNPred<T> p, Mat4<T> Tm,
                                                         const int32_t* __restrict__ ids,
                                                         const P4<T>* __restrict__ nbr_n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int64_t i = k == 1 ? e : e / k;
    const int32_t id = ids[e];
    bool keep = false;
    if (id >= 0) {
        const P4<T> qn = nbr_n ? gld(nbr_n, i) : gld(p.nrm, (int64_t)id * p.rs);
        keep = sn_pass(p, Tm, gld(p.rn, i), qn);
    }
    w[e] = w[e] * (keep ? (T)1 : (T)0);
}

template <typename T>
void launch_sn_weights(T* w, int64_t n, int k, const SNPred<T>& p, const Mat4<T>& Tm, const int32_t* ids,
                       const P4<T>* nbr_n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sn_weights_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, n, k, p, Tm, ids,
                       nbr_n);
}

#define PMX_INST(T)                                                                                              \
    template void launch_reading_normals<T>(const T*, int, const int32_t*, int64_t, const Mat4<T>&, P4<T>*,     \
                                            hipStream_t);                                                        \
    template void launch_sn_weights<T>(T*, int64_t, int, const SNPred<T>&, const Mat4<T>&, const int32_t*,      \
                                       const P4<T>*, hipStream_t);
PMX_INST(float)
PMX_INST(double)
#undef PMX_INST

}  // namespace pmx

// pmx_snormal.hip — SurfaceNormalOutlierFilter (pointmatcher/
// OutlierFiltersImpl.cpp:225-285) on the device: the reading's normals made
// resident (pmx_set_reading_normals).  The predicate itself is sn_pass
// (pmx_weight.h), evaluated inside the chain's weight by the reductions and
// the materialising kernel (pmx_reduce.hip).
#include "pmx_internal.h"

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

template void launch_reading_normals<float>(const float*, int, const int32_t*, int64_t, const Mat4<float>&, P4<float>*,
                                            hipStream_t);
template void launch_reading_normals<double>(const double*, int, const int32_t*, int64_t, const Mat4<double>&,
                                             P4<double>*, hipStream_t);

}  // namespace pmx

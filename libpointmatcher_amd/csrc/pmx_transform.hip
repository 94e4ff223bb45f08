// pmx_transform.hip — a transformation applied to a whole cloud on the device:
// one point per lane, elementwise, memory-bound.  Two entries: a caller's
// cloud (transform_cloud_kernel) and the context's resident reading
// (transform_reading_kernel, below).
//
// Replaces Transformation::compute (pointmatcher/TransformationsImpl.cpp:49-87
// RigidTransformation, :157-195 SimilarityTransformation, :215-231
// PureTranslation): `parameters * features`, and `R * descriptor` for the spans
// the caller lists ("normals", "observationDirections"; R the top-left D x D
// block).  Inside the ICP loop the same arithmetic stays fused into the match
// (pmx_match.hip); this kernel is for the cloud the user keeps afterwards.
//
// Arithmetic contract (the project's, pmx_match.hip): every feature row r, the
// homogeneous one included, is
//   3-D  ((P_r0 x + P_r1 y) + P_r2 z) + P_r3 h
//   2-D  (P_r0 x + P_r1 y) + P_r2 h
// and every span row is the same sequential sum over R's row, every multiply
// and add rounded on its own (the pragma below).  NaN and infinities go through
// the expression like any other value.
//
// Kernel shape: a 3-D point is one 16-byte (float) / 32-byte (double) load and
// one store of the same width; a 2-D point three scalars each way.  The span
// list (at most kXformMaxSpans row offsets into a descriptor record of `stride`
// rows) lives in the kernel arguments; rows outside the spans are not touched.
// A lane reads its whole point and every span before it writes, so an output
// may be its own input.  2 * rows * sizeof(T) bytes move per point plus the
// spans, and nothing else: no LDS, no atomics, no cross-lane traffic.
#pragma clang fp contract(off)

#include "pmx_internal.h"

namespace pmx {

template <typename T, int D>
__global__ __launch_bounds__(256) void transform_cloud_kernel(const T* feat, int64_t n, const XformArgs<T> a,
                                                              const T* desc, int stride, T* feat_out, T* desc_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T* P = a.p;  // (D + 1) x (D + 1), row-major
    if (D == 3) {
        typedef typename Vec4Of<T>::V V;
        const V v = ((const V*)feat)[i];
        V o;
        o.x = ((P[0] * v.x + P[1] * v.y) + P[2] * v.z) + P[3] * v.w;
        o.y = ((P[4] * v.x + P[5] * v.y) + P[6] * v.z) + P[7] * v.w;
        o.z = ((P[8] * v.x + P[9] * v.y) + P[10] * v.z) + P[11] * v.w;
        o.w = ((P[12] * v.x + P[13] * v.y) + P[14] * v.z) + P[15] * v.w;
        ((V*)feat_out)[i] = o;
    } else {
        const T* p = feat + i * 3;
        const T x = p[0], y = p[1], h = p[2];
        T* o = feat_out + i * 3;
        o[0] = (P[0] * x + P[1] * y) + P[2] * h;
        o[1] = (P[3] * x + P[4] * y) + P[5] * h;
        o[2] = (P[6] * x + P[7] * y) + P[8] * h;
    }
    for (int k = 0; k < a.nspan; ++k) {  // (uniform: the offsets are scalar loads of the arguments)
        const int64_t at = i * stride + a.off[k];
        const T* d = desc + at;
        T* o = desc_out + at;
        if (D == 3) {
            const T x = d[0], y = d[1], z = d[2];
            o[0] = (P[0] * x + P[1] * y) + P[2] * z;
            o[1] = (P[4] * x + P[5] * y) + P[6] * z;
            o[2] = (P[8] * x + P[9] * y) + P[10] * z;
        } else {
            const T x = d[0], y = d[1];
            o[0] = P[0] * x + P[1] * y;
            o[1] = P[3] * x + P[4] * y;
        }
    }
}

template <typename T>
void launch_transform_cloud(const T* feat, int rows, int64_t n, const XformArgs<T>& a, const T* desc, int stride,
                            T* feat_out, T* desc_out, hipStream_t st) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (rows == 4)
        hipLaunchKernelGGL((transform_cloud_kernel<T, 3>), grid, dim3(256), 0, st, feat, n, a, desc, stride, feat_out,
                           desc_out);
    else
        hipLaunchKernelGGL((transform_cloud_kernel<T, 2>), grid, dim3(256), 0, st, feat, n, a, desc, stride, feat_out,
                           desc_out);
}

// The same transformation on the context's resident reading (pmx_transform_reading):
// no upload, one download.  rd are the reading's records in slot order
// (pmx_set_reading: T0 already applied; a 2-D record is (x, y, 0, w)), order the
// slot -> caller's index table (null: identity), nrm the resident normals'
// records (pmx_set_reading_normals; null: none asked for).  One slot per lane:
// the 16 / 32-byte record load is coalesced, the result goes to the caller's
// index q = order[s], point-major (rows values at feat_out + q * rows, D at
// nrm_out + q * D).  The scatter sits on the store side because the inverse
// table (index -> slot) is not resident: building it would be a scatter of its
// own plus a gathered record load.  Every store is a whole point (one 16 / 32
// byte vector store in 3-D), and the staging buffer is small enough to merge
// partial lines in the caches before they reach HBM (16 MB at 1M float points).
//
// The matrix is a.p, or, when Tdev is not null, the finished device loop's
// T_iter read here from LoopState (rows x rows, uniform loads): no host round
// trip.  Rows are the expression at the top of this file; with a.add_mean the
// un-centring translation follows as a separate step, (...) + mean[r], one
// more rounding (the host chain's reading is centred on the reference mean).
template <typename T, int D>
__global__ __launch_bounds__(256) void transform_reading_kernel(const P4<T>* __restrict__ rd,
                                                                const P4<T>* __restrict__ nrm,
                                                                const int32_t* __restrict__ order, int64_t n,
                                                                const XformReadingArgs<T> a,
                                                                const T* __restrict__ Tdev, T* __restrict__ feat_out,
                                                                T* __restrict__ nrm_out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int64_t q = order ? (int64_t)order[s] : s;
    if ((uint64_t)q >= (uint64_t)n) return;  // (a permutation of [0, n): never taken; no store leaves the buffer)
    constexpr int R = D + 1;
    T P[R * R];
#pragma unroll
    for (int e = 0; e < R * R; ++e) P[e] = Tdev ? Tdev[e] : a.p[e];
    const P4<T> v = gld(rd, s);
    if (D == 3) {
        typedef typename Vec4Of<T>::V V;
        V o;
        o.x = ((P[0] * v.x + P[1] * v.y) + P[2] * v.z) + P[3] * v.w;
        o.y = ((P[4] * v.x + P[5] * v.y) + P[6] * v.z) + P[7] * v.w;
        o.z = ((P[8] * v.x + P[9] * v.y) + P[10] * v.z) + P[11] * v.w;
        o.w = ((P[12] * v.x + P[13] * v.y) + P[14] * v.z) + P[15] * v.w;
        if (a.add_mean) {
            o.x = o.x + a.mean[0];
            o.y = o.y + a.mean[1];
            o.z = o.z + a.mean[2];
        }
        ((V*)feat_out)[q] = o;
    } else {
        T ox = (P[0] * v.x + P[1] * v.y) + P[2] * v.w;
        T oy = (P[3] * v.x + P[4] * v.y) + P[5] * v.w;
        const T ow = (P[6] * v.x + P[7] * v.y) + P[8] * v.w;
        if (a.add_mean) {
            ox = ox + a.mean[0];
            oy = oy + a.mean[1];
        }
        T* o = feat_out + q * 3;
        o[0] = ox;
        o[1] = oy;
        o[2] = ow;
    }
    if (nrm) {  // (uniform)
        const P4<T> m = gld(nrm, s);
        T* o = nrm_out + q * D;
        if (D == 3) {
            o[0] = (P[0] * m.x + P[1] * m.y) + P[2] * m.z;
            o[1] = (P[4] * m.x + P[5] * m.y) + P[6] * m.z;
            o[2] = (P[8] * m.x + P[9] * m.y) + P[10] * m.z;
        } else {
            o[0] = P[0] * m.x + P[1] * m.y;
            o[1] = P[3] * m.x + P[4] * m.y;
        }
    }
}

template <typename T>
void launch_transform_reading(const P4<T>* rd, const P4<T>* nrm, const int32_t* order, int rows, int64_t n,
                              const XformReadingArgs<T>& a, const T* Tdev, T* feat_out, T* nrm_out, hipStream_t st) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (rows == 4)
        hipLaunchKernelGGL((transform_reading_kernel<T, 3>), grid, dim3(256), 0, st, rd, nrm, order, n, a, Tdev,
                           feat_out, nrm_out);
    else
        hipLaunchKernelGGL((transform_reading_kernel<T, 2>), grid, dim3(256), 0, st, rd, nrm, order, n, a, Tdev,
                           feat_out, nrm_out);
}

template void launch_transform_cloud<float>(const float*, int, int64_t, const XformArgs<float>&, const float*, int,
                                            float*, float*, hipStream_t);
template void launch_transform_cloud<double>(const double*, int, int64_t, const XformArgs<double>&, const double*, int,
                                             double*, double*, hipStream_t);

template void launch_transform_reading<float>(const P4<float>*, const P4<float>*, const int32_t*, int, int64_t,
                                              const XformReadingArgs<float>&, const float*, float*, float*,
                                              hipStream_t);
template void launch_transform_reading<double>(const P4<double>*, const P4<double>*, const int32_t*, int, int64_t,
                                               const XformReadingArgs<double>&, const double*, double*, double*,
                                               hipStream_t);

// (pmx_ctx_create's code-object preload, as the other translation units')
void preload_transform() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&transform_reading_kernel<float, 3>));
}

}  // namespace pmx

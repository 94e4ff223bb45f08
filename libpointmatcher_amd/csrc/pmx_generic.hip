// pmx_generic.hip — GenericDescriptorOutlierFilter (pointmatcher/
// OutlierFiltersImpl.cpp:290-374) on the device: what the filter needs
// besides its per-pair factor (gd_weight, pmx_weight.h).
//
//   gd_permute_kernel  a grid level's copy of the reference's one-row weight
//                      descriptor in position order, out[pos] = desc[gidx[pos]],
//                      once per level and upload: a pair then costs one 4- or
//                      8-byte gather by its match id instead of two dependent
//                      ones (id -> gidx -> desc).
//   gd_max_kernel      soft mode's divisor m = max_e (id_e valid ? desc[id_e] : 0)
//                      over all k x N entries, the zeros of the entries without
//                      a neighbour included (the reference's weights.maxCoeff()
//                      of the matrix it has just filled, :365-371).
//
// The maximum: one grid-stride pass over the ids (4 B per entry + one gather),
// a wave maximum by shuffles, one LDS word per wave, one partial per block;
// the last block to arrive (a ticket) folds the partials in the same launch.
// A floating-point maximum is the same in every order (the descriptor holds
// no NaN: precondition of pmx_set_reference_weight_descriptor), so the fold
// needs no fixed order.  Every running maximum starts at -inf, never at 0: a
// match whose entries are all valid with negative descriptors has m < 0.
#include "pmx_internal.h"

namespace pmx {

template <typename T>
__global__ __launch_bounds__(256) void gd_permute_kernel(const T* __restrict__ desc, const int32_t* __restrict__ gidx,
                                                         int64_t n, T* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = desc[gidx[i]];
}

template <typename T>
void launch_gd_permute(const T* desc, const int32_t* gidx, int64_t n, T* out, hipStream_t s) {
    if (n <= 0) return;
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(gd_permute_kernel<T>, dim3((unsigned)g), dim3(256), 0, s, desc, gidx, n, out);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// the maximum of 256 per-thread values in thread 0 (red: 4 words of LDS)
__device__ __forceinline__ double block_max(double v, double* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double a = red[0] > red[1] ? red[0] : red[1];
    const double b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

template <typename T>
__global__ __launch_bounds__(256) void gd_max_kernel(const int32_t* __restrict__ ids, int64_t n,
                                                     const T* __restrict__ desc, double* __restrict__ partials,
                                                     unsigned int* __restrict__ ticket, double* __restrict__ out,
                                                     const LoopCtl* __restrict__ ctl,
                                                     const GridDesc<T>* __restrict__ gd) {
    __shared__ double red[4];
    __shared__ bool last;
    if (ctl) {  // device loop
        if (ctl->done) return;
        desc = gd[ctl->level].gw;
    }
    double m = -__builtin_huge_val();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int32_t id = gld(ids, e);
        const double v = id >= 0 ? (double)gd_load(desc, id) : 0.0;
        m = v > m ? v : m;
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) {
        // publish (write-through), then the ticket behind a release (as finalize_step_kernel, pmx_loop.hip)
        __hip_atomic_store(&partials[blockIdx.x], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __atomic_thread_fence(__ATOMIC_RELEASE);
        const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = old == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;  // (block-uniform)
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    double f = -__builtin_huge_val();
    for (int b = threadIdx.x; b < (int)gridDim.x; b += blockDim.x) {
        const double v = __hip_atomic_load(&partials[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f = v > f ? v : f;
    }
    __syncthreads();  // (red is read by block_max above)
    f = block_max(f, red);
    if (threadIdx.x == 0) {
        *out = f;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the next launch starts at 0)
    }
}

template <typename T>
void launch_gd_max(const int32_t* ids, int64_t n, const T* desc, double* partials, unsigned int* ticket, double* out,
                   const LoopCtl* ctl, const GridDesc<T>* gd, hipStream_t s) {
    int64_t g = (n + 1023) / 1024;
    g = g < 1 ? 1 : g > kGDMaxBlocks ? kGDMaxBlocks : g;
    hipLaunchKernelGGL(gd_max_kernel<T>, dim3((unsigned)g), dim3(256), 0, s, ids, n, desc, partials, ticket, out, ctl,
                       gd);
}

#define PMX_INST(T)                                                                                  \
    template void launch_gd_permute<T>(const T*, const int32_t*, int64_t, T*, hipStream_t);          \
    template void launch_gd_max<T>(const int32_t*, int64_t, const T*, double*, unsigned int*, double*, \
                                   const LoopCtl*, const GridDesc<T>*, hipStream_t);
PMX_INST(float)
PMX_INST(double)
#undef PMX_INST

}  // namespace pmx

// pmx_columns.h — the two small kernels the subsampling filters share
// (pmx_octree.hip, pmx_nss.hip): a = 0, 1, 2, ... for the flagged selects and
// sorts, and the gather of whole feature and descriptor columns once the kept
// columns are known.  Each includes pmx_sort.h beside it for the stable
// onesweep sort.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace pmx {

template <typename I>
__global__ __launch_bounds__(256) void iota_kernel(I* __restrict__ a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (I)i;
}

// output column k = input column src[k] (f: rows x n, d: desc_dim x n, point-major)
template <typename T>
__global__ __launch_bounds__(256) void gather_columns_kernel(const T* __restrict__ f, const T* __restrict__ d,
                                                             int rows, int desc_dim,
                                                             const int32_t* __restrict__ src, int64_t L,
                                                             T* __restrict__ of, T* __restrict__ od) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const int64_t s = src[k];
    for (int r = 0; r < rows; ++r) of[k * rows + r] = f[s * rows + r];
    for (int r = 0; r < desc_dim; ++r) od[k * desc_dim + r] = d[s * desc_dim + r];
}

static inline unsigned column_blocks(int64_t n) { return (unsigned)(n > 256 ? (n + 255) / 256 : 1); }

}  // namespace pmx

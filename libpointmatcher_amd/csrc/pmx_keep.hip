// pmx_keep.hip — the keep-filters on the device: a per-point predicate, then a
// stable compaction of whole feature and descriptor columns.
//
// Replaces the loops of
//   ShadowDataPointsFilter                    DataPointsFilters/Shadow.cpp:62-94
//   MaxQuantileOnAxisDataPointsFilter         DataPointsFilters/MaxQuantileOnAxis.cpp:65-98
//   RemoveNaNDataPointsFilter                 DataPointsFilters/RemoveNaN.cpp:47-66
//   CutAtDescriptorThresholdDataPointsFilter  DataPointsFilters/CutAtDescriptorThreshold.cpp:61-102
// which all walk the points once, copy column i to column j when the point is
// kept and resize to j.
//
// Predicates: evaluated in T in the reference's operation order (Eigen's dot
// and squaredNorm of a 2- or 3-vector are sequential sums; normalized() divides
// by sqrt(squaredNorm) when that is > 0 and returns the vector as it is
// otherwise, Eigen 3.3 Dot.h).  Every multiply and add is rounded on its own:
// the unit is compiled with -ffp-contract=off like the rest of the library, and
// the pragma below holds for this file whatever the command line says.
//
// MaxQuantileOnAxis's limit is the element of rank size_t(n * ratio) of one
// feature row.  The select kernels of pmx_select.hip order keys by their IEEE
// bit pattern, which is the numeric order of non-negative values only, so the
// row is split by sign first (one counting pass): the rank falls among the
// negative values, whose order is the reverse of their magnitudes', or among
// the non-negative ones (-0 counted as +0), and the select runs on that group
// with the rank inside it (kRatioRankBase).  No sort.
//
// Compaction: stable, deterministic, two passes and a scan, no atomics.
//   keep_flag_kernel     one point per thread; the wave's 64-bit ballot is
//                        stored (the scatter reads it back instead of
//                        evaluating the predicate twice) and the block's kept
//                        count is the sum of its four popcounts
//   keep_scan_kernel     exclusive scan of the block counts (one block)
//   keep_scatter_kernel  lane prefix = popcount of the ballot below the lane;
//                        the block lists its kept points in LDS, then copies
//                        their columns element by element: the block's output
//                        is one contiguous run, so the stores are coalesced
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "pmx_internal.h"

#include "../../include/pmx.h"

namespace pmx {

// (kKeepBlock points per block, one per thread, four waves: pmx_internal.h)

template <typename T>
struct KeepArgs {
    int pred;      // PMX_KEEP_*
    int rows;      // feature rows (D + 1)
    int desc_dim;  // descriptor rows
    int index;     // Shadow: row offset of "normals"; MaxQuantile: dim; CutAtDescriptor: descriptor row
    int flag;      // CutAtDescriptor: useLargerThan
    T value;       // Shadow: sin(eps); MaxQuantile: limit; CutAtDescriptor: threshold
};

template <typename T>
__device__ __forceinline__ T keep_sqrt(T v);
template <>
__device__ __forceinline__ float keep_sqrt<float>(float v) {
    return sqrtf(v);
}
template <>
__device__ __forceinline__ double keep_sqrt<double>(double v) {
    return sqrt(v);
}

// |normalized(n) . normalized(p)| (Shadow.cpp:80-84)
template <typename T>
__device__ __forceinline__ T shadow_value(const T* __restrict__ p, const T* __restrict__ nrm, int D) {
    T n0 = nrm[0], n1 = nrm[1], n2 = (T)0;
    T p0 = p[0], p1 = p[1], p2 = (T)0;
    T zn = n0 * n0;
    zn = zn + n1 * n1;
    T zp = p0 * p0;
    zp = zp + p1 * p1;
    if (D == 3) {
        n2 = nrm[2];
        p2 = p[2];
        zn = zn + n2 * n2;
        zp = zp + p2 * p2;
    }
    if (zn > (T)0) {
        const T s = keep_sqrt<T>(zn);
        n0 = n0 / s;
        n1 = n1 / s;
        n2 = n2 / s;
    }
    if (zp > (T)0) {
        const T s = keep_sqrt<T>(zp);
        p0 = p0 / s;
        p1 = p1 / s;
        p2 = p2 / s;
    }
    T dot = n0 * p0;
    dot = dot + n1 * p1;
    if (D == 3) dot = dot + n2 * p2;
    return dot < (T)0 ? -dot : dot;  // anyabs (Functions.h:44-50)
}

template <typename T>
__device__ __forceinline__ bool keep_pred(const KeepArgs<T>& a, const T* __restrict__ f, const T* __restrict__ d) {
    switch (a.pred) {
        case PMX_KEEP_SHADOW:
            return shadow_value<T>(f, d + a.index, a.rows - 1) > a.value;
        case PMX_KEEP_MAX_QUANTILE:
            return f[a.index] < a.value;
        case PMX_KEEP_REMOVE_NAN: {  // !(col == col).all() over every feature row, the homogeneous one included
            bool all = true;
            for (int r = 0; r < a.rows; ++r) all = all && (f[r] == f[r]);
            return all;
        }
        default: {  // PMX_KEEP_CUT_DESCRIPTOR
            const T v = d[a.index];
            return a.flag ? (v <= a.value) : (v >= a.value);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kKeepBlock) void keep_flag_kernel(const T* __restrict__ f, const T* __restrict__ d,
                                                               int64_t n, KeepArgs<T> a,
                                                               unsigned long long* __restrict__ masks,
                                                               uint32_t* __restrict__ block_cnt) {
    const int64_t i = (int64_t)blockIdx.x * kKeepBlock + threadIdx.x;
    bool k = false;
    if (i < n) k = keep_pred<T>(a, f + i * a.rows, d + i * a.desc_dim);
    keep_block_ballot(k, masks, block_cnt);
}

// off[b] = kept points of the blocks before b; off[nb] = the kept count
__global__ __launch_bounds__(256) void keep_scan_kernel(const uint32_t* __restrict__ cnt, int64_t nb,
                                                        uint32_t* __restrict__ off) {
    __shared__ uint32_t wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (int64_t base = 0; base < nb; base += 256) {  // uniform
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? cnt[i] : 0u;
        uint32_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(x, o);
            if (lane >= o) x += u;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wsum[w];
            tot += wsum[w];
        }
        if (i < nb) off[i] = carry + before + x - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nb] = carry;
}

template <typename T>
__global__ __launch_bounds__(kKeepBlock) void keep_scatter_kernel(const T* __restrict__ f, const T* __restrict__ d,
                                                                  int rows, int desc_dim,
                                                                  const unsigned long long* __restrict__ masks,
                                                                  const uint32_t* __restrict__ off,
                                                                  T* __restrict__ of, T* __restrict__ od) {
    __shared__ uint32_t src[kKeepBlock];  // the block's kept points (thread ids), in point order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* bm = masks + (int64_t)blockIdx.x * kKeepWaves;
    const unsigned long long m = bm[wave];
    uint32_t wpre = 0, cnt = 0;
    for (int w = 0; w < kKeepWaves; ++w) {
        const uint32_t c = (uint32_t)__popcll(bm[w]);
        if (w < wave) wpre += c;
        cnt += c;
    }
    if ((m >> lane) & 1ull) src[wpre + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = threadIdx.x;
    __syncthreads();
    if (cnt == 0) return;  // uniform
    const int64_t p0 = (int64_t)blockIdx.x * kKeepBlock;  // (a set bit is a point below n: keep_flag_kernel)
    const int64_t o0 = (int64_t)off[blockIdx.x];
    T* bf = of + o0 * rows;
    for (uint32_t e = threadIdx.x; e < cnt * (uint32_t)rows; e += kKeepBlock) {
        const uint32_t q = e / (uint32_t)rows, r = e - q * (uint32_t)rows;
        bf[e] = f[(p0 + src[q]) * rows + r];
    }
    if (desc_dim > 0) {
        T* bd = od + o0 * desc_dim;
        for (uint32_t e = threadIdx.x; e < cnt * (uint32_t)desc_dim; e += kKeepBlock) {
            const uint32_t q = e / (uint32_t)desc_dim, r = e - q * (uint32_t)desc_dim;
            bd[e] = d[(p0 + src[q]) * desc_dim + r];
        }
    }
}

// ---- MaxQuantileOnAxis: the limit ----
// classes of one feature row, in ascending order: -inf, negative, non-negative
// (both zeros), +inf, NaN (no order in the reference: placed last)
constexpr int kAxisClasses = 5;
constexpr int kAxisBlocks = 256;

template <typename T>
__device__ __forceinline__ int axis_class(T v) {
    if (!(v == v)) return 4;
    if (v == -(T)__builtin_huge_val()) return 0;
    if (v == (T)__builtin_huge_val()) return 3;
    return v < (T)0 ? 1 : 2;
}

template <typename T>
__global__ __launch_bounds__(256) void keep_axis_count_kernel(const T* __restrict__ f, int rows, int dim, int64_t n,
                                                              uint32_t* __restrict__ part) {
    __shared__ uint32_t sc[kAxisClasses][4];
    uint32_t c[kAxisClasses] = {0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int k = axis_class<T>(f[i * rows + dim]);
#pragma unroll
        for (int q = 0; q < kAxisClasses; ++q) c[q] += k == q ? 1u : 0u;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kAxisClasses; ++q) {
        uint32_t x = c[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if (lane == 0) sc[q][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < kAxisClasses)
        part[blockIdx.x * kAxisClasses + threadIdx.x] =
            sc[threadIdx.x][0] + sc[threadIdx.x][1] + sc[threadIdx.x][2] + sc[threadIdx.x][3];
}

// the select's keys: the magnitudes of the group the rank falls in, +inf
// (which the select leaves out) for every other point
template <typename T>
__global__ __launch_bounds__(256) void keep_axis_key_kernel(const T* __restrict__ f, int rows, int dim, int64_t n,
                                                            int group, T* __restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const T v = f[i * rows + dim];
        T k = (T)__builtin_huge_val();
        if (axis_class<T>(v) == group) k = group == 1 ? -v : (v == (T)0 ? (T)0 : v);  // (-0 -> +0)
        key[i] = k;
    }
}

static unsigned keep_stream_grid(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
}

// The element of rank `rank` (0-based, < n) of feature row dim, as
// std::nth_element leaves it at that position; NaN rows: see above.
template <typename T>
static int axis_rank_value(const T* d_f, int rows, int dim, int64_t n, int64_t rank, T* limit, hipStream_t st) {
    char* buf = nullptr;
    const size_t kb = (sizeof(T) * (size_t)n + 255) & ~(size_t)255;
    const size_t pb = sizeof(uint32_t) * kAxisBlocks * kAxisClasses, hb = sizeof(uint32_t) * 2048;
    if (hipMalloc(&buf, kb + pb + hb + 512) != hipSuccess) return PMX_E_HIP;
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    T* key = (T*)buf;
    uint32_t* part = (uint32_t*)(buf + kb);
    uint32_t* hist = part + kAxisBlocks * kAxisClasses;
    SelectState* sel = (SelectState*)((char*)(hist + 2048));
    int* ierr = (int*)((char*)sel + 256);
    const unsigned cb = std::min<unsigned>(keep_stream_grid(n), kAxisBlocks);
    hipLaunchKernelGGL(keep_axis_count_kernel<T>, dim3(cb), dim3(256), 0, st, d_f, rows, dim, n, part);
    std::vector<uint32_t> hp((size_t)cb * kAxisClasses);
    if (hipMemcpyAsync(hp.data(), part, sizeof(uint32_t) * hp.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    int64_t cls[kAxisClasses] = {0, 0, 0, 0, 0};
    for (unsigned b = 0; b < cb; ++b)
        for (int q = 0; q < kAxisClasses; ++q) cls[q] += hp[(size_t)b * kAxisClasses + q];
    int group = 0;
    int64_t below = 0;
    while (group < kAxisClasses - 1 && rank >= below + cls[group]) below += cls[group++];
    if (group == 0) *limit = -(T)INFINITY;
    if (group == 3) *limit = (T)INFINITY;
    if (group == 4) *limit = (T)NAN;
    if (group != 1 && group != 2) return PMX_OK;
    // negative values ascend as their magnitudes descend
    const int64_t r = group == 1 ? cls[1] - 1 - (rank - below) : rank - below;
    if (hipMemsetAsync(hist, 0, hb + 512, st) != hipSuccess) return PMX_E_HIP;
    hipLaunchKernelGGL(keep_axis_key_kernel<T>, dim3(keep_stream_grid(n)), dim3(256), 0, st, d_f, rows, dim, n, group,
                       key);
    for (int p = 0; p < select_passes<T>(); ++p) {
        launch_select_hist<T>(key, n, hist, sel, p, nullptr, nullptr, st);
        launch_select_pick<T>(hist, sel, p, kRatioRankBase + (double)r, nullptr, ierr, nullptr, nullptr, st);
    }
    SelectState hs;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&hs, sel, sizeof(hs), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    if (hs.err) return PMX_E_STATE;  // (cannot happen: the group holds the rank)
    *limit = group == 1 ? -(T)hs.limit : (T)hs.limit;
    return PMX_OK;
}

// d_f: rows x n point-major on the device, d_desc desc_dim x n (or null).
// Outputs (device, capacity n): d_of, d_od; *n_out.
template <typename T>
int keep_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int pred, int index, int flag,
             double value, T* d_of, T* d_od, int64_t* n_out, hipStream_t st, std::string& err) {
    *n_out = 0;
    if (rows != 3 && rows != 4) {
        err = "keep filter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (desc_dim < 0) {
        err = "keep filter: negative descriptor dimension";
        return PMX_E_BAD_PARAM;
    }
    const int D = rows - 1;
    switch (pred) {
        case PMX_KEEP_SHADOW:
            if (index < 0 || index + D > desc_dim) {
                err = "keep filter: Shadow needs the row offset of a normals descriptor of the cloud's dimension";
                return PMX_E_BAD_PARAM;
            }
            break;
        case PMX_KEEP_MAX_QUANTILE:
            if (index < 0 || index >= rows) {
                err = "keep filter: MaxQuantileOnAxis dim is not a feature row";
                return PMX_E_BAD_PARAM;
            }
            break;
        case PMX_KEEP_REMOVE_NAN:
            break;
        case PMX_KEEP_CUT_DESCRIPTOR:
            if (index < 0 || index >= desc_dim) {
                err = "keep filter: CutAtDescriptorThreshold needs the row of a descriptor";
                return PMX_E_BAD_PARAM;
            }
            break;
        default:
            err = "keep filter: unknown predicate";
            return PMX_E_BAD_PARAM;
    }
    if (n <= 0) return PMX_OK;
    if (n > (int64_t)0x7fffffff) {
        err = "keep filter: more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    KeepArgs<T> a;
    a.pred = pred;
    a.rows = rows;
    a.desc_dim = desc_dim;
    a.index = index;
    a.flag = flag;
    a.value = (T)value;
    if (pred == PMX_KEEP_MAX_QUANTILE) {
        // MaxQuantileOnAxis.cpp:73-85: nth_element at size * ratio, the product in T
        int64_t rank = (int64_t)(size_t)((T)n * (T)value);
        if (rank >= n) rank = n - 1;  // (the reference reads past its vector there)
        const int rc = axis_rank_value<T>(d_f, rows, index, n, rank, &a.value, st);
        if (rc) {
            err = "keep filter: the quantile select failed";
            return rc;
        }
    }
    KeepScratch sc;
    if (sc.alloc(n) != PMX_OK) {
        err = "keep filter: device allocation failed";
        return PMX_E_HIP;
    }
    hipLaunchKernelGGL(keep_flag_kernel<T>, dim3((unsigned)sc.nb), dim3(kKeepBlock), 0, st, d_f, d_desc, n, a,
                       sc.masks, sc.cnt);
    if (keep_compact<T>(d_f, rows, d_desc, desc_dim, sc, d_of, d_od, n_out, st) != PMX_OK) {
        err = "keep filter: HIP failure";
        return PMX_E_HIP;
    }
    return PMX_OK;
}

int KeepScratch::alloc(int64_t n) {
    nb = (n + kKeepBlock - 1) / kKeepBlock;
    char* buf = nullptr;
    const size_t mb = sizeof(unsigned long long) * (size_t)nb * kKeepWaves;
    const size_t cb = (sizeof(uint32_t) * (size_t)nb + 255) & ~(size_t)255;
    const size_t ob = sizeof(uint32_t) * (size_t)(nb + 1);
    if (hipMalloc(&buf, mb + cb + ob) != hipSuccess) return PMX_E_HIP;
    masks = (unsigned long long*)buf;
    cnt = (uint32_t*)(buf + mb);
    off = (uint32_t*)(buf + mb + cb);
    return PMX_OK;
}

void launch_keep_scan(const KeepScratch& s, hipStream_t st) {
    hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(256), 0, st, s.cnt, s.nb, s.off);
}

// the scan and the scatter over the ballots and block counts a flag kernel left in s
template <typename T>
int keep_compact(const T* d_f, int rows, const T* d_desc, int desc_dim, const KeepScratch& s, T* d_of,
                 T* d_od, int64_t* n_out, hipStream_t st) {
    hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(256), 0, st, s.cnt, s.nb, s.off);
    hipLaunchKernelGGL(keep_scatter_kernel<T>, dim3((unsigned)s.nb), dim3(kKeepBlock), 0, st, d_f, d_desc, rows,
                       desc_dim, s.masks, s.off, d_of, d_od);
    uint32_t kept = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&kept, s.off + s.nb, sizeof(kept), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    *n_out = (int64_t)kept;
    return PMX_OK;
}

template int keep_compact<float>(const float*, int, const float*, int, const KeepScratch&, float*, float*,
                                 int64_t*, hipStream_t);
template int keep_compact<double>(const double*, int, const double*, int, const KeepScratch&, double*, double*,
                                  int64_t*, hipStream_t);

template int keep_run<float>(const float*, int, int64_t, const float*, int, int, int, int, double, float*, float*,
                             int64_t*, hipStream_t, std::string&);
template int keep_run<double>(const double*, int, int64_t, const double*, int, int, int, int, double, double*, double*,
                              int64_t*, hipStream_t, std::string&);

}  // namespace pmx

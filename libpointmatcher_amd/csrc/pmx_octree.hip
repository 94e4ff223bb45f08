// pmx_octree.hip — OctreeGridDataPointsFilter on the device
// (DataPointsFilters/OctreeGrid.cpp:48-366, the tree utils/octree.hpp:229-385).
//
// The reference builds the tree by recursion: a node is a leaf when
// double(radius) * 2 <= maxSizeByNode or it holds <= maxPointByNode points,
// else each point goes to child sum_i (p_i > center_i) << i, whose radius is
// radius * 0.5 and whose centre is center +- 0.5 * radius per axis, all in T
// (octree.hpp:312-341).  The visit is depth first, children in index order,
// and a sampler keeps one point per non-empty leaf.
//
// A point's path depends on the point alone, so here every point descends by
// itself and the tree is never built:
//   oct_key_kernel   one point per lane walks K levels from its node (the root
//                    in the first round), centre and radius recomputed in T
//                    exactly as above, and packs the child indices into a
//                    64-bit key below the number of the run it belongs to
//   pmx_sort_pairs   a stable sort of (key, point): visit order between nodes,
//                    input order inside one
//   oct_leaf_kernel  a point's leaf is the shortest key prefix whose run of
//                    equal-prefix neighbours holds <= maxPointByNode points (a
//                    bounded binary search on the sorted keys: the run is
//                    longer iff its ends are more than maxPointByNode apart),
//                    or the depth of the size limit, the same for every point
//   a run still longer than maxPointByNode after K levels goes to a further
//   round: its points are compacted (two scans), numbered by run, and descend
//   K more levels from the node they stopped in; the run number is the top of
//   the next key, so one sort keeps every run in place.
//   Inside a leaf the sorted keys order the members by their deeper path, not
//   by index as the reference lists them (children receive their points in the
//   parent's order): a last stable sort of (leaf number, point), the points
//   taken in index order, puts every leaf's members in rising index.
// Termination: with maxSizeByNode 0 duplicates separate only when the radius
// underflows to 0, up to ~150 levels in float and ~2100 in double.  A node
// whose candidate child centres all equal its own centre separates its points
// once more and never again (every deeper node has the same centre, so every
// point repeats its child index): the descent stops one level below it and
// calls that a leaf.  The leaves and their order are the recursion's.
//
// Samplers (leaf k in visit order, members by rising input index):
//   first, random   one pick per leaf; the random factors are drawn on the host
//                   and the reference's swapCols / mapidx sequence is replayed
//                   there on column numbers (common/pmx_octree_replay.h), then
//                   whole columns are gathered: bit-identical to the
//                   reference, its stale lookups included
//   centroid, medoid  one leaf per lane, sequential sums in member order in T;
//                   column k is computed from the input cloud (the reference
//                   reads columns through the stale table: see DESIGN.md)
// No atomics; deterministic.  Non-finite coordinates are outside the contract
// (an infinite root box is refused).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "common/pmx_octree_replay.h"
#include "pmx_columns.h"
#include "pmx_internal.h"
#include "pmx_sort.h"

#include "../../include/pmx.h"

namespace pmx {

constexpr int kOctNoStop = 255;  // no forced leaf within this round's levels

template <typename T>
struct OctNode {
    T c[3];
    T r;
};

template <typename T>
__global__ __launch_bounds__(256) void oct_minmax_kernel(const T* __restrict__ f, int rows, int64_t n,
                                                         T* __restrict__ part) {
    const int D = rows - 1;
    T mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        mn[a] = (T)__builtin_huge_val();
        mx[a] = -(T)__builtin_huge_val();
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        for (int a = 0; a < D; ++a) {
            const T v = f[i * rows + a];
            mn[a] = v < mn[a] ? v : mn[a];
            mx[a] = v > mx[a] ? v : mx[a];
        }
    __shared__ T smn[3][256], smx[3][256];
    for (int a = 0; a < 3; ++a) {
        smn[a][threadIdx.x] = mn[a];
        smx[a][threadIdx.x] = mx[a];
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                const T b = smn[a][threadIdx.x + s], c = smx[a][threadIdx.x + s];
                smn[a][threadIdx.x] = b < smn[a][threadIdx.x] ? b : smn[a][threadIdx.x];
                smx[a][threadIdx.x] = c > smx[a][threadIdx.x] ? c : smx[a][threadIdx.x];
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int a = 0; a < 3; ++a) {
            part[blockIdx.x * 6 + a] = smn[a][0];
            part[blockIdx.x * 6 + 3 + a] = smx[a][0];
        }
}

// One active point per lane: K levels down from its node.  aidx / aseg: the
// point and the run of slot j (null in the first round: point j, run 0, node
// = root).  limit: the levels left before the size limit's depth (>= 0; the
// node at that level is a leaf whatever it holds).  Writes the key (run number
// above K * DIM path bits, zero below a forced leaf), by point the level of
// the forced leaf on its path (kOctNoStop when there is none up to K) and the
// node reached after K levels.
template <typename T, int DIM>
__global__ __launch_bounds__(256) void oct_key_kernel(const T* __restrict__ f, int rows,
                                                      const uint32_t* __restrict__ aidx,
                                                      const uint32_t* __restrict__ aseg, int64_t m, OctNode<T> root,
                                                      int K, int limit, T* __restrict__ state,
                                                      unsigned long long* __restrict__ key,
                                                      uint8_t* __restrict__ stop) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int64_t idx = aidx ? (int64_t)aidx[j] : j;
    T p[DIM], c[DIM], r;
#pragma unroll
    for (int a = 0; a < DIM; ++a) p[a] = f[idx * rows + a];
    if (aidx) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) c[a] = state[idx * (DIM + 1) + a];
        r = state[idx * (DIM + 1) + DIM];
    } else {
#pragma unroll
        for (int a = 0; a < DIM; ++a) c[a] = root.c[a];
        r = root.r;
    }
    const int levels = limit < K ? limit : K;
    int st = limit <= K ? limit : kOctNoStop;
    unsigned long long bits = 0;
    int l = 0;
    while (l < levels) {
        const T h = r * (T)0.5;  // the children's radius and, signed, their centre offset (octree.hpp:335-340)
        unsigned child = 0;
        bool stalled = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const T up = c[a] + h, dn = c[a] - h;
            stalled = stalled && up == c[a] && dn == c[a];
            const bool gt = p[a] > c[a];  // octree.hpp:186
            child |= (gt ? 1u : 0u) << a;
            c[a] = gt ? up : dn;
        }
        r = h;
        bits = (bits << DIM) | child;
        ++l;
        if (stalled) {  // the child just entered never separates its points again
            st = l;
            break;
        }
    }
    bits <<= DIM * (K - l);
    const unsigned long long seg = aseg ? (unsigned long long)aseg[j] : 0ull;
    key[j] = (seg << (DIM * K)) | bits;  // (DIM * K <= 63)
    stop[idx] = (uint8_t)st;
    if (l == K) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) state[idx * (DIM + 1) + a] = c[a];
        state[idx * (DIM + 1) + DIM] = r;
    }
}

// Whether the run of keys equal to key[j] above `shift` holds more than w
// entries; w < m.  The keys are sorted, so the run is an interval and only the
// w entries on either side of j matter.
__device__ __forceinline__ bool oct_run_longer(const unsigned long long* __restrict__ key, int64_t m, int64_t j,
                                               int shift, int64_t w) {
    const unsigned long long pk = key[j] >> shift;
    int64_t lo = j - w < 0 ? 0 : j - w, hi = j;  // first entry of the run, in [lo, hi]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((key[mid] >> shift) == pk)
            hi = mid;
        else
            lo = mid + 1;
    }
    const int64_t first = lo;
    lo = j + 1;
    hi = j + w + 1 > m ? m : j + w + 1;  // first entry past the run, in [lo, hi]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((key[mid] >> shift) == pk)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - first > w;
}

// One sorted slot per lane: its leaf level, the point's place in the visit
// order, whether it starts a leaf, or that it needs another round (unres) and
// starts a run of it (uhead).  apos: the slots' positions in the order (null
// in the first round: slot j).  Slot m of unres / uhead is zeroed for the
// scans' totals.
template <int DIM>
__global__ __launch_bounds__(256) void oct_leaf_kernel(const unsigned long long* __restrict__ key,
                                                       const uint32_t* __restrict__ sidx,
                                                       const uint32_t* __restrict__ apos,
                                                       const uint8_t* __restrict__ stop, int64_t m, int K,
                                                       int64_t max_pts, uint32_t* __restrict__ order,
                                                       uint32_t* __restrict__ head, uint32_t* __restrict__ unres,
                                                       uint32_t* __restrict__ uhead) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    if (j == 0) {
        unres[m] = 0;
        uhead[m] = 0;
    }
    const uint32_t idx = sidx[j];
    const int st = stop[idx];
    const int top = st < K ? st : K;  // the deepest level this round can call a leaf by its count
    int lo = 0, hi = top + 1;         // first level whose run holds <= max_pts points; top + 1: none
    if (max_pts >= m) {
        hi = 0;
    }
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (oct_run_longer(key, m, j, DIM * (K - mid), max_pts))
            lo = mid + 1;
        else
            hi = mid;
    }
    const bool resolved = lo <= top || st <= K;
    const int level = lo <= top ? lo : top;
    const unsigned long long k = key[j];
    const unsigned long long prev = j > 0 ? key[j - 1] : 0ull;
    const int shift = DIM * (K - level);
    const int64_t pos = apos ? (int64_t)apos[j] : j;
    order[pos] = idx;
    head[pos] = (resolved && (j == 0 || (prev >> shift) != (k >> shift))) ? 1u : 0u;
    unres[j] = resolved ? 0u : 1u;
    uhead[j] = (!resolved && (j == 0 || prev != k)) ? 1u : 0u;
}

// the next round's slots: the unresolved ones, in order, numbered by run
__global__ __launch_bounds__(256) void oct_compact_kernel(const uint32_t* __restrict__ sidx,
                                                          const uint32_t* __restrict__ apos,
                                                          const uint32_t* __restrict__ unres,
                                                          const uint32_t* __restrict__ uhead,
                                                          const uint32_t* __restrict__ uoff,
                                                          const uint32_t* __restrict__ hoff, int64_t m,
                                                          uint32_t* __restrict__ nidx, uint32_t* __restrict__ npos,
                                                          uint32_t* __restrict__ nseg) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || !unres[j]) return;
    const uint32_t t = uoff[j];
    nidx[t] = sidx[j];
    npos[t] = apos ? apos[j] : (uint32_t)j;
    nseg[t] = hoff[j] + uhead[j] - 1u;
}

// by point: the number of its leaf (hoff: the exclusive scan of the head flags)
__global__ __launch_bounds__(256) void oct_leaf_of_point_kernel(const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ head,
                                                                const uint32_t* __restrict__ hoff, int64_t n,
                                                                uint32_t* __restrict__ leaf) {
    const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < n) leaf[order[pos]] = hoff[pos] + head[pos] - 1u;
}

// first / random: the pick of leaf k (OctreeGrid.cpp:53, 104-109); fac null: the first member
__global__ __launch_bounds__(256) void oct_pick_kernel(const uint32_t* __restrict__ order,
                                                       const uint32_t* __restrict__ segs, int64_t L, int64_t n,
                                                       const float* __restrict__ fac, int32_t* __restrict__ pick) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t a = segs[k];
    const uint32_t b = k + 1 < L ? segs[k + 1] : (uint32_t)n;
    unsigned long long id = 0;
    if (fac) {
        const unsigned long long last = (unsigned long long)(b - a - 1u);
        id = (unsigned long long)((float)last * fac[k]);  // size_t(nbData * float): the product in float
        if (id > last) id = last;  // (float(last) rounds up beyond 2^24 members; the reference reads past its vector)
    }
    pick[k] = (int32_t)order[a + (uint32_t)id];
}

template <typename T>
__device__ __forceinline__ T oct_sqrt(T v);
template <>
__device__ __forceinline__ float oct_sqrt<float>(float v) {
    return sqrtf(v);
}
template <>
__device__ __forceinline__ double oct_sqrt<double>(double v) {
    return sqrt(v);
}

template <typename T>
__device__ __forceinline__ T oct_max();  // numeric_limits<T>::max()
template <>
__device__ __forceinline__ float oct_max<float>() {
    return __FLT_MAX__;
}
template <>
__device__ __forceinline__ double oct_max<double>() {
    return __DBL_MAX__;
}

// centroid / medoid: one leaf per lane, every sum sequential in member order
// (OctreeGrid.cpp:147-210, 219-282, read from the input cloud's own columns)
template <typename T>
__global__ __launch_bounds__(256) void oct_record_kernel(const T* __restrict__ f, const T* __restrict__ d, int rows,
                                                         int desc_dim, const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ segs, int64_t L, int64_t n,
                                                         int medoid, T* __restrict__ of, T* __restrict__ od) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const int D = rows - 1;
    const uint32_t a = segs[k];
    const uint32_t b = k + 1 < L ? segs[k + 1] : (uint32_t)n;
    const T cnt = (T)(unsigned long long)(b - a);
    if (!medoid) {
        const int64_t first = order[a];
        for (int r = 0; r < D; ++r) {
            T s = f[first * rows + r];
            for (uint32_t q = a + 1; q < b; ++q) s += f[(int64_t)order[q] * rows + r];
            of[k * rows + r] = s / cnt;
        }
        of[k * rows + D] = f[first * rows + D];
        for (int r = 0; r < desc_dim; ++r) {
            T s = d[first * desc_dim + r];
            for (uint32_t q = a + 1; q < b; ++q) s += d[(int64_t)order[q] * desc_dim + r];
            od[k * desc_dim + r] = s / cnt;
        }
        return;
    }
    T c[3] = {(T)0, (T)0, (T)0};
    for (int r = 0; r < D; ++r) {
        T s = (T)0;
        for (uint32_t q = a; q < b; ++q) s += f[(int64_t)order[q] * rows + r];
        c[r] = s / cnt;
    }
    T best = oct_max<T>();
    int64_t med = 0;  // (the reference's medId = 0 when no distance is below max())
    for (uint32_t q = a; q < b; ++q) {
        const int64_t i = order[q];
        T z = (T)0;
        for (int r = 0; r < D; ++r) {
            const T e = f[i * rows + r] - c[r];
            const T e2 = e * e;
            z = r == 0 ? e2 : z + e2;
        }
        const T dist = oct_sqrt<T>(z);
        if (dist < best) {
            best = dist;
            med = i;
        }
    }
    for (int r = 0; r < rows; ++r) of[k * rows + r] = f[med * rows + r];
    for (int r = 0; r < desc_dim; ++r) od[k * desc_dim + r] = d[med * desc_dim + r];
}

static unsigned oct_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

template <typename T, int DIM>
static void launch_oct_key(const T* f, int rows, const uint32_t* aidx, const uint32_t* aseg, int64_t m,
                           const OctNode<T>& root, int K, int limit, T* state, unsigned long long* key, uint8_t* stop,
                           hipStream_t st) {
    hipLaunchKernelGGL((oct_key_kernel<T, DIM>), dim3(oct_blocks(m)), dim3(256), 0, st, f, rows, aidx, aseg, m, root,
                       K, limit, state, key, stop);
}

// d_f: rows x n point-major on the device, d_desc desc_dim x n (or null).
// Outputs (device, capacity n): d_of, d_od; *n_out.
template <typename T>
int octree_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int64_t max_pts, double max_size,
               int method, T* d_of, T* d_od, int64_t* n_out, hipStream_t st, std::string& err) {
    *n_out = 0;
    if (rows != 3 && rows != 4) {
        err = "OctreeGridDataPointsFilter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    if (method < 0 || method > 3) {
        err = "OctreeGridDataPointsFilter: samplingMethod must be 0 (first), 1 (random), 2 (centroid) or 3 (medoid)";
        return PMX_E_BAD_PARAM;
    }
    if (desc_dim < 0 || max_pts < 1 || !(max_size >= 0.0)) {
        err = "OctreeGridDataPointsFilter: maxPointByNode must be >= 1, maxSizeByNode >= 0, the descriptor dimension "
              ">= 0";
        return PMX_E_BAD_PARAM;
    }
    if (n <= 0) return PMX_OK;
    if (n > (int64_t)0x7fffffff) {
        err = "OctreeGridDataPointsFilter: more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    const int D = rows - 1;
    // ---- the root box (octree.hpp:238-251), in T ----
    const unsigned nb = (unsigned)std::min<int64_t>(oct_blocks(n), 1024);
    // one allocation: the arrays below, each aligned to 256 bytes
    uint32_t *order, *head, *idxA, *idxB, *posA, *posB, *seg, *unres, *uhead, *uoff, *hoff, *segs;
    unsigned long long *keyA, *keyB;
    uint8_t* stop;
    T *state, *part;
    int64_t* nsel;
    void* temp;
    size_t tsort = 0, tsort32 = 0, tscan = 0, tsel = 0;
    {
        unsigned long long* k0 = nullptr;
        uint32_t* v0 = nullptr;
        int64_t* c0 = nullptr;
        (void)pmx_sort_pairs(nullptr, tsort, k0, k0, v0, v0, (int)n, 0, 64, st);
        (void)pmx_sort_pairs(nullptr, tsort32, v0, v0, v0, v0, (int)n, 0, 32, st);
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tscan, v0, v0, (int)n + 1, st);
        (void)hipcub::DeviceSelect::Flagged(nullptr, tsel, v0, v0, v0, c0, (int)n, st);
    }
    const size_t tb = std::max(std::max(tsort, tsort32), std::max(tscan, tsel));
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t w = sizeof(uint32_t) * (size_t)(n + 1);
    const size_t o_order = take(w), o_head = take(w), o_idxA = take(w), o_idxB = take(w), o_posA = take(w),
                 o_posB = take(w), o_seg = take(w), o_unres = take(w), o_uhead = take(w), o_uoff = take(w),
                 o_hoff = take(w), o_segs = take(w), o_keyA = take(2 * w), o_keyB = take(2 * w),
                 o_stop = take((size_t)n), o_state = take(sizeof(T) * (size_t)n * (D + 1)),
                 o_part = take(sizeof(T) * 6 * nb), o_nsel = take(sizeof(int64_t)), o_temp = take(tb);
    char* buf = nullptr;
    if (hipMalloc(&buf, total) != hipSuccess) {
        err = "OctreeGridDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    std::unique_ptr<void, void (*)(void*)> free_buf(buf, [](void* p) { (void)hipFree(p); });
    order = (uint32_t*)(buf + o_order);
    head = (uint32_t*)(buf + o_head);
    idxA = (uint32_t*)(buf + o_idxA);
    idxB = (uint32_t*)(buf + o_idxB);
    posA = (uint32_t*)(buf + o_posA);
    posB = (uint32_t*)(buf + o_posB);
    seg = (uint32_t*)(buf + o_seg);
    unres = (uint32_t*)(buf + o_unres);
    uhead = (uint32_t*)(buf + o_uhead);
    uoff = (uint32_t*)(buf + o_uoff);
    hoff = (uint32_t*)(buf + o_hoff);
    segs = (uint32_t*)(buf + o_segs);
    keyA = (unsigned long long*)(buf + o_keyA);
    keyB = (unsigned long long*)(buf + o_keyB);
    stop = (uint8_t*)(buf + o_stop);
    state = (T*)(buf + o_state);
    part = (T*)(buf + o_part);
    nsel = (int64_t*)(buf + o_nsel);
    temp = buf + o_temp;

    hipLaunchKernelGGL(oct_minmax_kernel<T>, dim3(nb), dim3(256), 0, st, d_f, rows, n, part);
    std::vector<T> hp((size_t)6 * nb);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(hp.data(), part, sizeof(T) * 6 * nb, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    OctNode<T> root;
    root.r = (T)0;
    for (int a = 0; a < 3; ++a) {
        root.c[a] = (T)0;
        if (a >= D) continue;
        T mn = (T)INFINITY, mx = -(T)INFINITY;
        for (unsigned b = 0; b < nb; ++b) {
            mn = std::min(mn, hp[b * 6 + a]);
            mx = std::max(mx, hp[b * 6 + 3 + a]);
        }
        const T radii = mx - mn;
        root.c[a] = mn + radii * (T)0.5;
        if (a == 0 || root.r < radii) root.r = radii;
    }
    root.r = root.r * (T)0.5;
    bool finite = std::isfinite(root.r);
    for (int a = 0; a < D; ++a) finite = finite && std::isfinite(root.c[a]);
    if (!finite) {
        err = "OctreeGridDataPointsFilter: the bounding box is not finite (non-finite coordinates are not supported)";
        return PMX_E_BAD_PARAM;
    }
    // the depth of the size limit (octree.hpp:312; the radius halves exactly as the descent's does)
    int64_t size_depth = 0;
    for (T r = root.r; !((double)r * 2.0 <= max_size); r = r * (T)0.5) ++size_depth;

    // ---- rounds of K levels ----
    int64_t m = n, nseg = 1, depth = 0;
    bool first = true;
    for (int round = 0; m > 0; ++round) {
        if (round > 4096) {  // (cannot happen: the radius of a finite box reaches 0 within ~2200 levels)
            err = "OctreeGridDataPointsFilter: the descent did not end";
            return PMX_E_STATE;
        }
        int segbits = 0;
        while (((int64_t)1 << segbits) < nseg) ++segbits;
        const int K = std::min((64 - segbits) / D, D == 3 ? 21 : 31);
        const int limit = (int)std::min<int64_t>(size_depth - depth, (int64_t)K + 1);
        const uint32_t* aidx = first ? nullptr : idxA;
        const uint32_t* aseg = first ? nullptr : seg;
        const uint32_t* apos = first ? nullptr : posA;
        if (first) hipLaunchKernelGGL(iota_kernel<uint32_t>, dim3(oct_blocks(m)), dim3(256), 0, st, idxA, m);
        if (D == 3)
            launch_oct_key<T, 3>(d_f, rows, aidx, aseg, m, root, K, limit, state, keyA, stop, st);
        else
            launch_oct_key<T, 2>(d_f, rows, aidx, aseg, m, root, K, limit, state, keyA, stop, st);
        size_t t = tb;
        if (pmx_sort_pairs(temp, t, keyA, keyB, idxA, idxB, (int)m, 0, segbits + K * D, st) != hipSuccess)
            return PMX_E_HIP;
        if (D == 3)
            hipLaunchKernelGGL(oct_leaf_kernel<3>, dim3(oct_blocks(m)), dim3(256), 0, st, keyB, idxB, apos, stop, m, K,
                               max_pts, order, head, unres, uhead);
        else
            hipLaunchKernelGGL(oct_leaf_kernel<2>, dim3(oct_blocks(m)), dim3(256), 0, st, keyB, idxB, apos, stop, m, K,
                               max_pts, order, head, unres, uhead);
        t = tb;
        if (hipcub::DeviceScan::ExclusiveSum(temp, t, unres, uoff, (int)m + 1, st) != hipSuccess) return PMX_E_HIP;
        t = tb;
        if (hipcub::DeviceScan::ExclusiveSum(temp, t, uhead, hoff, (int)m + 1, st) != hipSuccess) return PMX_E_HIP;
        uint32_t left = 0, runs = 0;
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(&left, uoff + m, sizeof(left), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&runs, hoff + m, sizeof(runs), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PMX_E_HIP;
        if (left > 0) {
            hipLaunchKernelGGL(oct_compact_kernel, dim3(oct_blocks(m)), dim3(256), 0, st, idxB, apos, unres, uhead,
                               uoff, hoff, m, idxA, posB, seg);
            std::swap(posA, posB);
        }
        m = (int64_t)left;
        nseg = (int64_t)runs;
        depth += K;
        first = false;
    }

    // ---- the leaves: the positions whose head flag is set ----
    hipLaunchKernelGGL(iota_kernel<uint32_t>, dim3(oct_blocks(n)), dim3(256), 0, st, posA, n);
    size_t t = tb;
    if (hipcub::DeviceSelect::Flagged(temp, t, posA, head, segs, nsel, (int)n, st) != hipSuccess) return PMX_E_HIP;
    int64_t L = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&L, nsel, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PMX_E_HIP;
    if (L <= 0 || L > n) {
        err = "OctreeGridDataPointsFilter: inconsistent leaf count";
        return PMX_E_STATE;
    }
    // every leaf's members by rising index: (leaf of point i, i) sorted by leaf, stably.  The leaves keep
    // their places and sizes, so segs stays as it is.
    {
        int lbits = 1;
        while (((int64_t)1 << lbits) < L) ++lbits;
        t = tb;
        if (hipcub::DeviceScan::ExclusiveSum(temp, t, head, hoff, (int)n, st) != hipSuccess) return PMX_E_HIP;
        hipLaunchKernelGGL(oct_leaf_of_point_kernel, dim3(oct_blocks(n)), dim3(256), 0, st, order, head, hoff, n,
                           uhead);
        t = tb;  // (posA: the iota above; unres: the sorted leaf numbers, unused)
        if (pmx_sort_pairs(temp, t, uhead, unres, posA, order, (int)n, 0, lbits, st) != hipSuccess) return PMX_E_HIP;
    }

    // ---- samplers ----
    if (method >= 2) {
        hipLaunchKernelGGL(oct_record_kernel<T>, dim3(oct_blocks(L)), dim3(256), 0, st, d_f, d_desc, rows, desc_dim,
                           order, segs, L, n, method == 3 ? 1 : 0, d_of, d_od);
    } else {
        float* d_fac = nullptr;
        if (method == 1) {
            std::vector<float> fac((size_t)L);
            octree_rand_factors(L, fac.data());
            d_fac = (float*)unres;
            if (hipMemcpyAsync(d_fac, fac.data(), sizeof(float) * (size_t)L, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)  // (fac is a local)
                return PMX_E_HIP;
        }
        int32_t* d_pick = (int32_t*)idxA;
        hipLaunchKernelGGL(oct_pick_kernel, dim3(oct_blocks(L)), dim3(256), 0, st, order, segs, L, n, d_fac, d_pick);
        std::vector<int32_t> pick((size_t)L);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(pick.data(), d_pick, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, st) !=
                hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PMX_E_HIP;
        const std::vector<int32_t> col = octree_replay_columns(pick.data(), L, n);
        int32_t* d_col = (int32_t*)idxB;
        if (hipMemcpyAsync(d_col, col.data(), sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, st) != hipSuccess)
            return PMX_E_HIP;
        hipLaunchKernelGGL(gather_columns_kernel<T>, dim3(oct_blocks(L)), dim3(256), 0, st, d_f, d_desc, rows, desc_dim,
                           d_col, L, d_of, d_od);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PMX_E_HIP;
    *n_out = L;
    return PMX_OK;
}

template int octree_run<float>(const float*, int, int64_t, const float*, int, int64_t, double, int, float*, float*,
                               int64_t*, hipStream_t, std::string&);
template int octree_run<double>(const double*, int, int64_t, const double*, int, int64_t, double, int, double*,
                                double*, int64_t*, hipStream_t, std::string&);

}  // namespace pmx

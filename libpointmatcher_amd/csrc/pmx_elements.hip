// pmx_elements.hip — the kept pairs of the last match as columns
// (pmx_elements.h has the contract and the order scheme).
//
// Asked for at most once per ICP, after the loop stopped, never inside an
// iteration (no LoopCtl).  Three launches of their own and pmx_keep.hip's scan:
//   elements_inverse_kernel  inv[order[s]] = s (a permutation: every word is
//                            written once)
//   elements_flag_kernel     one entry of the index order per thread: the
//                            wave's ballot and the block's count, as the keep
//                            filters leave them; the two rejected counts by one
//                            integer atomic per wave (exact in any order)
//   launch_keep_scan         the block counts' exclusive scan
//   elements_scatter_kernel  column = block offset + the popcounts of the
//                            ballots below the lane; each kept thread writes
//                            its column's values
// Every output is a copy of a stored value or xform3's transform of the
// reading point, with no contraction (-ffp-contract=off and the pragma).
#pragma clang fp contract(off)

#include "pmx_elements.h"
#include "pmx_p2plane.h"

namespace pmx {

__global__ __launch_bounds__(256) void elements_inverse_kernel(const int32_t* __restrict__ order, int64_t N,
                                                               int32_t* __restrict__ inv,
                                                               unsigned long long* __restrict__ counters) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    // order is a permutation of [0, N) (reading_order_device); an entry outside
    // it is never written through and is reported (kElBadOrder)
    const int32_t i = order[s];
    if (i >= 0 && (int64_t)i < N)
        inv[i] = (int32_t)s;
    else
        atomicAdd(&counters[kElBadOrder], 1ull);
}

// entry e' of the index order -> its reading index, rank and slot entry
template <typename T>
__device__ __forceinline__ int64_t elements_entry(const ElementsIn<T>& in, int64_t ei, int32_t& i, int32_t& s,
                                                  int64_t& slot) {
    i = (int32_t)(ei / in.m.k);
    s = (int32_t)(ei - (int64_t)i * in.m.k);
    slot = (int64_t)i;
    if (in.inv) {  // (kept inside the arrays whatever the word holds: a bad order map is an error, not a fault)
        const int64_t v = (int64_t)in.inv[i];
        slot = v < 0 ? 0 : (v >= in.m.N ? in.m.N - 1 : v);
    }
    return slot * in.m.k + s;
}

template <typename T>
__global__ __launch_bounds__(kKeepBlock) void elements_flag_kernel(ElementsIn<T> in,
                                                                   unsigned long long* __restrict__ masks,
                                                                   uint32_t* __restrict__ block_cnt,
                                                                   unsigned long long* __restrict__ counters) {
    const int64_t n = in.m.N * in.m.k;
    const int64_t ei = (int64_t)blockIdx.x * kKeepBlock + threadIdx.x;
    bool kept = false, rej_match = false, rej_point = false;
    if (ei < n) {
        int32_t i, s;
        int64_t slot;
        const int64_t e = elements_entry(in, ei, i, s, slot);
        const bool finite = in.m.d[e] != (T)__builtin_huge_val();
        kept = finite && in.w[e] != (T)0;
        rej_match = finite && !kept;
        if (s == 0) {  // (the point's first entry answers for the point)
            bool any = kept;
            for (int r = 1; r < in.m.k && !any; ++r) {
                const int64_t er = slot * in.m.k + r;
                any = in.m.d[er] != (T)__builtin_huge_val() && in.w[er] != (T)0;
            }
            rej_point = !any;
        }
    }
    const unsigned long long bm = __ballot(rej_match), bp = __ballot(rej_point);
    if ((threadIdx.x & 63) == 0) {
        if (bm) atomicAdd(&counters[kElRejMatches], (unsigned long long)__popcll(bm));
        if (bp) atomicAdd(&counters[kElRejPoints], (unsigned long long)__popcll(bp));
    }
    keep_block_ballot(kept, masks, block_cnt);
}

template <typename T>
__global__ __launch_bounds__(kKeepBlock) void elements_scatter_kernel(ElementsIn<T> in, Mat4<T> Tm, int rows,
                                                                      const unsigned long long* __restrict__ masks,
                                                                      const uint32_t* __restrict__ off,
                                                                      ElementsOut<T> out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* bm = masks + (int64_t)blockIdx.x * kKeepWaves;
    const unsigned long long m = bm[wave];
    if (!((m >> lane) & 1ull)) return;  // (a set bit is an entry below N * k: elements_flag_kernel)
    uint32_t wpre = 0;
    for (int w = 0; w < wave; ++w) wpre += (uint32_t)__popcll(bm[w]);
    const int64_t j = (int64_t)off[blockIdx.x] + wpre + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    const int64_t ei = (int64_t)blockIdx.x * kKeepBlock + threadIdx.x;
    int32_t i, s;
    int64_t slot;
    const int64_t e = elements_entry(in, ei, i, s, slot);
    const int32_t id = in.m.ids[e];
    const bool id_ok = id >= 0 && (int64_t)id < in.ref_count;
    if (out.reading) {
        const P4<T> p = in.m.rd[slot];
        T x, y, z;
        xform3(Tm, p, x, y, z);
        T* o = out.reading + j * rows;
        o[0] = x;
        o[1] = y;
        if (rows == 4) o[2] = z;
        o[rows - 1] = p.w;
    }
    if (out.reference) {
        P4<T> q{(T)0, (T)0, (T)0, (T)0};
        if (id_ok) q = gld(in.m.ref, (int64_t)id);
        T* o = out.reference + j * rows;
        o[0] = q.x;
        o[1] = q.y;
        if (rows == 4) o[2] = q.z;
        o[rows - 1] = q.w;
    }
    if (out.ref_normals) {
        P4<T> q{(T)0, (T)0, (T)0, (T)0};
        if (id_ok) q = gld(in.m.nrm, (int64_t)id * in.m.rs);
        const int D = rows - 1;
        T* o = out.ref_normals + j * D;
        o[0] = q.x;
        o[1] = q.y;
        if (D == 3) o[2] = q.z;
    }
    if (out.dists) out.dists[j] = in.m.d[e];
    if (out.ids) out.ids[j] = (in.m.gidx && id_ok) ? gld(in.m.gidx, (int64_t)id) : id;
    if (out.weights) out.weights[j] = in.w[e];
    if (out.reading_index) out.reading_index[j] = i;
    if (out.link_rank) out.link_rank[j] = s;
}

void launch_elements_inverse(const int32_t* order, int64_t N, int32_t* inv, unsigned long long* counters,
                             hipStream_t s) {
    if (N <= 0) return;
    hipLaunchKernelGGL(elements_inverse_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, order, N, inv,
                       counters);
}

template <typename T>
void launch_elements_flag(const ElementsIn<T>& in, const KeepScratch& sc, unsigned long long* counters,
                          hipStream_t s) {
    hipLaunchKernelGGL(elements_flag_kernel<T>, dim3((unsigned)sc.nb), dim3(kKeepBlock), 0, s, in, sc.masks, sc.cnt,
                       counters);
}

template <typename T>
void launch_elements_scatter(const ElementsIn<T>& in, const Mat4<T>& Tm, int rows, const KeepScratch& sc,
                             const ElementsOut<T>& out, hipStream_t s) {
    hipLaunchKernelGGL(elements_scatter_kernel<T>, dim3((unsigned)sc.nb), dim3(kKeepBlock), 0, s, in, Tm, rows,
                       sc.masks, sc.off, out);
}

#define PMX_INST(T)                                                                                             \
    template void launch_elements_flag<T>(const ElementsIn<T>&, const KeepScratch&, unsigned long long*,       \
                                          hipStream_t);                                                        \
    template void launch_elements_scatter<T>(const ElementsIn<T>&, const Mat4<T>&, int, const KeepScratch&,    \
                                             const ElementsOut<T>&, hipStream_t);
PMX_INST(float)
PMX_INST(double)
#undef PMX_INST

}  // namespace pmx

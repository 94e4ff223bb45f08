// pmx_nss.h — the host side of NormalSpaceDataPointsFilter
// (DataPointsFilters/NormalSpace.cpp:47-181): plain C++, no device code, so a
// stand-alone program can include it.  The device groups the points by bucket
// (pmx_nss.hip); what is sequential or tied to the host library stays here:
//   nss_bucket_counts  the bucket grid of an epsilon (:53, :180)
//   nss_bucket_of      the literal bucket of one normal, in T with the host
//                      library's acos / atan2 / fmod (:114-116, :169-181)
//   nss_shuffle        std::random_shuffle of 0..n-1 as libstdc++ runs it, on
//                      the process's rand() state (:100-102)
//   nss_picks          the pick loop over the grouped points (:129-145)
// The column order of the output is the swapCols / mapidx sequence of
// OctreeGrid (:149-165): octree_replay_columns of pmx_octree_replay.h.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <random>
#include <vector>

namespace pmx {

// cols = ceil(2 pi / eps), rows = ceil(pi / eps) in double, eps the T value
// widened; nbBucket = size_t(cols * rows) (NormalSpace.cpp:53).  For a float
// eps the quotients are not the integers they look like (T(pi / k) is a step
// above or below pi / k), so the counts must come from this expression.
template <typename T>
inline void nss_bucket_counts(T eps, double& cols, double& rows, std::size_t& nb_bucket) {
    cols = std::ceil(2.0 * M_PI / eps);
    rows = std::ceil(M_PI / eps);
    nb_bucket = (std::size_t)(cols * rows);
}

// A normal the reference leaves undefined (its asserts, NormalSpace.cpp:111): a
// NaN component, or |nz| > 1 (acos gives NaN).
template <typename T>
inline bool nss_normal_defined(T nx, T ny, T nz) {
    return !(nx != nx) && !(ny != ny) && nz >= (T)-1 && nz <= (T)1;
}

// The bucket of one normal (NormalSpace.cpp:114-116, 169-181).  theta and the
// atan2 are T calls, the add and the fmod double; the two divisions and floors
// are in T, the product and the sum in double.  theta == T(pi) and phi ==
// 2 * T(pi) wrap to 0, so nz = -1 lands in row 0.  The result may be >=
// nbBucket (the T division can round theta / eps up to rows).
template <typename T>
inline std::size_t nss_bucket_of(T nx, T ny, T nz, T eps) {
    T theta = std::acos(nz);
    T phi = (T)std::fmod((double)std::atan2(ny, nx) + 2. * M_PI, 2. * M_PI);
    if (theta == (T)M_PI) theta = (T)0;
    if (phi == 2 * (T)M_PI) phi = (T)0;
    const T qt = theta / eps, qp = phi / eps;
    return (std::size_t)((double)std::floor(qt) * std::ceil(2.0 * M_PI / eps) + (double)std::floor(qp));
}

// std::random_shuffle(0..n-1) of libstdc++ (stl_algo.h): for i = 1 .. n-1,
// j = rand() % (i + 1), swap when i != j.  n - 1 draws from the process's
// rand() state on the calling thread.
inline void nss_shuffle(int64_t n, int32_t* perm) {
    for (int64_t i = 0; i < n; ++i) perm[i] = (int32_t)i;
    for (int64_t i = 1; i < n; ++i) {
        const int64_t j = (int64_t)std::rand() % (i + 1);
        if (i != j) {
            const int32_t t = perm[i];
            perm[i] = perm[j];
            perm[j] = t;
        }
    }
}

// The caller's rand() state set aside while the GPU runtime works.  On the
// first GPU use of a process the runtime was observed to leave the process's
// generator outside the sequence the caller had seeded, which would break the
// contract above.  glibc's
// rand() and random() share one generator, so initstate() moves the process to
// a scratch state and hands back the caller's; draw() runs f on the caller's
// state, and the destructor puts it back whatever happened in between.
class NssRandState {
public:
    NssRandState() : caller_(initstate(1u, scratch_, sizeof(scratch_))) {}
    ~NssRandState() {
        if (caller_) setstate(caller_);
    }
    NssRandState(const NssRandState&) = delete;
    NssRandState& operator=(const NssRandState&) = delete;
    template <typename F>
    void draw(F f) {
        if (caller_) setstate(caller_);
        f();
        if (caller_) setstate(scratch_);
    }

private:
    char scratch_[128];
    char* caller_;
};

// The picks (NormalSpace.cpp:129-145).  ids: the n points grouped by bucket,
// buckets in index order, each bucket's members in shuffled order; begin[b]:
// where non-empty bucket b starts (nb of them, the last ends at n).  Each of
// the nb_sample (< n) picks draws a bucket from mt19937(seed) with
// uniform_int_distribution<size_t>(0, buckets left - 1), takes and pops its
// last member, and erases the bucket from the list once empty.
inline std::vector<int32_t> nss_picks(const int32_t* ids, const uint32_t* begin, int64_t nb, int64_t n,
                                      int64_t nb_sample, uint64_t seed) {
    struct Range {
        uint32_t b, e;
    };
    std::vector<Range> left((std::size_t)nb);
    for (int64_t b = 0; b < nb; ++b) left[(std::size_t)b] = Range{begin[b], b + 1 < nb ? begin[b + 1] : (uint32_t)n};
    std::mt19937 gen((std::size_t)seed);
    std::vector<int32_t> picks;
    picks.reserve((std::size_t)nb_sample);
    for (int64_t i = 0; i < nb_sample; ++i) {
        std::uniform_int_distribution<std::size_t> uni(0, left.size() - 1);
        const std::size_t cur = uni(gen);
        Range& r = left[cur];
        picks.push_back(ids[--r.e]);
        if (r.e == r.b) left.erase(left.begin() + (std::ptrdiff_t)cur);
    }
    return picks;
}

}  // namespace pmx

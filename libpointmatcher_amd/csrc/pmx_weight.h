// pmx_weight.h — the outlier chain and the weight of one match entry.
//
// Included by pmx_internal.h (behind the types it uses: P4, Mat4, LoopCtl,
// GridDesc, SelectState); include that.
//
// Every supported OutlierFilter but one produces 0/1 weights and a chain
// multiplies them (OutlierFilter.cpp:63-103), so the chain is a conjunction of
// predicates on the distance.  It is evaluated inline by the reductions (no
// weight array is written or read on the hot path) and materialised only for
// the host mirror (pmx_get_weights) and the quality reductions.
// The RobustOutlierFilter (OutlierFiltersImpl.cpp:394-598) is the one
// filter with real-valued weights: w = robust(e^2), e^2 = dist / scale^2,
// multiplied with the predicates' 0/1 (kWPRobust, at most one per chain; the
// reductions take the weighted path only then).
// The SurfaceNormalOutlierFilter (OutlierFiltersImpl.cpp:225-285) is the one
// predicate that reads no distance (kWPNormal): it compares the reading's and
// the matched reference point's normals (SNPred, sn_pass).  The reductions
// evaluate it in instantiations of their own, selected at launch when the
// chain holds it.
// The GenericDescriptorOutlierFilter (OutlierFiltersImpl.cpp:290-374) reads no
// distance either (kWPGeneric): its weight comes from a one-row descriptor of
// the matched reference point (GDPred, gd_weight).  Its hard form is a 0/1
// predicate (the exact path, in instantiations of their own as SurfaceNormal's),
// its soft form the second filter with real-valued weights (the weighted path).
// entry_weight (below) is the one statement of the product.
#pragma once

namespace pmx {

enum WPred { kWPDefault = 0, kWPNull = 1, kWPLe = 2, kWPGe = 3, kWPState = 4, kWPRobust = 5, kWPNormal = 6,
             kWPGeneric = 7 };
// rn != null: the filter is in the chain and both clouds carry normals.
template <typename T>
struct SNPred {
    const P4<T>* rn = nullptr;   // [N]: the reading's normals, rotated by T_refMean_dataIn, slot order
    const P4<T>* nrm = nullptr;  // the reference normal records the match ids index (device loop: from GridDesc)
    int rs = 1;                 // their index stride (2: a grid level's interleaved records)
    int dim = 3;
    T eps = 0;                  // cos(maxAngle) in T (several filters: the largest)
};
// GenericDescriptorOutlierFilter.  desc != null: the filter is in the chain.
// desc holds one value per reference point in the order of the match ids (a
// grid level's permuted copy after a grid match, GridDesc::gw; the uploaded
// array after a brute-force match), so a pair costs one gather.
enum GDMode { kGDSoft = 0, kGDLess = 1, kGDGreater = 2 };
template <typename T>
struct GDPred {
    const T* desc = nullptr;
    int mode = kGDSoft;
    T thr = 0;                  // hard modes: the threshold in T
    const double* m = nullptr;  // soft: the maximum over all k x N entries (device, a T value; gd_max_kernel)
};
enum RobustFct { kRFCauchy = 0, kRFWelsch = 1, kRFSC = 2, kRFGM = 3, kRFTukey = 4, kRFHuber = 5, kRFL1 = 6,
                 kRFStudent = 7 };
constexpr int kMaxChain = 8;
template <typename T>
struct WChain {
    int n = 0;
    int type[kMaxChain] = {};
    T thr[kMaxChain] = {};                        // kWPLe / kWPGe: threshold; kWPState: scale
    const SelectState* st[kMaxChain] = {};        // kWPState: resolved quantile (limit)
    // kWPRobust (robust != 0): function, tuning k, squared approximation,
    // the scale (device, T value), point-to-plane distance
    int robust = 0;
    int rb_fct = 0;
    T rb_k = 1;
    T rb_sqa = 0;
    const double* rb_scale = nullptr;
    int rb_p2pl = 0;
    const T* w_arr = nullptr;  // materialised weights (a robust point-to-plane distance, point-to-point minimiser)
    SNPred<T> sn;              // kWPNormal
    GDPred<T> gd;              // kWPGeneric
    // real-valued weights: the reductions take the weighted path
    __host__ __device__ bool real() const { return robust != 0 || (gd.desc != nullptr && gd.mode == kGDSoft); }
};
// robustFiltering's weight of one scaled squared error (OutlierFiltersImpl.cpp:541-596)
template <typename T>
__device__ __forceinline__ T robust_weight(int fct, T k, T sqa, T e2) {
    const T k2 = k * k;
    T w;
    switch (fct) {
    case kRFCauchy: w = (T)1 / ((T)1 + e2 / k2); break;
    case kRFWelsch: w = exp(-e2 / k2); break;
    case kRFSC: {
        const T s = k + e2;
        w = e2 >= k ? (T)(4.0 * (double)k2) * ((T)1 / (s * s)) : (T)1;
        break;
    }
    case kRFGM: {
        const T s = k + e2;
        w = k2 * ((T)1 / (s * s));
        break;
    }
    case kRFTukey: {
        const T a = (T)1 - e2 / k2;
        w = e2 >= k2 ? (T)0 : a * a;
        break;
    }
    case kRFHuber: w = e2 >= k2 ? k * ((T)1 / sqrt(e2)) : (T)1; break;
    case kRFL1: w = (T)1 / sqrt(e2); break;
    default: {  // Student, d = 3
        const T d = 3;
        const T p = pow((T)1 + e2 / k, -(k + d) / (T)2);
        w = p * (k + d) * ((T)1 / (k + e2));
        break;
    }
    }
    // ARBITRARY_SMALL_VALUE (1e-50 as T: 0 in float), then the approximation
    const T tiny = (T)1e-50;
    w = w <= tiny ? tiny : w;
    if (sqa != (T)__builtin_huge_val() && e2 >= sqa) w = 0;
    return w;
}
// per-thread resolved thresholds (kWPState: scale * limit in T, as the
// reference's `factor * quantile`, OutlierFiltersImpl.cpp:121-122)
// A conjunction of `d <= t` / `d >= t` / `d != inf` predicates is one
// interval test: keep = (d != inf if required) && lo <= d && d <= hi with
// hi = min of the upper thresholds, lo = max of the lower ones.  A NaN
// threshold (failed quantile) rejects everything, as `d <= NaN` does; the
// min/max below propagate it.
template <typename T>
struct WRange {
    T lo, hi;
    bool finite;
};
template <typename T>
__device__ __forceinline__ WRange<T> chain_resolve(const WChain<T>& c) {
    WRange<T> r{-(T)__builtin_huge_val(), (T)__builtin_huge_val(), false};
    for (int i = 0; i < c.n; ++i) {  // uniform, once per thread
        const int t = c.type[i];
        if (t == kWPDefault) {
            r.finite = true;
        } else if (t == kWPGe) {
            const T v = c.thr[i];
            r.lo = (v != v || r.lo != r.lo) ? v + r.lo : (v > r.lo ? v : r.lo);
        } else if (t == kWPLe || t == kWPState) {
            const T v = t == kWPState ? c.thr[i] * (T)c.st[i]->limit : c.thr[i];
            r.hi = (v != v || r.hi != r.hi) ? v + r.hi : (v < r.hi ? v : r.hi);
        }
    }
    return r;
}
template <typename T>
__device__ __forceinline__ bool chain_keep(const WRange<T>& r, T d) {
    return (!r.finite || d != (T)__builtin_huge_val()) && d >= r.lo && d <= r.hi;
}

// the squared point-to-plane distance of a RobustOutlierFilter with
// distanceType point2plane (computePointToPlaneDistance,
// OutlierFiltersImpl.cpp:460-489), with the normalised reference normal
template <typename T>
__device__ __forceinline__ T p2pl_distance(T px, T py, T pz, const P4<T>& q, const P4<T>& n) {
    // Eigen normalized(): v / sqrt(squaredNorm), v itself when the norm is 0
    const T sq = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const T nn = sq > (T)0 ? sqrt(sq) : (T)1;
    const T dot = ((n.x / nn) * (px - q.x) + (n.y / nn) * (py - q.y)) + (n.z / nn) * (pz - q.z);
    return dot * dot;  // (pow(dot, 2) rounds to the same T)
}

// ---- the SurfaceNormalOutlierFilter's per-pair predicate ----
// The filter sees the step reading (ICP.cpp:381-390), whose normals are
// R_iter (R_0 n): R_0 n is resident (SNPred::rn, rounded to T at upload) and
// R_iter is applied here from the iteration's step transform, so no second
// copy of the normals exists.  Every product and sum is rounded to T
// separately and summed left to right, as the reference's dense products:
//   r_c   = (m_c0 n_0 + m_c1 n_1) + m_c2 n_2        (2-D: no third term)
//   |v|   = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2),  v^ = v / |v|
//   w     = |(a^_0 b^_0 + a^_1 b^_1) + a^_2 b^_2| < eps ? 0 : 1
// A zero normal normalises to NaN and `NaN < eps` is false: the pair is kept.

// device loop: the reference normal records of this iteration's grid level
template <typename T>
__device__ __forceinline__ void sn_bind(SNPred<T>& p, const LoopCtl* ctl, const GridDesc<T>* gd) {
    if (ctl) {
        p.nrm = gd[ctl->level].gpn + 1;
        p.rs = 2;
    }
}

// rn: the reading point's resident normal; qn: the matched reference point's
// normal record; Tm: the step transform (embedded 4x4)
template <typename T>
__device__ __forceinline__ bool sn_pass(const SNPred<T>& p, const Mat4<T>& Tm, const P4<T>& rn, const P4<T>& qn) {
    T dot;
    if (p.dim == 3) {
        const T ax = (Tm.m[0] * rn.x + Tm.m[1] * rn.y) + Tm.m[2] * rn.z;
        const T ay = (Tm.m[4] * rn.x + Tm.m[5] * rn.y) + Tm.m[6] * rn.z;
        const T az = (Tm.m[8] * rn.x + Tm.m[9] * rn.y) + Tm.m[10] * rn.z;
        const T na = sqrt((ax * ax + ay * ay) + az * az);
        const T nb = sqrt((qn.x * qn.x + qn.y * qn.y) + qn.z * qn.z);
        dot = ((ax / na) * (qn.x / nb) + (ay / na) * (qn.y / nb)) + (az / na) * (qn.z / nb);
    } else {
        const T ax = Tm.m[0] * rn.x + Tm.m[1] * rn.y;
        const T ay = Tm.m[4] * rn.x + Tm.m[5] * rn.y;
        const T na = sqrt(ax * ax + ay * ay);
        const T nb = sqrt(qn.x * qn.x + qn.y * qn.y);
        dot = (ax / na) * (qn.x / nb) + (ay / na) * (qn.y / nb);
    }
    const T a = dot < (T)0 ? -dot : dot;
    return !(a < p.eps);
}

// ---- the GenericDescriptorOutlierFilter's per-pair factor ----
// device loop: the descriptor copy of this iteration's grid level
template <typename T>
__device__ __forceinline__ void gd_bind(GDPred<T>& p, const LoopCtl* ctl, const GridDesc<T>* gd) {
    if (ctl) p.desc = gd[ctl->level].gw;
}
// one scalar gather through an explicitly global pointer (see gld)
template <typename T>
__device__ __forceinline__ T gd_load(const T* p, int64_t i) {
    return ((const __attribute__((address_space(1))) T*)p)[i];
}
// the hard forms (OutlierFiltersImpl.cpp:343-354): both comparisons strict, in T
template <typename T>
__device__ __forceinline__ bool gd_pass(const GDPred<T>& p, int32_t id) {
    const T v = gd_load(p.desc, id);
    return p.mode == kGDGreater ? v > p.thr : v < p.thr;
}
// The filter's weight of a pair: no neighbour gives 0; hard 0/1; soft
// desc[id], then every entry divided (a true division in T) by the maximum m
// over all entries, the zeros of the entries without a neighbour included
// (OutlierFiltersImpl.cpp:334-371).  m <= 0 is not guarded: IEEE decides.
template <typename T>
__device__ __forceinline__ T gd_weight(const GDPred<T>& p, int32_t id) {
    if (p.mode == kGDSoft) return (id >= 0 ? gd_load(p.desc, id) : (T)0) / (T)*p.m;
    return id >= 0 && gd_pass(p, id) ? (T)1 : (T)0;
}

// A chain of 0/1 factors only keeps the pair (entry_weight != 0 there): the
// distance predicates, then each id-reading predicate of a valid id.  The
// point-to-plane body evaluates it in this form around its own order of loads.
template <typename T, bool SN, bool GD>
__device__ __forceinline__ bool pair_keep(const WChain<T>& c, const GDPred<T>& gd, const WRange<T>& wr,
                                          const Mat4<T>& Tm, T dv, int32_t id, const P4<T>& rn, const P4<T>& n) {
    bool keep = chain_keep(wr, dv);
    if (SN) keep = keep && id >= 0 && sn_pass(c.sn, Tm, rn, n);
    if (GD) keep = keep && id >= 0 && gd_pass(gd, id);
    return keep;
}

// ---- the weight of one match entry ----
// a value the caller has loaded, in the callable form entry_weight takes
template <typename V>
__device__ __forceinline__ auto loaded(const V& v) {
    return [&v]() -> const V& { return v; };
}

// The chain's weight of the entry (distance dv, reference id) of the reading
// point whose step point is p, in the reference's order of the product
// (OutlierFilter.cpp:63-103):
//   w    = pred(dv) * robust(dist / s^2) * sn * gd
//   pred = the distance predicates' 0/1 (wr: chain_resolve of the chain)
//   dist = rb_p2pl ? (id >= 0 ? p2pl_distance(p, q, n) : 0) : dv
//          (the predicates judge the match distance, the robust function the
//          chosen one; 0 for an invalid match, OutlierFiltersImpl.cpp:460-489);
//          s the chain's scale in T
//   sn   = id >= 0 && sn_pass(rn, n)
//   gd   = gd_weight(id): 0/1 (hard), or (id >= 0 ? desc[id] : 0) / m (soft)
// The robust factor is absent for a chain without the filter, the SurfaceNormal
// factor when SN is false (sn: the caller's SNPred, chain.sn or a bound copy),
// the GenericDescriptor factor when GD is false (gd: likewise, chain.gd or bound).
// At most one RobustOutlierFilter and one GenericDescriptorOutlierFilter per
// chain: with at most two real-valued factors (robust, soft gd) and 0/1
// factors otherwise, the product in T is the same in every order (a product of
// two T values commutes, and a 0/1 factor is exact wherever it stands), so the
// fixed order here gives the reference's bits for any chain order.  A third
// real-valued factor would make the rounding depend on the order.
// P2PL false: the caller's chains never ask for the point-to-plane distance
// (p, q and the normal are then not read for it).
// q: the matched reference point as loaded (anything for id < 0).  n, rn: the
// matched reference normal and the reading's resident normal as callables
// (loaded() for a value at hand), invoked only where the product needs them:
// the normal for the point-to-plane distance of a valid id, both for the
// SurfaceNormal factor of a valid id whose weight is non-zero so far.
// Skipping that factor at w == 0 changes no bit: +0 * (0|1) == +0.
// The hard GenericDescriptor factor is skipped likewise, by the same argument
// (w is +0 or non-zero there, the factor 0 or 1).  The soft factor is always
// formed: 0 * (desc / m) is -0 for a negative quotient and NaN for an
// infinite one, which a skip would lose.
// NaN: pred * robust is always formed, so a NaN scale or a NaN / infinite
// robust value gives a NaN weight even at pred == 0, and NaN != 0 counts as a
// non-zero weight everywhere, as Eigen's (w != 0) does.  A zero normal passes
// the SurfaceNormal factor (sn_pass).
template <typename T, bool SN, bool P2PL = true, bool GD = false, typename QN, typename RN>
__device__ __forceinline__ T entry_weight(const WChain<T>& c, const SNPred<T>& sn, const WRange<T>& wr,
                                          const Mat4<T>& Tm, T dv, int32_t id, T px, T py, T pz, const P4<T>& q,
                                          QN&& n, RN&& rn, const GDPred<T>& gd = GDPred<T>{}) {
    T w;
    if (c.robust) {
        T dist = dv;
        if (P2PL && c.rb_p2pl) dist = id >= 0 ? p2pl_distance(px, py, pz, q, n()) : (T)0;
        const T pred = chain_keep(wr, dv) ? (T)1 : (T)0;
        const T s = (T)*c.rb_scale;
        w = pred * robust_weight<T>(c.rb_fct, c.rb_k, c.rb_sqa, dist / (s * s));
    } else {
        w = chain_keep(wr, dv) ? (T)1 : (T)0;
    }
    if (SN && w != (T)0) w = w * (id >= 0 && sn_pass(sn, Tm, rn(), n()) ? (T)1 : (T)0);
    if (GD && (gd.mode == kGDSoft || w != (T)0)) w = w * gd_weight(gd, id);
    return w;
}

}  // namespace pmx

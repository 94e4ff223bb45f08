// pm_icp.cpp — modules, registry and the ICP loop of the GPU path.
//
// Module names, parameter names, defaults and bounds are those of the
// reference so that libpointmatcher YAML chain files load unchanged:
//   KDTreeMatcher, KDTreeVarDistMatcher  MatchersImpl.h:74-134
//   Null/MaxDist/MinDist/MedianDist/TrimmedDist/VarTrimmedDist/Robust OutlierFilter
//                                 OutlierFiltersImpl.h:51-260
//   PointToPlane / PointToPlaneWithCov / PointToPoint / PointToPointSimilarity ErrorMinimizer
//                                 ErrorMinimizers/PointToPlane.h:61-90, PointToPlaneWithCov.h:60-86,
//                                 PointToPoint.h, PointToPointSimilarity.h
//   Counter / Differential / Bound TransformationChecker
//                                 TransformationCheckersImpl.h:60-130
//   Identity / SurfaceNormal / MaxDist / MinDist / RandomSampling / FixStepSampling /
//   BoundingBox DataPointsFilter  DataPointsFilters/{SurfaceNormal,MaxDist,MinDist,RandomSampling,FixStepSampling,BoundingBox}.h
//   NullInspector, NullLogger (+ no-op stand-ins for
//   the VTK/Performance inspectors and FileLogger, accepted for config
//   compatibility)
#include "pm_icp.h"

#include <cstdlib>
#include <cstring>
#include <iostream>

namespace pm {

// ------------------------------------------------------------------ Device --
Device::~Device() {
    if (ctx) pmx_ctx_destroy(ctx);
}

void Device::ensure() {
    if (ctx) return;
    const int rc = pmx_ctx_create(device, dtype, &ctx);
    if (rc != PMX_OK) {
        ctx = nullptr;
        throw std::runtime_error("pmx_ctx_create failed (" + std::to_string(rc) + "): no usable HIP device " +
                                 std::to_string(device) + " (" + std::to_string(pmx_device_count()) + " visible)");
    }
    if (host_ar) {
        check(pmx_comm_init_host(ctx, nranks, rank, host_ar, host_ag, host_user));
    } else if (!uid.empty()) {  // (a communicator issues its collectives at any nranks, also 1)
        if (uid.size() != 128) throw std::runtime_error("multi-rank ICP needs a 128-byte RCCL unique id");
        check(pmx_comm_init(ctx, uid.data(), nranks, rank));
    }
}

void Device::check(int rc) const {
    if (rc == PMX_OK) return;
    const std::string msg = ctx ? pmx_last_error(ctx) : "no device context";
    switch (rc) {
    case PMX_E_NO_POINTS:
    case PMX_E_EMPTY_QUANTILE:
        throw ConvergenceError(msg);
    case PMX_E_CONVERGENCE:
        throw ConvergenceError(msg);
    case PMX_E_BAD_PARAM:
        throw InvalidParameter(msg);
    case PMX_E_TRANSFORMATION:
        throw TransformationError(msg);
    default:
        throw std::runtime_error("pmx error " + std::to_string(rc) + ": " + msg);
    }
}

template <typename T>
static int dtype_of() {
    return sizeof(T) == 8 ? PMX_F64 : PMX_F32;
}

// ----------------------------------------------------------------- Matches --
template <typename T>
void PointMatcher<T>::Matches::mirror() const {
    if (mirrored) return;
    dists.resize((size_t)n * knn);
    ids.resize((size_t)n * knn);
    dev->check(pmx_get_matches(dev->ctx, dists.data(), ids.data()));
    mirrored = true;
}

template <typename T>
T PointMatcher<T>::Matches::getDistsQuantile(T quantile) const {
    mirror();
    std::vector<T> v;
    v.reserve(dists.size());
    for (T d : dists)
        if (d != std::numeric_limits<T>::infinity()) v.push_back(d);
    if (v.empty()) throw ConvergenceError("no outlier to filter");
    if (quantile < (T)0 || quantile > (T)1) throw ConvergenceError("quantile must be between 0 and 1");
    if (quantile == (T)1) return *std::max_element(v.begin(), v.end());
    size_t idx = (size_t)((T)v.size() * quantile);
    if (idx >= v.size()) idx = v.size() - 1;
    std::nth_element(v.begin(), v.begin() + idx, v.end());
    return v[idx];
}

// ================================================================= modules ==
namespace {

template <typename T>
using PM = PointMatcher<T>;

// ---- KDTreeMatcher on the GPU (exact search; see pmx_match.hip) ----------
// Matcher::init of both kd-tree matchers: the reference (and its normals,
// for the point-to-plane minimiser) to HBM, the search structure built there
template <typename T>
void matcher_init(Device& dev, const DataPoints<T>& ref, int searchType, const T* centre, T* mean_out) {
    dev.ensure();
    std::vector<T> nrm;
    const T* np = nullptr;
    if (ref.descriptorLabels.size() == 1 && ref.descriptorLabels[0].text == "normals" &&
        ref.descriptorLabels[0].span == ref.rows - 1) {
        np = ref.desc();  // (the only descriptor: already the dense D x n block, no copy)
    } else if (ref.descriptorExists("normals")) {
        int span = 0;
        nrm = ref.descriptor("normals", &span);
        if (span < ref.rows - 1) throw InvalidElement("normals descriptor has fewer rows than the dimension");
        if (span != ref.rows - 1) {
            std::vector<T> t((size_t)(ref.rows - 1) * ref.n);
            for (int64_t i = 0; i < ref.n; ++i)
                for (int r = 0; r < ref.rows - 1; ++r) t[i * (ref.rows - 1) + r] = nrm[i * span + r];
            nrm.swap(t);
        }
        np = nrm.data();
    }
    dev.check(pmx_set_search(dev.ctx, searchType));  // 0: brute force, 1/2: exact grid search
    if (mean_out)
        dev.check(pmx_set_reference_mean_centred(dev.ctx, ref.feat(), ref.rows, ref.n, np, mean_out));
    else if (centre)
        dev.check(pmx_set_reference_centred(dev.ctx, ref.feat(), ref.rows, ref.n, np, centre));
    else
        dev.check(pmx_set_reference(dev.ctx, ref.feat(), ref.rows, ref.n, np));
}
template <typename T>
typename PM<T>::Matches device_matches(Device& dev, int knn) {
    typename PM<T>::Matches m;
    m.dev = &dev;
    m.knn = knn;
    int64_t n = 0;
    pmx_get_shape(dev.ctx, &n, nullptr);
    m.n = n;
    return m;
}

template <typename T>
struct KDTreeMatcherGPU : PM<T>::Matcher {
    typedef typename PM<T>::Matches Matches;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("knn", "number of nearest neighbors to consider it the reference", "1", "1", "2147483647",
                     &Parametrizable::Comp<unsigned>),
                PDoc("epsilon", "approximation to use for the nearest-neighbor search", "0", "0", "inf",
                     &Parametrizable::Comp<T>),
                PDoc("searchType", "Nabo search type (the GPU search is exact for every type)", "1", "0", "2",
                     &Parametrizable::Comp<unsigned>),
                PDoc("maxDist", "maximum distance to consider for neighbors", "inf", "0", "inf",
                     &Parametrizable::Comp<T>)};
    }
    int knn;
    T epsilon;
    int searchType;
    T maxDist;
    explicit KDTreeMatcherGPU(const Parametrizable::Parameters& p)
        : PM<T>::Matcher("KDTreeMatcher", doc(), p),
          knn(this->template get<int>("knn")),
          epsilon(this->template get<T>("epsilon")),
          searchType(this->template get<int>("searchType")),
          maxDist(this->template get<T>("maxDist")) {}

    void init(Device& dev, const DataPoints<T>& ref, const T* centre, T* mean_out) override {
        matcher_init<T>(dev, ref, searchType, centre, mean_out);
    }
    Matches findClosests(Device& dev, const std::vector<T>& T_iter) override {
        // PointCountTouched is added from the minimiser's pmx_stats.visited
        // once the (asynchronous) match has completed, see ICP::step
        dev.check(pmx_match(dev.ctx, T_iter.data(), knn, (double)maxDist, (double)epsilon, nullptr));
        return device_matches<T>(dev, knn);
    }
    bool loopConfig(pmx_loop_cfg& cfg) const override {
        cfg.knn = knn;
        cfg.max_dist = (double)maxDist;
        return true;
    }
};

// ---- KDTreeVarDistMatcher (MatchersImpl.h:105-134, MatchersImpl.cpp:106-150):
// the radius of each reading point is its maxDistField descriptor; the GPU
// search takes the radii per query (pmx_set_reading_radii)
template <typename T>
struct KDTreeVarDistMatcherGPU : PM<T>::Matcher {
    typedef typename PM<T>::Matches Matches;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("knn", "number of nearest neighbors to consider it the reference", "1", "1", "2147483647",
                     &Parametrizable::Comp<unsigned>),
                PDoc("epsilon", "approximation to use for the nearest-neighbor search", "0", "0", "inf",
                     &Parametrizable::Comp<T>),
                PDoc("searchType", "Nabo search type (the GPU search is exact for every type)", "1", "0", "2",
                     &Parametrizable::Comp<unsigned>),
                PDoc("maxDistField", "descriptor field name used to set a maximum distance to consider for neighbors "
                                     "per point", "maxSearchDist")};
    }
    int knn;
    T epsilon;
    int searchType;
    std::string maxDistField;
    explicit KDTreeVarDistMatcherGPU(const Parametrizable::Parameters& p)
        : PM<T>::Matcher("KDTreeVarDistMatcher", doc(), p),
          knn(this->template get<int>("knn")),
          epsilon(this->template get<T>("epsilon")),
          searchType(this->template get<int>("searchType")),
          maxDistField(this->template get<std::string>("maxDistField")) {}
    void init(Device& dev, const DataPoints<T>& ref, const T* centre, T* mean_out) override {
        matcher_init<T>(dev, ref, searchType, centre, mean_out);
    }
    void initReading(Device& dev, const DataPoints<T>& reading) override {
        // getDescriptorViewByName(maxDistField).transpose(): one radius per point
        int span = 0;
        const std::vector<T> r = reading.descriptor(maxDistField, &span);
        if (span != 1)
            throw InvalidElement("KDTreeVarDistMatcher: descriptor " + maxDistField + " must have one row, not " +
                                 std::to_string(span));
        dev.check(pmx_set_reading_radii(dev.ctx, r.data()));
    }
    Matches findClosests(Device& dev, const std::vector<T>& T_iter) override {
        dev.check(pmx_match(dev.ctx, T_iter.data(), knn, INFINITY, (double)epsilon, nullptr));
        return device_matches<T>(dev, knn);
    }
    bool loopConfig(pmx_loop_cfg& cfg) const override {
        cfg.knn = knn;
        cfg.max_dist = INFINITY;  // (the per-point radii stay set on the context)
        return true;
    }
};

// ---- outlier filters ------------------------------------------------------
template <typename T>
struct NullOF : PM<T>::OutlierFilter {
    explicit NullOF(const Parametrizable::Parameters&) {}
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_null(d.ctx, pos));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_NULL;
        return true;
    }
};
template <typename T>
struct MaxDistOF : PM<T>::OutlierFilter {
    T maxDist;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("maxDist", "threshold distance (Euclidean norm)", "1", "0.0000001", "inf", &Parametrizable::Comp<T>)};
    }
    explicit MaxDistOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("MaxDistOutlierFilter", doc(), p), maxDist(this->template get<T>("maxDist")) {}
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_maxdist(d.ctx, pos, (double)maxDist));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_MAXDIST;
        cfg.filter_p[pos][0] = (double)maxDist;
        return true;
    }
};
template <typename T>
struct MinDistOF : PM<T>::OutlierFilter {
    T minDist;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("minDist", "threshold distance (Euclidean norm)", "1", "0.0000001", "inf", &Parametrizable::Comp<T>)};
    }
    explicit MinDistOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("MinDistOutlierFilter", doc(), p), minDist(this->template get<T>("minDist")) {}
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_mindist(d.ctx, pos, (double)minDist));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_MINDIST;
        cfg.filter_p[pos][0] = (double)minDist;
        return true;
    }
};
template <typename T>
struct MedianDistOF : PM<T>::OutlierFilter {
    T factor;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("factor", "points farther away factor * median will be considered outliers.", "3", "0.0000001",
                     "inf", &Parametrizable::Comp<T>)};
    }
    explicit MedianDistOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("MedianDistOutlierFilter", doc(), p), factor(this->template get<T>("factor")) {}
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_mediandist(d.ctx, pos, (double)factor));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_MEDIANDIST;
        cfg.filter_p[pos][0] = (double)factor;
        return true;
    }
};
template <typename T>
struct TrimmedDistOF : PM<T>::OutlierFilter {
    T ratio;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("ratio", "percentage to keep", "0.85", "0.0000001", "1.0", &Parametrizable::Comp<T>)};
    }
    explicit TrimmedDistOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("TrimmedDistOutlierFilter", doc(), p), ratio(this->template get<T>("ratio")) {}
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_trimmed(d.ctx, pos, (double)ratio));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_TRIMMED;
        cfg.filter_p[pos][0] = (double)ratio;
        return true;
    }
};
template <typename T>
struct VarTrimmedDistOF : PM<T>::OutlierFilter {
    T minRatio, maxRatio, lambda;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("minRatio", "min ratio", "0.05", "0.0000001", "1", &Parametrizable::Comp<T>),
                PDoc("maxRatio", "max ratio", "0.99", "0.0000001", "1", &Parametrizable::Comp<T>),
                PDoc("lambda", "lambda (part of the term that balance the rmsd: 1/ratio^lambda", "2.35")};
    }
    explicit VarTrimmedDistOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("VarTrimmedDistOutlierFilter", doc(), p),
          minRatio(this->template get<T>("minRatio")),
          maxRatio(this->template get<T>("maxRatio")),
          lambda(this->template get<T>("lambda")) {
        if (minRatio >= maxRatio)  // OutlierFiltersImpl.cpp:160-163
            throw InvalidParameter("VarTrimmedDistOutlierFilter: minRatio (" + std::to_string(minRatio) +
                                   ") should be smaller than maxRatio (" + std::to_string(maxRatio) + ")");
    }
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_vartrimmed(d.ctx, pos, (double)minRatio, (double)maxRatio, (double)lambda));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_VARTRIMMED;
        cfg.filter_p[pos][0] = (double)minRatio;
        cfg.filter_p[pos][1] = (double)maxRatio;
        cfg.filter_p[pos][2] = (double)lambda;
        return true;
    }
};

// RobustOutlierFilter (OutlierFiltersImpl.h:220-260, OutlierFiltersImpl.cpp:380-598):
// the parameters and the filter's state (iteration, berg target, tuning
// substitution) stay here as in the reference object; the scale and the
// weights are computed on the device (pmx_outlier_robust).  In the device
// loop the same schedule runs from the loop's iteration index (loopConfig
// hands over the call counter; loopAdvance counts the iterations that ran).
template <typename T>
struct RobustOF : PM<T>::OutlierFilter {
    std::string robustFctName, scaleEstimator, distanceType;
    T tuning, squaredApproximation, approximation;
    int nbIterationForScale;
    int robustFctId = -1;
    int iteration = 1;
    T berg_target_scale = 0;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("robustFct", "Type of robust function used. Available fct: 'cauchy', 'welsch', 'sc', 'gm', "
                                  "'tukey', 'huber', 'L1' and 'student'.", "cauchy"),
                PDoc("tuning", "Tuning parameter used to limit the influence of outliers (the target scale with "
                               "'berg').", "1.0", "0.0000001", "inf", &Parametrizable::Comp<T>),
                PDoc("scaleEstimator", "'none', 'mad', 'berg' or 'std'", "mad"),
                PDoc("nbIterationForScale", "iterations the scale is recomputed for (0: every iteration)", "0", "0",
                     "100", &Parametrizable::Comp<int>),
                PDoc("distanceType", "'point2point' or 'point2plane'", "point2point"),
                PDoc("approximation", "weights of errors above this threshold are forced to zero (inf: none)", "inf",
                     "0.0", "inf", &Parametrizable::Comp<T>)};
    }
    explicit RobustOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("RobustOutlierFilter", doc(), p),
          robustFctName(this->template get<std::string>("robustFct")),
          scaleEstimator(this->template get<std::string>("scaleEstimator")),
          distanceType(this->template get<std::string>("distanceType")),
          tuning(this->template get<T>("tuning")),
          approximation(this->template get<T>("approximation")),
          nbIterationForScale(this->template get<int>("nbIterationForScale")) {
        squaredApproximation = (T)std::pow(approximation, 2);
        if (scaleEstimator != "none" && scaleEstimator != "mad" && scaleEstimator != "berg" && scaleEstimator != "std")
            throw InvalidParameter("Invalid scale estimator name.");
        if (distanceType != "point2point" && distanceType != "point2plane")
            throw InvalidParameter("Invalid distance type name.");
        static const char* names[] = {"cauchy", "welsch", "sc", "gm", "tukey", "huber", "L1", "student"};
        for (int i = 0; i < 8; ++i)
            if (robustFctName == names[i]) robustFctId = i;  // (PMX_RF_* order)
        if (robustFctId < 0) throw InvalidParameter("Invalid robust function name.");
        if (scaleEstimator == "berg") {  // Bergstrom 2014 tunings (:419-433)
            berg_target_scale = tuning;
            if (robustFctId == PMX_RF_CAUCHY) tuning = (T)4.3040;
            else if (robustFctId == PMX_RF_TUKEY) tuning = (T)7.0589;
            else if (robustFctId == PMX_RF_HUBER) tuning = (T)2.0138;
        }
    }
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        // robustFiltering's scale schedule (:500-531); iteration counts the
        // filter's calls over its lifetime, as the reference member does
        const bool recompute = iteration <= nbIterationForScale || nbIterationForScale == 0;
        int mode = PMX_RS_NONE;
        if (scaleEstimator == "mad") mode = recompute ? PMX_RS_MAD : PMX_RS_KEEP;
        else if (scaleEstimator == "std") mode = recompute ? PMX_RS_STD : PMX_RS_KEEP;
        else if (scaleEstimator == "berg")
            mode = !recompute ? PMX_RS_KEEP : (iteration == 1 ? PMX_RS_BERG_FIRST : PMX_RS_BERG_NEXT);
        ++iteration;
        d.check(pmx_outlier_robust(d.ctx, pos, robustFctId, (double)tuning, (double)approximation, mode,
                                   (double)berg_target_scale, distanceType == "point2plane" ? 1 : 0));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_ROBUST;
        cfg.robust_fct = robustFctId;
        cfg.robust_estimator = scaleEstimator == "mad"   ? PMX_RSE_MAD
                               : scaleEstimator == "std" ? PMX_RSE_STD
                               : scaleEstimator == "berg" ? PMX_RSE_BERG
                                                          : PMX_RSE_NONE;
        cfg.robust_p2pl = distanceType == "point2plane" ? 1 : 0;
        cfg.robust_nb_iter_for_scale = nbIterationForScale;
        cfg.robust_first_call = iteration;
        cfg.robust_tuning = (double)tuning;
        cfg.robust_approx = (double)approximation;
        cfg.robust_berg_target = (double)berg_target_scale;
        return true;
    }
    void loopAdvance(int64_t iterations) override { iteration += (int)iterations; }
};

// SurfaceNormalOutlierFilter (OutlierFiltersImpl.h:176-194,
// OutlierFiltersImpl.cpp:225-285): eps = cos(maxAngle) in T, here; the
// weights on the device from the reading's resident normals
// (ICP::uploadReadingNormals) and the matched reference normals.
template <typename T>
struct SurfaceNormalOF : PM<T>::OutlierFilter {
    T eps;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("maxAngle", "largest angle allowed between the two surface normals (radian)", "1.57", "0.0",
                     "3.1416", &Parametrizable::Comp<T>)};
    }
    explicit SurfaceNormalOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("SurfaceNormalOutlierFilter", doc(), p),
          eps(std::cos(this->template get<T>("maxAngle"))) {}
    bool needsReadingNormals() const override { return true; }
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_surface_normal(d.ctx, pos, (double)eps));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_SURFACENORMAL;
        cfg.filter_p[pos][0] = (double)eps;
        return true;
    }
};

// GenericDescriptorOutlierFilter (OutlierFiltersImpl.h:196-221,
// OutlierFiltersImpl.cpp:290-374): the weights on the device from a one-row
// descriptor of the filtered reference, uploaded when the matcher is
// initialised (initReference).  `source` chooses nothing: the reference reads
// the filtered reference's descriptor in both branches (:322-325), and so does
// this filter.
template <typename T>
struct GenericDescriptorOF : PM<T>::OutlierFilter {
    const std::string source, descName;
    const bool useSoftThreshold, useLargerThan;
    const T threshold;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("source", "Point cloud from which the descriptor will be used: reference or reading", "reference"),
                PDoc("descName", "Descriptor name used to weight paired points", "none"),
                PDoc("useSoftThreshold",
                     "If set to 1 (true), uses the value of the descriptor as a weight. If set to 0 (false), uses the "
                     "parameter 'threshold' to set binary weights.",
                     "0", "0", "1", &Parametrizable::Comp<bool>),
                PDoc("useLargerThan",
                     "If set to 1 (true), values over the 'threshold' will have a weight of one.  If set to 0 (false), "
                     "values under the 'threshold' will have a weight of one. All other values will have a weight of "
                     "zero.",
                     "1", "0", "1", &Parametrizable::Comp<bool>),
                PDoc("threshold", "Value used to determine the binary weights", "0.1", "0.0000001", "inf",
                     &Parametrizable::Comp<T>)};
    }
    explicit GenericDescriptorOF(const Parametrizable::Parameters& p)
        : PM<T>::OutlierFilter("GenericDescriptorOutlierFilter", doc(), p),
          source(this->template get<std::string>("source")),
          descName(this->template get<std::string>("descName")),
          useSoftThreshold(this->template get<bool>("useSoftThreshold")),
          useLargerThan(this->template get<bool>("useLargerThan")),
          threshold(this->template get<T>("threshold")) {
        if (source != "reference" && source != "reading")  // OutlierFiltersImpl.cpp:300-304
            throw InvalidParameter("GenericDescriptorOutlierFilter: Error, the parameter named 'source' can only be "
                                   "set to 'reference' or 'reading' but was set to " + source);
    }
    void checkReference(const DataPoints<T>& reference) const override {
        if (!reference.descriptorExists(descName))  // getDescriptorViewByName, :327
            throw InvalidField("Cannot find descriptor " + descName);
        int span = 0;
        for (auto& l : reference.descriptorLabels)
            if (l.text == descName) span = l.span;
        if (span != 1)  // :329-333
            throw InvalidParameter("GenericDescriptorOutlierFilter: Error, the parameter named 'descName' must be a "
                                   "1D descriptor but the field " + descName + " is " + std::to_string(span) + "D");
    }
    void initReference(Device& d, const DataPoints<T>& reference) override {
        checkReference(reference);
        const std::vector<T> v = reference.descriptor(descName);
        d.check(pmx_set_reference_weight_descriptor(d.ctx, v.data()));
    }
    void compute(Device& d, const typename PM<T>::Matches&, int pos) override {
        d.check(pmx_outlier_generic_descriptor(d.ctx, pos, useSoftThreshold ? 1 : 0, useLargerThan ? 1 : 0,
                                               (double)threshold));
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.filter_kind[pos] = PMX_FILTER_GENERICDESCRIPTOR;
        cfg.filter_p[pos][0] = useSoftThreshold ? 1.0 : 0.0;
        cfg.filter_p[pos][1] = useLargerThan ? 1.0 : 0.0;
        cfg.filter_p[pos][2] = (double)threshold;
        return true;
    }
};

// The outlier chain against the filtered reference, on the host, before the
// matcher indexes it.  One GenericDescriptorOutlierFilter per chain: the device
// keeps one weight descriptor, and a second real-valued factor of this kind
// would make the chain's product depend on the order (csrc/pmx_weight.h).
template <typename T>
void check_outlier_reference(const typename PM<T>::OutlierFilters& filters, const DataPoints<T>& reference) {
    int generic = 0;
    for (auto& f : filters) generic += f->className == "GenericDescriptorOutlierFilter" ? 1 : 0;
    if (generic > 1) throw ConfigurationError("at most one GenericDescriptorOutlierFilter per outlier chain");
    for (auto& f : filters) f->checkReference(reference);
}

// ---- error minimisers -----------------------------------------------------
template <typename T>
void build_p2plane_transform(int rows, const T* x, std::vector<T>& out) {
    // PointToPlane.cpp:245-312 (shared with the device loop: pmx_dense.h)
    out.assign((size_t)rows * rows, (T)0);
    dense::p2plane_transform(rows, x, out.data());
}

template <typename T>
struct PointToPlaneEM : PM<T>::ErrorMinimizer {
    bool force2D, force4DOF;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("force2D",
                     "If set to true(1), the minimization will be forced to give a solution in 2D (i.e., on the "
                     "XY-plane) even with 3D inputs.",
                     "0", "0", "1", &Parametrizable::Comp<bool>),
                PDoc("force4DOF",
                     "If set to true(1), the minimization will optimize only yaw and translation, pitch and roll "
                     "will follow the prior.",
                     "0", "0", "1", &Parametrizable::Comp<bool>)};
    }
    explicit PointToPlaneEM(const Parametrizable::Parameters& p)
        : PointToPlaneEM("PointToPlaneErrorMinimizer", doc(), p) {}
    // (a derived minimiser's name and parameters, PointToPlane.cpp:66-76)
    PointToPlaneEM(const std::string& name, const Parametrizable::ParametersDoc& d, const Parametrizable::Parameters& p)
        : PM<T>::ErrorMinimizer(name, d, p),
          force2D(this->template get<T>("force2D") != (T)0),
          force4DOF(this->template get<T>("force4DOF") != (T)0) {
        if (force2D && force4DOF)
            throw ConfigurationError("Force 2D cannot be used together with force4DOF.");
    }
    // PMX_FORCE_* of the parameters (PointToPlane.cpp:177-210)
    int force() const { return force2D ? PMX_FORCE_2D : force4DOF ? PMX_FORCE_4DOF : PMX_FORCE_NONE; }
    // (a derived minimiser whose estimate has no forced form refuses the flags here)
    virtual void checkForce() const {}
    std::vector<T> compute(Device& d, int rows) override {
        checkForce();
        // (a dimension mismatch in the reference: an Eigen assertion)
        if (force4DOF && rows != 4)
            throw ConfigurationError("PointToPlaneErrorMinimizer: force4DOF needs a 3-D cloud");
        // force2D on a 2-D cloud changes nothing (PointToPlane.cpp:179, 296-309)
        const int f = rows == 4 ? force() : PMX_FORCE_NONE;
        const int n = f == PMX_FORCE_4DOF ? 4 : f == PMX_FORCE_2D ? 3 : rows == 4 ? 6 : 3;
        double A[36], b[6];
        pmx_stats st;
        d.check(pmx_p2plane_system_forced(d.ctx, f, A, b, &st));
        this->setStats(st);
        T At[36], bt[6], x[6];
        for (int i = 0; i < n * n; ++i) At[i] = (T)A[i];
        for (int i = 0; i < n; ++i) bt[i] = (T)b[i];
        dense::solve_underdetermined(At, bt, n, x);
        std::vector<T> out;
        if (f == PMX_FORCE_4DOF) {  // (shared with the device loop: pmx_dense.h)
            out.assign(16, (T)0);
            dense::p2plane_transform_4dof(x, out.data());
        } else if (f == PMX_FORCE_2D) {
            out.assign(16, (T)0);
            dense::p2plane_transform_force2d(x, out.data());
        } else {
            build_p2plane_transform(rows, x, out);
        }
        return out;
    }
    int qualityKind() const override { return 0; }
    bool loopConfig(pmx_loop_cfg& cfg) const override {
        cfg.minimizer = 0;
        cfg.force = force();  // (4-DOF on a 2-D cloud: pmx_loop_begin refuses, compute() raises)
        return true;
    }
};

// PointToPlaneWithCovErrorMinimizer (ErrorMinimizers/PointToPlaneWithCov.cpp):
// PointToPlane's transforms, and the covariance of the last iteration's
// estimate (Censi's closed form, :72-162).  The reference estimates it in
// every compute and getCovariance returns the last (:61-69, 165-169); here it
// is estimated once, when the loop has stopped.  The two 6 x 6 sums over the
// kept pairs come from the device (pmx_p2plane_covariance /
// pmx_loop_covariance); the inverse and the products are the reference's, in T.
template <typename T>
struct PointToPlaneWithCovEM : PointToPlaneEM<T> {
    const T sensorStdDev;
    std::vector<T> covMatrix;
    static Parametrizable::ParametersDoc doc() {
        Parametrizable::ParametersDoc d = PointToPlaneEM<T>::doc();
        d.push_back(PDoc("sensorStdDev", "sensor standard deviation", "0.01", "0.", "inf", &Parametrizable::Comp<T>));
        return d;
    }
    explicit PointToPlaneWithCovEM(const Parametrizable::Parameters& p)
        : PointToPlaneEM<T>("PointToPlaneWithCovErrorMinimizer", doc(), p),
          sensorStdDev(this->template get<T>("sensorStdDev")),
          covMatrix(36, (T)0) {}
    int qualityKind() const override { return 2; }
    void checkForce() const override {
        if (this->force2D || this->force4DOF)
            throw ConfigurationError("PointToPlaneWithCovErrorMinimizer: force2D / force4DOF are outside the GPU path");
    }
    bool loopConfig(pmx_loop_cfg& cfg) const override {
        cfg.minimizer = 2;  // (PointToPlane's iterations; the step keeps the increments)
        return !this->force2D && !this->force4DOF;
    }
    std::vector<T> getCovariance() const override { return covMatrix; }
    void loopStopped(Device& d, int rows, const T* dT) override {
        covMatrix.assign(36, (T)0);
        if (rows != 4) {  // normals.rows() < 3 (PointToPlaneWithCov.cpp:91-92)
            for (int i = 0; i < 6; ++i) covMatrix[(size_t)i * 7] = std::numeric_limits<T>::max();
            return;
        }
        double H[36], Q[36];
        int64_t pairs = 0;
        d.check(dT ? pmx_p2plane_covariance(d.ctx, dT, H, Q, &pairs) : pmx_loop_covariance(d.ctx, H, Q, &pairs));
        T Ht[36], Qt[36], Hi[36], HiQ[36], cov[36];
        for (int i = 0; i < 36; ++i) {
            Ht[i] = (T)H[i];
            Qt[i] = (T)Q[i];
        }
        dense::lu_inverse(Ht, 6, Hi);      // J_hessian.inverse(), :156
        dense::matmul6(Hi, Qt, 6, HiQ);    // inv_J_hessian * covariance * inv_J_hessian, :159
        dense::matmul6(HiQ, Hi, 6, cov);
        const T s2 = sensorStdDev * sensorStdDev;  // :161
        for (int i = 0; i < 36; ++i) covMatrix[(size_t)i] = s2 * cov[i];
    }
};

template <typename T>
struct PointToPointEM : PM<T>::ErrorMinimizer {
    explicit PointToPointEM(const Parametrizable::Parameters&) { this->className = "PointToPointErrorMinimizer"; }
    std::vector<T> compute(Device& d, int rows) override {
        // PointToPoint.cpp:61-101
        const int D = rows - 1;
        double mp[3], mq[3], md[9];
        pmx_stats st;
        d.check(pmx_p2point_system(d.ctx, mp, mq, md, &st));
        this->setStats(st);
        T m[9], mpT[3], mqT[3];
        for (int i = 0; i < D * D; ++i) m[i] = (T)md[i];
        for (int i = 0; i < D; ++i) {
            mpT[i] = (T)mp[i];
            mqT[i] = (T)mq[i];
        }
        std::vector<T> out((size_t)rows * rows, (T)0);
        dense::p2point_transform(rows, m, mpT, mqT, out.data());  // (shared with the device loop)
        return out;
    }
    int qualityKind() const override { return 1; }
    bool loopConfig(pmx_loop_cfg& cfg) const override {
        cfg.minimizer = 1;
        return true;
    }
};

// PointToPointSimilarityErrorMinimizer (ErrorMinimizers/PointToPointSimilarity.cpp:43-98):
// PointToPoint's means and moments plus sigma from the device, the SVD, the
// reflection fix on V^T's row and its singular value, and the scale in T.  No
// parameters (ADD_TO_REGISTRAR_NO_PARAM).  Statistics and getOverlap() without
// a "simpleSensorNoise" descriptor are PointToPoint's.
template <typename T>
struct PointToPointSimilarityEM : PM<T>::ErrorMinimizer {
    explicit PointToPointSimilarityEM(const Parametrizable::Parameters&) {
        this->className = "PointToPointSimilarityErrorMinimizer";
    }
    std::vector<T> compute(Device& d, int rows) override {
        const int D = rows - 1;
        double mp[3], mq[3], md[9], sigma = 0;
        pmx_stats st;
        d.check(pmx_p2point_similarity_system(d.ctx, mp, mq, md, &sigma, &st));
        this->setStats(st);
        T m[9], mpT[3], mqT[3];
        for (int i = 0; i < D * D; ++i) m[i] = (T)md[i];
        for (int i = 0; i < D; ++i) {
            mpT[i] = (T)mp[i];
            mqT[i] = (T)mq[i];
        }
        std::vector<T> out((size_t)rows * rows, (T)0);
        dense::p2point_similarity_transform(rows, m, mpT, mqT, (T)sigma, out.data());  // (shared with the device loop)
        return out;
    }
    int qualityKind() const override { return 3; }
    bool loopConfig(pmx_loop_cfg& cfg) const override {
        cfg.minimizer = 3;
        return true;
    }
    bool similarity() const override { return true; }
};

// ---- transformation checkers ------------------------------------------------
template <typename T>
void rot3(const std::vector<T>& M, int rows, T* m3) {
    // topLeftCorner(3,3) — in 2-D this is the whole 3x3 homogeneous matrix,
    // exactly as the reference's check() uses it
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m3[r * 3 + c] = M[r * rows + c];
}

template <typename T>
struct CounterTC : PM<T>::TransformationChecker {
    unsigned maxIterationCount;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("maxIterationCount", "maximum number of iterations ", "40", "0", "2147483647",
                     &Parametrizable::Comp<unsigned>)};
    }
    explicit CounterTC(const Parametrizable::Parameters& p)
        : PM<T>::TransformationChecker("CounterTransformationChecker", doc(), p),
          maxIterationCount(this->template get<unsigned>("maxIterationCount")) {
        this->limits = {(T)maxIterationCount};
        this->conditionVariableNames = {"Iteration"};
        this->limitNames = {"Max iteration"};
    }
    void init(const std::vector<T>&, int, bool&) override { this->conditionVariables = {(T)0}; }
    void check(const std::vector<T>&, int, bool& iterate) override {
        this->conditionVariables[0] = this->conditionVariables[0] + (T)1;
        if (this->conditionVariables[0] >= this->limits[0]) {  // TransformationCheckersImpl.cpp:71-75
            iterate = false;
            throw typename PM<T>::MaxNumIterationsReached();
        }
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.checker_kind[pos] = PMX_CHECK_COUNTER;
        cfg.checker_p[pos][0] = (double)this->limits[0];
        return true;
    }
};

template <typename T>
struct DifferentialTC : PM<T>::TransformationChecker {
    T minDiffRotErr, minDiffTransErr;
    unsigned smoothLength;
    std::vector<std::array<T, 4>> rotations;
    std::vector<std::array<T, 3>> translations;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("minDiffRotErr", "threshold for rotation error (radian)", "0.001", "0.", "6.2831854",
                     &Parametrizable::Comp<T>),
                PDoc("minDiffTransErr", "threshold for translation error", "0.001", "0.", "inf", &Parametrizable::Comp<T>),
                PDoc("smoothLength", "number of iterations over which to average the differencial error", "3", "0",
                     "2147483647", &Parametrizable::Comp<unsigned>)};
    }
    explicit DifferentialTC(const Parametrizable::Parameters& p)
        : PM<T>::TransformationChecker("DifferentialTransformationChecker", doc(), p),
          minDiffRotErr(this->template get<T>("minDiffRotErr")),
          minDiffTransErr(this->template get<T>("minDiffTransErr")),
          smoothLength(this->template get<unsigned>("smoothLength")) {
        this->limits = {minDiffRotErr, minDiffTransErr};
    }
    void push(const std::vector<T>& M, int rows, bool init2d) {
        T m3[9], q[4];
        if (init2d) {
            // TransformationCheckersImpl.cpp:107-110: 2-D init uses [R 0; 0 1]
            for (int i = 0; i < 9; ++i) m3[i] = (i % 4 == 0) ? (T)1 : (T)0;
            m3[0] = M[0];
            m3[1] = M[1];
            m3[3] = M[3];
            m3[4] = M[4];
        } else {
            rot3(M, rows, m3);
        }
        dense::quat_from_matrix(m3, q);
        rotations.push_back({q[0], q[1], q[2], q[3]});
        std::array<T, 3> t{0, 0, 0};
        for (int r = 0; r < rows - 1; ++r) t[r] = M[r * rows + rows - 1];
        translations.push_back(t);
    }
    void init(const std::vector<T>& M, int rows, bool&) override {
        this->conditionVariables = {(T)0, (T)0};
        rotations.clear();
        translations.clear();
        push(M, rows, rows != 4);
    }
    void check(const std::vector<T>& M, int rows, bool& iterate) override {
        push(M, rows, false);
        T cv0 = 0, cv1 = 0;
        if (rotations.size() > smoothLength) {
            for (size_t i = rotations.size() - 1; i >= rotations.size() - smoothLength; i--) {
                cv0 = cv0 + std::fabs(dense::angular_distance(rotations[i].data(), rotations[i - 1].data()));
                T nn = 0;
                for (int r = 0; r < rows - 1; ++r) {
                    const T d = translations[i][r] - translations[i - 1][r];
                    nn = nn + d * d;
                }
                cv1 = cv1 + std::fabs(std::sqrt(nn));
            }
            cv0 = cv0 / (T)smoothLength;
            cv1 = cv1 / (T)smoothLength;
            if (cv0 < this->limits[0] && cv1 < this->limits[1]) iterate = false;
        }
        this->conditionVariables = {cv0, cv1};
        if (cv0 != cv0) throw ConvergenceError("abs rotation norm not a number");
        if (cv1 != cv1) throw ConvergenceError("abs translation norm not a number");
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.checker_kind[pos] = PMX_CHECK_DIFFERENTIAL;
        cfg.checker_p[pos][0] = (double)minDiffRotErr;
        cfg.checker_p[pos][1] = (double)minDiffTransErr;
        cfg.checker_p[pos][2] = (double)smoothLength;
        return smoothLength < 64;  // the device history ring
    }
};

template <typename T>
struct BoundTC : PM<T>::TransformationChecker {
    T maxRotationNorm, maxTranslationNorm;
    std::array<T, 4> q0{};
    T rot2d0 = 0;
    std::array<T, 3> t0{};
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("maxRotationNorm", "rotation bound", "1", "0", "inf", &Parametrizable::Comp<T>),
                PDoc("maxTranslationNorm", "translation bound", "1", "0", "inf", &Parametrizable::Comp<T>)};
    }
    explicit BoundTC(const Parametrizable::Parameters& p)
        : PM<T>::TransformationChecker("BoundTransformationChecker", doc(), p),
          maxRotationNorm(this->template get<T>("maxRotationNorm")),
          maxTranslationNorm(this->template get<T>("maxTranslationNorm")) {
        this->limits = {maxRotationNorm, maxTranslationNorm};
    }
    void init(const std::vector<T>& M, int rows, bool&) override {
        this->conditionVariables = {(T)0, (T)0};
        if (rows == 4) {
            T m3[9];
            rot3(M, rows, m3);
            dense::quat_from_matrix(m3, q0.data());
        } else {
            rot2d0 = std::acos(M[0]);
        }
        for (int r = 0; r < rows - 1; ++r) t0[r] = M[r * rows + rows - 1];
    }
    void check(const std::vector<T>& M, int rows, bool&) override {
        T cv0;
        if (rows == 4) {
            T m3[9], q[4];
            rot3(M, rows, m3);
            dense::quat_from_matrix(m3, q);
            cv0 = dense::angular_distance(q, q0.data());
        } else {
            T v = std::acos(M[0]) - rot2d0;
            while (v > (T)3.14159265358979323846) v -= (T)(2 * 3.14159265358979323846);
            while (v < (T)-M_PI) v += (T)(2 * 3.14159265358979323846);
            cv0 = v;
        }
        T nn = 0;
        for (int r = 0; r < rows - 1; ++r) {
            const T d = M[r * rows + rows - 1] - t0[r];
            nn = nn + d * d;
        }
        const T cv1 = std::sqrt(nn);
        this->conditionVariables = {cv0, cv1};
        if (cv0 > this->limits[0] || cv1 > this->limits[1]) {
            std::ostringstream oss;
            oss << "limit out of bounds: rot: " << cv0 << "/" << this->limits[0] << " tr: " << cv1 << "/"
                << this->limits[1];
            throw ConvergenceError(oss.str());
        }
    }
    bool loopConfig(pmx_loop_cfg& cfg, int pos) const override {
        cfg.checker_kind[pos] = PMX_CHECK_BOUND;
        cfg.checker_p[pos][0] = (double)maxRotationNorm;
        cfg.checker_p[pos][1] = (double)maxTranslationNorm;
        return true;
    }
};

// ---- data filters / inspectors / loggers -----------------------------------
template <typename T>
struct IdentityDPF : PM<T>::DataPointsFilter {
    explicit IdentityDPF(const Parametrizable::Parameters&) { this->className = "IdentityDataPointsFilter"; }
    void inPlaceFilter(DataPoints<T>&) override {}
};

// SurfaceNormalDataPointsFilter (DataPointsFilters/SurfaceNormal.cpp:50-290,
// parameters SurfaceNormal.h:64-80): the self k-NN and the per-point
// statistics on the GPU (pmx_surface_normals, pmx_normals.hip); descriptors
// in the reference's label order.  epsilon > 0 is accepted: the search is
// exact, which any approximation bound admits.
template <typename T>
struct SurfaceNormalDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("knn", "number of nearest neighbors to consider, including the point itself", "5", "3",
                     "2147483647", &P::Comp<unsigned>),
                PDoc("maxDist", "maximum distance to consider for neighbors", "inf", "0", "inf", &P::Comp<T>),
                PDoc("epsilon", "approximation to use for the nearest-neighbor search", "0", "0", "inf", &P::Comp<T>),
                PDoc("keepNormals", "whether the normals should be added as descriptors to the resulting cloud", "1"),
                PDoc("keepDensities", "whether the point densities should be added as descriptors to the resulting cloud",
                     "0"),
                PDoc("keepEigenValues", "whether the eigen values should be added as descriptors to the resulting cloud",
                     "0"),
                PDoc("keepEigenVectors",
                     "whether the eigen vectors should be added as descriptors to the resulting cloud", "0"),
                PDoc("keepMatchedIds",
                     "whether the identifiers of matches points should be added as descriptors to the resulting cloud",
                     "0"),
                PDoc("keepMeanDist", "whether the distance to the nearest neighbor mean should be added as descriptors "
                                     "to the resulting cloud",
                     "0"),
                PDoc("sortEigen", "whether the eigenvalues and eigenvectors should be sorted (ascending) based on the "
                                  "eigenvalues",
                     "0"),
                PDoc("smoothNormals", "whether the normal vector should be average with the nearest neighbors", "0")};
    }
    unsigned knn;
    T maxDist, epsilon;
    bool keepNormals, keepDensities, keepEigenValues, keepEigenVectors, keepMatchedIds, keepMeanDist, sortEigen,
        smoothNormals;
    explicit SurfaceNormalDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("SurfaceNormalDataPointsFilter", doc(), p),
          knn(this->template get<unsigned>("knn")),
          maxDist(this->template get<T>("maxDist")),
          epsilon(this->template get<T>("epsilon")),
          keepNormals(this->template get<bool>("keepNormals")),
          keepDensities(this->template get<bool>("keepDensities")),
          keepEigenValues(this->template get<bool>("keepEigenValues")),
          keepEigenVectors(this->template get<bool>("keepEigenVectors")),
          keepMatchedIds(this->template get<bool>("keepMatchedIds")),
          keepMeanDist(this->template get<bool>("keepMeanDist")),
          sortEigen(this->template get<bool>("sortEigen")),
          smoothNormals(this->template get<bool>("smoothNormals")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const int D = cloud.rows - 1;
        const int64_t n = cloud.n;
        // (eigenpairs are always returned in ascending order: sortEigen's
        // order, and the order computeNormal's choice does not depend on)
        std::vector<T> nrm, dens, eva, eve, ids, md;
        if (keepNormals || smoothNormals) nrm.resize((size_t)(n * D));
        if (keepDensities) dens.resize((size_t)n);
        if (keepEigenValues) eva.resize((size_t)(n * D));
        if (keepEigenVectors) eve.resize((size_t)(n * D * D));
        if (keepMatchedIds) ids.resize((size_t)(n * knn));
        if (keepMeanDist) md.resize((size_t)n);
        auto ptr = [](std::vector<T>& v) { return v.empty() ? nullptr : (void*)v.data(); };
        int64_t degenerate = 0;
        const int rc = pmx_surface_normals(this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                           (int)std::min<unsigned>(knn, 1u << 30), (double)maxDist,
                                           smoothNormals ? PMX_SN_SMOOTH : 0u, ptr(nrm), ptr(dens), ptr(eva), ptr(eve),
                                           ptr(ids), ptr(md), &degenerate);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(std::string("SurfaceNormalDataPointsFilter: ") + pmx_last_error(nullptr));
        if (keepNormals) cloud.setDescriptor("normals", D, nrm.data());
        if (keepDensities) cloud.setDescriptor("densities", 1, dens.data());
        if (keepEigenValues) cloud.setDescriptor("eigValues", D, eva.data());
        if (keepEigenVectors) cloud.setDescriptor("eigVectors", D * D, eve.data());
        if (keepMatchedIds) cloud.setDescriptor("matchedIds", (int)knn, ids.data());
        if (keepMeanDist) cloud.setDescriptor("meanDists", 1, md.data());
    }
};

// Stable in-place compaction of a cloud's points (features and descriptors),
// keep(f) called once per point in index order — DataPoints::setColFrom +
// conservativeResize of the reference's subsampling filters.
template <typename T, typename Keep>
void compact_points(DataPoints<T>& cloud, Keep keep) {
    int64_t j = 0;
    for (int64_t i = 0; i < cloud.n; ++i) {
        const T* f = &cloud.features[(size_t)i * cloud.rows];
        if (!keep(f)) continue;
        if (j != i) {
            std::copy(f, f + cloud.rows, &cloud.features[(size_t)j * cloud.rows]);
            const T* d = &cloud.descriptors[(size_t)i * cloud.descDim];
            std::copy(d, d + cloud.descDim, &cloud.descriptors[(size_t)j * cloud.descDim]);
        }
        ++j;
    }
    cloud.n = j;
    cloud.features.resize((size_t)j * cloud.rows);
    cloud.descriptors.resize((size_t)j * cloud.descDim);
}

// MaxDist / MinDist data filters (DataPointsFilters/MaxDist.cpp:55-96,
// MinDist.cpp:55-96, parameters MaxDist.h:57-61, MinDist.h:57-61): keep the
// points whose coordinate `dim` (or Euclidean norm when dim == -1, against
// |limit|) is strictly below (Max) / strictly above (Min) the limit,
// stable compaction of features and descriptors; dim >= D throws.  Host code,
// once per compute and outside the ICP loop, as in the reference.
template <typename T, bool kMax>
struct DistDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static const char* pname() { return kMax ? "maxDist" : "minDist"; }
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("dim", "dimension on which the filter will be applied. x=0, y=1, z=2, radius=-1", "-1", "-1", "2",
                     &P::Comp<int>),
                PDoc(pname(), kMax ? "maximum distance authorized" : "minimum value authorized", "1", "-inf", "inf",
                     &P::Comp<T>)};
    }
    const int dim;
    const T limit;
    explicit DistDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter(kMax ? "MaxDistDataPointsFilter" : "MinDistDataPointsFilter", doc(), p),
          dim(this->template get<int>("dim")),
          limit(this->template get<T>(pname())) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const int D = cloud.rows - 1;
        if (dim >= D)
            throw InvalidParameter(this->className + ": Error, filtering on dimension number " + std::to_string(dim) +
                                   ", larger than authorized axis id " + std::to_string(D - 1));
        const T absLimit = std::abs(limit);
        compact_points(cloud, [&](const T* f) {
            if (dim == -1) {
                T s = 0;
                for (int r = 0; r < D; ++r) s += f[r] * f[r];
                const T norm = std::sqrt(s);
                return kMax ? (norm < absLimit) : (norm > absLimit);
            }
            return kMax ? (f[dim] < limit) : (f[dim] > limit);
        });
    }
};

// SimpleSensorNoiseDataPointsFilter (DataPointsFilters/SimpleSensorNoise.cpp:
// 44-136, parameters SimpleSensorNoise.h:62-63): the descriptor
// "simpleSensorNoise" (span 1) from each point's Euclidean norm, by one of five
// sensor models: max(minRadius, beamAngle * norm + beamConst) for the four
// lasers, norm^2 * (0.5 * 0.00285) for Kinect / Xtion, every operation in T.
// gain is read and unused, as in the reference.  Host code, elementwise, once
// per compute, like the MaxDist filter above.
template <typename T>
struct SimpleSensorNoiseDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("sensorType",
                     "Type of the sensor used. Choices: 0=Sick LMS-1xx, 1=Hokuyo URG-04LX, 2=Hokuyo UTM-30LX, "
                     "3=Kinect/Xtion",
                     "0", "0", "2147483647", &P::Comp<unsigned>),
                PDoc("gain",
                     "If the point cloud is coming from an untrusty source, you can use the gain to augment the "
                     "uncertainty",
                     "1", "1", "inf", &P::Comp<T>)};
    }
    const unsigned sensorType;
    const T gain;
    explicit SimpleSensorNoiseDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("SimpleSensorNoiseDataPointsFilter", doc(), p),
          sensorType(this->template get<unsigned>("sensorType")),
          gain(this->template get<T>("gain")) {
        if (sensorType >= 5)  // (the five sensor names, SimpleSensorNoise.cpp:53-61)
            throw InvalidParameter("SimpleSensorNoiseDataPointsFilter: Error, sensorType id " +
                                   std::to_string(sensorType) + " does not exist.");
    }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        // {minRadius, beamAngle, beamConst} of computeLaserNoise, :87-113
        static const double laser[5][3] = {{0.012, 0.0068, 0.0008}, {0.028, 0.0013, 0.0001}, {0.018, 0.0006, 0.0015},
                                           {0, 0, 0}, {0.004, 0.0053, -0.0092}};
        const int dim = cloud.rows, D = dim - 1;
        std::vector<T> noise((size_t)cloud.n);
        const T minRadius = (T)laser[sensorType][0], beamAngle = (T)laser[sensorType][1],
                beamConst = (T)laser[sensorType][2];
        for (int64_t j = 0; j < cloud.n; ++j) {
            const T* f = &cloud.features[(size_t)j * dim];
            T s = f[0] * f[0];
            for (int r = 1; r < D; ++r) s = s + f[r] * f[r];
            const T norm = std::sqrt(s);
            if (sensorType == 3) {
                noise[(size_t)j] = (norm * norm) * (T)(0.5 * 0.00285);  // :105-106
            } else {
                const T v = beamAngle * norm + beamConst;  // :131-135
                noise[(size_t)j] = v > minRadius ? v : minRadius;
            }
        }
        cloud.setDescriptor("simpleSensorNoise", 1, noise.data());
    }
};

// ObservationDirectionDataPointsFilter (DataPointsFilters/ObservationDirection.cpp:
// 39-88, parameters ObservationDirection.h:63-70): the descriptor
// "observationDirections" (span D) = centre - p, the sensor centre (x, y[, z])
// in the cloud's frame.  Host code, elementwise, once per compute, like
// SimpleSensorNoise above; nothing in the ICP loop reads it, so it is not
// uploaded.
template <typename T>
struct ObservationDirectionDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("x", "x-coordinate of sensor", "0"), PDoc("y", "y-coordinate of sensor", "0"),
                PDoc("z", "z-coordinate of sensor", "0")};
    }
    const T centerX, centerY, centerZ;
    explicit ObservationDirectionDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("ObservationDirectionDataPointsFilter", doc(), p),
          centerX(this->template get<T>("x")),
          centerY(this->template get<T>("y")),
          centerZ(this->template get<T>("z")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const int dim = cloud.rows, D = dim - 1;
        if (D != 2 && D != 3)
            throw InvalidField("ObservationDirectionDataPointsFilter: Error, works only in 2 or 3 dimensions, cloud has " +
                               std::to_string(D) + " dimensions.");
        const T center[3] = {centerX, centerY, centerZ};
        std::vector<T> obs((size_t)cloud.n * D);
        const T* f = cloud.feat();
        for (int64_t j = 0; j < cloud.n; ++j)
            for (int r = 0; r < D; ++r) obs[(size_t)j * D + r] = center[r] - f[(size_t)j * dim + r];
        cloud.setDescriptor("observationDirections", D, obs.data());
    }
};

// OrientNormalsDataPointsFilter (DataPointsFilters/OrientNormals.cpp:40-92,
// parameter OrientNormals.h:59-64): "normals" flipped where they point away
// from (towardCenter 1: obs . n < 0) or towards (0: obs . n > 0) the sensor;
// the dot is formed in T and compared as a double, as in the reference.  Both
// descriptors must exist (InvalidField).  Host code, elementwise.
template <typename T>
struct OrientNormalsDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("towardCenter",
                     "If true (1), every normal is turned to point toward the observation point; if false (0), away "
                     "from it.",
                     "1", "0", "1", &P::Comp<bool>)};
    }
    const bool towardCenter;
    explicit OrientNormalsDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("OrientNormalsDataPointsFilter", doc(), p),
          towardCenter(this->template get<bool>("towardCenter")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if (!cloud.descriptorExists("normals"))
            throw InvalidField("OrientNormalsDataPointsFilter: Error, cannot find normals in descriptors.");
        if (!cloud.descriptorExists("observationDirections"))
            throw InvalidField(
                "OrientNormalsDataPointsFilter: Error, cannot find observation directions in descriptors.");
        int span = 0, ospan = 0;
        std::vector<T> nrm = cloud.descriptor("normals", &span);
        const std::vector<T> obs = cloud.descriptor("observationDirections", &ospan);
        if (span != ospan)  // (an assertion in the reference)
            throw InvalidField("OrientNormalsDataPointsFilter: normals and observationDirections differ in rows");
        for (int64_t j = 0; j < cloud.n; ++j) {
            T* n = &nrm[(size_t)j * span];
            const T* o = &obs[(size_t)j * span];
            T s = o[0] * n[0];  // (Eigen's dot: sequential in T)
            for (int r = 1; r < span; ++r) s = s + o[r] * n[r];
            const double scalar = (double)s;
            if (towardCenter ? scalar < 0 : scalar > 0)
                for (int r = 0; r < span; ++r) n[r] = -n[r];
        }
        cloud.setDescriptor("normals", span, nrm.data());
    }
};

// DistanceLimitDataPointsFilter (DataPointsFilters/DistanceLimit.cpp:57-128,
// DistanceLimit.h:57-63): MaxDist (removeInside 0: keep < dist) and MinDist
// (removeInside 1: keep > dist) in one filter, on coordinate dim or the
// Euclidean norm against |dist| (dim -1); dim >= D throws.
template <typename T>
struct DistanceLimitDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("dim", "dimension on which the filter will be applied. x=0, y=1, z=2, radius=-1", "-1", "-1", "2",
                     &P::Comp<int>),
                PDoc("dist",
                     "distance limit of the filter. If dim is set to -1 (radius), the absolute value of dist will be used",
                     "1", "-inf", "inf", &P::Comp<T>),
                PDoc("removeInside",
                     "If set to true (1), remove points before the distance limit; else (0), remove points beyond the "
                     "distance limit",
                     "1", "0", "1", &P::Comp<bool>)};
    }
    const int dim;
    const T dist;
    const bool removeInside;
    explicit DistanceLimitDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("DistanceLimitDataPointsFilter", doc(), p),
          dim(this->template get<int>("dim")),
          dist(this->template get<T>("dist")),
          removeInside(this->template get<bool>("removeInside")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const int D = cloud.rows - 1;
        if (dim >= D)
            throw InvalidParameter("DistanceLimitDataPointsFilter: Error, filtering on dimension number " +
                                   std::to_string(dim) + ", larger than authorized axis id " + std::to_string(D - 1));
        const T absMaxDist = std::abs(dist);
        compact_points(cloud, [&](const T* f) {
            if (dim == -1) {
                T s = 0;
                for (int r = 0; r < D; ++r) s += f[r] * f[r];
                const T norm = std::sqrt(s);
                return removeInside ? (norm > absMaxDist) : (norm < absMaxDist);
            }
            return removeInside ? (f[dim] > dist) : (f[dim] < dist);
        });
    }
};

// RandomSamplingDataPointsFilter (DataPointsFilters/RandomSampling.cpp:55-74,
// RandomSampling.h:59-62): keep point i when (float)std::rand() /
// (float)RAND_MAX < prob, one draw per point in order — the same C library
// generator and state as the reference, so the kept set is identical for the
// same srand seed.
template <typename T>
struct RandomSamplingDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("prob", "probability to keep a point, one over decimation factor ", "0.75", "0", "1",
                     &P::Comp<T>)};
    }
    const double prob;
    explicit RandomSamplingDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("RandomSamplingDataPointsFilter", doc(), p), prob(this->template get<double>("prob")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        compact_points(cloud, [&](const T*) {
            const float r = (float)std::rand() / (float)RAND_MAX;
            return r < prob;
        });
    }
    bool usesRandState() const override { return true; }
};

// BoundingBoxDataPointsFilter (DataPointsFilters/BoundingBox.cpp:76-108,
// BoundingBox.h:57-67): open box (strict < / >) on x, y and z (z ignored for
// 2-D clouds); removeInside keeps the points outside the box, else inside.
template <typename T>
struct BoundingBoxDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("xMin", "minimum value on x-axis defining one side of the bounding box", "-1", "-inf", "inf",
                     &P::Comp<T>),
                PDoc("xMax", "maximum value on x-axis defining one side of the bounding box", "1", "-inf", "inf",
                     &P::Comp<T>),
                PDoc("yMin", "minimum value on y-axis defining one side of the bounding box", "-1", "-inf", "inf",
                     &P::Comp<T>),
                PDoc("yMax", "maximum value on y-axis defining one side of the bounding box", "1", "-inf", "inf",
                     &P::Comp<T>),
                PDoc("zMin", "minimum value on z-axis defining one side of the bounding box", "-1", "-inf", "inf",
                     &P::Comp<T>),
                PDoc("zMax", "maximum value on z-axis defining one side of the bounding box", "1", "-inf", "inf",
                     &P::Comp<T>),
                PDoc("removeInside",
                     "If set to true (1), remove points inside the bounding box; else (0), remove points outside the "
                     "bounding box",
                     "1", "0", "1", &P::Comp<bool>)};
    }
    const T xMin, xMax, yMin, yMax, zMin, zMax;
    const bool removeInside;
    explicit BoundingBoxDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("BoundingBoxDataPointsFilter", doc(), p),
          xMin(this->template get<T>("xMin")),
          xMax(this->template get<T>("xMax")),
          yMin(this->template get<T>("yMin")),
          yMax(this->template get<T>("yMax")),
          zMin(this->template get<T>("zMin")),
          zMax(this->template get<T>("zMax")),
          removeInside(this->template get<bool>("removeInside")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const bool flat = cloud.rows == 3;
        compact_points(cloud, [&](const T* f) {
            const bool in = f[0] > xMin && f[0] < xMax && f[1] > yMin && f[1] < yMax &&
                            ((f[2] > zMin && f[2] < zMax) || flat);
            return removeInside ? !in : in;
        });
    }
};

// FixStepSamplingDataPointsFilter (DataPointsFilters/FixStepSampling.cpp:37-93,
// FixStepSampling.h:57-72): keep every step-th point from a random phase
// rand() % step; step starts at startStep (reset by init) and is multiplied by
// stepMult after each application, clamped at endStep.
template <typename T>
struct FixStepSamplingDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("startStep", "initial number of point to skip (initial decimation factor)", "10", "1",
                     "2147483647", &P::Comp<unsigned>),
                PDoc("endStep", "maximal or minimal number of points to skip (final decimation factor)", "10", "1",
                     "2147483647", &P::Comp<unsigned>),
                PDoc("stepMult", "multiplication factor to compute the new decimation factor for each iteration", "1",
                     "0.0000001", "inf", &P::Comp<double>)};
    }
    const unsigned startStep, endStep;
    const double stepMult;
    double step;
    explicit FixStepSamplingDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("FixStepSamplingDataPointsFilter", doc(), p),
          startStep(this->template get<unsigned>("startStep")),
          endStep(this->template get<unsigned>("endStep")),
          stepMult(this->template get<double>("stepMult")),
          step(startStep) {}
    void init() override { step = startStep; }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const int iStep((int)step);
        const int64_t phase = std::rand() % iStep;
        int64_t i = -1;
        compact_points(cloud, [&](const T*) {
            ++i;
            return i >= phase && (i - phase) % iStep == 0;
        });
        const double deltaStep(startStep * stepMult - startStep);
        step *= stepMult;
        if (deltaStep < 0 && step < endStep) step = endStep;
        if (deltaStep > 0 && step > endStep) step = endStep;
    }
    bool usesRandState() const override { return true; }
};

// SamplingSurfaceNormalDataPointsFilter (DataPointsFilters/SamplingSurfaceNormal.cpp:80-342,
// parameters SamplingSurfaceNormal.h:64-79): the recursive median split and
// the leaf statistics on the GPU, the sampling on the process's rand() state
// (pmx_sampling_surface_normals, pmx_ssn.hip); existing descriptors averaged
// per leaf (samplingMethod 1) or kept, the new ones in the reference's label
// order.
// VoxelGridDataPointsFilter (DataPointsFilters/VoxelGrid.h:40-98,
// VoxelGrid.cpp:60-343) on the device (pmx_voxel_grid)
template <typename T>
struct VoxelGridDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("vSizeX", "Dimension of each voxel cell in x direction", "1.0", "0.001", "+inf", &P::Comp<T>),
                PDoc("vSizeY", "Dimension of each voxel cell in y direction", "1.0", "0.001", "+inf", &P::Comp<T>),
                PDoc("vSizeZ", "Dimension of each voxel cell in z direction", "1.0", "0.001", "+inf", &P::Comp<T>),
                PDoc("useCentroid", "If 1 (true), down-sample by using centroid of voxel cell.  If false (0), use "
                                    "center of voxel cell.", "1", "0", "1", &P::Comp<bool>),
                PDoc("averageExistingDescriptors", "whether the filter keep the existing point descriptors and average "
                                                   "them or should it drop them", "1", "0", "1", &P::Comp<bool>)};
    }
    T vSizeX, vSizeY, vSizeZ;
    bool useCentroid, averageExistingDescriptors;
    explicit VoxelGridDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("VoxelGridDataPointsFilter", doc(), p),
          vSizeX(this->template get<T>("vSizeX")),
          vSizeY(this->template get<T>("vSizeY")),
          vSizeZ(this->template get<T>("vSizeZ")),
          useCentroid(this->template get<bool>("useCentroid")),
          averageExistingDescriptors(this->template get<bool>("averageExistingDescriptors")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if (averageExistingDescriptors) {  // (VoxelGrid.cpp:83-90)
            int sum = 0;
            for (auto& l : cloud.descriptorLabels) sum += l.span;
            if (sum != cloud.descDim)
                throw InvalidElement("VoxelGridDataPointsFilter: Error, descriptor labels do not match descriptor data");
        }
        const int64_t n = cloud.n;
        std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim));
        const double vs[3] = {(double)vSizeX, (double)vSizeY, (double)vSizeZ};
        int64_t nout = 0;
        const int rc = pmx_voxel_grid(this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                      cloud.descDim ? cloud.descriptors.data() : nullptr, cloud.descDim, vs,
                                      useCentroid ? 1 : 0, averageExistingDescriptors ? 1 : 0, feat.data(),
                                      cloud.descDim ? desc.data() : nullptr, &nout);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(std::string("VoxelGridDataPointsFilter: ") + pmx_last_error(nullptr));
        cloud.n = nout;
        feat.resize((size_t)(nout * cloud.rows));
        cloud.features.swap(feat);
        desc.resize((size_t)(nout * cloud.descDim));
        cloud.descriptors.swap(desc);
    }
};

// OctreeGridDataPointsFilter (DataPointsFilters/OctreeGrid.h:80-83,
// OctreeGrid.cpp:284-366) on the device (pmx_octree_grid, pmx_octree.hip): one
// point per non-empty leaf, in the reference's visit order.  First and random
// sampling are bit-identical to the reference, its swapCols / mapidx column
// order included; centroid and medoid are computed per leaf from the input
// cloud (the reference addresses columns through a table that goes stale: see
// include/pmx.h).  buildParallel is accepted and changes nothing.  The random
// sampler brackets its draws with srand(1) as the reference does, so every
// call resets the process's rand() state.
template <typename T>
struct OctreeGridDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("buildParallel", "If 1 (true), use threads to build the octree.", "1", "0", "1", &P::Comp<bool>),
                PDoc("maxPointByNode", "Number of point under which the octree stop dividing.", "1", "1", "4294967295",
                     &P::Comp<std::size_t>),
                PDoc("maxSizeByNode", "Size of the bounding box under which the octree stop dividing.", "0", "0", "+inf",
                     &P::Comp<T>),
                PDoc("samplingMethod", "Method to sample the Octree: First Point (0), Random (1), Centroid (2) (more "
                                       "accurate but costly), Medoid (3) (more accurate but costly)",
                     "0", "0", "3", &P::Comp<int>)};
    }
    const bool buildParallel;
    const std::size_t maxPointByNode;
    const T maxSizeByNode;
    const int samplingMethod;
    explicit OctreeGridDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("OctreeGridDataPointsFilter", doc(), p),
          buildParallel(this->template get<bool>("buildParallel")),
          maxPointByNode(this->template get<std::size_t>("maxPointByNode")),
          maxSizeByNode(this->template get<T>("maxSizeByNode")),
          samplingMethod(this->template get<int>("samplingMethod")) {}
    bool usesRandState() const override { return samplingMethod == 1; }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        cloud.materialize();
        const int64_t n = cloud.n;
        std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim));
        int64_t nout = 0;
        const int rc = pmx_octree_grid(this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                       cloud.descDim ? cloud.descriptors.data() : nullptr, cloud.descDim,
                                       (int64_t)maxPointByNode, (double)maxSizeByNode, samplingMethod, feat.data(),
                                       cloud.descDim ? desc.data() : nullptr, &nout);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(std::string("OctreeGridDataPointsFilter: ") + pmx_last_error(nullptr));
        cloud.n = nout;
        feat.resize((size_t)(nout * cloud.rows));
        cloud.features.swap(feat);
        desc.resize((size_t)(nout * cloud.descDim));
        cloud.descriptors.swap(desc);
    }
};

// The keep-filters on the device (pmx_keep_filter, pmx_keep.hip): a per-point
// predicate and a stable compaction of features and descriptors.
template <typename T>
void keep_on_device(DataPoints<T>& cloud, int device, const char* who, int pred, int index, int flag, double value) {
    cloud.materialize();
    const int64_t n = cloud.n;
    std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim));
    int64_t nout = 0;
    const int rc = pmx_keep_filter(device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                   cloud.descDim ? cloud.descriptors.data() : nullptr, cloud.descDim, pred, index, flag,
                                   value, feat.data(), cloud.descDim ? desc.data() : nullptr, &nout);
    if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
    if (rc) throw std::runtime_error(std::string(who) + ": " + pmx_last_error(nullptr));
    cloud.n = nout;
    feat.resize((size_t)(nout * cloud.rows));
    cloud.features.swap(feat);
    desc.resize((size_t)(nout * cloud.descDim));
    cloud.descriptors.swap(desc);
}

// row offset and span of a descriptor; false when the cloud has none of that name
template <typename T>
bool descriptor_rows(const DataPoints<T>& cloud, const std::string& name, int& off, int& span) {
    off = 0;
    for (auto& l : cloud.descriptorLabels) {
        if (l.text == name) {
            span = l.span;
            return true;
        }
        off += l.span;
    }
    return false;
}

// NormalSpaceDataPointsFilter (DataPointsFilters/NormalSpace.h:63-70,
// NormalSpace.cpp:47-181) on the device (pmx_normal_space, pmx_nss.hip): nbSample
// points drawn from the buckets of the normals' directions, bit-identical to
// the reference, its column order included (include/pmx.h).  The early exits in
// the reference's order: a 2-D cloud is left as it is with a message, then
// nbSample >= n, then the missing normals.  The shuffle draws n - 1 times from
// the process's rand() state; seed only feeds the mt19937 of the picks.
template <typename T>
struct NormalSpaceDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("nbSample", "Number of point to select.", "5000", "1", "4294967295", &P::Comp<std::size_t>),
                PDoc("seed", "Seed for the random generator.", "1", "0", "4294967295", &P::Comp<std::size_t>),
                PDoc("epsilon", "Step of discretization for the angle spaces", "0.09817477042", "0.04908738521",
                     "3.14159265359", &P::Comp<T>)};
    }
    const std::size_t nbSample;
    const std::size_t seed;
    const T epsilon;
    explicit NormalSpaceDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("NormalSpaceDataPointsFilter", doc(), p),
          nbSample(this->template get<std::size_t>("nbSample")),
          seed(this->template get<std::size_t>("seed")),
          epsilon(this->template get<T>("epsilon")) {}
    bool usesRandState() const override { return true; }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if (cloud.rows < 4) {  // NormalSpace.cpp:73-77
            std::cerr << "ERROR: NormalSpaceDataPointsFilter does not support 2D point cloud yet (does nothing)"
                      << std::endl;
            return;
        }
        if (nbSample >= (std::size_t)cloud.n) return;  // :81
        int off = 0, span = 0;
        if (!descriptor_rows(cloud, "normals", off, span))  // :85-86 (the reference's text)
            throw InvalidField("OrientNormalsDataPointsFilter: Error, cannot find normals in descriptors.");
        cloud.materialize();
        const int64_t n = cloud.n;
        std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim));
        int64_t nout = 0;
        const int rc = pmx_normal_space(this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                        cloud.descriptors.data(), cloud.descDim, off, (int64_t)nbSample,
                                        (uint64_t)seed, (double)epsilon, feat.data(), desc.data(), &nout, nullptr);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(std::string("NormalSpaceDataPointsFilter: ") + pmx_last_error(nullptr));
        cloud.n = nout;
        feat.resize((size_t)(nout * cloud.rows));
        cloud.features.swap(feat);
        desc.resize((size_t)(nout * cloud.descDim));
        cloud.descriptors.swap(desc);
    }
};

// CovarianceSamplingDataPointsFilter (DataPointsFilters/CovarianceSampling.h:
// 70-76, CovarianceSampling.cpp:74-250) on the device (pmx_covariance_sampling,
// pmx_covs.hip) with the library's own basis (include/pmx.h).  nbSample >= n
// leaves the cloud as it is before the filter looks for normals (:81-86).
// torqueNorm follows its documented meaning (0 L = 1, 1 Lavg, 2 Lmax): the
// reference reads it with get<std::uint8_t>, i.e. as a character code, so no
// branch of :115-133 matches there and L stays 1.
template <typename T>
struct CovarianceSamplingDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("nbSample", "Number of point to select.", "5000", "1", "4294967295", &P::Comp<std::size_t>),
                PDoc("torqueNorm",
                     "Method for torque normalization: (0) L=1 (no normalization, more t-normals), (1) L=Lavg "
                     "(average distance, torque is scale-independent), (2) L=Lmax (scale in unit ball, more "
                     "r-normals)",
                     "1", "0", "2", &P::Comp<int>)};
    }
    const std::size_t nbSample;
    const int torqueNorm;
    explicit CovarianceSamplingDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("CovarianceSamplingDataPointsFilter", doc(), p),
          nbSample(this->template get<std::size_t>("nbSample")),
          torqueNorm(this->template get<int>("torqueNorm")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if (cloud.rows != 4)
            throw InvalidParameter("CovarianceSamplingDataPointsFilter: 3-D clouds only (4 homogeneous rows)");
        if (nbSample >= (std::size_t)cloud.n) return;  // :81
        int off = 0, span = 0;
        if (!descriptor_rows(cloud, "normals", off, span))  // :85-86 (the reference's text names OrientNormals)
            throw InvalidField("CovarianceSamplingDataPointsFilter: Error, cannot find normals in descriptors.");
        cloud.materialize();
        const int64_t n = cloud.n;
        std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim));
        int64_t nout = 0;
        const int rc = pmx_covariance_sampling(this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                               cloud.descriptors.data(), cloud.descDim, off, (int64_t)nbSample,
                                               torqueNorm, nullptr, feat.data(), desc.data(), &nout, nullptr);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(std::string("CovarianceSamplingDataPointsFilter: ") + pmx_last_error(nullptr));
        cloud.n = nout;
        feat.resize((size_t)(nout * cloud.rows));
        cloud.features.swap(feat);
        desc.resize((size_t)(nout * cloud.descDim));
        cloud.descriptors.swap(desc);
    }
};

// ShadowDataPointsFilter (DataPointsFilters/Shadow.cpp:44-94, parameter
// Shadow.h:60-65): keep |normalized(normal) . normalized(point)| > sin(eps);
// the constructor takes the sine in T.
template <typename T>
struct ShadowDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("eps", "Small angle (in rad) around which a normal shoudn't be observable", "0.1", "0.0", "3.1416",
                     &P::Comp<T>)};
    }
    const T eps;  // sin(eps)
    explicit ShadowDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("ShadowDataPointsFilter", doc(), p), eps(std::sin(this->template get<T>("eps"))) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        int off = 0, span = 0;
        if (!descriptor_rows(cloud, "normals", off, span))
            throw InvalidField("ShadowDataPointsFilter, Error: cannot find normals in descriptors");
        if (span != cloud.rows - 1)  // (an Eigen size assertion in the reference's dot)
            throw InvalidField("ShadowDataPointsFilter: normals and points differ in rows");
        keep_on_device(cloud, this->device, "ShadowDataPointsFilter", PMX_KEEP_SHADOW, off, 0, (double)eps);
    }
};

// MaxQuantileOnAxisDataPointsFilter (DataPointsFilters/MaxQuantileOnAxis.cpp:
// 44-98, parameters MaxQuantileOnAxis.h:56-62): keep feature[dim] < limit,
// limit the element of rank size_t(n * ratio); strict, so an axis of equal
// values gives an empty cloud.  An empty cloud is left as it is (the reference
// reads past an empty vector).
template <typename T>
struct MaxQuantileOnAxisDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("dim", "dimension on which the filter will be applied. x=0, y=1, z=2", "0", "0", "2",
                     &P::Comp<unsigned>),
                PDoc("ratio", "maximum quantile authorized. All points beyond that will be filtered.", "0.5",
                     "0.0000001", "0.9999999", &P::Comp<T>)};
    }
    const unsigned dim;
    const T ratio;
    explicit MaxQuantileOnAxisDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("MaxQuantileOnAxisDataPointsFilter", doc(), p),
          dim(this->template get<unsigned>("dim")),
          ratio(this->template get<T>("ratio")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if ((int)dim >= cloud.rows)
            throw InvalidParameter("MaxQuantileOnAxisDataPointsFilter: Error, filtering on dimension number " +
                                   std::to_string(dim) + ", larger than feature dimensionality " +
                                   std::to_string(cloud.rows));
        keep_on_device(cloud, this->device, "MaxQuantileOnAxisDataPointsFilter", PMX_KEEP_MAX_QUANTILE, (int)dim, 0,
                       (double)ratio);
    }
};

// RemoveNaNDataPointsFilter (DataPointsFilters/RemoveNaN.cpp:47-66; no
// parameter): drop the points with a NaN in any feature row.
template <typename T>
struct RemoveNaNDPF : PM<T>::DataPointsFilter {
    explicit RemoveNaNDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("RemoveNaNDataPointsFilter", Parametrizable::ParametersDoc(), p) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        keep_on_device(cloud, this->device, "RemoveNaNDataPointsFilter", PMX_KEEP_REMOVE_NAN, 0, 0, 0.0);
    }
};

// CutAtDescriptorThresholdDataPointsFilter (DataPointsFilters/
// CutAtDescriptorThreshold.cpp:41-102, parameters CutAtDescriptorThreshold.h:
// 62-68): the first row of descName against the threshold; useLargerThan cuts
// the larger values (keep <=), else the smaller ones (keep >=).
template <typename T>
struct CutAtDescriptorThresholdDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("descName", "Descriptor name used to cut points", "none"),
                PDoc("useLargerThan",
                     "If set to 1 (true), points with values above the 'threshold' will be cut.  If set to 0 (false), "
                     "points with values below the 'threshold' will be cut.",
                     "1", "0", "1", &P::Comp<bool>),
                PDoc("threshold", "Value at which to cut.", "0", "-inf", "inf", &P::Comp<T>)};
    }
    const std::string descName;
    const bool useLargerThan;
    const T threshold;
    explicit CutAtDescriptorThresholdDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("CutAtDescriptorThresholdDataPointsFilter", doc(), p),
          descName(this->template get<std::string>("descName")),
          useLargerThan(this->template get<bool>("useLargerThan")),
          threshold(this->template get<T>("threshold")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        int off = 0, span = 0;
        if (!descriptor_rows(cloud, descName, off, span))
            throw InvalidField("CutAtDescriptorThresholdDataPointsFilter: Error, field not found in descriptors.");
        keep_on_device(cloud, this->device, "CutAtDescriptorThresholdDataPointsFilter", PMX_KEEP_CUT_DESCRIPTOR, off,
                       useLargerThan ? 1 : 0, (double)threshold);
    }
};

// IncidenceAngleDataPointsFilter (DataPointsFilters/IncidenceAngle.cpp:50-74;
// no parameter, IncidenceAngle.h:57-59): the descriptor "incidenceAngles" =
// acos(normalized(observationDirection) . normal) on the device
// (pmx_incidence_angles, pmx_sensor.hip).
template <typename T>
struct IncidenceAngleDPF : PM<T>::DataPointsFilter {
    explicit IncidenceAngleDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("IncidenceAngleDataPointsFilter", Parametrizable::ParametersDoc(), p) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if (!cloud.descriptorExists("normals"))
            throw InvalidField("IncidenceAngleDataPointsFilter: Error, cannot find normals in descriptors.");
        if (!cloud.descriptorExists("observationDirections"))
            throw InvalidField(
                "IncidenceAngleDataPointsFilter: Error, cannot find observation directions in descriptors.");
        int span = 0, ospan = 0;
        const std::vector<T> nrm = cloud.descriptor("normals", &span);
        const std::vector<T> obs = cloud.descriptor("observationDirections", &ospan);
        if (span != ospan)  // (an assertion in the reference)
            throw InvalidField("IncidenceAngleDataPointsFilter: normals and observationDirections differ in rows");
        std::vector<T> angles((size_t)cloud.n);
        const int rc = pmx_incidence_angles(this->device, dtype_of<T>(), nrm.data(), obs.data(), span, cloud.n,
                                            angles.data());
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(pmx_last_error(nullptr));
        cloud.setDescriptor("incidenceAngles", 1, angles.data());
    }
};

// RemoveSensorBiasDataPointsFilter (DataPointsFilters/RemoveSensorBias.cpp:
// 47-129, parameters RemoveSensorBias.h:67-73): the points whose incidence
// angle is a number in [0, angleThreshold) move along their observation
// direction by the sensor's bias model, the others are dropped
// (pmx_remove_sensor_bias, pmx_sensor.hip).  The constructor takes the
// threshold to radians in T.
template <typename T>
struct RemoveSensorBiasDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("sensorType", "Type of the sensor used. Choices: 0=Sick LMS-1xx, 1=Velodyne HDL-32E", "0", "0",
                     "1", &P::Comp<int>),
                PDoc("angleThreshold", "Threshold at which angle the correction is not applied, in degrees", "88.",
                     "0.", "90.", &P::Comp<T>)};
    }
    const int sensorType;
    const T angleThreshold;
    explicit RemoveSensorBiasDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("RemoveSensorBiasDataPointsFilter", doc(), p),
          sensorType(this->template get<int>("sensorType")),
          angleThreshold((T)(this->template get<T>("angleThreshold") / 180. * M_PI)) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        int inc = 0, ispan = 0, obs = 0, ospan = 0;
        if (!descriptor_rows(cloud, "incidenceAngles", inc, ispan))
            throw InvalidField("RemoveSensorBiasDataPointsFilter: Error, cannot find incidence angles in descriptors.");
        if (!descriptor_rows(cloud, "observationDirections", obs, ospan))
            throw InvalidField(
                "RemoveSensorBiasDataPointsFilter: Error, cannot find observationDirections in descriptors.");
        if (sensorType != 0 && sensorType != 1)
            throw InvalidParameter("RemoveSensorBiasDataPointsFilter: Error, cannot remove bias for sensorType id " +
                                   std::to_string(sensorType) + " .");
        if (ospan != cloud.rows - 1)  // (an Eigen size assertion in the reference's +=)
            throw InvalidField("RemoveSensorBiasDataPointsFilter: observationDirections and points differ in rows");
        cloud.materialize();
        const int64_t n = cloud.n;
        std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim));
        int64_t nout = 0;
        const int rc = pmx_remove_sensor_bias(this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
                                              cloud.descriptors.data(), cloud.descDim, inc, obs, sensorType,
                                              (double)angleThreshold, feat.data(), desc.data(), &nout);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(pmx_last_error(nullptr));
        cloud.n = nout;
        feat.resize((size_t)(nout * cloud.rows));
        cloud.features.swap(feat);
        desc.resize((size_t)(nout * cloud.descDim));
        cloud.descriptors.swap(desc);
    }
};

// SphericalityDataPointsFilter (DataPointsFilters/Sphericality.cpp:49-177,
// parameters Sphericality.h:72-78): the descriptor "sphericality", and
// "unstructureness" / "structureness" when kept, from the three "eigValues"
// (pmx_sphericality, pmx_sensor.hip).  keepStructureness is read as a T and
// tested for non-zero, as in the reference.
template <typename T>
struct SphericalityDPF : PM<T>::DataPointsFilter {
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("keepUnstructureness",
                     "whether the value of the unstructureness should be added to the pointcloud", "0"),
                PDoc("keepStructureness", "whether the value of the structureness should be added to the pointcloud",
                     "0")};
    }
    const int keepUnstructureness;
    const T keepStructureness;
    explicit SphericalityDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("SphericalityDataPointsFilter", doc(), p),
          keepUnstructureness(this->template get<int>("keepUnstructureness")),
          keepStructureness(this->template get<T>("keepStructureness")) {}
    void inPlaceFilter(DataPoints<T>& cloud) override {
        if (!cloud.descriptorExists("eigValues"))
            throw InvalidField("SphericalityDataPointsFilter: Error, no eigValues found in descriptors.");
        int sum = 0;
        for (auto& l : cloud.descriptorLabels) sum += l.span;
        if (sum != cloud.descDim)  // (the reference's message names SurfaceNormal: Sphericality.cpp:94)
            throw InvalidField(
                "SurfaceNormalDataPointsFilter: Error, descriptor labels do not match descriptor data");
        int span = 0;
        const std::vector<T> eig = cloud.descriptor("eigValues", &span);
        if (span != 3)
            throw InvalidField("SphericalityDataPointsFilter: Error, the number of eigValues is not 3.");
        const bool un = keepUnstructureness != 0, st = keepStructureness != (T)0;
        const size_t n = (size_t)cloud.n;
        std::vector<T> sph(n), uv(un ? n : 0), sv(st ? n : 0);
        const int rc = pmx_sphericality(this->device, dtype_of<T>(), eig.data(), cloud.n,
                                        (un ? PMX_SPH_UNSTRUCTURENESS : 0u) | (st ? PMX_SPH_STRUCTURENESS : 0u),
                                        sph.data(), un ? uv.data() : nullptr, st ? sv.data() : nullptr);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(pmx_last_error(nullptr));
        cloud.setDescriptor("sphericality", 1, sph.data());
        if (un) cloud.setDescriptor("unstructureness", 1, uv.data());
        if (st) cloud.setDescriptor("structureness", 1, sv.data());
    }
};

// MaxDensityDataPointsFilter (DataPointsFilters/MaxDensity.cpp:44-105,
// parameter MaxDensity.h:57-62): a point denser than maxDensity is kept when
// (float)rand() / RAND_MAX < maxDensity / density, one draw per such point in
// order — host code on the process's rand() state, like RandomSampling.  The
// saturation term is restated as written: nbSaturatedPts / nbPointsIn is an
// integer division, 0 unless every point has the maximum density (then the
// ratio of those points is 0 and none passes).
template <typename T>
struct MaxDensityDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("maxDensity", "Maximum density of points to target. Unit: number of points per m^3.", "10",
                     "0.0000001", "inf", &P::Comp<T>)};
    }
    const T maxDensity;
    explicit MaxDensityDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("MaxDensityDataPointsFilter", doc(), p),
          maxDensity(this->template get<T>("maxDensity")) {}
    bool usesRandState() const override { return true; }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        int off = 0, span = 0;
        if (!descriptor_rows(cloud, "densities", off, span))
            throw InvalidField("MaxDensityDataPointsFilter: Error, no densities found in descriptors.");
        cloud.materialize();
        const int nbPointsIn = (int)cloud.n;
        if (nbPointsIn == 0) return;  // (maxCoeff of an empty view in the reference)
        const int dd = cloud.descDim;
        // maxCoeff / count over the whole view (span rows; densities has one)
        T lastDensity = cloud.descriptors[(size_t)off];
        for (int64_t i = 0; i < cloud.n; ++i)
            for (int r = 0; r < span; ++r) {
                const T v = cloud.descriptors[(size_t)i * dd + off + r];
                if (v > lastDensity) lastDensity = v;
            }
        int nbSaturatedPts = 0;
        for (int64_t i = 0; i < cloud.n; ++i)
            for (int r = 0; r < span; ++r)
                nbSaturatedPts += cloud.descriptors[(size_t)i * dd + off + r] == lastDensity ? 1 : 0;
        int64_t i = -1;
        compact_points(cloud, [&](const T*) {
            ++i;
            const T density = cloud.descriptors[(size_t)i * dd + off];
            if (!(density > maxDensity)) return true;
            const float r = (float)std::rand() / (float)RAND_MAX;
            float acceptRatio = maxDensity / density;
            if (density == lastDensity) acceptRatio = acceptRatio * (1 - nbSaturatedPts / nbPointsIn);
            return r < acceptRatio;
        });
    }
};

// MaxPointCountDataPointsFilter (DataPointsFilters/MaxPointCount.cpp:41-102,
// parameters MaxPointCount.h:56-63): with maxCount <= N = n - 1, srand(seed) on
// every call, then for j < maxCount an index idx = j + size_t((N - j) *
// float(rand() / float(RAND_MAX))) and the reference's "switch" of columns j
// and idx — whose temporary is a view of column j, not a copy, so column j
// takes column idx and column idx keeps its value (a sample with repetition,
// not a shuffle).  Restated as the code runs, descriptors alike; the first
// maxCount columns stay.  maxCount > N: nothing happens.  (seed and maxCount
// are size_t in the reference; their bounds fit unsigned.)
template <typename T>
struct MaxPointCountDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("seed", "srand seed", "1", "0", "2147483647", &P::Comp<unsigned>),
                PDoc("maxCount", "maximum number of points", "1000", "0", "2147483647", &P::Comp<unsigned>)};
    }
    const size_t maxCount;
    const size_t seed;
    explicit MaxPointCountDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("MaxPointCountDataPointsFilter", doc(), p),
          maxCount(this->template get<unsigned>("maxCount")),
          seed(this->template get<unsigned>("seed")) {}
    bool usesRandState() const override { return true; }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const size_t N = (size_t)(cloud.n - 1);  // (an empty cloud wraps, as in the reference: nothing to drop)
        if (cloud.n == 0 || maxCount > N) return;
        cloud.materialize();
        std::srand((unsigned)seed);
        const int rows = cloud.rows, dd = cloud.descDim;
        for (size_t j = 0; j < maxCount; ++j) {
            size_t idx = j + (size_t)((N - j) * ((float)(std::rand() / (float)RAND_MAX)));
            if (idx > N) idx = N;  // (float(N - j) rounds up beyond 2^24 points; the reference indexes past its matrix)
            if (idx == j) continue;
            std::copy(&cloud.features[idx * rows], &cloud.features[idx * rows] + rows, &cloud.features[j * rows]);
            if (dd > 0)
                std::copy(&cloud.descriptors[idx * dd], &cloud.descriptors[idx * dd] + dd, &cloud.descriptors[j * dd]);
        }
        cloud.n = (int64_t)maxCount;
        cloud.features.resize(maxCount * rows);
        cloud.descriptors.resize(maxCount * (size_t)dd);
    }
};

template <typename T>
struct SamplingSurfaceNormalDPF : PM<T>::DataPointsFilter {
    typedef Parametrizable P;
    static Parametrizable::ParametersDoc doc() {
        return {PDoc("ratio", "ratio of points to keep with random subsampling. Matrix (normal, density, etc.) will be "
                              "associated to all points in the same bin.",
                     "0.5", "0.0000001", "1.0", &P::Comp<T>),
                PDoc("knn", "determined how many points are used to compute the normals. Direct link with the "
                            "rapidity of the computation (large = fast). Technically, limit over which a box is "
                            "splitted in two",
                     "7", "3", "2147483647", &P::Comp<unsigned>),
                PDoc("samplingMethod", "if set to 0, random subsampling using the parameter ratio. If set to 1, bin "
                                       "subsampling with the resulting number of points being 1/knn.",
                     "0", "0", "1", &P::Comp<unsigned>),
                PDoc("maxBoxDim", "maximum length of a box above which the box is discarded", "inf"),
                PDoc("averageExistingDescriptors",
                     "whether the filter keep the existing point descriptors and average them or should it drop them",
                     "1"),
                PDoc("keepNormals", "whether the normals should be added as descriptors to the resulting cloud", "1"),
                PDoc("keepDensities", "whether the point densities should be added as descriptors to the resulting cloud",
                     "0"),
                PDoc("keepEigenValues", "whether the eigen values should be added as descriptors to the resulting cloud",
                     "0"),
                PDoc("keepEigenVectors",
                     "whether the eigen vectors should be added as descriptors to the resulting cloud", "0")};
    }
    T ratio;
    unsigned knn, samplingMethod;
    T maxBoxDim;
    bool averageExistingDescriptors, keepNormals, keepDensities, keepEigenValues, keepEigenVectors;
    explicit SamplingSurfaceNormalDPF(const Parametrizable::Parameters& p)
        : PM<T>::DataPointsFilter("SamplingSurfaceNormalDataPointsFilter", doc(), p),
          ratio(this->template get<T>("ratio")),
          knn(this->template get<unsigned>("knn")),
          samplingMethod(this->template get<unsigned>("samplingMethod")),
          maxBoxDim(this->template get<T>("maxBoxDim")),
          averageExistingDescriptors(this->template get<bool>("averageExistingDescriptors")),
          keepNormals(this->template get<bool>("keepNormals")),
          keepDensities(this->template get<bool>("keepDensities")),
          keepEigenValues(this->template get<bool>("keepEigenValues")),
          keepEigenVectors(this->template get<bool>("keepEigenVectors")) {}
    bool usesRandState() const override { return samplingMethod == 0; }
    void inPlaceFilter(DataPoints<T>& cloud) override {
        const int D = cloud.rows - 1;
        const int64_t n = cloud.n;
        if (averageExistingDescriptors) {  // (:93-101)
            int sum = 0;
            for (auto& l : cloud.descriptorLabels) sum += l.span;
            if (sum != cloud.descDim)
                throw InvalidParameter("SamplingSurfaceNormalDataPointsFilter: Error, descriptor labels do not match "
                                       "descriptor data");
        }
        std::vector<T> feat((size_t)(n * cloud.rows)), desc((size_t)(n * cloud.descDim)), nrm, dens, eva, eve;
        if (keepNormals) nrm.resize((size_t)(n * D));
        if (keepDensities) dens.resize((size_t)n);
        if (keepEigenValues) eva.resize((size_t)(n * D));
        if (keepEigenVectors) eve.resize((size_t)(n * D * D));
        auto ptr = [](std::vector<T>& v) { return v.empty() ? nullptr : (void*)v.data(); };
        unsigned flags = (keepNormals ? PMX_SSN_NORMALS : 0u) | (keepDensities ? PMX_SSN_DENSITIES : 0u) |
                         (keepEigenValues ? PMX_SSN_EIGVALUES : 0u) | (keepEigenVectors ? PMX_SSN_EIGVECTORS : 0u) |
                         (averageExistingDescriptors ? PMX_SSN_AVERAGE : 0u);
        int64_t nout = 0, unfit = 0;
        const int rc = pmx_sampling_surface_normals(
            this->device, dtype_of<T>(), cloud.features.data(), cloud.rows, n,
            cloud.descDim ? cloud.descriptors.data() : nullptr, cloud.descDim,
            (int)std::min<unsigned>(knn, 0x7fffffffu), (int)samplingMethod, (double)ratio, (double)maxBoxDim, flags,
            feat.data(), ptr(desc), ptr(nrm), ptr(dens), ptr(eva), ptr(eve), &nout, &unfit);
        if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
        if (rc) throw std::runtime_error(std::string("SamplingSurfaceNormalDataPointsFilter: ") + pmx_last_error(nullptr));
        cloud.n = nout;
        feat.resize((size_t)(nout * cloud.rows));
        cloud.features.swap(feat);
        desc.resize((size_t)(nout * cloud.descDim));
        cloud.descriptors.swap(desc);
        if (keepNormals) cloud.setDescriptor("normals", D, nrm.data());
        if (keepDensities) cloud.setDescriptor("densities", 1, dens.data());
        if (keepEigenValues) cloud.setDescriptor("eigValues", D, eva.data());
        if (keepEigenVectors) cloud.setDescriptor("eigVectors", D * D, eve.data());
    }
};

// no-op stand-in accepting a reference module's parameters (reads them all so
// the "set but not used" check passes)
template <typename Base>
struct NoOp : Base {
    NoOp(const std::string& name, const Parametrizable::ParametersDoc& d, const Parametrizable::Parameters& p)
        : Base(name, d, p) {
        for (auto& pd : d) this->getParamValueString(pd.name);
    }
};

template <typename T>
Parametrizable::ParametersDoc perf_doc() {
    return {PDoc("baseFileName", "base file name for the statistics files (if empty, disabled)", ""),
            PDoc("dumpPerfOnExit", "dump performance statistics to stderr on exit", "0"),
            PDoc("dumpStats", "dump the statistics on first and last step", "0")};
}
template <typename T>
Parametrizable::ParametersDoc vtk_doc() {
    return {PDoc("baseFileName", "base file name for the VTK files ", "point-matcher-output"),
            PDoc("dumpPerfOnExit", "dump performance statistics to stderr on exit", "0"),
            PDoc("dumpStats", "dump the statistics on first and last step", "0"),
            PDoc("dumpIterationInfo", "dump iteration info", "0"),
            PDoc("dumpDataLinks", "dump data links at each iteration", "0"),
            PDoc("dumpReading", "dump the reading cloud at each iteration", "0"),
            PDoc("dumpReference", "dump the reference cloud at each iteration", "0"),
            PDoc("writeBinary", "write binary VTK files", "0")};
}
inline Parametrizable::ParametersDoc filelogger_doc() {
    return {PDoc("infoFileName", "name of the file to output infos to", ""),
            PDoc("warningFileName", "name of the file to output warnings to", ""),
            PDoc("displayLocation", "display the location of message in source code", "0")};
}

}  // namespace

// --------------------------------------------------------------- registry --
template <typename T>
PointMatcher<T>::PointMatcher() {
    typedef Parametrizable::Parameters Ps;
    MatcherRegistrar.reg("KDTreeMatcher", [](const Ps& p) { return std::make_shared<KDTreeMatcherGPU<T>>(p); }, true,
                         "This matcher matches a point from the reading to its closest neighbors in the reference.");
    MatcherRegistrar.reg("KDTreeVarDistMatcher",
                         [](const Ps& p) { return std::make_shared<KDTreeVarDistMatcherGPU<T>>(p); }, true,
                         "This matcher matches a point from the reading to its closest neighbors in the reference. A "
                         "maximum search radius per point can be defined.");
    OutlierFilterRegistrar.reg("NullOutlierFilter", [](const Ps& p) { return std::make_shared<NullOF<T>>(p); }, false);
    OutlierFilterRegistrar.reg("MaxDistOutlierFilter", [](const Ps& p) { return std::make_shared<MaxDistOF<T>>(p); }, true);
    OutlierFilterRegistrar.reg("MinDistOutlierFilter", [](const Ps& p) { return std::make_shared<MinDistOF<T>>(p); }, true);
    OutlierFilterRegistrar.reg("MedianDistOutlierFilter", [](const Ps& p) { return std::make_shared<MedianDistOF<T>>(p); },
                               true);
    OutlierFilterRegistrar.reg("TrimmedDistOutlierFilter", [](const Ps& p) { return std::make_shared<TrimmedDistOF<T>>(p); },
                               true);
    OutlierFilterRegistrar.reg("VarTrimmedDistOutlierFilter",
                               [](const Ps& p) { return std::make_shared<VarTrimmedDistOF<T>>(p); }, true);
    OutlierFilterRegistrar.reg("RobustOutlierFilter", [](const Ps& p) { return std::make_shared<RobustOF<T>>(p); },
                               true);
    OutlierFilterRegistrar.reg("SurfaceNormalOutlierFilter",
                               [](const Ps& p) { return std::make_shared<SurfaceNormalOF<T>>(p); }, true);
    OutlierFilterRegistrar.reg("GenericDescriptorOutlierFilter",
                               [](const Ps& p) { return std::make_shared<GenericDescriptorOF<T>>(p); }, true);
    ErrorMinimizerRegistrar.reg("PointToPlaneErrorMinimizer",
                                [](const Ps& p) { return std::make_shared<PointToPlaneEM<T>>(p); }, true);
    ErrorMinimizerRegistrar.reg("PointToPlaneWithCovErrorMinimizer",
                                [](const Ps& p) { return std::make_shared<PointToPlaneWithCovEM<T>>(p); }, true);
    ErrorMinimizerRegistrar.reg("PointToPointErrorMinimizer",
                                [](const Ps& p) { return std::make_shared<PointToPointEM<T>>(p); }, false);
    ErrorMinimizerRegistrar.reg("PointToPointSimilarityErrorMinimizer",
                                [](const Ps& p) { return std::make_shared<PointToPointSimilarityEM<T>>(p); }, false);
    TransformationCheckerRegistrar.reg("CounterTransformationChecker",
                                       [](const Ps& p) { return std::make_shared<CounterTC<T>>(p); }, true);
    TransformationCheckerRegistrar.reg("DifferentialTransformationChecker",
                                       [](const Ps& p) { return std::make_shared<DifferentialTC<T>>(p); }, true);
    TransformationCheckerRegistrar.reg("BoundTransformationChecker",
                                       [](const Ps& p) { return std::make_shared<BoundTC<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("IdentityDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<IdentityDPF<T>>(p); }, false);
    DataPointsFilterRegistrar.reg("SurfaceNormalDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<SurfaceNormalDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("RandomSamplingDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<RandomSamplingDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("BoundingBoxDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<BoundingBoxDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("FixStepSamplingDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<FixStepSamplingDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("MaxDistDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<DistDPF<T, true>>(p); }, true);
    DataPointsFilterRegistrar.reg("MinDistDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<DistDPF<T, false>>(p); }, true);
    DataPointsFilterRegistrar.reg("SimpleSensorNoiseDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<SimpleSensorNoiseDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("ObservationDirectionDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<ObservationDirectionDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("OrientNormalsDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<OrientNormalsDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("DistanceLimitDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<DistanceLimitDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("VoxelGridDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<VoxelGridDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("OctreeGridDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<OctreeGridDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("NormalSpaceDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<NormalSpaceDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("CovarianceSamplingDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<CovarianceSamplingDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("SamplingSurfaceNormalDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<SamplingSurfaceNormalDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("ShadowDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<ShadowDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("MaxQuantileOnAxisDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<MaxQuantileOnAxisDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("RemoveNaNDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<RemoveNaNDPF<T>>(p); }, false);
    DataPointsFilterRegistrar.reg("CutAtDescriptorThresholdDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<CutAtDescriptorThresholdDPF<T>>(p); },
                                  true);
    DataPointsFilterRegistrar.reg("IncidenceAngleDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<IncidenceAngleDPF<T>>(p); }, false);
    DataPointsFilterRegistrar.reg("RemoveSensorBiasDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<RemoveSensorBiasDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("SphericalityDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<SphericalityDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("MaxDensityDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<MaxDensityDPF<T>>(p); }, true);
    DataPointsFilterRegistrar.reg("MaxPointCountDataPointsFilter",
                                  [](const Ps& p) { return std::make_shared<MaxPointCountDPF<T>>(p); }, true);
    InspectorRegistrar.reg("NullInspector", [](const Ps& p) {
        return std::make_shared<NoOp<Inspector>>("NullInspector", Parametrizable::ParametersDoc(), p);
    }, false);
    InspectorRegistrar.reg("PerformanceInspector", [](const Ps& p) {
        return std::make_shared<NoOp<Inspector>>("PerformanceInspector", perf_doc<T>(), p);
    }, true);
    InspectorRegistrar.reg("VTKFileInspector", [](const Ps& p) {
        return std::make_shared<NoOp<Inspector>>("VTKFileInspector", vtk_doc<T>(), p);
    }, true);
    LoggerRegistrar.reg("NullLogger", [](const Ps& p) {
        return std::make_shared<NoOp<Logger>>("NullLogger", Parametrizable::ParametersDoc(), p);
    }, false);
    LoggerRegistrar.reg("FileLogger", [](const Ps& p) {
        return std::make_shared<NoOp<Logger>>("FileLogger", filelogger_doc(), p);
    }, true);
    registerTransformations();
}

template <typename T>
const PointMatcher<T>& PointMatcher<T>::get() {
    static const PointMatcher<T> instance;
    return instance;
}

template <typename T>
void PointMatcher<T>::ErrorMinimizer::setStats(const pmx_stats& st) {
    const double kn = (double)st.n_total;
    keptPoints = st.kept;
    pointUsedRatio = (T)((double)st.kept / kn);
    weightedPointUsedRatio = (T)(st.sum_w / kn);
    nbRejectedMatches = st.rejected_matches;
    nbRejectedPoints = st.rejected_points;
    lastVisited = st.visited;
}

template <typename T>
void PointMatcher<T>::OutlierFilters::compute(Device& dev, const Matches& m) {
    if (this->empty()) {
        dev.check(pmx_outlier_default(dev.ctx));
        return;
    }
    int pos = 0;
    for (auto& f : *this) f->compute(dev, m, pos++);
}

template <typename T>
void PointMatcher<T>::TransformationCheckers::init(const TransformationParameters& T_, int rows, bool& iterate) {
    for (auto& c : *this) c->init(T_, rows, iterate);
}
template <typename T>
void PointMatcher<T>::TransformationCheckers::check(const TransformationParameters& T_, int rows, bool& iterate) {
    for (auto& c : *this) c->check(T_, rows, iterate);
}

// ==================================================================== ICP ==
template <typename T>
PointMatcher<T>::ICP::ICP(int device) {
    dev.device = device;
    dev.dtype = dtype_of<T>();
    if (const char* e = std::getenv("PMX_DEVICE_LOOP")) deviceLoop = std::strcmp(e, "0") != 0;
}

template <typename T>
void PointMatcher<T>::ICP::cleanup() {
    readingDataPointsFilters.clear();
    readingStepDataPointsFilters.clear();
    referenceDataPointsFilters.clear();
    matcher.reset();
    outlierFilters.clear();
    errorMinimizer.reset();
    transformationCheckers.clear();
    inspector.reset();
}

template <typename T>
void PointMatcher<T>::ICP::setDefault() {
    // ICP.cpp:99-113: RandomSampling (prob 0.75) on the reading,
    // SamplingSurfaceNormal on the reference, TrimmedDist, KDTreeMatcher,
    // PointToPlane, Counter + Differential, NullInspector.
    cleanup();
    const PointMatcher& pm = PointMatcher::get();
    readingDataPointsFilters.push_back(pm.DataPointsFilterRegistrar.create("RandomSamplingDataPointsFilter"));
    referenceDataPointsFilters.push_back(pm.DataPointsFilterRegistrar.create("SamplingSurfaceNormalDataPointsFilter"));
    outlierFilters.push_back(pm.OutlierFilterRegistrar.create("TrimmedDistOutlierFilter"));
    matcher = pm.MatcherRegistrar.create("KDTreeMatcher");
    errorMinimizer = pm.ErrorMinimizerRegistrar.create("PointToPlaneErrorMinimizer");
    transformationCheckers.push_back(pm.TransformationCheckerRegistrar.create("CounterTransformationChecker"));
    transformationCheckers.push_back(pm.TransformationCheckerRegistrar.create("DifferentialTransformationChecker"));
    inspector = pm.InspectorRegistrar.create("NullInspector");
    reinitMap();  // ICPSequence::setDefault, ICP.cpp:520-528
}

template <typename T>
void PointMatcher<T>::ICP::loadFromYaml(const std::string& text) {
    cleanup();
    const YNode doc = parse_yaml(text);
    if (doc.kind != YNode::Map && doc.kind != YNode::Null) throw ConfigurationError("YAML chain must be a map");
    const PointMatcher& pm = PointMatcher::get();
    std::set<std::string> used;
    auto many = [&](const std::string& key, auto& reg, auto& vec) {
        used.insert(key);
        const YNode* n = doc.find(key);
        if (!n) return;
        for (const YNode& item : n->seq) vec.push_back(reg.createFromYAML(item));
    };
    auto one = [&](const std::string& key, auto& reg, auto& ptr) {
        used.insert(key);
        const YNode* n = doc.find(key);
        if (n)
            ptr = reg.createFromYAML(*n);
        else
            ptr.reset();
    };
    one("logger", pm.LoggerRegistrar, logger);  // ICP.cpp:131-135 (logger first)
    many("readingDataPointsFilters", pm.DataPointsFilterRegistrar, readingDataPointsFilters);
    many("readingStepDataPointsFilters", pm.DataPointsFilterRegistrar, readingStepDataPointsFilters);
    many("referenceDataPointsFilters", pm.DataPointsFilterRegistrar, referenceDataPointsFilters);
    one("matcher", pm.MatcherRegistrar, matcher);
    many("outlierFilters", pm.OutlierFilterRegistrar, outlierFilters);
    one("errorMinimizer", pm.ErrorMinimizerRegistrar, errorMinimizer);
    many("transformationCheckers", pm.TransformationCheckerRegistrar, transformationCheckers);
    one("inspector", pm.InspectorRegistrar, inspector);
    for (const auto& kv : doc.map)  // ICP.cpp:158-166
        if (!used.count(kv.first)) throw InvalidModuleType("Module type " + kv.first + " does not exist");
    reinitMap();  // ICPSequence::loadFromYaml, ICP.cpp:530-539
}

template <typename T>
typename PointMatcher<T>::TransformationParameters PointMatcher<T>::ICP::operator()(const DataPoints& reading,
                                                                                     const DataPoints& reference) {
    const int dim = reading.rows;
    TransformationParameters I((size_t)dim * dim, (T)0);
    for (int i = 0; i < dim; ++i) I[i * dim + i] = 1;
    return compute(reading, reference, I);
}

template <typename T>
typename PointMatcher<T>::TransformationParameters PointMatcher<T>::ICP::compute(
    const DataPoints& reading, const DataPoints& reference, const TransformationParameters& T_init) {
    prepare(reading, reference, T_init);
    while (iterate(1 << 30)) {
    }
    return finish();
}

template <typename T>
static double since(const std::chrono::steady_clock::time_point& t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

// a caller's cloud as a shared pointer that owns nothing (the caller keeps it alive)
template <typename C>
static std::shared_ptr<const C> borrowed_cloud(const C& c) {
    return std::shared_ptr<const C>(std::shared_ptr<const C>(), &c);
}

template <typename T>
void PointMatcher<T>::ICP::prepare(const DataPoints& readingIn, const DataPoints& referenceIn,
                                   const TransformationParameters& T_init) {
    prepare(borrowed_cloud(readingIn), borrowed_cloud(referenceIn), T_init);
}

template <typename T>
void PointMatcher<T>::ICP::prepare(std::shared_ptr<const DataPoints> readingPtr,
                                   std::shared_ptr<const DataPoints> referencePtr,
                                   const TransformationParameters& T_init) {
    const DataPoints& referenceIn = *referencePtr;
    filteredReading_.reset();  // (readingTransformed: the last compute's reading goes with its reference frame)
    readingResident_ = loopOwnT_ = false;
    // ICP::compute, ICP.cpp:265-313
    if (!matcher) throw std::runtime_error("You must setup a matcher before running ICP");
    if (!errorMinimizer) throw std::runtime_error("You must setup an error minimizer before running ICP");
    if (!inspector) throw std::runtime_error("You must setup an inspector before running ICP");
    auto t = std::chrono::steady_clock::now();
    const int dim = referenceIn.rows;
    if (dim != 3 && dim != 4) throw std::runtime_error("clouds must be 2-D or 3-D (3 or 4 homogeneous rows)");
    if (dev.sharded())  // (every rank filters its own reading shard)
        for (const DataPointsFilters* chain :
             {&readingDataPointsFilters, &readingStepDataPointsFilters, &referenceDataPointsFilters})
            for (const auto& f : *chain)
                if (f->usesRandState())
                    throw ConfigurationError(f->className + " draws from the process's rand() state: it cannot run on "
                                             "the reading shards of a multi-rank ICP");
    for (auto& f : referenceDataPointsFilters) f->device = dev.device;
    for (auto& f : readingDataPointsFilters) f->device = dev.device;
    // (no reference filters: the caller's cloud is uploaded as it is and
    // centred on the device — no host copy of the reference)
    const bool filtered = !referenceDataPointsFilters.empty();
    if (filtered) {  // (the one filtered copy, kept for getErrorElements' gathers)
        auto refCopy = std::make_shared<DataPoints>(referenceIn);
        referenceDataPointsFilters.init();
        referenceDataPointsFilters.apply(*refCopy);
        referencePtr = std::move(refCopy);
    }
    const DataPoints& reference = *referencePtr;
    elemReference_.reset();
    const int64_t M = reference.n;
    if (M <= 0) throw ConvergenceError("empty reference");
    // mean of the reference columns in T, ICP.cpp:291-292 (each coordinate's
    // sum sequential in point order), computed by the matcher's init on a
    // host thread while the cloud uploads (pmx_set_reference_mean_centred)
    T_refIn_refMean_.assign((size_t)dim * dim, (T)0);
    for (int i = 0; i < dim; ++i) T_refIn_refMean_[i * dim + i] = 1;
    T mean[3] = {0, 0, 0};
    check_outlier_reference<T>(outlierFilters, reference);
    dev.ensure();
    mapIndexed_ = false;  // (an ICPSequence map is no longer the device's reference, even if init throws)
    matcher->init(dev, reference, nullptr, mean);  // ICP.cpp:302 (features - mean, ICP.cpp:299, on the device)
    keepReferenceDescriptors(reference);
    for (int r = 0; r < dim - 1; ++r) T_refIn_refMean_[r * dim + dim - 1] = mean[r];
    referencePreprocessingDuration = since<T>(t);
    prefilteredReferencePtsCount = M;
    elemReference_ = std::move(referencePtr);
    prepareReading(std::move(readingPtr), T_init);
}

// computeWithTransformedReference up to the loop, ICP.cpp:317-370
// (T_refIn_refMean_ and the matcher describe the reference)
template <typename T>
void PointMatcher<T>::ICP::prepareReading(std::shared_ptr<const DataPoints> readingPtr,
                                          const TransformationParameters& T_init) {
    const DataPoints& readingIn = *readingPtr;
    const int dim = (int)std::lround(std::sqrt((double)T_refIn_refMean_.size()));
    if ((int64_t)T_init.size() != (int64_t)dim * dim)
        throw std::runtime_error("The shape of initial transformation matrix must be NxN. Where N is the number of "
                                 "rows in the read/reference scans.");
    if (readingIn.rows != dim) throw std::runtime_error("reading and reference dimensions differ");
    const auto t = std::chrono::steady_clock::now();
    // (no reading filters: the caller's cloud directly, no host copy)
    if (!readingDataPointsFilters.empty()) {  // (the one filtered copy, kept for getErrorElements' gathers)
        auto readCopy = std::make_shared<DataPoints>(readingIn);
        readingDataPointsFilters.init();
        readingDataPointsFilters.apply(*readCopy);
        readingPtr = std::move(readCopy);
    }
    const DataPoints& reading = *readingPtr;
    elemReading_ = readingPtr;
    elemStep_ = elemNormalsPre_ = false;
    filteredReading_.reset();
    readingResident_ = loopOwnT_ = false;
    // T_refMean_dataIn = T_refIn_refMean^-1 * T_init (the inverse of a pure
    // translation is exact), ICP.cpp:345-346
    TransformationParameters inv((size_t)dim * dim, (T)0);
    for (int i = 0; i < dim; ++i) inv[i * dim + i] = 1;
    for (int r = 0; r < dim - 1; ++r) inv[r * dim + dim - 1] = -T_refIn_refMean_[r * dim + dim - 1];
    T_refMean_dataIn_.assign((size_t)dim * dim, (T)0);
    dense::matmul(inv.data(), T_init.data(), dim, T_refMean_dataIn_.data());
    // (RigidTransformation::compute's check, TransformationsImpl.cpp:62-63; a
    // SimilarityTransformation checks nothing, :197-203)
    if (!similarityTransformation() &&
        std::fabs((T)1 - dense::det_rot(T_refMean_dataIn_.data(), dim)) > (T)0.001)
        throw TransformationError("RigidTransformation: Error, rotation matrix is not orthogonal.");
    // transformations.apply(reading, T_refMean_dataIn): done on the device
    dev.check(pmx_set_reading(dev.ctx, reading.feat(), dim, reading.n, T_refMean_dataIn_.data()));
    filteredReading_ = readingPtr;  // (readingTransformed: the device holds it in <refMean> until a step filter's upload)
    readingResident_ = true;
    matcher->initReading(dev, reading);  // (per-reading matcher inputs: KDTreeVarDistMatcher's radii)
    uploadReadingNormals(reading);       // (SurfaceNormalOutlierFilter; rotated by T_refMean_dataIn on the device)
    keepReadingNoise(reading);
    errorMinimizer->quality_.stopped = errorMinimizer->quality_.valid = false;  // (a new compute: the cache goes)
    errorMinimizer->elements_ = typename ErrorMinimizer::Elements();
    // readingStepDataPointsFilters (ICP.cpp:349-350, 373-377): the step
    // filters see the reading in <refMean> every iteration; keep that copy on
    // the host (the device's transform, restated: the same separately rounded
    // terms in the same order) — each iteration filters it and uploads the result
    stepBase_ = DataPoints();
    if (!readingStepDataPointsFilters.empty()) {
        stepBase_ = reading;
        const int D = dim - 1;
        for (int64_t j = 0; j < reading.n; ++j) {
            const T* f = reading.feat() + (size_t)j * dim;
            T* o = &stepBase_.features[(size_t)j * dim];
            for (int r = 0; r < D; ++r) {
                const T* m = &T_refMean_dataIn_[(size_t)r * dim];
                T v = m[0] * f[0];
                v = v + m[1] * f[1];
                v = v + (D == 3 ? m[2] * f[2] : (T)0 * (T)0);
                v = v + m[D] * f[D];
                o[r] = v;
            }
        }
        // (its normals as the reference's transformation leaves them: the
        // rotation block applied in T, the same terms as the device's upload)
        bool wantNormals = false;
        for (auto& f : outlierFilters) wantNormals = wantNormals || f->needsReadingNormals();
        if (wantNormals && stepBase_.descriptorExists("normals")) {
            int span = 0;
            std::vector<T> nr = stepBase_.descriptor("normals", &span);
            if (span == D) {
                const T* m = T_refMean_dataIn_.data();
                for (int64_t j = 0; j < stepBase_.n; ++j) {
                    T* v = &nr[(size_t)j * D];
                    T o[3] = {0, 0, 0};
                    for (int r = 0; r < D; ++r) {
                        T s = m[r * dim + 0] * v[0] + m[r * dim + 1] * v[1];
                        if (D == 3) s = s + m[r * dim + 2] * v[2];
                        o[r] = s;
                    }
                    for (int r = 0; r < D; ++r) v[r] = o[r];
                }
                stepBase_.setDescriptor("normals", span, nr.data());
                elemNormalsPre_ = true;
            }
        }
        for (auto& f : readingStepDataPointsFilters) f->device = dev.device;
        readingStepDataPointsFilters.init();
    }
    rows_ = dim;
    T_iter_.assign((size_t)dim * dim, (T)0);
    for (int i = 0; i < dim; ++i) T_iter_[i * dim + i] = 1;
    iterate_ = true;
    maxNumIterationsReached = false;
    transformationCheckers.init(T_iter_, dim, iterate_);
    iterationCount = 0;
    trace.clear();
    loopMode_ = 0;
    loopIters_ = 0;
    loopTouched_ = 0;
    readingPreprocessingDuration = since<T>(t);
    prefilteredReadingPtsCount = reading.n;
    t0_ = std::chrono::steady_clock::now();
}

// ------------------------------------------------------------ ICPSequence --
template <typename T>
bool PointMatcher<T>::ICP::setMap(const DataPoints& inputCloud) {
    // ICP.cpp:464-508
    if (!matcher) throw std::runtime_error("You must setup a matcher before running ICP");
    if (!inspector) throw std::runtime_error("You must setup an inspector before running ICP");
    auto t = std::chrono::steady_clock::now();
    const int dim = inputCloud.rows;
    const int64_t ptCount = inputCloud.n;
    if (ptCount == 0) return false;  // "Ignoring attempt to create a map from an empty cloud"
    if (dim != 3 && dim != 4) throw std::runtime_error("clouds must be 2-D or 3-D (3 or 4 homogeneous rows)");
    if (dev.sharded())
        for (const auto& f : referenceDataPointsFilters)
            if (f->usesRandState())
                throw ConfigurationError(f->className + " draws from the process's rand() state: it cannot run on "
                                         "the reading shards of a multi-rank ICP");
    // the new map is built in locals and committed only once it is indexed:
    // a filter or Matcher::init that throws leaves the previous map (or none),
    // and mapIndexed_ false — the device reference may be half replaced
    mapIndexed_ = false;
    DataPoints map(inputCloud);
    // the mean of the map BEFORE the reference filters (ICP.cpp:490-497; ICP::compute
    // filters first), sequential sums in T as prepare
    TransformationParameters T_map((size_t)dim * dim, (T)0);
    for (int i = 0; i < dim; ++i) T_map[i * dim + i] = 1;
    for (int r = 0; r < dim - 1; ++r) {
        T s = 0;
        for (int64_t j = 0; j < ptCount; ++j) s = s + map.features[j * dim + r];
        const T mean = s / (T)ptCount;
        T_map[r * dim + dim - 1] = mean;
        for (int64_t j = 0; j < ptCount; ++j) map.features[j * dim + r] = map.features[j * dim + r] - mean;
    }
    for (auto& f : referenceDataPointsFilters) f->device = dev.device;
    referenceDataPointsFilters.init();
    referenceDataPointsFilters.apply(map);
    if (map.n <= 0) throw ConvergenceError("empty reference");
    check_outlier_reference<T>(outlierFilters, map);
    dev.ensure();
    matcher->init(dev, map);  // ICP.cpp:503 (the grid stays on the device)
    keepReferenceDescriptors(map);
    if (errorMinimizer) errorMinimizer->quality_.stopped = errorMinimizer->quality_.valid = false;
    if (errorMinimizer) errorMinimizer->elements_ = typename ErrorMinimizer::Elements();
    elemReference_.reset();
    map_ = std::move(map);
    T_map_ = std::move(T_map);
    mapIndexed_ = true;
    referencePreprocessingDuration = since<T>(t);  // (SetMapDuration)
    prefilteredReferencePtsCount = map_.n;
    return true;
}

template <typename T>
void PointMatcher<T>::ICP::clearMap() {
    if (errorMinimizer) errorMinimizer->elements_ = typename ErrorMinimizer::Elements();
    elemReference_.reset();
    map_ = DataPoints();
    T_map_.clear();
    mapIndexed_ = false;
}

template <typename T>
typename PointMatcher<T>::DataPoints PointMatcher<T>::ICP::getPrefilteredMap() const {
    DataPoints g(map_);
    if (hasMap()) {
        const int dim = map_.rows;
        for (int r = 0; r < dim - 1; ++r) {
            const T m = T_map_[r * dim + dim - 1];
            for (int64_t j = 0; j < g.n; ++j) g.features[j * dim + r] = g.features[j * dim + r] + m;
        }
    }
    return g;
}

template <typename T>
void PointMatcher<T>::ICP::reinitMap() {
    if (!hasMap() || !matcher) return;
    dev.ensure();
    matcher->init(dev, map_);
    keepReferenceDescriptors(map_);
    mapIndexed_ = true;
}

template <typename T>
bool PointMatcher<T>::ICP::prepareSequence(const DataPoints& readingIn, const TransformationParameters& T_init) {
    return prepareSequence(borrowed_cloud(readingIn), T_init);
}

template <typename T>
bool PointMatcher<T>::ICP::prepareSequence(std::shared_ptr<const DataPoints> readingIn,
                                           const TransformationParameters& T_init) {
    if (!hasMap()) return false;  // "Ignoring attempt to perform ICP with an empty map"
    if (!matcher) throw std::runtime_error("You must setup a matcher before running ICP");
    if (!errorMinimizer) throw std::runtime_error("You must setup an error minimizer before running ICP");
    if (!inspector) throw std::runtime_error("You must setup an inspector before running ICP");
    if (dev.sharded())
        for (const auto& f : readingDataPointsFilters)
            if (f->usesRandState())
                throw ConfigurationError(f->className + " draws from the process's rand() state: it cannot run on "
                                         "the reading shards of a multi-rank ICP");
    if (dev.sharded())
        for (const auto& f : readingStepDataPointsFilters)
            if (f->usesRandState())
                throw ConfigurationError(f->className + " draws from the process's rand() state: it cannot run on "
                                         "the reading shards of a multi-rank ICP");
    for (auto& f : readingDataPointsFilters) f->device = dev.device;
    if (!mapIndexed_) reinitMap();  // (a plain compute replaced the device's reference)
    T_refIn_refMean_ = T_map_;
    elemReference_ = borrowed_cloud(map_);  // (the held map: dropped by setMap / clearMap)
    prepareReading(std::move(readingIn), T_init);
    return true;
}

template <typename T>
typename PointMatcher<T>::TransformationParameters PointMatcher<T>::ICP::computeSequence(
    const DataPoints& reading, const TransformationParameters& T_init) {
    if (!prepareSequence(reading, T_init)) {
        const int dim = reading.rows;
        TransformationParameters I((size_t)dim * dim, (T)0);
        for (int i = 0; i < dim; ++i) I[i * dim + i] = 1;
        return I;
    }
    while (iterate(1 << 30)) {
    }
    return finish();
}

template <typename T>
bool PointMatcher<T>::ICP::step() {
    return iterate(1);
}

template <typename T>
void PointMatcher<T>::ICP::uploadReadingNormals(const DataPoints& reading) {
    bool want = false;
    for (auto& f : outlierFilters) want = want || f->needsReadingNormals();
    if (!want || !reading.descriptorExists("normals")) return;  // (pmx_set_reading cleared the last reading's)
    int span = 0;
    const std::vector<T> nr = reading.descriptor("normals", &span);
    if (span != reading.rows - 1)
        throw InvalidElement("SurfaceNormalOutlierFilter: descriptor normals must have " +
                             std::to_string(reading.rows - 1) + " rows, not " + std::to_string(span));
    dev.check(pmx_set_reading_normals(dev.ctx, nr.data()));
}

template <typename T>
void PointMatcher<T>::ICP::keepReadingNoise(const DataPoints& reading) {
    rdNoise_.clear();
    if (!reading.descriptorExists("simpleSensorNoise")) return;
    int span = 0;
    std::vector<T> v = reading.descriptor("simpleSensorNoise", &span);
    if (span != 1) throw InvalidElement("descriptor simpleSensorNoise must have 1 row, not " + std::to_string(span));
    rdNoise_ = std::move(v);
}

template <typename T>
void PointMatcher<T>::ICP::keepReferenceDescriptors(const DataPoints& reference) {
    // (the matcher has just indexed this cloud: the filters' device inputs from it)
    for (auto& f : outlierFilters) f->initReference(dev, reference);
    refNoise_.reset();
    refDens_.reset();
    for (const char* name : {"simpleSensorNoise", "densities"}) {
        if (!reference.descriptorExists(name)) continue;
        int span = 0;
        std::vector<T> v = reference.descriptor(name, &span);
        if (span != 1)
            throw InvalidElement(std::string("descriptor ") + name + " must have 1 row, not " + std::to_string(span));
        (name[0] == 's' ? refNoise_ : refDens_) = std::make_shared<const std::vector<T>>(std::move(v));
    }
}

// a checker stopped the loop: the last match stays resident until the next
// prepare / setMap, and the minimiser may be asked about it
template <typename T>
void PointMatcher<T>::ICP::stopped(bool deviceLoop) {
    auto& q = errorMinimizer->quality_;
    q.dev = &dev;
    q.stopped = true;
    q.loop = deviceLoop;
    q.valid = false;
    q.readingNoise = rdNoise_;
    q.refNoise = refNoise_;
    q.refDens = refDens_;
    auto& e = errorMinimizer->elements_;
    e = typename ErrorMinimizer::Elements();
    e.dev = &dev;
    e.stopped = true;
    e.loop = deviceLoop;
    e.reading = elemReading_;
    e.reference = elemReference_;
    e.T_pre = T_refMean_dataIn_;
    e.normalsPre = elemStep_ && elemNormalsPre_;
    e.rows = rows_;
}

// every descriptor of src's points idx[0, P), point-major, into dst
template <typename T>
static void gather_descriptors(const DataPoints<T>& src, const std::vector<int32_t>& idx, DataPoints<T>& dst) {
    dst.descriptorLabels = src.descriptorLabels;
    dst.descDim = src.descDim;
    dst.descriptors.resize((size_t)src.descDim * idx.size());
    const T* d = src.desc();
    for (size_t j = 0; j < idx.size(); ++j) {
        if (idx[j] < 0 || (int64_t)idx[j] >= src.n)
            throw std::runtime_error("getErrorElements: a column's index lies outside the filtered cloud");
        std::memcpy(&dst.descriptors[j * src.descDim], d + (size_t)idx[j] * src.descDim, sizeof(T) * src.descDim);
    }
}

// the rotation block of M (rows x rows) applied to the D-vectors of descriptor
// `name`, each component (m0 n0 + m1 n1) + m2 n2 in T (TransformationsImpl.cpp:72-84)
template <typename T>
static void rotate_descriptor(DataPoints<T>& c, const char* name, const T* M, int rows) {
    const int D = rows - 1;
    int off = 0;
    for (auto& l : c.descriptorLabels) {
        if (l.text == name && l.span == D) {
            for (int64_t j = 0; j < c.n; ++j) {
                T* v = &c.descriptors[(size_t)j * c.descDim + off];
                T o[3] = {0, 0, 0};
                for (int r = 0; r < D; ++r) {
                    T s = M[r * rows + 0] * v[0] + M[r * rows + 1] * v[1];
                    if (D == 3) s = s + M[r * rows + 2] * v[2];
                    o[r] = s;
                }
                for (int r = 0; r < D; ++r) v[r] = o[r];
            }
            return;
        }
        off += l.span;
    }
}

template <typename T>
const typename PointMatcher<T>::ErrorMinimizer::ErrorElements& PointMatcher<T>::ErrorMinimizer::getErrorElements()
    const {
    Elements& s = elements_;
    if (!s.stopped || !s.dev || s.valid) return s.e;  // (empty before any compute)
    const Device& d = *s.dev;
    pmx_elements_info info;
    d.check(s.loop ? pmx_loop_error_elements_prepare(d.ctx, &info) : pmx_error_elements_prepare(d.ctx, nullptr, &info));
    const size_t P = (size_t)info.columns;
    const int rows = s.rows;
    ErrorElements e;
    e.reading.rows = e.reference.rows = rows;
    e.reading.n = e.reference.n = (int64_t)P;
    e.reading.features.resize(P * rows);
    e.reference.features.resize(P * rows);
    e.dists.resize(P);
    e.weights.resize(P);
    e.ids.resize(P);
    e.readingIndex.resize(P);
    d.check(pmx_error_elements(d.ctx, e.reading.features.data(), e.reference.features.data(), nullptr, e.dists.data(),
                               e.ids.data(), e.weights.data(), e.readingIndex.data(), nullptr));
    std::vector<T> Tm((size_t)rows * rows);
    d.check(pmx_get_step_transform(d.ctx, Tm.data()));
    e.nbRejectedMatches = info.rejected_matches;
    e.nbRejectedPoints = info.rejected_points;
    if (s.reading) {
        e.reading.featureLabels = s.reading->featureLabels;
        gather_descriptors<T>(*s.reading, e.readingIndex, e.reading);
        for (const char* name : {"normals", "observationDirections"}) {
            // (a step reading's normals may already carry T_refMean_dataIn's rotation: prepareReading)
            if (!(s.normalsPre && std::string(name) == "normals"))
                rotate_descriptor<T>(e.reading, name, s.T_pre.data(), rows);
            rotate_descriptor<T>(e.reading, name, Tm.data(), rows);
        }
    }
    if (s.reference) {
        e.reference.featureLabels = s.reference->featureLabels;
        gather_descriptors<T>(*s.reference, e.ids, e.reference);
    }
    s.e = std::move(e);
    s.valid = true;
    return s.e;
}

template <typename T>
const pmx_quality& PointMatcher<T>::ErrorMinimizer::quality() const {
    Quality& s = quality_;
    if (!s.stopped || !s.dev)  // PointToPlane.cpp:382-385, PointToPoint.cpp:126-129
        throw std::runtime_error("Error, last error element empty. Error minimizer needs to be called at least once "
                                 "before using this method.");
    if (s.valid) return s.q;
    const Device& d = *s.dev;
    d.check(pmx_set_reading_noise(d.ctx, s.readingNoise.empty() ? nullptr : s.readingNoise.data()));
    d.check(pmx_set_reference_descriptors(d.ctx, s.refNoise ? s.refNoise->data() : nullptr,
                                          s.refDens ? s.refDens->data() : nullptr));
    d.check(s.loop ? pmx_loop_quality(d.ctx, qualityKind(), &s.q)
                   : pmx_match_quality(d.ctx, nullptr, qualityKind(), &s.q));
    s.valid = true;
    return s.q;
}

template <typename T>
T PointMatcher<T>::ErrorMinimizer::getOverlap() const {
    if (qualityKind() < 0) return weightedPointUsedRatio;
    const pmx_quality& q = quality();
    if (q.branch == 0) return weightedPointUsedRatio;  // (no sensor noise: the reference's fallback)
    return (T)q.overlap_num / (T)q.overlap_den;        // PointToPlane.cpp:464, PointToPoint.cpp:151
}

template <typename T>
T PointMatcher<T>::ErrorMinimizer::getResidualError() const {
    if (qualityKind() < 0) return std::numeric_limits<T>::max();  // ErrorMinimizer.cpp:274-278
    return (T)quality().residual;
}

// every module's device form, or false (ICP.cpp:371-430 then runs through the
// module calls)
template <typename T>
bool PointMatcher<T>::ICP::loopConfig(pmx_loop_cfg& cfg) const {
    std::memset(&cfg, 0, sizeof(cfg));
    if (!matcher->loopConfig(cfg) || !errorMinimizer->loopConfig(cfg)) return false;
    if (outlierFilters.size() > 8 || transformationCheckers.size() > 8) return false;
    cfg.n_filters = (int)outlierFilters.size();
    for (size_t i = 0; i < outlierFilters.size(); ++i)
        if (!outlierFilters[i]->loopConfig(cfg, (int)i)) return false;
    cfg.n_checkers = (int)transformationCheckers.size();
    for (size_t i = 0; i < transformationCheckers.size(); ++i)
        if (!transformationCheckers[i]->loopConfig(cfg, (int)i)) return false;
    cfg.keep_trace = keepTrace ? 1 : 0;
    return true;
}

template <typename T>
bool PointMatcher<T>::ICP::iterate(int n) {
    if (!iterate_ || n <= 0) return iterate_;
    if (loopMode_ == 0) {  // first iterations after prepare: pick the mode
        loopMode_ = -1;
        pmx_loop_cfg cfg;
        // (step filters re-upload the reading every iteration: module calls)
        if (deviceLoop && readingStepDataPointsFilters.empty() && loopConfig(cfg)) {
            const int rc = pmx_loop_begin(dev.ctx, &cfg, T_iter_.data());
            if (rc == PMX_OK)
                loopMode_ = 1;
            else if (rc != PMX_E_BAD_PARAM)  // (BAD_PARAM: a configuration the loop does not take)
                dev.check(rc);
        }
    }
    if (loopMode_ < 0) {
        for (int i = 0; i < n && iterate_; ++i) stepModules();
        return iterate_;
    }
    pmx_loop_status st;
    std::memset(&st, 0, sizeof(st));
    const int rc = pmx_loop_run(dev.ctx, n, &st);
    if (rc != PMX_OK && st.error == 0) dev.check(rc);  // HIP / RCCL / state failure
    // mirror the device loop's state into the modules (what the per-module
    // calls would have left there)
    const int dim = rows_;
    const int64_t fresh = st.iterations - loopIters_;
    if (keepTrace && fresh > 0) {
        std::vector<T> buf((size_t)fresh * dim * dim);
        dev.check(pmx_loop_trace(dev.ctx, (int)loopIters_, (int)fresh, buf.data()));
        for (int64_t i = 0; i < fresh; ++i)
            trace.emplace_back(buf.begin() + i * dim * dim, buf.begin() + (i + 1) * dim * dim);
    }
    iterationCount += fresh;
    for (auto& f : outlierFilters) f->loopAdvance(fresh);
    loopIters_ = st.iterations;
    matcher->visitCounter += (uint64_t)(st.point_count_touched - loopTouched_);  // MatchersImpl.cpp:98
    loopTouched_ = st.point_count_touched;
    if (st.last.kept > 0) errorMinimizer->setStats(st.last);
    for (size_t i = 0; i < transformationCheckers.size(); ++i) {
        auto& cv = transformationCheckers[i]->conditionVariables;
        for (size_t j = 0; j < cv.size() && j < 2; ++j) cv[j] = (T)st.cond[i][j];
    }
    for (int i = 0; i < dim * dim; ++i) T_iter_[(size_t)i] = (T)st.T_iter[i];
    if (st.reason == 1) maxNumIterationsReached = true;
    if (st.done) iterate_ = false;
    if (rc != PMX_OK) dev.check(rc);  // the exception the loop raised
    loopOwnT_ = st.done != 0;  // (readingTransformed reads the finished loop's T_iter on the device)
    // (stopped by a checker: the last iteration's match is still resident,
    // nothing has replaced it yet)
    if (st.done && fresh > 0) {
        errorMinimizer->loopStopped(dev, dim, nullptr);
        stopped(true);
    }
    return iterate_;
}

template <typename T>
bool PointMatcher<T>::ICP::stepModules() {
    // one pass of the loop body, ICP.cpp:371-430
    if (!iterate_) return false;
    const int dim = rows_;
    if (!similarityTransformation() &&
        std::fabs((T)1 - dense::det_rot(T_iter_.data(), dim)) > (T)0.001)  // TransformationsImpl.cpp:62-63
        throw TransformationError("RigidTransformation: Error, rotation matrix is not orthogonal.");
    if (!readingStepDataPointsFilters.empty()) {  // ICP.cpp:373-377
        auto stepPtr = std::make_shared<DataPoints>(stepBase_);
        DataPoints& stepReading = *stepPtr;
        readingStepDataPointsFilters.apply(stepReading);
        elemReading_ = stepPtr;  // (the last iteration's is the one getErrorElements gathers from)
        elemStep_ = true;
        readingResident_ = false;  // (the device now holds the step reading)
        TransformationParameters I((size_t)dim * dim, (T)0);
        for (int i = 0; i < dim; ++i) I[(size_t)i * dim + i] = 1;
        dev.check(pmx_set_reading(dev.ctx, stepReading.features.data(), dim, stepReading.n, I.data()));
        matcher->initReading(dev, stepReading);
        uploadReadingNormals(stepReading);
        keepReadingNoise(stepReading);  // (the last iteration's is the one getOverlap reads)
    }
    const Matches matches = matcher->findClosests(dev, T_iter_);
    outlierFilters.compute(dev, matches);
    const TransformationParameters dT = errorMinimizer->compute(dev, dim);
    matcher->visitCounter += (uint64_t)errorMinimizer->lastVisited;  // MatchersImpl.cpp:98
    dense::matmul(dT.data(), T_iter_.data(), dim, T_iter_.data());
    try {
        transformationCheckers.check(T_iter_, dim, iterate_);
    } catch (const MaxNumIterationsReached&) {
        iterate_ = false;
        maxNumIterationsReached = true;
    }
    ++iterationCount;
    if (keepTrace) trace.push_back(T_iter_);
    // (the loop has stopped: this iteration's match is still resident)
    if (!iterate_) {
        errorMinimizer->loopStopped(dev, dim, dT.data());
        stopped(false);
    }
    return iterate_;
}

template <typename T>
typename PointMatcher<T>::TransformationParameters PointMatcher<T>::ICP::finish() {
    convergenceDuration = since<T>(t0_);
    return fullTransform();
}

template <typename T>
typename PointMatcher<T>::TransformationParameters PointMatcher<T>::ICP::fullTransform() const {
    const int dim = rows_;
    TransformationParameters tmp((size_t)dim * dim), out((size_t)dim * dim);
    dense::matmul(T_refIn_refMean_.data(), T_iter_.data(), dim, tmp.data());
    dense::matmul(tmp.data(), T_refMean_dataIn_.data(), dim, out.data());
    return out;  // ICP.cpp:448
}

template <typename T>
int64_t PointMatcher<T>::ICP::readingTransformedSize(int* rows) const {
    if (!filteredReading_ || rows_ == 0)
        throw std::runtime_error("readingTransformed: no compute has run on this object (state error)");
    if (rows) *rows = rows_;
    return filteredReading_->n;
}

template <typename T>
std::vector<T> PointMatcher<T>::ICP::readingTransformed(int64_t* n_out) {
    readingTransformedSize();
    const DataPoints& reading = *filteredReading_;
    const int dim = rows_;
    std::vector<T> out((size_t)dim * (size_t)reading.n);
    if (n_out) *n_out = reading.n;
    if (reading.n == 0) return out;
    if (readingResident_) {
        // T_refIn_refMean * (T_iter * resident): the mean added in the kernel
        T mean[3] = {0, 0, 0};
        for (int r = 0; r < dim - 1; ++r) mean[r] = T_refIn_refMean_[(size_t)r * dim + dim - 1];
        dev.check(pmx_transform_reading_offset(dev.ctx, loopOwnT_ ? nullptr : T_iter_.data(), mean, out.data(),
                                               nullptr));
    } else {
        const TransformationParameters Tf = fullTransform();
        const int rc = pmx_transform_cloud(dev.device, dtype_of<T>(), reading.feat(), dim, reading.n, Tf.data(),
                                           nullptr, 0, nullptr, 0, out.data(), nullptr, nullptr);
        if (rc != PMX_OK)
            throw std::runtime_error("readingTransformed: pmx error " + std::to_string(rc) + ": " +
                                     pmx_last_error(nullptr));
    }
    return out;
}

template struct PointMatcher<float>;
template struct PointMatcher<double>;

}  // namespace pm

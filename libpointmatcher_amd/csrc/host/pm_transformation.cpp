// pm_transformation.cpp — the Transformation modules of the host chain:
// RigidTransformation, SimilarityTransformation and PureTranslation
// (pointmatcher/TransformationsImpl.h:54-90, TransformationsImpl.cpp:49-272),
// registered under the reference's names (Registry.cpp:60-64; the reference
// constructs its SimilarityTransformation directly, ICP.cpp:145-148 — here it
// has a registrar entry like the other two).
//
// compute is the device's (pmx_transform_cloud, include/pmx.h): parameters *
// features, and the rotation block times every descriptor labelled "normals" or
// "observationDirections".  checkParameters and correctParameters are a few
// operations on a 3 x 3 or 4 x 4 matrix: host arithmetic in T, every multiply
// and add rounded on its own (the build's -ffp-contract=off), in the
// reference's expression order.
#include <cmath>
#include <cstring>

#include "pm_icp.h"

namespace pm {
namespace {

template <typename T>
using PM = PointMatcher<T>;

template <typename T>
int dtype_of() {
    return sizeof(T) == 8 ? PMX_F64 : PMX_F32;
}

// the side of a square row-major matrix, 0 when the size is no square
inline int side_of(size_t size) {
    const int r = (int)std::lround(std::sqrt((double)size));
    return (size_t)r * (size_t)r == size ? r : 0;
}

// normalized() of a column (Eigen 3.3 Dot.h): the squared norm a sequential
// sum, a zero vector left as it is
template <typename T>
void normalized3(const T* M, int rows, int col, T (&v)[3]) {
    for (int r = 0; r < 3; ++r) v[r] = M[r * rows + col];
    T z = v[0] * v[0];
    z = z + v[1] * v[1];
    z = z + v[2] * v[2];
    if (z > (T)0) {
        const T s = std::sqrt(z);
        for (int r = 0; r < 3; ++r) v[r] = v[r] / s;
    }
}
// a.cross(b) (Eigen OrthoMethods.h)
template <typename T>
void cross3(const T (&a)[3], const T (&b)[3], T (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// What the three classes share: the size checks, the label walk and the call.
// rotate: multiply the "normals" / "observationDirections" spans by the
// rotation block (Rigid, Similarity) or leave every descriptor alone
// (PureTranslation)
template <typename T>
typename PM<T>::DataPoints transform_cloud(const typename PM<T>::DataPoints& input, const std::vector<T>& parameters,
                                           bool rotate, int device, const std::string& who) {
    const int rows = input.rows, D = rows - 1;
    if ((int64_t)parameters.size() != (int64_t)rows * rows)
        throw InvalidParameter(who + ": the transformation parameters hold " + std::to_string(parameters.size()) +
                               " values, a cloud of " + std::to_string(rows) + " homogeneous rows needs " +
                               std::to_string(rows) + " x " + std::to_string(rows));
    std::vector<int> spans;
    if (rotate) {
        int row = 0;
        for (const auto& l : input.descriptorLabels) {
            if (l.text == "normals" || l.text == "observationDirections") {
                // (R * inputDesc with mismatched sizes: an Eigen assertion in the reference)
                if (l.span != D)
                    throw InvalidField(who + ": descriptor " + l.text + " has " + std::to_string(l.span) +
                                       " rows, the rotation of a " + std::to_string(D) + "-D cloud needs " +
                                       std::to_string(D));
                spans.push_back(row);
            }
            row += l.span;
        }
    }
    typename PM<T>::DataPoints out;
    out.rows = rows;
    out.n = input.n;
    out.featureLabels = input.featureLabels;
    out.descriptorLabels = input.descriptorLabels;
    out.descDim = input.descDim;
    out.features.resize((size_t)rows * (size_t)input.n);
    out.descriptors.resize((size_t)input.descDim * (size_t)input.n);
    const bool hasDesc = input.descDim > 0;
    const int rc = pmx_transform_cloud(device, dtype_of<T>(), input.feat(), rows, input.n, parameters.data(),
                                       hasDesc ? input.desc() : nullptr, input.descDim, spans.data(),
                                       (int)spans.size(), out.features.data(),
                                       hasDesc ? out.descriptors.data() : nullptr, nullptr);
    if (rc == PMX_E_BAD_PARAM) throw InvalidParameter(pmx_last_error(nullptr));
    if (rc) throw std::runtime_error(who + ": " + pmx_last_error(nullptr));
    return out;
}

template <typename T>
struct RigidTransformation : PM<T>::Transformation {
    typedef typename PM<T>::DataPoints DataPoints;
    typedef typename PM<T>::TransformationParameters TP;
    RigidTransformation()
        : PM<T>::Transformation("RigidTransformation", Parametrizable::ParametersDoc(), Parametrizable::Parameters()) {}
    // |1 - det R| <= 0.001 in T (TransformationsImpl.cpp:91-105): the chain's check
    bool checkParameters(const TP& p) const override {
        const int rows = side_of(p.size());
        if (rows != 3 && rows != 4) throw InvalidParameter("RigidTransformation: the parameters must be 3 x 3 or 4 x 4");
        return !(std::fabs((T)1 - dense::det_rot(p.data(), rows)) > (T)0.001);
    }
    DataPoints compute(const DataPoints& input, const TP& p) const override {
        if ((int64_t)p.size() == (int64_t)input.rows * input.rows && !checkParameters(p))
            throw TransformationError("RigidTransformation: Error, rotation matrix is not orthogonal.");
        return transform_cloud<T>(input, p, true, this->device, "RigidTransformation");
    }
    // TransformationsImpl.cpp:109-151
    TP correctParameters(const TP& p) const override {
        const int rows = side_of(p.size());
        if (rows != 3 && rows != 4) throw InvalidParameter("RigidTransformation: the parameters must be 3 x 3 or 4 x 4");
        TP ortho = p;
        if (rows == 4) {
            T col1[3], col2[3], n0[3], n1[3];
            normalized3(p.data(), 4, 1, col1);
            normalized3(p.data(), 4, 2, col2);
            cross3(col1, col2, n0);
            cross3(col2, n0, n1);
            for (int r = 0; r < 3; ++r) {
                ortho[r * 4 + 0] = n0[r];
                ortho[r * 4 + 1] = n1[r];
                ortho[r * 4 + 2] = col2[r];
            }
        } else {
            const T epsilon = (T)0.001;
            // R = [ a b]
            //     [-b a]
            if (std::fabs(p[0] - p[4]) > epsilon || std::fabs(p[3] + p[1]) > epsilon)
                throw TransformationError(
                    "RigidTransformation: Error, only proper rigid transformations are supported.");
            T a = (p[0] + p[4]) / 2;
            T b = (-p[3] + p[1]) / 2;
            const T sum = std::sqrt(a * a + b * b);  // (pow(x, 2) is the rounded product)
            a = a / sum;
            b = b / sum;
            ortho[0] = a;
            ortho[1] = b;
            ortho[3] = -b;
            ortho[4] = a;
        }
        return ortho;
    }
};

template <typename T>
struct SimilarityTransformation : PM<T>::Transformation {
    typedef typename PM<T>::DataPoints DataPoints;
    typedef typename PM<T>::TransformationParameters TP;
    SimilarityTransformation()
        : PM<T>::Transformation("SimilarityTransformation", Parametrizable::ParametersDoc(),
                                Parametrizable::Parameters()) {}
    bool checkParameters(const TP&) const override { return true; }  // TransformationsImpl.cpp:197-203
    DataPoints compute(const DataPoints& input, const TP& p) const override {
        return transform_cloud<T>(input, p, true, this->device, "SimilarityTransformation");
    }
    TP correctParameters(const TP& p) const override { return p; }  // :205-210
};

template <typename T>
struct PureTranslation : PM<T>::Transformation {
    typedef typename PM<T>::DataPoints DataPoints;
    typedef typename PM<T>::TransformationParameters TP;
    PureTranslation()
        : PM<T>::Transformation("PureTranslation", Parametrizable::ParametersDoc(), Parametrizable::Parameters()) {}
    // TransformationsImpl.cpp:252-269: the translation column zeroed, then
    // isApprox(Identity).  Third-party semantics (Eigen 3.3 Fuzzy.h,
    // isApprox_selector and NumTraits<T>::dummy_precision()): A is approximately
    // B when ||A - B||_F^2 <= p^2 min(||A||_F^2, ||B||_F^2), p = 1e-5 for float
    // and 1e-12 for double, the norms in T.  The squared norms are summed here in
    // Eigen's storage order (column-major), sequentially; Eigen may add packets
    // in another order, which moves the bound by an ulp.
    bool checkParameters(const TP& p) const override {
        const int rows = side_of(p.size());
        if (rows < 2) throw InvalidParameter("PureTranslation: the parameters must be a square matrix");
        const T prec = sizeof(T) == 8 ? (T)1e-12 : (T)1e-5;
        T diff = 0, na = 0, nb = 0;
        for (int c = 0; c < rows; ++c)
            for (int r = 0; r < rows; ++r) {
                const T a = (c == rows - 1 && r < rows - 1) ? (T)0 : p[r * rows + c];
                const T b = r == c ? (T)1 : (T)0;
                diff = diff + (a - b) * (a - b);
                na = na + a * a;
                nb = nb + b * b;
            }
        return diff <= prec * prec * std::min(na, nb);
    }
    DataPoints compute(const DataPoints& input, const TP& p) const override {
        if ((int64_t)p.size() == (int64_t)input.rows * input.rows && !checkParameters(p))
            throw TransformationError("PureTranslation: Error, left part  not identity.");
        return transform_cloud<T>(input, p, false, this->device, "PureTranslation");
    }
    // :233-250
    TP correctParameters(const TP& p) const override {
        const int rows = side_of(p.size());
        if (rows < 2) throw InvalidParameter("PureTranslation: the parameters must be a square matrix");
        TP out = p;
        for (int r = 0; r < rows - 1; ++r)
            for (int c = 0; c < rows - 1; ++c) out[r * rows + c] = r == c ? (T)1 : (T)0;
        for (int c = 0; c < rows - 1; ++c) out[(rows - 1) * rows + c] = 0;
        out[(size_t)rows * rows - 1] = 1;
        return out;
    }
};

}  // namespace

template <typename T>
void PointMatcher<T>::registerTransformations() {
    typedef Parametrizable::Parameters Ps;
    TransformationRegistrar.reg("RigidTransformation",
                                [](const Ps&) { return std::make_shared<RigidTransformation<T>>(); }, false,
                                "Rigid transformation.");
    TransformationRegistrar.reg("SimilarityTransformation",
                                [](const Ps&) { return std::make_shared<SimilarityTransformation<T>>(); }, false,
                                "Similarity transformation (rotation + translation + scale).");
    TransformationRegistrar.reg("PureTranslation", [](const Ps&) { return std::make_shared<PureTranslation<T>>(); },
                                false, "Pure translation transformation\nA rigid transformation with no rotation.");
}

template void PointMatcher<float>::registerTransformations();
template void PointMatcher<double>::registerTransformations();

}  // namespace pm

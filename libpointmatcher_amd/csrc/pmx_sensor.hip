// pmx_sensor.hip — the sensor-bias family of data filters on the device: one
// point per lane, elementwise, memory-bound.
//
// Replaces the loops of
//   IncidenceAngleDataPointsFilter    DataPointsFilters/IncidenceAngle.cpp:67-73
//   SphericalityDataPointsFilter      DataPointsFilters/Sphericality.cpp:128-176
//   RemoveSensorBiasDataPointsFilter  DataPointsFilters/RemoveSensorBias.cpp:108-127
//                                     (getCoefficients / diffDist / ratioCurvature :132-187,
//                                     constants RemoveSensorBias.h:94-113)
//
// Types follow the reference expression by expression.  Vector work (dot,
// squaredNorm, normalized) is in T, sequential sums, a zero vector left as it
// is by normalized() (Eigen 3.3 Dot.h, as in pmx_keep.hip).  The bias
// correction is double throughout, except the trigonometry of the incidence
// angle: theta is a T in getCoefficients, so tan / cos / sin(theta) are T calls
// whose results widen where they meet a double.  Every std::pow(x, 2) is the
// rounded product x * x (what a correctly rounded pow returns); the powers of
// the constants (sigma, c, aperture) come from the host.  What is left of
// per-point functions in double (cos^3, A^(3/2), erf, and tan / cos / sin of a
// double theta) is rounded once from double-double arithmetic: see below
// why.  Every multiply and add is rounded on its own (the pragma below).
//
// Sphericality uses + - * / and sqrt only: bit-identical to the reference.
// IncidenceAngle calls acos, the float correction tanf / cosf / sinf and both
// corrections exp, which differ from a host library's by a few ulp.  The keep decision of
// RemoveSensorBias uses none of them: the kept set is exact.
//
// RemoveSensorBias's compaction is the keep-filters' (pmx_keep.hip): the kernel
// writes the corrected features of the kept points to a scratch cloud and ends
// in keep_block_ballot; keep_compact scatters scratch features and the input
// descriptors.
#pragma clang fp contract(off)

#include <cmath>
#include <string>

#include "pmx_internal.h"

#include "../../include/pmx.h"

namespace pmx {

template <typename T>
struct SensorMath;
template <>
struct SensorMath<float> {
    static __device__ __forceinline__ float sqrt(float v) { return sqrtf(v); }
    static __device__ __forceinline__ float acos(float v) { return acosf(v); }
    static constexpr float kMin = 1.17549435e-38f;  // numeric_limits<float>::min()
};
template <>
struct SensorMath<double> {
    static __device__ __forceinline__ double sqrt(double v) { return ::sqrt(v); }
    static __device__ __forceinline__ double acos(double v) { return ::acos(v); }
    static constexpr double kMin = 2.2250738585072014e-308;  // numeric_limits<double>::min()
};

// v[0..D) and its squaredNorm (sequential); v[D..3) = 0
template <typename T, int D>
__device__ __forceinline__ T load_vec(const T* __restrict__ p, T (&v)[3]) {
    v[0] = p[0];
    v[1] = p[1];
    v[2] = (T)0;
    T z = v[0] * v[0];
    z = z + v[1] * v[1];
    if (D == 3) {
        v[2] = p[2];
        z = z + v[2] * v[2];
    }
    return z;
}

// normalized() in place (z: the squaredNorm)
template <typename T>
__device__ __forceinline__ void normalize_vec(T (&v)[3], T z) {
    if (z > (T)0) {
        const T s = SensorMath<T>::sqrt(z);
        v[0] = v[0] / s;
        v[1] = v[1] / s;
        v[2] = v[2] / s;
    }
}

// ---- IncidenceAngle ----
template <typename T, int D>
__global__ __launch_bounds__(256) void incidence_angle_kernel(const T* __restrict__ nrm, const T* __restrict__ obs,
                                                              int64_t n, T* __restrict__ angles) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T p[3], nv[3];
    const T z = load_vec<T, D>(obs + i * D, p);
    normalize_vec<T>(p, z);
    (void)load_vec<T, D>(nrm + i * D, nv);  // assumed to be normalized (IncidenceAngle.cpp:71)
    T dot = p[0] * nv[0];
    dot = dot + p[1] * nv[1];
    if (D == 3) dot = dot + p[2] * nv[2];
    angles[i] = SensorMath<T>::acos(dot);
}

template <typename T>
void launch_incidence_angles(const T* nrm, const T* obs, int span, int64_t n, T* angles, hipStream_t st) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (span == 2)
        hipLaunchKernelGGL((incidence_angle_kernel<T, 2>), grid, dim3(256), 0, st, nrm, obs, n, angles);
    else
        hipLaunchKernelGGL((incidence_angle_kernel<T, 3>), grid, dim3(256), 0, st, nrm, obs, n, angles);
}

// ---- Sphericality ----
template <typename T>
__global__ __launch_bounds__(256) void sphericality_kernel(const T* __restrict__ eig, int64_t n, T* __restrict__ sph,
                                                           T* __restrict__ unstruct, T* __restrict__ structure) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T e0 = eig[i * 3], e1 = eig[i * 3 + 1], e2 = eig[i * 3 + 2];
    // ascending (Sphericality.cpp:133)
    if (e1 < e0) {
        const T t = e0;
        e0 = e1;
        e1 = t;
    }
    if (e2 < e1) {
        const T t = e1;
        e1 = e2;
        e2 = t;
    }
    if (e1 < e0) {
        const T t = e0;
        e0 = e1;
        e1 = t;
    }
    T s, u, v;
    if (e2 < SensorMath<T>::kMin || e1 < (T)0 || e0 < (T)0) {
        s = u = v = (T)__builtin_nan("");
    } else if (e1 < SensorMath<T>::kMin) {
        s = u = v = (T)0;
    } else {
        u = e0 / e2;
        const T q = e0 * e0;
        const T root = SensorMath<T>::sqrt(q + e1 * e1);
        v = (e1 / e2) * ((e1 - e0) / root);
        s = u - v;
    }
    sph[i] = s;
    if (unstruct) unstruct[i] = u;
    if (structure) structure[i] = v;
}

template <typename T>
void launch_sphericality(const T* eig, int64_t n, T* sph, T* unstruct, T* structure, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sphericality_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, eig, n, sph, unstruct,
                       structure);
}

// ---- RemoveSensorBias ----
// what getCoefficients forms from constants alone, evaluated on the host with
// the reference's expressions
struct BiasConsts {
    double aperture, k1, k2;
    double c;             // celerity of light
    double pulse;         // pulse_intensity
    double w0;            // lambda_light / (M_PI * aperture)
    double sqrt_pi;       // std::sqrt(M_PI)
    double sigma_c;       // sigma * c
    double sigma_c2;      // std::pow(sigma * c, 2)
    double two_over_ap2;  // 2. / std::pow(aperture, 2)
    double ap2;           // std::pow(aperture, 2)
    double sigma2_c;      // std::pow(sigma, 2) * c
    double sigma4;        // std::pow(sigma, 4)
    double sigma6_c3;     // std::pow(sigma, 6) * std::pow(c, 3)
};

static BiasConsts bias_consts(int sensor_type) {
    const double tau = 50e-9, pulse_intensity = 0.39, lambda_light = 905e-9, c = 299792458.0;
    BiasConsts k;
    // RemoveSensorBias.h:107-113: LMS_1XX, HDL_32E
    k.aperture = sensor_type == 0 ? 0.0075049 : 0.0014835;
    k.k1 = sensor_type == 0 ? 6.08040951e+00 : 1.03211569e+01;
    k.k2 = sensor_type == 0 ? 3.17921789e-03 : 7.07893371e-03;
    const double sigma = tau / std::sqrt(2. * M_PI);
    k.c = c;
    k.pulse = pulse_intensity;
    k.w0 = lambda_light / (M_PI * k.aperture);
    k.sqrt_pi = std::sqrt(M_PI);
    k.sigma_c = sigma * c;
    k.sigma_c2 = std::pow(sigma * c, 2);
    k.two_over_ap2 = 2. / std::pow(k.aperture, 2);
    k.ap2 = std::pow(k.aperture, 2);
    k.sigma2_c = std::pow(sigma, 2) * c;
    k.sigma4 = std::pow(sigma, 4);
    k.sigma6_c3 = std::pow(sigma, 6) * std::pow(c, 3);
    return k;
}

// ---- double functions rounded once from double-double arithmetic ----
// The double correction cancels.  a2 holds 2 (cos d)^2 - 2 d^2 and diffDist
// the root -2 a2 - sqrt(4 a2^2 - 12 a1 a3), which loses eight digits: one ulp
// in cos(theta), in erf or in a pow moves the corrected point by millions of
// ulp, and no two math libraries agree to the ulp.  So the functions that
// reach a2 are evaluated in double-double arithmetic (error-free sums and
// products, about 104 bits) and rounded once: correctly rounded barring exact
// values within about 2^-100 of a rounding tie, and what the tests' reference
// takes too.  Ranges: the angle of a kept point is
// in [0, pi / 2); erf's argument aperture * sqrt(A) stays below 3 to some 60 m
// of depth; outside them the device library's function is used.
struct DD {
    double h, l;
};
__device__ __forceinline__ DD dd_two_sum(double a, double b) {
    const double s = a + b, v = s - a;
    return DD{s, (a - (s - v)) + (b - v)};
}
__device__ __forceinline__ DD dd_two_prod(double a, double b) {
    const double p = a * b;
    return DD{p, fma(a, b, -p)};
}
__device__ __forceinline__ DD dd_mul(DD a, DD b) {
    const DD p = dd_two_prod(a.h, b.h);
    return dd_two_sum(p.h, p.l + (a.h * b.l + a.l * b.h));
}
__device__ __forceinline__ DD dd_add(DD a, DD b) {
    const DD s = dd_two_sum(a.h, b.h);
    return dd_two_sum(s.h, s.l + (a.l + b.l));
}
__device__ __forceinline__ DD dd_neg(DD a) { return DD{-a.h, -a.l}; }
__device__ __forceinline__ DD dd_div_d(DD a, double d) {
    const double q = a.h / d;
    const DD p = dd_two_prod(q, d);
    return dd_two_sum(q, (((a.h - p.h) - p.l) + a.l) / d);
}
__device__ __forceinline__ DD dd_div(DD a, DD b) {
    const double q = a.h / b.h;
    const DD r = dd_add(a, dd_neg(dd_mul(b, DD{q, 0.})));
    return dd_two_sum(q, (r.h + r.l) / b.h);
}

constexpr double kPio2Hi = 1.5707963267948966, kPio2Lo = 6.123233995736766e-17;

// sin, cos, tan of x in [0, pi / 2]: the Taylor series of the argument folded
// into [0, pi / 4], nested from the fifteenth term
__device__ __forceinline__ void cr_sin_cos_tan(double x, double& sn, double& cs, double& tn) {
    const bool fold = x > 0.7853981633974483;
    DD r{x, 0.};
    if (fold) {
        const DD f = dd_two_sum(kPio2Hi, -x);
        r = dd_two_sum(f.h, f.l + kPio2Lo);
    }
    const DD y = dd_mul(r, r), one{1., 0.};
    DD c = one, s = one;
#pragma unroll 1
    for (int n = 15; n >= 1; --n) {
        c = dd_add(one, dd_neg(dd_div_d(dd_mul(y, c), (double)((2 * n - 1) * (2 * n)))));
        s = dd_add(one, dd_neg(dd_div_d(dd_mul(y, s), (double)((2 * n) * (2 * n + 1)))));
    }
    s = dd_mul(s, r);
    const DD S = fold ? c : s, C = fold ? s : c;
    sn = S.h;
    cs = C.h;
    tn = dd_div(S, C).h;
}

// erf(x), x in [0, 3]: 2 / sqrt(pi) * sum of (-1)^n x^(2n+1) / (n! (2n+1)), 80 terms
__device__ __forceinline__ double cr_erf(double x) {
    const DD y = dd_mul(DD{x, 0.}, DD{x, 0.});
    DD t{x, 0.}, acc{x, 0.};
#pragma unroll 1
    for (int n = 1; n < 80; ++n) {
        t = dd_div_d(dd_mul(t, y), (double)n);
        const DD q = dd_div_d(t, (double)(2 * n + 1));
        acc = dd_add(acc, (n & 1) ? dd_neg(q) : q);
    }
    return dd_mul(acc, DD{1.1283791670955126, 1.533545961316588e-17}).h;
}

// std::pow(x, 3) and std::pow(x, 3. / 2.) for x > 0
__device__ __forceinline__ double pow3(double x) { return dd_mul(dd_two_prod(x, x), DD{x, 0.}).h; }
__device__ __forceinline__ double pow3_2(double x) {
    const double s = ::sqrt(x);
    const DD p = dd_two_prod(s, s);
    return dd_mul(dd_two_sum(s, ((x - p.h) - p.l) / (2. * s)), DD{x, 0.}).h;
}

// tan, cos, sin of theta in T (RemoveSensorBias.cpp:137-139: theta is a T there)
__device__ __forceinline__ void bias_trig(float theta, float& tn, float& cs, float& sn) {
    tn = tanf(theta);
    cs = cosf(theta);
    sn = sinf(theta);
}
__device__ __forceinline__ void bias_trig(double theta, double& tn, double& cs, double& sn) {
    if (theta >= 0. && theta <= kPio2Hi) {
        cr_sin_cos_tan(theta, sn, cs, tn);
    } else {
        tn = ::tan(theta);
        cs = ::cos(theta);
        sn = ::sin(theta);
    }
}

// a[1..3] of getCoefficients (RemoveSensorBias.cpp:132-153; a0 is never read)
template <typename T>
__device__ __forceinline__ void bias_coefficients(const BiasConsts& k, double depth, T theta, double& a1, double& a2,
                                                  double& a3) {
    T tn, cs, sn;
    bias_trig(theta, tn, cs, sn);
    const double dt = depth * tn;
    const double dt2 = dt * dt;
    const double A = 2. * dt2 / k.sigma_c2 + k.two_over_ap2;
    const double K1 = pow3((double)cs);
    const double cs2 = (double)cs * (double)cs;
    const double K2 = 3. * cs2 * sn;
    const double wr = k.w0 / (k.aperture * depth * cs);
    const double wq = wr * wr;
    const double ex = k.aperture * ::sqrt(A);
    const double L1 = k.pulse * wq * k.sqrt_pi * (ex <= 3. ? cr_erf(ex) : erf(ex)) / (2. * pow3_2(A));
    const double L2 = k.pulse * wq * K2 / (2. * A);
    a1 = -(2. * tn * depth * (L1 * K2 - 2. * L2 * k.aperture * exp(-A * k.ap2))) / k.sigma2_c;
    const double scc = k.sigma_c * cs, cd = cs * depth, cc = k.c * cs;
    a2 = -L1 * 2. * A * K1 * (scc * scc * A + 2. * (cd * cd) - 2. * (depth * depth)) / (2 * (cc * cc) * k.sigma4 * A);
    a3 = L1 * K2 * depth * tn * (k.sigma_c2 * A - 2. * dt2) / (k.sigma6_c3 * A);
}

// k1 * diffDist + k2 * ratioCurvature (RemoveSensorBias.cpp:119, 155-187)
template <typename T>
__device__ __forceinline__ double bias_correction(const BiasConsts& k, double depth, T theta) {
    double a1, a2, a3, b1, b2, b3;
    bias_coefficients<T>(k, depth, theta, a1, a2, a3);
    bias_coefficients<T>(k, depth, (T)0., b1, b2, b3);
    double Tmax;
    if (theta < 1e-5)  // approx. 0
        Tmax = 0.;
    else
        Tmax = (-2 * a2 - ::sqrt(4 * (a2 * a2) - 12 * a1 * a3)) / (6 * a3);
    const double diff = Tmax * k.c / 2.;
    const double ratio = 1. - 2 * b2 / (2 * a2 + 6 * Tmax * a3);
    return k.k1 * diff + k.k2 * ratio;
}

template <typename T, int D>
__global__ __launch_bounds__(kKeepBlock) void sensor_bias_kernel(const T* __restrict__ f, const T* __restrict__ d,
                                                                 int64_t n, int desc_dim, int inc_row, int obs_row,
                                                                 T threshold, BiasConsts k, T* __restrict__ cf,
                                                                 unsigned long long* __restrict__ masks,
                                                                 uint32_t* __restrict__ block_cnt) {
    constexpr int rows = D + 1;
    const int64_t i = (int64_t)blockIdx.x * kKeepBlock + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const T* di = d + i * desc_dim;
        const T inc = di[inc_row];
        keep = (inc == inc) && inc >= (T)0 && inc < threshold;  // RemoveSensorBias.cpp:117
        if (keep) {
            T o[3];
            const T z = load_vec<T, D>(di + obs_row, o);
            const double depth = (double)SensorMath<T>::sqrt(z);  // vObs.norm(), in T
            const T corr = (T)bias_correction<T>(k, depth, inc);
            normalize_vec<T>(o, z);
            const T* p = f + i * rows;
            T* q = cf + i * rows;
#pragma unroll
            for (int r = 0; r < D; ++r) q[r] = p[r] + corr * o[r];
            q[D] = p[D];
        }
    }
    keep_block_ballot(keep, masks, block_cnt);
}

int sensor_bias_check(int rows, int64_t n, int desc_dim, int inc_row, int obs_row, int sensor_type, std::string& err) {
    if (rows != 3 && rows != 4) {
        err = "RemoveSensorBiasDataPointsFilter: clouds must be 2-D or 3-D (3 or 4 homogeneous rows)";
        return PMX_E_BAD_PARAM;
    }
    const int D = rows - 1;
    if (inc_row < 0 || inc_row >= desc_dim) {
        err = "RemoveSensorBiasDataPointsFilter: the incidenceAngles row is not a descriptor row";
        return PMX_E_BAD_PARAM;
    }
    if (obs_row < 0 || obs_row + D > desc_dim) {
        err = "RemoveSensorBiasDataPointsFilter: observationDirections needs the row offset of a descriptor of the "
              "cloud's dimension";
        return PMX_E_BAD_PARAM;
    }
    if (sensor_type != 0 && sensor_type != 1) {  // RemoveSensorBias.cpp:96-98
        err = "RemoveSensorBiasDataPointsFilter: Error, cannot remove bias for sensorType id " +
              std::to_string(sensor_type) + " .";
        return PMX_E_BAD_PARAM;
    }
    if (n > (int64_t)0x7fffffff) {
        err = "RemoveSensorBiasDataPointsFilter: more than 2^31 points";
        return PMX_E_BAD_PARAM;
    }
    return PMX_OK;
}

template <typename T>
int sensor_bias_run(const T* d_f, int rows, int64_t n, const T* d_desc, int desc_dim, int inc_row, int obs_row,
                    int sensor_type, double angle_threshold, T* d_cf, T* d_of, T* d_od, int64_t* n_out,
                    hipStream_t st, std::string& err) {
    *n_out = 0;
    const int rc = sensor_bias_check(rows, n, desc_dim, inc_row, obs_row, sensor_type, err);
    if (rc) return rc;
    const int D = rows - 1;
    if (n <= 0) return PMX_OK;
    KeepScratch sc;
    if (sc.alloc(n) != PMX_OK) {
        err = "RemoveSensorBiasDataPointsFilter: device allocation failed";
        return PMX_E_HIP;
    }
    const BiasConsts k = bias_consts(sensor_type);
    const dim3 grid((unsigned)sc.nb), block(kKeepBlock);
    if (D == 2)
        hipLaunchKernelGGL((sensor_bias_kernel<T, 2>), grid, block, 0, st, d_f, d_desc, n, desc_dim, inc_row, obs_row,
                           (T)angle_threshold, k, d_cf, sc.masks, sc.cnt);
    else
        hipLaunchKernelGGL((sensor_bias_kernel<T, 3>), grid, block, 0, st, d_f, d_desc, n, desc_dim, inc_row, obs_row,
                           (T)angle_threshold, k, d_cf, sc.masks, sc.cnt);
    if (keep_compact<T>(d_cf, rows, d_desc, desc_dim, sc, d_of, d_od, n_out, st) != PMX_OK) {
        err = "RemoveSensorBiasDataPointsFilter: HIP failure";
        return PMX_E_HIP;
    }
    return PMX_OK;
}

template void launch_incidence_angles<float>(const float*, const float*, int, int64_t, float*, hipStream_t);
template void launch_incidence_angles<double>(const double*, const double*, int, int64_t, double*, hipStream_t);
template void launch_sphericality<float>(const float*, int64_t, float*, float*, float*, hipStream_t);
template void launch_sphericality<double>(const double*, int64_t, double*, double*, double*, hipStream_t);
template int sensor_bias_run<float>(const float*, int, int64_t, const float*, int, int, int, int, double, float*,
                                    float*, float*, int64_t*, hipStream_t, std::string&);
template int sensor_bias_run<double>(const double*, int, int64_t, const double*, int, int, int, int, double, double*,
                                     double*, double*, int64_t*, hipStream_t, std::string&);

}  // namespace pmx

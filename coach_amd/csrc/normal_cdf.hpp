// The standard normal distribution function and its inverse in fp64 on the device, for the truncated-normal draw by
// inverse CDF (explore_dist.hip).  Written from the published formulas:
//
//   ndtr(x)  = 1/2 erfc(-x / sqrt 2)                                                     (Abramowitz & Stegun 26.2.29)
//   ndtri(y) = Cephes' ndtri (S. Moshier, Cephes Math Library 2.1, "ndtri.c"): three rational approximations,
//     |y - 1/2| <= 1/2 - exp(-2):  x = sqrt(2 pi) (w + w w^2 P0(w^2) / Q0(w^2)),  w = y - 1/2
//     z = sqrt(-2 ln y) in [2, 8)   (exp(-32) < y <= exp(-2)):  x = -(z - ln z / z - P1(1/z) / (z Q1(1/z)))
//     z >= 8                        (y <= exp(-32)):            the same with P2 / Q2
//   and ndtri(y) = -ndtri(1 - y) above 1 - exp(-2).  The coefficients are the published ones, digit for digit.
//
// Error account (relative, fp64; eps = 2^-53):
//   * erfc is the device library's (ocml), stated at <= 5 ulp over the whole range; its argument -x / sqrt 2 carries
//     1.5 eps, which the slope x^2 of ln erfc turns into <= 1.5 x^2 eps: ndtr(-9) is good to about 1.3e-14, and a lower
//     tail keeps its RELATIVE accuracy down to the underflow of erfc (x = -38.4).  Above 0 the value tends to 1 and
//     only the absolute error 1 eps is kept, which is why a window to the right of the centre is drawn through the
//     upper tail: ndtr_upper(x) = ndtr(-x), no cancellation.
//   * ndtri: Cephes states a peak relative error of 4.7e-16 ([0.125, 1]), 1.9e-16 and 1.1e-16 (tails) for the rational
//     forms on correctly rounded arithmetic; here ln and sqrt are the device library's (<= 1 ulp, sqrt correctly
//     rounded), and z - ln z / z - x1 does not cancel (z >= 2, the corrections are below z / 2).  The central form
//     cancels nowhere either (|w| <= 0.365).  What dominates is CONDITIONING, not the approximation: d ln|x| / d ln y
//     = y / (x phi(x)) grows without bound at y = 1/2 (x = 0: only the absolute error eps sqrt(2 pi) is meaningful there)
//     and an argument formed as 1 - y carries the absolute error of y.  tests/test_truncated_normal.py measures the
//     total against bisection on the host's erfc on arguments that include every joint; the bound is in DESIGN.md.
//   * ndtri(0) = -inf, ndtri(1) = +inf, outside [0, 1] NaN, as Cephes returns them; the caller clamps.
// No fused multiply-add is assumed or needed (the file that includes this is compiled with -ffp-contract=off; the
// account above holds either way).
#pragma once
#include <hip/hip_runtime.h>

namespace rlx {

constexpr double kSqrt2Pi = 2.50662827463100050242;
constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kExpM2 = 0.13533528323661269189;       // exp(-2): the joint of the central and the tail forms

__device__ __forceinline__ double ndtr(double x) { return 0.5 * erfc(-x * kInvSqrt2); }
__device__ __forceinline__ double ndtr_upper(double x) { return 0.5 * erfc(x * kInvSqrt2); }   // 1 - ndtr(x), no cancellation

namespace detail {
template <int N>
__device__ __forceinline__ double horner(double x, const double (&c)[N]) {
    double r = c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) r = r * x + c[i];
    return r;
}
}  // namespace detail

__device__ __forceinline__ double ndtri(double y0) {
    // |y - 1/2| <= 3/8 and a little beyond
    const double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1,
                          1.39312609387279679503E1, -1.23916583867381258016E0};
    const double Q0[9] = {1.00000000000000000000E0, 1.95448858338141759834E0, 4.67627912898881538453E0,
                          8.63602421390890590575E1, -2.25462687854119370527E2, 2.00260212380060660359E2,
                          -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0};
    // z = sqrt(-2 ln y) in [2, 8)
    const double P1[9] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1,
                          4.40805073893200834700E1, 1.46849561928858024014E1, 2.18663306850790267539E0,
                          -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4};
    const double Q1[9] = {1.00000000000000000000E0, 1.57799883256466749731E1, 4.53907635128879210584E1,
                          4.13172038254672030440E1, 1.50425385692907503408E1, 2.50464946208309415979E0,
                          -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4};
    // z in [8, 64]
    const double P2[9] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0,
                          1.33303460815807542389E0, 2.01485389549179081538E-1, 1.23716634817820021358E-2,
                          3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9};
    const double Q2[9] = {1.00000000000000000000E0, 6.02427039364742014255E0, 3.67983563856160859403E0,
                          1.37702099489081330271E0, 2.16236993594496635890E-1, 1.34204006088543189037E-2,
                          3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9};
    if (y0 == 0.0) return -__builtin_inf();
    if (y0 == 1.0) return __builtin_inf();
    if (!(y0 > 0.0 && y0 < 1.0)) return __builtin_nan("");
    bool lower = true;                                   // the result is the negated tail quantile
    double y = y0;
    if (y > 1.0 - kExpM2) {
        y = 1.0 - y;                                     // exact (Sterbenz): y0 >= 1/2
        lower = false;
    }
    if (y > kExpM2) {
        const double w = y - 0.5;
        const double w2 = w * w;
        return (w + w * (w2 * detail::horner(w2, P0) / detail::horner(w2, Q0))) * kSqrt2Pi;
    }
    const double z = __builtin_sqrt(-2.0 * log(y));
    const double x0 = z - log(z) / z;
    const double r = 1.0 / z;
    const double x1 = z < 8.0 ? r * detail::horner(r, P1) / detail::horner(r, Q1)
                              : r * detail::horner(r, P2) / detail::horner(r, Q2);
    const double x = x0 - x1;
    return lower ? -x : x;
}

}  // namespace rlx

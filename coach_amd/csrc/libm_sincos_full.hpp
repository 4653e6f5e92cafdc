// rlx::libm_sin_full / rlx::libm_cos_full — sin(x), cos(x) for |x| < 2^20, rounded like the host libm's, on the device.
//
// Why it exists: gym 0.12.5's Pendulum-v0 never wraps its angle (about +-85 rad after 200 steps) and Acrobot-v1 takes
// cos(theta1 + theta2 - pi/2) over several radians inside its Runge-Kutta step (csrc/classic_control.hip).  The table
// functions of libm_sincos.hpp stop at |x| < 0.855469, the first branch of glibc's __sin / __cos
// (sysdeps/ieee754/dbl-64/s_sin.c, >= 2.28).  This header adds the branches behind it, in glibc's structure:
//
//   |x| < 0.855469           rlx::libm_sin / libm_cos themselves: unchanged bits.
//   |x| < 2.426265           the complementary function of t = hp0 - |x|, hp0 + hp1 = pi/2 to 107 bits: sin takes
//                            do_cos(t, hp1); cos renormalises (t, hp1) to a double-double and takes do_sin of it.
//   |x| < 2^20               n = round(x * 2/pi) (the 2^52 * 1.5 trick; n mod 4 sits in the sum's low word), then
//                            Cody-Waite in four pieces of pi/2: x - n mp1 - n mp2 (one rounding each, see below), then
//                            pp3 and pp4 with the rounding errors collected in the tail:  x - n pi/2 = a + da.
//                            Quadrant n (n + 1 for cos) selects do_sin or do_cos on (a, da), and the sign.
//   beyond                   *status is set and the ordinary sin() / cos() is returned, as libm_sin does outside its domain.
//                            (glibc's own reduction holds to 105414350; 2^20 is the range the simulators are held to.)
//
// do_sin / do_cos / taylor_sin below are glibc's kernels with their dx argument: libm_sincos.hpp has them inlined for
// dx = 0, and the fused operations are the same ones (the x86-64 FMA build of glibc, the variant every FMA-capable CPU
// dispatches to; where a product feeds only sums that build fuses it, and so does this file, explicitly).
//
// Error account of the reduction, for |x| < 2^20, so |n| <= 667544 < 2^20:
//   * mp1, mp2 and pp3 carry 26, 27 and 26 significant bits, so n * mp1, n * mp2 and n * pp3 are exact doubles (at most
//     47 bits) and each fused step rounds once.  x - n mp1 is exact: x (>= 2.4) and n mp1 (a multiple of 2^-25)
//     are multiples of ulp(x) >= 2^-51 and their difference is below 1.  The mp2 step rounds by at most 2^-54 |y| with
//     |y| <= pi/4 + 2^-34.
//   * the pp3 and pp4 steps return their roundings into the tail: t2 = y - n pp3 rounds, and (y - t2) - n pp3 is that
//     rounding error (one fused step); likewise b and (t2 - b) - n pp4.  What is lost is the rounding of the tail's own
//     sum and of n * pp4 inside its fused step: below 2^-106 absolute.
//   * the constant: |pi/2 - (mp1 + mp2 + pp3 + pp4)| = 2^-141.8, times |n| < 2^20: below 2^-121 absolute.
//   * the mp2 step's rounding is NOT recovered — glibc does not recover it either.  It is exact whenever the reduced
//     argument is small (x - n mp1 - n mp2 then has few bits), which is when it would matter relative to |a|: the
//     cancellation cases of the tests, multiples of pi/2 +- 2 ulps up to 2^20.
//     So the reduced argument is within 2^-54 |a| + 2^-106 of the true one, half an ulp of a at the most; sin and cos
//     have |derivative| <= 1 and the kernels add <= 0.55 ulp: within 1 ulp of the host's result, which runs the same
//     steps.  Bits can differ from the host's only where the two are compiled to different fusions (measured: DESIGN §8).
//
// Compiles as HIP device code and as plain host C++; must be compiled with -ffp-contract=off: every fusion is explicit.
#pragma once
#include "libm_sincos.hpp"

namespace rlx {
namespace sincos_detail {

LIBM_SINCOS_CONST double k_hp0 = 0x1.921fb54442d18p+0;      // pi/2 = hp0 + hp1
LIBM_SINCOS_CONST double k_hp1 = 0x1.1a62633145c07p-54;
LIBM_SINCOS_CONST double k_mp1 = 0x1.921fb58p+0;            // pi/2 = mp1 + mp2 + pp3 + pp4, the first three short
LIBM_SINCOS_CONST double k_mp2 = -0x1.dde973cp-27;
LIBM_SINCOS_CONST double k_pp3 = -0x1.cb3b398p-55;
LIBM_SINCOS_CONST double k_pp4 = -0x1.d747f23e32ed7p-83;
LIBM_SINCOS_CONST double k_hpinv = 0x1.45f306dc9c883p-1;    // 2/pi
LIBM_SINCOS_CONST double k_toint = 0x1.8p+52;
LIBM_SINCOS_CONST double k_full_range = 1048576.0;          // 2^20

// TAYLOR_SIN(xx, x, dx): ((POLYNOMIAL(xx) * x - 0.5 * dx) * xx + dx), then x + that
LIBM_SINCOS_FN double taylor_sin(double xx, double x, double dx) {
    double p = fma(xx, k_s5, k_s4);
    p = fma(xx, p, k_s3);
    p = fma(xx, p, k_s2);
    p = fma(xx, p, k_s1);
    const double a = fma(x, p, -(0.5 * dx));
    const double t = fma(a, xx, dx);
    return x + t;
}

LIBM_SINCOS_FN double do_sin(double x, double dx) {
    const double xold = x;
    if (fabs(x) < k_taylor_below) return taylor_sin(x * x, x, dx);
    if (x <= 0.0) dx = -dx;
    double r;
    const int k = split(fabs(x), &r);
    const double sn = k_sincostab[4 * k], ssn = k_sincostab[4 * k + 1];
    const double cs = k_sincostab[4 * k + 2], ccs = k_sincostab[4 * k + 3];
    const double xx = r * r;
    const double p = fma(xx, k_sn5, k_sn3);
    const double t = fma(r * xx, p, dx);
    const double s = r + t;
    double q = fma(xx, k_cs6, k_cs4);
    q = fma(xx, q, k_cs2);
    const double c = fma(r, dx, xx * q);
    const double a = fma(s, ccs, ssn);
    const double b = fma(-c, sn, a);
    const double cor = fma(s, cs, b);
    return copysign(sn + cor, xold);
}

LIBM_SINCOS_FN double do_cos(double x, double dx) {
    if (x < 0.0) dx = -dx;
    double r;
    const int k = split(fabs(x), &r);
    r = r + dx;
    const double sn = k_sincostab[4 * k], ssn = k_sincostab[4 * k + 1];
    const double cs = k_sincostab[4 * k + 2], ccs = k_sincostab[4 * k + 3];
    const double xx = r * r;
    const double p = fma(xx, k_sn5, k_sn3);
    const double s = fma(r * xx, p, r);
    double q = fma(xx, k_cs6, k_cs4);
    q = fma(xx, q, k_cs2);
    const double c = xx * q;
    const double a = fma(-s, ssn, ccs);
    const double b = fma(-c, cs, a);
    const double cor = fma(-s, sn, b);
    return cs + cor;
}

// x - n pi/2 = *a + *da with n = round(x 2/pi); returns n mod 4.  |x| < 2^20 (see the account above).
LIBM_SINCOS_FN int reduce_sincos(double x, double *a, double *da) {
    const double t = fma(x, k_hpinv, k_toint);
    const double xn = t - k_toint;
    const double y = fma(-xn, k_mp2, fma(-xn, k_mp1, x));
    const int n = (int)((uint32_t)bits(t) & 3u);
    const double t2 = fma(-xn, k_pp3, y);
    double db = fma(-xn, k_pp3, y - t2);
    const double b = fma(-xn, k_pp4, t2);
    db += fma(-xn, k_pp4, t2 - b);
    *a = b;
    *da = db;
    return n;
}

// sin (n even) or cos (n odd) of a + da, negated in quadrants 2 and 3
LIBM_SINCOS_FN double do_sincos(double a, double da, int n) {
    // do_sin alone decides between the Taylor branch and the table (|a| < 0.126), as glibc 2.35 does; testing a * a
    // against 0.01588 first, as s_sin.c once did, sends 0.126 <= |a| < 0.126016 to the other branch: 1 ulp off in 1e-7 of cases
    const double v = (n & 1) ? do_cos(a, da) : do_sin(a, da);
    return (n & 2) ? -v : v;
}

}  // namespace sincos_detail

LIBM_SINCOS_FN double libm_sin_full(double x, int *status) {
    using namespace sincos_detail;
    const uint32_t hx = (uint32_t)(bits(x) >> 32) & 0x7fffffffu;
    if (hx < 0x3feb6000u) {                                           // |x| < 0.855469: the table functions
        int dom = 0;
        return libm_sin(x, &dom);
    }
    if (hx < 0x400368fdu) return copysign(do_cos(k_hp0 - fabs(x), k_hp1), x);
    if (!(fabs(x) < k_full_range)) {
        *status = 1;
        return sin(x);
    }
    double a, da;
    const int n = reduce_sincos(x, &a, &da);
    return do_sincos(a, da, n);
}

LIBM_SINCOS_FN double libm_cos_full(double x, int *status) {
    using namespace sincos_detail;
    const uint32_t hx = (uint32_t)(bits(x) >> 32) & 0x7fffffffu;
    if (hx < 0x3feb6000u) {
        int dom = 0;
        return libm_cos(x, &dom);
    }
    if (hx < 0x400368fdu) {
        const double y = k_hp0 - fabs(x);
        const double a = y + k_hp1;
        const double da = (y - a) + k_hp1;
        return do_sin(a, da);
    }
    if (!(fabs(x) < k_full_range)) {
        *status = 1;
        return cos(x);
    }
    double a, da;
    const int n = reduce_sincos(x, &a, &da);
    return do_sincos(a, da, n + 1);
}

}  // namespace rlx

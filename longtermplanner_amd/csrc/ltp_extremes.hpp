// ltp_extremes.hpp — the candidate rule of the analytic envelopes (k_envelope's analytic form, k_envelope_walk, k_envelope_knots,
// k_envelope_knots_arrays; ltp_consumers.hip): inside a run every array is a polynomial in the run-local index m, so its extreme
// SAMPLES over a stretch m0 .. m1 of the run are the stretch's two end samples or the samples either side of a real root of the
// polynomial's derivative. Here: the roots of a quadratic or linear derivative, and the fold over a stretch that is handed the
// evaluator of a sample. Host logic without HIP headers, in the manner of ltp_intervals.hpp:
// tests/cpp/envelope_arrays_extremes_test.cc runs the same functions the kernels run, against the exhaustive loop and on
// coefficients that are NaN, infinite or huge (every candidate index stays in [m0, m1], no double is converted to int before it
// is known to lie in range).
#pragma once
#include "ltp_knots.hpp"

namespace ltp {

// the real roots of a derivative, NaN where there is none
struct StretchRoots { double r1, r2; };

// A m^2 + B m + C = 0 (A == 0: the linear case)
LTP_KNOTS_HD inline StretchRoots quadratic_roots(double A, double B, double C)
{
    double r1 = __builtin_nan(""), r2 = r1;
    if (A == 0.0) {
        if (B != 0.0) r1 = -C / B;
    } else {
        const double disc = B * B - 4.0 * A * C;
        if (disc >= 0.0) {
            const double sq = __builtin_sqrt(disc);
            const double qq = -0.5 * (B + (B < 0.0 ? -sq : sq));   // the cancellation-free root first
            r1 = qq / A;
            r2 = qq != 0.0 ? C / qq : r1;
        }
    }
    return StretchRoots{r1, r2};
}

// B m + C = 0
LTP_KNOTS_HD inline StretchRoots linear_root(double B, double C)
{
    const double none = __builtin_nan("");
    return StretchRoots{B != 0.0 ? -C / B : none, none};
}

// q(m) = c[0] + c[1] m + c[2] m^2 + c[3] m^3 (run_eval_q): the roots of q'(m) = c[1] + 2 c[2] m + 3 c[3] m^2
LTP_KNOTS_HD inline StretchRoots qprime_roots(const double* c4) { return quadratic_roots(3.0 * c4[3], 2.0 * c4[2], c4[1]); }
// v(m) = c[4] + c[5] m + c[6] m^2 (run_eval): the root -c[5] / (2 c[6]) of v'(m), none for c[6] == 0
LTP_KNOTS_HD inline StretchRoots vprime_root(const double* c) { return linear_root(2.0 * c[6], c[5]); }

// The candidates of the stretch m0 .. m1 (m0 <= m1) of a run, each handed to fold(m) once or twice: the two end samples and, for
// m1 - m0 > 1 (the only stretches whose roots are read), the samples either side of a root that lies in (m0 - 1, m1 + 1). The
// range test is made on the double: a NaN, an infinite or a huge root fails it, and only then is the root converted.
template <class Roots, class Fold>
LTP_KNOTS_HD inline void fold_candidates(int m0, int m1, Roots&& roots_of_run, Fold&& fold)
{
    fold(m0);
    if (m1 > m0) fold(m1);
    if (m1 - m0 > 1) {
        const StretchRoots roots = roots_of_run();
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int which = 0; which < 2; ++which) {
            const double rho = which ? roots.r2 : roots.r1;
            if (rho > (double)m0 - 1.0 && rho < (double)m1 + 1.0) {   // false for NaN
                const int k = (int)__builtin_floor(rho);
                if (k > m0 && k < m1) fold(k);
                if (k + 1 > m0 && k + 1 < m1) fold(k + 1);
            }
        }
    }
}

// a monotone array (a(m) = fma(c[8], m, c[7]): one rounding of a monotone function of m): the two end samples are exhaustive
template <class Fold>
LTP_KNOTS_HD inline void fold_ends(int m0, int m1, Fold&& fold)
{
    fold(m0);
    if (m1 > m0) fold(m1);
}

}  // namespace ltp

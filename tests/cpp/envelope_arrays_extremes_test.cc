// envelope_arrays_extremes_test.cc — the candidate rule of the analytic envelopes (longtermplanner_amd/csrc/ltp_extremes.hpp) on the
// host, as k_envelope_knots_arrays runs it: for random runs of the sampler's magnitudes and stretches of 1 .. 3000 samples the fold
// over the candidates against the exhaustive loop over the same fma expressions (include/ltp_run_tables.hpp: run_eval) —
//   v  inside the exhaustive [min, max] and within 1e-12 of it,
//   a  equal to it (two end samples), j equal to it (one value).
// Also c[6] == 0, c[5] == c[6] == 0, stretches of 1, 2 and 3 samples, and coefficients that are NaN, infinite or 1e300: no
// undefined behaviour (the program is also built with -fsanitize=address,undefined,float-cast-overflow) and every candidate index
// inside [m0, m1]. A stand-alone program; tests/test_envelope_arrays_cpu.py compiles and runs it.
//
// The magnitudes. A run of n samples lasts T = m1 * Ts. The sampler's runs obey the limits of a robot joint (|v| <= ~3 rad/s,
// |a| <= 20, |j| <= 1e4): a long run cannot hold a large jerk or acceleration, because the state would leave the limits. The draw
// keeps |a_s| T <= 6, |J| T <= 40 and |J| T^2 <= 12, so |v| <= 3 + 12 + 6 over the stretch and an ulp of v is <= 3.6e-15: a
// rounding wiggle of a few ulps is two orders of magnitude below the bar of 1e-12.
#include "ltp_extremes.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                  \
    } while (0)

// the lines of run_eval
double eval_q(const double* c, int m)
{
    const double md = (double)m;
    return __builtin_fma(__builtin_fma(__builtin_fma(c[3], md, c[2]), md, c[1]), md, c[0]);
}
double eval_v(const double* c, int m)
{
    const double md = (double)m;
    return __builtin_fma(__builtin_fma(c[6], md, c[5]), md, c[4]);
}
double eval_a(const double* c, int m) { return __builtin_fma(c[8], (double)m, c[7]); }

// run_coef of an ordinary run (include/ltp_run_tables.hpp), separate roundings
void run_coef(double* c, double J, double a_s, double v_s, double q_s, double Ts)
{
    const double tj = Ts * J;
    const double v1 = Ts * a_s, v2 = 0.5 * (Ts * tj);
    const double q1 = Ts * v_s, q2 = 0.5 * (Ts * (Ts * a_s)), q3 = (Ts * (Ts * tj)) * (1.0 / 6.0);
    c[0] = q_s; c[1] = q1 + (q2 + 2.0 * q3); c[2] = q2 + 3.0 * q3; c[3] = q3;
    c[4] = v_s; c[5] = v1 + v2; c[6] = v2;
    c[7] = a_s; c[8] = tj;
    c[9] = J;
}

struct Pair {
    double lo = std::numeric_limits<double>::infinity(), hi = -std::numeric_limits<double>::infinity();
    void fold(double x) { lo = std::fmin(lo, x); hi = std::fmax(hi, x); }
};

struct Tally {
    long long cases = 0, interior = 0, v_identical = 0, calls = 0, most_calls = 0;
    double worst = 0.0;
};

// one stretch: the folds against the exhaustive loops; `realistic`: the values are compared, else only the indices are
void one_stretch(const double* c, int m0, int m1, bool realistic, Tally& t)
{
    long long calls = 0;
    bool outside = false;
    auto seen = [&](int m) {
        ++calls;
        if (m < m0 || m > m1) outside = true;
    };
    Pair q, v, a, j;
    ltp::fold_candidates(m0, m1, [&] { return ltp::qprime_roots(c); }, [&](int m) { seen(m); q.fold(eval_q(c, m)); });
    CHECK(!outside && calls <= 6, "q candidates of [%d, %d]: %lld calls", m0, m1, calls);
    calls = 0;
    ltp::fold_candidates(m0, m1, [&] { return ltp::vprime_root(c); }, [&](int m) { seen(m); v.fold(eval_v(c, m)); });
    CHECK(!outside && calls <= 4, "v candidates of [%d, %d]: %lld calls", m0, m1, calls);
    t.most_calls = std::max(t.most_calls, calls);
    t.calls += calls;
    calls = 0;
    ltp::fold_ends(m0, m1, [&](int m) { seen(m); a.fold(eval_a(c, m)); });
    CHECK(!outside && calls <= 2, "a candidates of [%d, %d]: %lld calls", m0, m1, calls);
    j.fold(c[9]);
    ++t.cases;
    if (!realistic) return;
    Pair ev, ea, ej, eq;
    int at_lo = m0, at_hi = m0;
    for (int m = m0; m <= m1; ++m) {
        const double x = eval_v(c, m);
        if (x < ev.lo) at_lo = m;
        if (x > ev.hi) at_hi = m;
        ev.fold(x);
        ea.fold(eval_a(c, m));
        ej.fold(c[9]);
        eq.fold(eval_q(c, m));
    }
    if ((at_lo != m0 && at_lo != m1) || (at_hi != m0 && at_hi != m1)) ++t.interior;
    CHECK(v.lo >= ev.lo && v.hi <= ev.hi, "v of [%d, %d] outside the samples: [%.17g, %.17g] vs [%.17g, %.17g]", m0, m1, v.lo, v.hi, ev.lo, ev.hi);
    const double d = std::fmax(std::fabs(v.lo - ev.lo), std::fabs(v.hi - ev.hi));
    CHECK(d <= 1e-12, "v of [%d, %d]: |d| = %.3e", m0, m1, d);
    t.worst = std::fmax(t.worst, d);
    if (v.lo == ev.lo && v.hi == ev.hi) ++t.v_identical;
    CHECK(a.lo == ea.lo && a.hi == ea.hi, "a of [%d, %d]: [%.17g, %.17g] vs [%.17g, %.17g]", m0, m1, a.lo, a.hi, ea.lo, ea.hi);
    CHECK(j.lo == ej.lo && j.hi == ej.hi, "j of [%d, %d]", m0, m1);
    CHECK(q.lo >= eq.lo && q.hi <= eq.hi, "q of [%d, %d] outside the samples", m0, m1);
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20260101);
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    const double sample_times[3] = {1e-3, 1.0 / 1024.0, 4e-3};
    Tally t;
    for (double Ts : sample_times) {
        for (int it = 0; it < 6000; ++it) {
            // lengths: 1, 2, 3 and short stretches often, long ones too
            const int kind = it % 6;
            const int n = kind == 0 ? 1 + it / 6 % 3 : kind <= 2 ? pick(1, 40) : pick(1, 3000);
            const int m0 = pick(1, 60), m1 = m0 + n - 1;
            const double T = (double)m1 * Ts;
            double J = uni(-1.0, 1.0) * std::min({1e4, 40.0 / T, 12.0 / (T * T)});
            double a_s = uni(-1.0, 1.0) * std::min(20.0, 6.0 / T);
            const double v_s = uni(-3.0, 3.0), q_s = uni(-3.0, 3.0);
            const int shape = it % 5;
            if (shape == 0) J = 0.0;                                          // c[6] == 0: v is linear in m
            if (shape == 1) { J = 0.0; a_s = 0.0; }                           // c[5] == c[6] == 0: v is constant
            if (shape >= 3 && J != 0.0) {                                     // the vertex of v near or inside the stretch
                const double rho = uni((double)m0 - 2.0, (double)m1 + 2.0);
                a_s = -J * Ts * (rho + 0.5);                                  // v'(m) = Ts a_s + Ts^2 J (m + 1/2)
            }
            double c[10];
            run_coef(c, J, a_s, v_s, q_s, Ts);
            if (shape == 0) CHECK(c[6] == 0.0, "c[6]");
            if (shape == 1) CHECK(c[5] == 0.0 && c[6] == 0.0, "c[5], c[6]");
            one_stretch(c, m0, m1, true, t);
        }
    }
    CHECK(t.interior * 10 >= t.cases, "only %lld of %lld stretches have an extreme sample of v inside: the test says little", t.interior, t.cases);
    CHECK(t.most_calls == 4, "no stretch read both samples beside the root");
    std::printf("%lld stretches, %lld with an extreme sample of v strictly inside, v bit-identical to the exhaustive result in %.6f, worst |d| %.3e\n",
                t.cases, t.interior, (double)t.v_identical / (double)t.cases, t.worst);

    // coefficients no run has: the candidate indices stay in [m0, m1] and nothing is undefined
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double odd[] = {nan, inf, -inf, 1e300, -1e300, 1e-300, 0.0, -0.0, 1.0, -3.5, 4.9e-324, 1.7976931348623157e308};
    const int n_odd = (int)(sizeof(odd) / sizeof(odd[0]));
    Tally u;
    const int stretches[][2] = {{1, 1}, {1, 2}, {1, 3}, {7, 9}, {1, 3000}, {2147480000, 2147483000}, {1, 2147483646}};
    for (const auto& s : stretches)
        for (int i = 0; i < n_odd; ++i)
            for (int k = 0; k < n_odd; ++k)
                for (int l = 0; l < n_odd; ++l) {
                    // q'(m) = c1 + 2 c2 m + 3 c3 m^2 from (i, k, l), v'(m) from (k, l)
                    const double c[10] = {0.0, odd[i], odd[k], odd[l], 0.0, odd[k], odd[l], odd[i], odd[k], odd[l]};
                    one_stretch(c, s[0], s[1], false, u);
                }
    for (int it = 0; it < 200000; ++it) {                                     // random bit patterns as coefficients
        double c[10];
        for (double& x : c) {
            const unsigned long long bits = rng();
            __builtin_memcpy(&x, &bits, sizeof x);
        }
        const int m0 = pick(1, 2147480000), m1 = m0 + pick(0, 3000);
        one_stretch(c, m0, m1, false, u);
    }
    std::printf("%lld stretches of coefficients outside any run: every candidate inside its stretch\n", u.cases);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}

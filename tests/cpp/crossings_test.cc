// crossings_test.cc — the two crossing rules of longtermplanner_amd/csrc/ltp_crossings.hpp on the host, as k_first_exit and k_settle
// run them. `crossings_test first` checks first_outside against the exhaustive forward loop, `crossings_test last` checks
// last_outside against the exhaustive REVERSE loop, both over the same fma expressions (include/ltp_run_tables.hpp: run_eval): for
// random runs of the sampler's magnitudes (the draw of envelope_arrays_extremes_test.cc), Ts in {1e-3, 1/1024, 4e-3} and stretches
// of 1, 2, 3 .. 3000 samples, with boxes at random fractions of the stretch's own range, boxes that contain everything, boxes that
// contain nothing and one-sided boxes; `last` also with boxes centred on the stretch's last sample (the shape of a tolerance around
// the value a joint comes to rest at):
//   a, j  identical to the exhaustive index;
//   q, v  never on the wrong side of it (first: never earlier, last: never later); the reported sample is outside; where the result
//         differs (or is none), every skipped outside sample is outside by <= 1e-12 — such cases are counted and the count is printed.
// Also the two halves the kernel calls (the candidate and the locate function) against the whole rule, and coefficients no run has
// (c[3] == 0, c[2] == c[3] == 0, all zero, NaN, infinite, 1e300, random bit patterns): the result is -1 or inside [m0, m1], every
// evaluated index is inside [m0, m1] and a call makes at most kCrossingCandidates + kBisectSteps evaluations. No undefined
// behaviour: the program is also built with -fsanitize=address,undefined,float-cast-overflow. A stand-alone program;
// tests/test_first_exit_cpu.py and tests/test_settle_cpu.py compile and run it.
#include "ltp_crossings.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

constexpr int kBound = ltp::kCrossingCandidates + ltp::kBisectSteps;
static_assert(kBound == 37, "the documented bound: 6 + 31 evaluations per call");

// The two directions: the rule's functions, the end the exhaustive loop starts from, the side on which a q / v result may be
// excused, and the words of the report.
struct First {
    static constexpr unsigned long long kSeed = 20260102;
    static constexpr int kNone = ltp::kNoCandidate;
    static constexpr bool kBoxesAtTheLastSample = false;
    static constexpr const char* kRule = "first_outside";
    static constexpr const char* kFound = "with an exit";
    static constexpr const char* kExcused = "later";
    static constexpr const char* kWrong = "earlier";
    template <class R, class E> static int whole(int m0, int m1, R&& r, E&& e, double lo, double hi) { return ltp::first_outside(m0, m1, r, e, lo, hi); }
    template <class R, class E> static int candidate(int m0, int m1, R&& r, E&& e, double lo, double hi) { return ltp::first_outside_candidate(m0, m1, r, e, lo, hi); }
    template <class R, class E> static int locate(int m0, int m1, R&& r, E&& e, double lo, double hi, int bad) { return ltp::locate_outside(m0, m1, r, e, lo, hi, bad); }
    static int constant(int m0, int, double value, double lo, double hi) { return ltp::first_outside_constant(m0, value, lo, hi); }
    template <class R> static void check_candidate(const char*, int, int, R&&, int) {}
    static int loop_from(int m0, int) { return m0; }
    static constexpr int kLoopStep = 1;
    static bool excusable(int got, int want) { return want >= 0 && (got < 0 || got > want); }
    // the samples the rule passed over on its way to `got`, the loop's answer among them
    static int skipped_from(int, int, int want) { return want; }
    static int skipped_to(int m1, int got, int) { return got < 0 ? m1 : got - 1; }
};

struct Last {
    static constexpr unsigned long long kSeed = 20260103;
    static constexpr int kNone = ltp::kNoLastCandidate;
    static constexpr bool kBoxesAtTheLastSample = true;
    static constexpr const char* kRule = "last_outside";
    static constexpr const char* kFound = "with an outside sample";
    static constexpr const char* kExcused = "earlier";
    static constexpr const char* kWrong = "later";
    template <class R, class E> static int whole(int m0, int m1, R&& r, E&& e, double lo, double hi) { return ltp::last_outside(m0, m1, r, e, lo, hi); }
    template <class R, class E> static int candidate(int m0, int m1, R&& r, E&& e, double lo, double hi) { return ltp::last_outside_candidate(m0, m1, r, e, lo, hi); }
    template <class R, class E> static int locate(int m0, int m1, R&& r, E&& e, double lo, double hi, int bad) { return ltp::locate_last_outside(m0, m1, r, e, lo, hi, bad); }
    static int constant(int, int m1, double value, double lo, double hi) { return ltp::last_outside_constant(m1, value, lo, hi); }
    template <class R> static void check_candidate(const char* letter, int m0, int m1, R&& roots, int bad)
    {
        CHECK(bad == kNone || (bad >= m0 && bad <= m1), "%s of [%d, %d]: candidate %d", letter, m0, m1, bad);
        if (bad != kNone && bad < m1) {
            const int next = ltp::candidate_after(m0, m1, roots, bad);
            CHECK(next > bad && next <= m1, "%s of [%d, %d]: candidate_after(%d) = %d", letter, m0, m1, bad, next);
        }
    }
    static int loop_from(int, int m1) { return m1; }
    static constexpr int kLoopStep = -1;
    // (the settling sample is the last outside sample + 1: never later than the loop's)
    static bool excusable(int got, int want) { return want >= 0 && got < want; }
    static int skipped_from(int m0, int got, int) { return got < 0 ? m0 : got + 1; }
    static int skipped_to(int, int, int want) { return want; }
};

struct Tally {
    long long calls = 0, found = 0, none = 0, bisected = 0, excused = 0, most_evals = 0;
    double worst_excused = 0.0;
};

// the rule of direction D for array x (0 q, 1 v, 2 a, 3 j) on the stretch, with every evaluation counted and its index checked
template <class D>
int rule(const double* c, int x, int m0, int m1, double lo, double hi, Tally& t)
{
    long long evals = 0;
    bool beyond = false;
    auto seen = [&](int m) {
        ++evals;
        if (m < m0 || m > m1) beyond = true;
    };
    // q and v: the whole rule with counted evaluations, then the two halves the kernel calls
    auto with_roots = [&](const char* letter, auto roots, auto value_at) {
        const int got = D::whole(m0, m1, roots, [&](int m) { seen(m); return value_at(c, m); }, lo, hi);
        const int bad = D::candidate(m0, m1, roots, [&](int m) { return value_at(c, m); }, lo, hi);
        D::check_candidate(letter, m0, m1, roots, bad);
        const int two = bad == D::kNone ? -1 : D::locate(m0, m1, roots, [&](int m) { return value_at(c, m); }, lo, hi, bad);
        CHECK(two == got, "%s of [%d, %d]: the two halves give %d, %s %d", letter, m0, m1, two, D::kRule, got);
        return got;
    };
    int got;
    if (x == 0) {
        got = with_roots("q", [&] { return ltp::qprime_roots(c); }, eval_q);
    } else if (x == 1) {
        got = with_roots("v", [&] { return ltp::vprime_root(c); }, eval_v);
    } else if (x == 2) {
        got = D::whole(m0, m1, [] { return ltp::no_roots(); }, [&](int m) { seen(m); return eval_a(c, m); }, lo, hi);
    } else {
        got = D::constant(m0, m1, c[9], lo, hi);
    }
    CHECK(!beyond, "array %d of [%d, %d]: an index outside the stretch was evaluated", x, m0, m1);
    CHECK(evals <= kBound, "array %d of [%d, %d]: %lld evaluations", x, m0, m1, evals);
    CHECK(got == -1 || (got >= m0 && got <= m1), "array %d of [%d, %d]: result %d", x, m0, m1, got);
    t.most_evals = std::max(t.most_evals, evals);
    if (evals > ltp::kCrossingCandidates) ++t.bisected;
    ++t.calls;
    return got;
}

double value(const double* c, int x, int m) { return x == 0 ? eval_q(c, m) : x == 1 ? eval_v(c, m) : x == 2 ? eval_a(c, m) : c[9]; }

// one (array, stretch, box) of a realistic run against the exhaustive loop, run from D's end of the stretch
template <class D>
void against_the_loop(const double* c, int x, int m0, int m1, double lo, double hi, Tally& t)
{
    const int got = rule<D>(c, x, m0, m1, lo, hi, t);
    int want = -1;
    for (int m = D::loop_from(m0, m1); m >= m0 && m <= m1 && want < 0; m += D::kLoopStep)
        if (ltp::outside_box(value(c, x, m), lo, hi)) want = m;
    if (want >= 0) ++t.found; else ++t.none;
    if (got >= 0) CHECK(ltp::outside_box(value(c, x, got), lo, hi), "array %d of [%d, %d]: the reported sample %d is inside", x, m0, m1, got);
    if (x >= 2) {
        CHECK(got == want, "array %d of [%d, %d] box [%.17g, %.17g]: %d, the loop gives %d", x, m0, m1, lo, hi, got, want);
        return;
    }
    if (got == want) return;
    CHECK(D::excusable(got, want), "array %d of [%d, %d]: %d is %s than the loop's %d", x, m0, m1, got, D::kWrong, want);
    if (want < 0) return;
    // excused, or none: every outside sample that was skipped is outside by rounding alone
    ++t.excused;
    const int end = D::skipped_to(m1, got, want);
    for (int m = D::skipped_from(m0, got, want); m <= end; ++m) {
        const double s = value(c, x, m);
        if (!ltp::outside_box(s, lo, hi)) continue;
        const double by = s < lo ? lo - s : s - hi;
        t.worst_excused = std::fmax(t.worst_excused, by);
        CHECK(by <= 1e-12, "array %d of [%d, %d]: sample %d skipped although it is outside by %.3e (got %d)", x, m0, m1, m, by, got);
    }
}

template <class D>
int run()
{
    std::mt19937_64 rng(D::kSeed);
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    const double sample_times[3] = {1e-3, 1.0 / 1024.0, 4e-3};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    Tally t;
    for (double Ts : sample_times) {
        for (int it = 0; it < 6000; ++it) {
            // lengths: 1, 2, 3 and short stretches often, long ones too (the draw of envelope_arrays_extremes_test.cc)
            const int kind = it % 6;
            const int n = kind == 0 ? 1 + it / 6 % 3 : kind <= 2 ? pick(1, 40) : pick(1, 3000);
            const int m0 = pick(1, 60), m1 = m0 + n - 1;
            const double T = (double)m1 * Ts;
            double J = uni(-1.0, 1.0) * std::min({1e4, 40.0 / T, 12.0 / (T * T)});
            double a_s = uni(-1.0, 1.0) * std::min(20.0, 6.0 / T);
            double v_s = uni(-3.0, 3.0);
            const double q_s = uni(-3.0, 3.0);
            const int shape = it % 7;
            if (shape == 0) J = 0.0;                                          // c[3] == c[6] == 0
            if (shape == 1) { J = 0.0; a_s = 0.0; }                           // q linear, v constant
            if (shape == 2 && J != 0.0) {                                     // the vertex of v near or inside the stretch
                const double rho = uni((double)m0 - 2.0, (double)m1 + 2.0);
                a_s = -J * Ts * (rho + 0.5);
            }
            if (shape == 3 && J != 0.0) {                                     // ... and a turning point of q there too: v changes sign
                const double rho = uni((double)m0 - 2.0, (double)m1 + 2.0);
                a_s = -J * Ts * (rho + 0.5);
                const double mid = uni((double)m0, (double)m1);
                v_s = -Ts * (mid * a_s + Ts * J * mid * (mid + 1.0) / 2.0);
            }
            double c[10];
            run_coef(c, J, a_s, v_s, q_s, Ts);
            for (int x = 0; x < 4; ++x) {
                double mn = inf, mx = -inf;
                for (int m = m0; m <= m1; ++m) {
                    mn = std::fmin(mn, value(c, x, m));
                    mx = std::fmax(mx, value(c, x, m));
                }
                const double w = mx - mn;
                for (int b = 0; b < 4; ++b)                                   // boxes at random fractions of the stretch's own range
                    against_the_loop<D>(c, x, m0, m1, mn + uni(0.0, 1.0) * w, mx - uni(0.0, 1.0) * w, t);
                against_the_loop<D>(c, x, m0, m1, mn + uni(0.05, 0.45) * w, mx - uni(0.05, 0.45) * w, t);
                if (D::kBoxesAtTheLastSample) {
                    const double e = value(c, x, m1);
                    for (int b = 0; b < 3; ++b)                               // boxes centred on the stretch's last sample
                        against_the_loop<D>(c, x, m0, m1, e - uni(0.05, 0.45) * w, e + uni(0.05, 0.45) * w, t);
                    against_the_loop<D>(c, x, m0, m1, e - uni(0.0, 0.02) * w, e + uni(0.0, 0.02) * w, t);
                }
                against_the_loop<D>(c, x, m0, m1, mn, mx, t);                 // contains everything, the extremes on its faces
                against_the_loop<D>(c, x, m0, m1, -inf, inf, t);
                against_the_loop<D>(c, x, m0, m1, mn - 1.0, mx + 1.0, t);
                against_the_loop<D>(c, x, m0, m1, mx + 1.0, mx + 2.0, t);     // contains nothing
                against_the_loop<D>(c, x, m0, m1, inf, -inf, t);
                against_the_loop<D>(c, x, m0, m1, mn + uni(0.0, 1.0) * w, inf, t);    // one-sided
                against_the_loop<D>(c, x, m0, m1, -inf, mx - uni(0.0, 1.0) * w, t);
                against_the_loop<D>(c, x, m0, m1, nan, mx - uni(0.0, 1.0) * w, t);    // a NaN bound is no bound
            }
        }
    }
    CHECK(t.found * 4 >= t.calls && t.none * 10 >= t.calls, "%lld %s and %lld without one among %lld calls: the test says little", t.found, D::kFound, t.none, t.calls);
    CHECK(t.bisected * 40 >= t.calls, "only %lld of %lld calls bisected", t.bisected, t.calls);
    std::printf("%lld calls, %lld %s, %lld bisected, most evaluations %lld (bound %d); q / v %s than the exhaustive loop by rounding alone: %lld "
                "(worst %.3e)\n", t.calls, t.found, D::kFound, t.bisected, t.most_evals, kBound, D::kExcused, t.excused, t.worst_excused);

    // coefficients no run has: results and evaluated indices stay in [m0, m1], the evaluation count under the bound
    const double odd[] = {nan, inf, -inf, 1e300, -1e300, 1e-300, 0.0, -0.0, 1.0, -3.5, 4.9e-324, 1.7976931348623157e308};
    const int n_odd = (int)(sizeof(odd) / sizeof(odd[0]));
    const double boxes[][2] = {{-1.0, 1.0}, {0.0, 0.0}, {-inf, inf}, {inf, -inf}, {nan, nan}, {-1e300, 1e300}, {1.0, inf}, {-inf, -1.0}, {nan, 0.5}};
    const int stretches[][2] = {{1, 1}, {1, 2}, {1, 3}, {7, 9}, {1, 3000}, {2147480000, 2147483000}, {1, 2147483646}};
    Tally u;
    for (const auto& s : stretches)
        for (int i = 0; i < n_odd; ++i)
            for (int k = 0; k < n_odd; ++k)
                for (int l = 0; l < n_odd; ++l) {
                    // (i, k, l) as (c1, c2, c3) of q, (c4, c5, c6) of v and, its first two, (c7, c8) of a: c[3] == 0, c[2] == c[3] == 0
                    // and all zero are among them
                    const double c[10] = {odd[(i + k) % n_odd], odd[i], odd[k], odd[l], odd[i], odd[k], odd[l], odd[i], odd[k], odd[l]};
                    const double* b = boxes[(i + 5 * k + 7 * l) % 9];
                    for (int x = 0; x < 4; ++x) rule<D>(c, x, s[0], s[1], b[0], b[1], u);
                }
    for (int it = 0; it < 200000; ++it) {                                     // random bit patterns as coefficients and bounds
        double c[10], b[2];
        for (double& x : c) {
            const unsigned long long bits = rng();
            __builtin_memcpy(&x, &bits, sizeof x);
        }
        for (double& x : b) {
            const unsigned long long bits = rng();
            __builtin_memcpy(&x, &bits, sizeof x);
        }
        const int m0 = pick(1, 2147480000), m1 = m0 + pick(0, 3000);
        for (int x = 0; x < 4; ++x) rule<D>(c, x, m0, m1, b[0], b[1], u);
    }
    CHECK(u.most_evals > 30, "no degenerate call bisected a long stretch (most evaluations %lld)", u.most_evals);
    std::printf("%lld calls on coefficients outside any run: every index inside its stretch, most evaluations %lld (bound %d)\n", u.calls, u.most_evals, kBound);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "first")) return run<First>();
    if (argc == 2 && !std::strcmp(argv[1], "last")) return run<Last>();
    std::printf("usage: %s first|last\n", argv[0]);
    return 2;
}

// ltp_crossings.hpp — the first-exit rule (k_first_exit, ltp_consumers.hip; ltp_first_exit_batch, include/ltp_hip.h): the first
// sample of a stretch m0 .. m1 of a run that lies outside a box [lo, hi]. Inside a run every array is a polynomial in the run-local
// index m (run_eval), so the stretch is cut at the candidates of ltp_extremes.hpp — its two end samples and the samples either side
// of a real root of the derivative — into pieces on which the polynomial is monotone:
//   (1) first_outside_candidate: fold_candidates with a fold that keeps the smallest candidate whose sample is outside. None: the
//       stretch holds no exit (its minimum and maximum are candidates: the envelope's rule). This is the bulk path, and it costs what
//       the envelope fold costs: the same candidates, two compares per sample instead of a minimum and a maximum.
//   (2) otherwise the candidates before that one are inside, so the first exit lies in the piece that ends at it: candidate_before
//       names the piece's left end (the same candidates again, indices only, nothing is evaluated), and bisect_outside finds the
//       first outside sample of the piece under the invariant "left is not outside, right is outside".
// "outside" is x < lo || x > hi, the comparison of beyond_end_limits: false for a NaN sample and for a NaN bound. Every sample is
// handed to the caller's eval(m), which evaluates it as run_eval does: a reported sample IS outside the box, bit for bit.
//
// Guarantees.
//   a (fma(c[8], m, c[7]): one rounding of a monotone function of m) with fold_ends' candidates and j (the run's constant) are
//     exhaustive by construction: the result is the first outside sample of the stretch.
//   q and v equal the exhaustive scan unless an earlier sample lies outside by rounding alone (<= 1e-12, the project's bound for the
//     analytic envelope form): the call never reports an exit the row does not have; it may report a later one only past samples
//     that are outside by <= 1e-12.
//   Whatever the coefficients (NaN, infinite, 1e300): no double is converted to int before it is known to lie in range
//     (fold_candidates' rule), every index handed to eval and every result lies in [m0, m1] (or is -1), and a call makes at most
//     kCrossingCandidates + kBisectSteps = 6 + 31 evaluations: <= 6 in (1), none in candidate_before, <= 31 in the bisection
//     (right - left < 2^31 halves to 1 in 31 steps; the loop is counted, not conditional on the data alone).
// Host logic without HIP headers, in the manner of ltp_extremes.hpp: tests/cpp/first_outside_test.cc runs the functions the kernel
// runs against the exhaustive loop.
#pragma once
#include "ltp_extremes.hpp"

namespace ltp {

constexpr int kNoCandidate = 0x7fffffff;   // first_outside_candidate: no candidate of the stretch is outside
constexpr int kCrossingCandidates = 6;     // evaluations of step (1) at the most (fold_candidates: 2 ends + 2 per root)
constexpr int kBisectSteps = 31;           // evaluations of step (2) at the most

// the comparison of beyond_end_limits (ltp_device.hpp): a NaN is never outside
LTP_KNOTS_HD inline bool outside_box(double x, double lo, double hi) { return x < lo || x > hi; }

// what a monotone array hands to the functions below for its roots: none, so its candidates are fold_ends'
LTP_KNOTS_HD inline StretchRoots no_roots()
{
    const double none = __builtin_nan("");
    return StretchRoots{none, none};
}

// (1) the smallest candidate of the stretch m0 .. m1 (m0 <= m1) whose sample is outside [lo, hi], kNoCandidate for none
template <class Roots, class Eval>
LTP_KNOTS_HD inline int first_outside_candidate(int m0, int m1, Roots&& roots_of_run, Eval&& eval, double lo, double hi)
{
    int bad = kNoCandidate;
    fold_candidates(m0, m1, roots_of_run, [&](int m) {
        const bool out = outside_box(eval(m), lo, hi);
        bad = out && m < bad ? m : bad;
    });
    return bad;
}

// the largest candidate of the stretch below `bad` (m0 < bad <= m1): the left end of the monotone piece that ends at bad
template <class Roots>
LTP_KNOTS_HD inline int candidate_before(int m0, int m1, Roots&& roots_of_run, int bad)
{
    int prev = m0;
    fold_candidates(m0, m1, roots_of_run, [&](int m) { prev = m < bad && m > prev ? m : prev; });
    return prev;
}

// the first outside sample of (left, right], given that right is outside and that the samples turn from inside to outside once
// between the two: at most kBisectSteps evaluations, all of them strictly between left and right
template <class Eval>
LTP_KNOTS_HD inline int bisect_outside(int left, int right, Eval&& eval, double lo, double hi)
{
    for (int step = 0; step < kBisectSteps && right - left > 1; ++step) {
        const int mid = left + (right - left) / 2;
        const bool out = outside_box(eval(mid), lo, hi);
        right = out ? mid : right;
        left = out ? left : mid;
    }
    return right;
}

// (2) given bad = first_outside_candidate(..) != kNoCandidate of the same stretch, roots and box
template <class Roots, class Eval>
LTP_KNOTS_HD inline int locate_outside(int m0, int m1, Roots&& roots_of_run, Eval&& eval, double lo, double hi, int bad)
{
    if (bad <= m0) return m0;
    return bisect_outside(candidate_before(m0, m1, roots_of_run, bad), bad, eval, lo, hi);
}

// the first m in [m0, m1] with eval(m) outside [lo, hi], -1 for none
template <class Roots, class Eval>
LTP_KNOTS_HD inline int first_outside(int m0, int m1, Roots&& roots_of_run, Eval&& eval, double lo, double hi)
{
    const int bad = first_outside_candidate(m0, m1, roots_of_run, eval, lo, hi);
    if (bad == kNoCandidate) return -1;
    return locate_outside(m0, m1, roots_of_run, eval, lo, hi, bad);
}

// a constant array (j: the run's jerk): its first sample or nothing
LTP_KNOTS_HD inline int first_outside_constant(int m0, double value, double lo, double hi) { return outside_box(value, lo, hi) ? m0 : -1; }

// ---------------------------------------------------------------------------------------
// The settling rule (k_settle, ltp_consumers.hip; ltp_settle_batch, include/ltp_hip.h): the LAST sample of a stretch m0 .. m1 that
// lies outside the box — the rule above read from the other end, with the same candidates, the same comparison and the same eval:
//   (1) last_outside_candidate: the LARGEST candidate whose sample is outside. None: the stretch holds no outside sample.
//   (2) otherwise every candidate after that one is inside, so each piece between two of them is inside throughout, and the piece
//       from `bad` to its successor (candidate_after: indices only, nothing is evaluated) turns from outside to inside once:
//       bisect_inside finds its last outside sample under the invariant "left is outside, right is not". One bisection is enough.
// Guarantees, as above: a and j are exhaustive by construction; for q and v the reported sample IS outside, bit for bit, and the
// rule may report an earlier last outside sample than the exhaustive scan only past samples that are outside by rounding alone
// (<= 1e-12). Whatever the coefficients: every index handed to eval and every result lies in [m0, m1] (or is -1), at most
// kCrossingCandidates + kBisectSteps evaluations per call, the loop counted. tests/cpp/last_outside_test.cc runs these functions
// against the exhaustive reverse loop.
constexpr int kNoLastCandidate = -0x7fffffff - 1;   // last_outside_candidate: no candidate of the stretch is outside

// (1) the largest candidate of the stretch m0 .. m1 (m0 <= m1) whose sample is outside [lo, hi], kNoLastCandidate for none
template <class Roots, class Eval>
LTP_KNOTS_HD inline int last_outside_candidate(int m0, int m1, Roots&& roots_of_run, Eval&& eval, double lo, double hi)
{
    int bad = kNoLastCandidate;
    fold_candidates(m0, m1, roots_of_run, [&](int m) {
        const bool out = outside_box(eval(m), lo, hi);
        bad = out && m > bad ? m : bad;
    });
    return bad;
}

// the smallest candidate of the stretch above `bad` (m0 <= bad < m1): the right end of the monotone piece that starts at bad
template <class Roots>
LTP_KNOTS_HD inline int candidate_after(int m0, int m1, Roots&& roots_of_run, int bad)
{
    int next = m1;
    fold_candidates(m0, m1, roots_of_run, [&](int m) { next = m > bad && m < next ? m : next; });
    return next;
}

// the last outside sample of [left, right), given that left is outside, right is not and that the samples turn from outside to
// inside once between the two: at most kBisectSteps evaluations, all of them strictly between left and right
template <class Eval>
LTP_KNOTS_HD inline int bisect_inside(int left, int right, Eval&& eval, double lo, double hi)
{
    for (int step = 0; step < kBisectSteps && right - left > 1; ++step) {
        const int mid = left + (right - left) / 2;
        const bool out = outside_box(eval(mid), lo, hi);
        left = out ? mid : left;
        right = out ? right : mid;
    }
    return left;
}

// (2) given bad = last_outside_candidate(..) != kNoLastCandidate of the same stretch, roots and box
template <class Roots, class Eval>
LTP_KNOTS_HD inline int locate_last_outside(int m0, int m1, Roots&& roots_of_run, Eval&& eval, double lo, double hi, int bad)
{
    if (bad >= m1) return m1;
    return bisect_inside(bad, candidate_after(m0, m1, roots_of_run, bad), eval, lo, hi);
}

// the last m in [m0, m1] with eval(m) outside [lo, hi], -1 for none
template <class Roots, class Eval>
LTP_KNOTS_HD inline int last_outside(int m0, int m1, Roots&& roots_of_run, Eval&& eval, double lo, double hi)
{
    const int bad = last_outside_candidate(m0, m1, roots_of_run, eval, lo, hi);
    if (bad == kNoLastCandidate) return -1;
    return locate_last_outside(m0, m1, roots_of_run, eval, lo, hi, bad);
}

// a constant array (j: the run's jerk): its last sample or nothing
LTP_KNOTS_HD inline int last_outside_constant(int m1, double value, double lo, double hi) { return outside_box(value, lo, hi) ? m1 : -1; }

}  // namespace ltp

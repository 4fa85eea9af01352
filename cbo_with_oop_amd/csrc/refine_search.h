// One start's L-BFGS ascent as a state machine: lockstep_lbfgs of utils_functions/causal_optimizer.py for ONE search,
// restated so that the caller owns the evaluations -- it asks the state for the point to evaluate (refine_point),
// evaluates value and gradient there however it likes (a device kernel between two tile solves, a host test on an
// analytic function) and feeds the pair back (refine_feed), once per round.  Plain C++17, no HIP headers: the same text
// compiles under hipcc and under g++ into the host simulators of the tests (tests/support/*_search_sim.cpp).
// The device's two searches are instantiations of it: RefineState, inside a set's box, in small_sets_refine_kernel
// (kernels_sets_refine.hip); and the hyper-parameter MLE's without a box (mle_search.h, which wraps the Logexp transform
// around it) in mle_sets_kernel (kernels_mle.hip).  Without a box the projected gradient is the gradient and nothing is
// clipped: those lines are not compiled, the rest is the same text.
//
// What it carries over from lockstep_lbfgs, operation for operation: the projected gradient; the two-loop recursion over at
// most 8 curvature pairs; the steepest-descent fallback (history cleared) when the direction is not a descent direction;
// the first step min(1, 1 / |pg|); trial points clipped to the box; the Armijo test (c1 = 1e-4) with halving on failure
// and the stop when t max|d| < 1e-14; the curvature test s.y > 1e-12 |s| |y|; pgtol = 1e-5 and ftol = 2.2e-9; a non-finite
// trial value counts as an Armijo failure.  One addition: a non-finite value at the start ends the search there
// (CBO_REFINE_NAN_START) instead of halving a step from nowhere until the rounds run out.
//
// The search MINIMISES -value, as lockstep_lbfgs does: f and g hold the negated value and gradient.
// Floating-point contraction must be off (-ffp-contract=off for g++; the pragma below for clang): the sums are the
// sequential sums written here, nothing fused.
#pragma once

#include <math.h>

#include "cbo_hip.h"

#if defined(__HIPCC__)
#define CBO_HD __host__ __device__
#define CBO_REFINE_UNROLL _Pragma("unroll")
#else
#define CBO_HD
#define CBO_REFINE_UNROLL
#endif
#if defined(__clang__)
#define CBO_REFINE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CBO_REFINE_NO_CONTRACT
#endif

namespace cbo {

constexpr int kRefineHistory = 8;
constexpr int kRefineRunning = -1;          // the status of a search that still wants evaluations (never reported)
constexpr double kRefinePgtol = 1e-5, kRefineFtol = 2.2e-9, kRefineC1 = 1e-4;
constexpr double kRefineMinStep = 1e-14, kRefineCurvature = 1e-12;

// x, f, g: the accepted point, -value and -gradient there.  dir, t: the search direction and the step of the next trial.
// xt: the point the caller is evaluating.  S, Y: the rings of curvature pairs, kRefineHistory x d doubles each in the
// caller's storage (pair p, oldest first, in slot (head + p) % kRefineHistory, element k at [slot * d + k]).
// N: the most unknowns a search can have (d <= N).  BOX: the search keeps to a box lo <= x <= hi; a search without one
// never reads the lo and hi of the functions below (pass nullptr).
template <int N, bool BOX>
struct RefineSearch {
    double x[N], g[N], dir[N], xt[N];
    double f, t;
    double *S, *Y;
    int d, pairs, head, status, rounds, started;
};
using RefineState = RefineSearch<CBO_MAX_DIM, true>;           // the gradient refinement's: a set's box, at most CBO_MAX_DIM wide

template <int N>
CBO_HD inline double refine_dot(const double *a, const double *b, int d)
{
    CBO_REFINE_NO_CONTRACT
    double s = 0.0;
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k)
        if (k < d) s = s + a[k] * b[k];
    return s;
}

// max |a_k|, NaN if any of them is (numpy.max)
template <int N>
CBO_HD inline double refine_max_abs(const double *a, int d)
{
    double m = 0.0;
    bool nan = false;
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k)
        if (k < d) {
            const double v = fabs(a[k]);
            nan = nan || (v != v);
            if (v > m) m = v;
        }
    return nan ? (double)NAN : m;
}

CBO_HD inline double refine_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
// ... to coordinate k of the box, where there is one
template <bool BOX>
CBO_HD inline double refine_into_box(double v, const double *lo, const double *hi, int k)
{
    if constexpr (BOX) return refine_clip(v, lo[k], hi[k]);
    else return v;
}

// g with the components that point out of the box at an active bound put to zero (written to buf); without a box, g itself
template <int N, bool BOX>
CBO_HD inline const double *refine_projected_gradient(const RefineSearch<N, BOX> &s, const double *lo, const double *hi,
                                                      double *buf)
{
    if constexpr (!BOX) {
        return s.g;
    } else {
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k)
            if (k < s.d) {
                double v = s.g[k];
                if (s.x[k] <= lo[k] && v > 0.0) v = 0.0;
                if (s.x[k] >= hi[k] && v < 0.0) v = 0.0;
                buf[k] = v;
            }
        return buf;
    }
}

// the two-loop recursion from the projected gradient pg; a direction that does not descend is replaced by -pg and the
// history cleared
template <int N, bool BOX>
CBO_HD inline void refine_direction(RefineSearch<N, BOX> &s, const double *pg)
{
    CBO_REFINE_NO_CONTRACT
    const int d = s.d;
    double q[N], alphas[kRefineHistory];
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k) q[k] = (k < d) ? pg[k] : 0.0;
    CBO_REFINE_UNROLL
    for (int p = kRefineHistory - 1; p >= 0; --p) {           // newest pair first
        if (p >= s.pairs) continue;
        const double *sp = s.S + ((s.head + p) % kRefineHistory) * d, *yp = s.Y + ((s.head + p) % kRefineHistory) * d;
        double sv[N], yv[N];
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) { sv[k] = (k < d) ? sp[k] : 0.0; yv[k] = (k < d) ? yp[k] : 0.0; }
        const double a = refine_dot<N>(sv, q, d) / refine_dot<N>(yv, sv, d);
        alphas[p] = a;
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k)
            if (k < d) q[k] = q[k] - a * yv[k];
    }
    if (s.pairs > 0) {
        const int slot = (s.head + s.pairs - 1) % kRefineHistory;
        double sv[N], yv[N];
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) { sv[k] = (k < d) ? s.S[slot * d + k] : 0.0; yv[k] = (k < d) ? s.Y[slot * d + k] : 0.0; }
        const double gamma = refine_dot<N>(sv, yv, d) / refine_dot<N>(yv, yv, d);
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k)
            if (k < d) q[k] = q[k] * gamma;
    }
    CBO_REFINE_UNROLL
    for (int p = 0; p < kRefineHistory; ++p) {                // oldest pair first
        if (p >= s.pairs) continue;
        const double *sp = s.S + ((s.head + p) % kRefineHistory) * d, *yp = s.Y + ((s.head + p) % kRefineHistory) * d;
        double sv[N], yv[N];
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) { sv[k] = (k < d) ? sp[k] : 0.0; yv[k] = (k < d) ? yp[k] : 0.0; }
        const double b = alphas[p] - refine_dot<N>(yv, q, d) / refine_dot<N>(yv, sv, d);
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k)
            if (k < d) q[k] = q[k] + b * sv[k];
    }
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k) s.dir[k] = (k < d) ? -q[k] : 0.0;
    if (refine_dot<N>(s.dir, pg, d) >= 0.0) {
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) s.dir[k] = (k < d) ? -pg[k] : 0.0;
        s.pairs = 0;
        s.head = 0;
    }
}

template <int N, bool BOX>
CBO_HD inline void refine_set_trial(RefineSearch<N, BOX> &s, const double *lo, const double *hi)
{
    CBO_REFINE_NO_CONTRACT
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k)
        s.xt[k] = (k < s.d) ? (s.status == kRefineRunning ? refine_into_box<BOX>(s.x[k] + s.t * s.dir[k], lo, hi, k) : s.x[k]) : 0.0;
}

// The search begins at x0 clipped to the box; the first point to evaluate is that point.
template <int N, bool BOX>
CBO_HD inline void refine_begin(RefineSearch<N, BOX> &s, int d, const double *x0, const double *lo, const double *hi, double *S, double *Y)
{
    s.d = d; s.pairs = 0; s.head = 0; s.status = kRefineRunning; s.rounds = 0; s.started = 0;
    s.S = S; s.Y = Y; s.f = 0.0; s.t = 0.0;
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k) {
        s.x[k] = (k < d) ? refine_into_box<BOX>(x0[k], lo, hi, k) : 0.0;
        s.xt[k] = s.x[k];
        s.g[k] = 0.0;
        s.dir[k] = 0.0;
    }
}

// the point whose value and gradient refine_feed expects next (the accepted point itself once the search has ended)
template <int N, bool BOX>
CBO_HD inline const double *refine_point(const RefineSearch<N, BOX> &s) { return s.xt; }
template <int N, bool BOX>
CBO_HD inline bool refine_done(const RefineSearch<N, BOX> &s) { return s.status != kRefineRunning; }

// value and gradient of the function being MAXIMISED at refine_point().  The first call is the start's own evaluation and
// counts as no round; every later one is a round.  After max_rounds rounds a search still running ends with
// CBO_REFINE_MAX_ROUNDS.  Feeding a search that has ended changes nothing.
// accepted(): called when the point just fed has become the accepted point -- the start, and every trial that passed the
// Armijo test -- before the next direction is taken from it: a caller that keeps something of its own beside x moves it there.
template <int N, bool BOX, class Accepted>
CBO_HD inline void refine_feed(RefineSearch<N, BOX> &s, const double *lo, const double *hi, double value, const double *grad,
                               int max_rounds, Accepted accepted)
{
    CBO_REFINE_NO_CONTRACT
    if (s.status != kRefineRunning) return;
    const int d = s.d;
    double buf[N];
    if (!s.started) {
        s.started = 1;
        s.f = -value;
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) s.g[k] = (k < d) ? -grad[k] : 0.0;
        accepted();
        if (!isfinite(s.f)) {
            s.status = CBO_REFINE_NAN_START;
            return;
        }
        const double *pg = refine_projected_gradient(s, lo, hi, buf);
        refine_direction(s, pg);
        const double n = sqrt(refine_dot<N>(pg, pg, d));
        s.t = (n > 0.0) ? (1.0 / n < 1.0 ? 1.0 / n : 1.0) : 0.0;
        if (refine_max_abs<N>(pg, d) <= kRefinePgtol) s.status = CBO_REFINE_PGTOL;
        else if (max_rounds <= 0) s.status = CBO_REFINE_MAX_ROUNDS;
        refine_set_trial(s, lo, hi);
        return;
    }
    s.rounds += 1;
    const double ft = -value;
    double step[N], gt[N];
    CBO_REFINE_UNROLL
    for (int k = 0; k < N; ++k) {
        step[k] = (k < d) ? s.xt[k] - s.x[k] : 0.0;
        gt[k] = (k < d) ? -grad[k] : 0.0;
    }
    if (!isfinite(ft) || ft > s.f + kRefineC1 * refine_dot<N>(s.g, step, d)) {
        s.t = s.t * 0.5;                                      // Armijo failed: a shorter step next round
        if (s.t * refine_max_abs<N>(s.dir, d) < kRefineMinStep) s.status = CBO_REFINE_STEP;
    } else {
        double y[N];
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) y[k] = (k < d) ? gt[k] - s.g[k] : 0.0;
        const double gain = s.f - ft;
        if (refine_dot<N>(step, y, d) > kRefineCurvature * sqrt(refine_dot<N>(step, step, d)) * sqrt(refine_dot<N>(y, y, d))) {
            int slot;
            if (s.pairs < kRefineHistory) {
                slot = (s.head + s.pairs) % kRefineHistory;
                s.pairs += 1;
            } else {
                slot = s.head;
                s.head = (s.head + 1) % kRefineHistory;
            }
            CBO_REFINE_UNROLL
            for (int k = 0; k < N; ++k)
                if (k < d) { s.S[slot * d + k] = step[k]; s.Y[slot * d + k] = y[k]; }
        }
        double big = fabs(s.f) > fabs(ft) ? fabs(s.f) : fabs(ft);
        big = big > 1.0 ? big : 1.0;
        const bool small = gain <= kRefineFtol * big;
        s.f = ft;
        CBO_REFINE_UNROLL
        for (int k = 0; k < N; ++k) { s.x[k] = s.xt[k]; s.g[k] = gt[k]; }
        accepted();
        const double *pg = refine_projected_gradient(s, lo, hi, buf);
        refine_direction(s, pg);
        s.t = 1.0;
        if (refine_max_abs<N>(pg, d) <= kRefinePgtol) s.status = CBO_REFINE_PGTOL;
        else if (small) s.status = CBO_REFINE_FTOL;
    }
    if (s.status == kRefineRunning && s.rounds >= max_rounds) s.status = CBO_REFINE_MAX_ROUNDS;
    refine_set_trial(s, lo, hi);
}

template <int N, bool BOX>
CBO_HD inline void refine_feed(RefineSearch<N, BOX> &s, const double *lo, const double *hi, double value, const double *grad,
                               int max_rounds)
{
    refine_feed(s, lo, hi, value, grad, max_rounds, [] {});
}

}  // namespace cbo

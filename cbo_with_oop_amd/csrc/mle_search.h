// One hyper-parameter MLE as a state machine: lockstep_lbfgs of utils_functions/causal_optimizer.py for ONE search with no
// box, over a model's Logexp-transformed parameters x (theta = Logexp.f(x): variance, lengthscale(s), noise variance when it
// is fitted; at most CBO_HMC_MAX_PARAMS of them).  The caller owns the evaluations: it asks the state for the parameters to
// evaluate (mle_theta), evaluates the log marginal likelihood and its gradients with respect to them however it likes (a
// device kernel between two factorisations, a host test on a closed form) and feeds the pair back (mle_feed), once per
// round.  Plain C++17, no HIP headers: the same text compiles under hipcc into mle_sets_kernel (kernels_mle.hip) and under
// g++ into the host simulator of the tests (tests/support/mle_search_sim.cpp).
//
// What it carries over from lockstep_lbfgs, operation for operation: the two-loop recursion over at most 8 curvature pairs;
// the steepest-descent fallback (history cleared) when the direction is not a descent direction; the first step
// min(1, 1 / |g|); the Armijo test (c1 = 1e-4) with halving on failure and the stop when t max|d| < 1e-14; the curvature
// test s.y > 1e-12 |s| |y|; pgtol = 1e-5 and ftol = 2.2e-9; a non-finite trial value counts as an Armijo failure; every sum
// sequential from 0 in index order.  A non-finite value at the start ends the search there (CBO_REFINE_NAN_START).
// The objective is hmc_chain.h's: f = -lml, g = -(dlml / dtheta) (1 - exp(-theta)), with that header's own Logexp functions;
// like HmcChain the state keeps theta AS EVALUATED beside x, so the reported parameters are the very doubles the likelihood
// was taken at and nothing is transformed twice.
//
// What it shares with refine_search.h: the iteration (both restate lockstep_lbfgs), the constants (kRefine*, used from
// there), the status codes (CBO_REFINE_*) and the ring layout in the caller's storage.  Why it is not a template of it:
// refine_search.h's arrays are sized CBO_MAX_DIM and its arithmetic is pinned bit for bit by its own tests; this search has
// CBO_MAX_DIM + 2 unknowns, no box (no projection of the gradient, no clip of the trial point -- with an infinite box both
// are the identity, so they are not written), and moves in x while it is fed gradients with respect to theta(x).  A common
// template would have to carry the box and the transform as policies through every function of a header that must not
// move; the text without them is the shorter one.
// Floating-point contraction must be off (-ffp-contract=off for g++; the pragma below for clang).
#pragma once

#include <math.h>

#include "cbo_hip.h"
#include "hmc_chain.h"
#include "refine_search.h"

namespace cbo {

constexpr int kMleMaxParams = CBO_HMC_MAX_PARAMS;

// x, th, f, g, dl: the accepted point, theta(x) as evaluated, -lml, its gradient with respect to x, and dlml / dtheta as
// fed there.  dir, t: the search direction and the step of the next trial.  xt, tht: the point the caller is evaluating and
// theta there.  S, Y: the rings of curvature pairs, kRefineHistory x P doubles each in the caller's storage (pair p, oldest
// first, in slot (head + p) % kRefineHistory, element k at [slot * P + k]).
struct MleSearch {
    double x[kMleMaxParams], th[kMleMaxParams], g[kMleMaxParams], dl[kMleMaxParams], dir[kMleMaxParams];
    double xt[kMleMaxParams], tht[kMleMaxParams];
    double f, t;
    double *S, *Y;
    int P, pairs, head, status, rounds, started;
};

CBO_HD inline double mle_dot(const double *a, const double *b, int P)
{
    CBO_REFINE_NO_CONTRACT
    double s = 0.0;
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k)
        if (k < P) s = s + a[k] * b[k];
    return s;
}

// max |a_k|, NaN if any of them is (numpy.max)
CBO_HD inline double mle_max_abs(const double *a, int P)
{
    double m = 0.0;
    bool nan = false;
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k)
        if (k < P) {
            const double v = fabs(a[k]);
            nan = nan || (v != v);
            if (v > m) m = v;
        }
    return nan ? (double)NAN : m;
}

// pair `slot` of a ring into v, zeros behind P
CBO_HD inline void mle_ring_read(const double *ring, int slot, int P, double *v)
{
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) v[k] = (k < P) ? ring[slot * P + k] : 0.0;
}

// the two-loop recursion from the gradient; a direction that does not descend is replaced by -g and the history cleared
CBO_HD inline void mle_direction(MleSearch &s)
{
    CBO_REFINE_NO_CONTRACT
    const int P = s.P;
    double q[kMleMaxParams], alphas[kRefineHistory], sv[kMleMaxParams], yv[kMleMaxParams];
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) q[k] = (k < P) ? s.g[k] : 0.0;
    CBO_REFINE_UNROLL
    for (int p = kRefineHistory - 1; p >= 0; --p) {           // newest pair first
        if (p >= s.pairs) continue;
        mle_ring_read(s.S, (s.head + p) % kRefineHistory, P, sv);
        mle_ring_read(s.Y, (s.head + p) % kRefineHistory, P, yv);
        const double a = mle_dot(sv, q, P) / mle_dot(yv, sv, P);
        alphas[p] = a;
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k)
            if (k < P) q[k] = q[k] - a * yv[k];
    }
    if (s.pairs > 0) {
        const int slot = (s.head + s.pairs - 1) % kRefineHistory;
        mle_ring_read(s.S, slot, P, sv);
        mle_ring_read(s.Y, slot, P, yv);
        const double gamma = mle_dot(sv, yv, P) / mle_dot(yv, yv, P);
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k)
            if (k < P) q[k] = q[k] * gamma;
    }
    CBO_REFINE_UNROLL
    for (int p = 0; p < kRefineHistory; ++p) {                // oldest pair first
        if (p >= s.pairs) continue;
        mle_ring_read(s.S, (s.head + p) % kRefineHistory, P, sv);
        mle_ring_read(s.Y, (s.head + p) % kRefineHistory, P, yv);
        const double b = alphas[p] - mle_dot(yv, q, P) / mle_dot(yv, sv, P);
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k)
            if (k < P) q[k] = q[k] + b * sv[k];
    }
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) s.dir[k] = (k < P) ? -q[k] : 0.0;
    if (mle_dot(s.dir, s.g, P) >= 0.0) {
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k) s.dir[k] = (k < P) ? -s.g[k] : 0.0;
        s.pairs = 0;
        s.head = 0;
    }
}

// the next point to evaluate: x + t dir while the search runs, the accepted point (its theta as evaluated) once it has ended
CBO_HD inline void mle_set_trial(MleSearch &s)
{
    CBO_REFINE_NO_CONTRACT
    const bool running = s.status == kRefineRunning;
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) {
        if (k < s.P && running) {
            s.xt[k] = s.x[k] + s.t * s.dir[k];
            s.tht[k] = hmc_logexp_f(s.xt[k]);
        } else {
            s.xt[k] = s.x[k];
            s.tht[k] = s.th[k];
        }
    }
}

// The search begins at x0 (P values); the first point to evaluate is that point.
CBO_HD inline void mle_begin_at(MleSearch &s, int P, const double *x0, double *S, double *Y)
{
    s.P = P; s.pairs = 0; s.head = 0; s.status = kRefineRunning; s.rounds = 0; s.started = 0;
    s.S = S; s.Y = Y; s.f = 0.0; s.t = 0.0;
    for (int k = 0; k < kMleMaxParams; ++k) {
        s.x[k] = (k < P) ? x0[k] : 0.0;
        s.th[k] = (k < P) ? hmc_logexp_f(s.x[k]) : 0.0;
        s.xt[k] = s.x[k];
        s.tht[k] = s.th[k];
        s.g[k] = s.dl[k] = s.dir[k] = 0.0;
    }
}

// ... from the parameters theta0, as optimize starts: x0 = Logexp.finv(theta0)
CBO_HD inline void mle_begin(MleSearch &s, int P, const double *theta0, double *S, double *Y)
{
    double x0[kMleMaxParams];
    for (int k = 0; k < kMleMaxParams; ++k) x0[k] = (k < P) ? hmc_logexp_finv(theta0[k]) : 0.0;
    mle_begin_at(s, P, x0, S, Y);
}

// the position and the parameters whose likelihood mle_feed expects next (the accepted point once the search has ended)
CBO_HD inline const double *mle_point(const MleSearch &s) { return s.xt; }
CBO_HD inline const double *mle_theta(const MleSearch &s) { return s.tht; }
CBO_HD inline bool mle_done(const MleSearch &s) { return s.status != kRefineRunning; }

// lml and dlml / dtheta (P doubles) at mle_theta().  The first call is the start's own evaluation and counts as no round;
// every later one is a round.  After max_rounds rounds a search still running ends with CBO_REFINE_MAX_ROUNDS.  Feeding a
// search that has ended changes nothing.
CBO_HD inline void mle_feed(MleSearch &s, double lml, const double *dlml, int max_rounds)
{
    CBO_REFINE_NO_CONTRACT
    if (s.status != kRefineRunning) return;
    const int P = s.P;
    double gt[kMleMaxParams];
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) gt[k] = (k < P) ? -(dlml[k] * hmc_logexp_factor(s.tht[k])) : 0.0;
    if (!s.started) {
        s.started = 1;
        s.f = -lml;
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k) {
            s.g[k] = gt[k];
            s.dl[k] = (k < P) ? dlml[k] : 0.0;
        }
        if (!isfinite(s.f)) {
            s.status = CBO_REFINE_NAN_START;
            return;
        }
        mle_direction(s);
        const double n = sqrt(mle_dot(s.g, s.g, P));
        s.t = (n > 0.0) ? (1.0 / n < 1.0 ? 1.0 / n : 1.0) : 0.0;
        if (mle_max_abs(s.g, P) <= kRefinePgtol) s.status = CBO_REFINE_PGTOL;
        else if (max_rounds <= 0) s.status = CBO_REFINE_MAX_ROUNDS;
        mle_set_trial(s);
        return;
    }
    s.rounds += 1;
    const double ft = -lml;
    double step[kMleMaxParams];
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) step[k] = (k < P) ? s.xt[k] - s.x[k] : 0.0;
    if (!isfinite(ft) || ft > s.f + kRefineC1 * mle_dot(s.g, step, P)) {
        s.t = s.t * 0.5;                                      // Armijo failed: a shorter step next round
        if (s.t * mle_max_abs(s.dir, P) < kRefineMinStep) s.status = CBO_REFINE_STEP;
    } else {
        double y[kMleMaxParams];
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k) y[k] = (k < P) ? gt[k] - s.g[k] : 0.0;
        const double gain = s.f - ft;
        if (mle_dot(step, y, P) > kRefineCurvature * sqrt(mle_dot(step, step, P)) * sqrt(mle_dot(y, y, P))) {
            int slot;
            if (s.pairs < kRefineHistory) {
                slot = (s.head + s.pairs) % kRefineHistory;
                s.pairs += 1;
            } else {
                slot = s.head;
                s.head = (s.head + 1) % kRefineHistory;
            }
            CBO_REFINE_UNROLL
            for (int k = 0; k < kMleMaxParams; ++k)
                if (k < P) { s.S[slot * P + k] = step[k]; s.Y[slot * P + k] = y[k]; }
        }
        double big = fabs(s.f) > fabs(ft) ? fabs(s.f) : fabs(ft);
        big = big > 1.0 ? big : 1.0;
        const bool small = gain <= kRefineFtol * big;
        s.f = ft;
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k) {
            s.x[k] = s.xt[k];
            s.th[k] = s.tht[k];
            s.g[k] = gt[k];
            s.dl[k] = (k < P) ? dlml[k] : 0.0;
        }
        mle_direction(s);
        s.t = 1.0;
        if (mle_max_abs(s.g, P) <= kRefinePgtol) s.status = CBO_REFINE_PGTOL;
        else if (small) s.status = CBO_REFINE_FTOL;
    }
    if (s.status == kRefineRunning && s.rounds >= max_rounds) s.status = CBO_REFINE_MAX_ROUNDS;
    mle_set_trial(s);
}

}  // namespace cbo

// One hyper-parameter MLE as a state machine: refine_search.h's search without a box, over a model's Logexp-transformed
// parameters x (theta = Logexp.f(x): variance, lengthscale(s), noise variance when it is fitted; at most
// CBO_HMC_MAX_PARAMS of them).  The caller owns the evaluations: it asks the state for the parameters to evaluate
// (mle_theta), evaluates the log marginal likelihood and its gradients with respect to them however it likes (a device
// kernel between two factorisations, a host test on a closed form) and feeds the pair back (mle_feed), once per round.
// Plain C++17, no HIP headers: the same text compiles under hipcc into mle_sets_kernel (kernels_mle.hip) and under g++ into
// the host simulator of the tests (tests/support/mle_search_sim.cpp).
//
// The iteration, its constants (kRefine*), its status codes (CBO_REFINE_*) and the ring layout are refine_search.h's; nothing
// of them is restated here.  What is the MLE's own is the transform, and it stays outside the search: the gradient handed
// in is hmc_chain.h's, (dlml / dtheta) (1 - exp(-theta)) with that header's own Logexp functions, and like HmcChain the
// state keeps theta AS EVALUATED beside x, so the reported parameters are the very doubles the likelihood was taken at and
// nothing is transformed twice.
// Floating-point contraction must be off (-ffp-contract=off for g++; refine_search.h's pragma for clang).
#pragma once

#include <math.h>

#include "cbo_hip.h"
#include "hmc_chain.h"
#include "refine_search.h"

namespace cbo {

constexpr int kMleMaxParams = CBO_HMC_MAX_PARAMS;

// The search over x, and beside it: th, dl -- theta(x) as evaluated and dlml / dtheta as fed at the accepted point; tht --
// theta at the point the caller is evaluating.
struct MleSearch : RefineSearch<kMleMaxParams, false> {
    double th[kMleMaxParams], dl[kMleMaxParams], tht[kMleMaxParams];
};

// The search begins at x0 (P values); the first point to evaluate is that point.
CBO_HD inline void mle_begin_at(MleSearch &s, int P, const double *x0, double *S, double *Y)
{
    refine_begin(s, P, x0, nullptr, nullptr, S, Y);
    for (int k = 0; k < kMleMaxParams; ++k) {
        s.th[k] = (k < P) ? hmc_logexp_f(s.x[k]) : 0.0;
        s.tht[k] = s.th[k];
        s.dl[k] = 0.0;
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

// theta at the trial point of a running search.  Kept out of line: ten inlined logarithms in mle_sets_kernel's body cost it
// 16 accumulator registers and 16 bytes of scratch per lane.
__attribute__((noinline)) CBO_HD inline void mle_trial_theta(MleSearch &s)
{
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) s.tht[k] = (k < s.d) ? hmc_logexp_f(s.xt[k]) : 0.0;
}

// lml and dlml / dtheta (P doubles) at mle_theta(): one refine_feed with the gradient with respect to x.  Feeding a search
// that has ended changes nothing.
CBO_HD inline void mle_feed(MleSearch &s, double lml, const double *dlml, int max_rounds)
{
    CBO_REFINE_NO_CONTRACT
    if (s.status != kRefineRunning) return;
    const int P = s.d;
    double grad[kMleMaxParams];
    CBO_REFINE_UNROLL
    for (int k = 0; k < kMleMaxParams; ++k) grad[k] = (k < P) ? dlml[k] * hmc_logexp_factor(s.tht[k]) : 0.0;
    refine_feed(s, nullptr, nullptr, lml, grad, max_rounds, [&] {
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k) {
            s.th[k] = s.tht[k];
            s.dl[k] = (k < P) ? dlml[k] : 0.0;
        }
    });
    if (s.status == kRefineRunning) {
        mle_trial_theta(s);
    } else {
        CBO_REFINE_UNROLL
        for (int k = 0; k < kMleMaxParams; ++k) s.tht[k] = s.th[k];
    }
}

}  // namespace cbo

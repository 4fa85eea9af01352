// One HMC chain over a model's Logexp-transformed hyper-parameters as a state machine: hmc_sample of
// utils_functions/integrated_hyper.py (GPy inference.mcmc.HMC with the unit mass matrix) for ONE chain, restated so that the
// caller owns the evaluations and the draws -- it asks the state for the parameters to evaluate (hmc_theta), evaluates the
// log marginal likelihood and its gradients with respect to them however it likes (a device kernel between two
// factorisations, a host test on a closed form) and feeds the pair back (hmc_feed), once per position.  Plain C++17, no HIP
// headers: the same text compiles under hipcc into hmc_sets_kernel (kernels_hmc.hip) and under g++ into the host simulator
// of the tests (tests/support/hmc_chain_sim.cpp).
//
// What it carries over from hmc_sample, operation for operation: x = Logexp.finv(theta0); per sample the momentum handed
// in, H_old = f + P log(2 pi) / 2 + p.p / 2 (the dot product summed from 0 in index order), the row = theta at the sample's
// start; hmc_iters leapfrog steps p = p + (-stepsize / 2) g, x = x + stepsize p, evaluate, p = p + (-stepsize / 2) g;
// k = H_old > H_new ? 1 : exp(H_old - H_new) and accept iff u < k (a NaN rejects: both comparisons are false); on an accept
// the row becomes theta at the proposal, on a reject x, f, g go back to the saved values.  The objective is f = -lml,
// g = -(dlml / dtheta) (1 - exp(-theta)), evaluated once per position: 1 + num_samples * hmc_iters evaluations.
// Floating-point contraction must be off (-ffp-contract=off for g++; the pragma below for clang): the leapfrog is then the
// element-wise IEEE arithmetic numpy performs.
#pragma once

#include <math.h>

#include "cbo_hip.h"

#if defined(__HIPCC__)
#define CBO_HMC_HD __host__ __device__
#else
#define CBO_HMC_HD
#endif
#if defined(__clang__)
#define CBO_HMC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CBO_HMC_NO_CONTRACT
#endif

namespace cbo {

constexpr int kHmcMaxParams = CBO_HMC_MAX_PARAMS;    // variance, at most CBO_MAX_DIM lengthscales, noise variance
constexpr double kLogexpLim = 36.0;                  // paramz transformations._lim_val
constexpr double kLogexpLogLim = 709.782712893384;   // log(DBL_MAX), paramz _exp_lim_val's logarithm
constexpr double kLog2Pi = 1.8378770664093453;

// x, th: the position and theta(x) there -- th holds the very doubles the caller evaluated (rows and the final state copy
// them, nothing is transformed twice).  f, g: -lml and its gradient with respect to x at the position; dl: dlml / dtheta as
// fed.  *_old: the sample's start, for a reject.  sample, step: where the chain is; started: the start has been evaluated.
struct HmcChain {
    double x[kHmcMaxParams], th[kHmcMaxParams], g[kHmcMaxParams], dl[kHmcMaxParams], p[kHmcMaxParams];
    double x_old[kHmcMaxParams], th_old[kHmcMaxParams], g_old[kHmcMaxParams], dl_old[kHmcMaxParams];
    double f, f_old, h_old, stepsize;
    int P, num_samples, hmc_iters, sample, step, started, done, evals;
};

// Logexp.f, Logexp.finv and the factor d theta / d x = 1 - exp(-theta)
CBO_HMC_HD inline double hmc_logexp_f(double x)
{
    if (x > kLogexpLim) return x;
    const double c = x < -kLogexpLogLim ? -kLogexpLogLim : x;      // (x <= 36 here: the clamp's upper end never binds)
    return log1p(exp(c));
}
CBO_HMC_HD inline double hmc_logexp_finv(double theta) { return theta > kLogexpLim ? theta : log(expm1(theta)); }
CBO_HMC_HD inline double hmc_logexp_factor(double theta) { return theta > kLogexpLim ? 1.0 : -expm1(-theta); }

// the chain at the position x0 (P values), nothing evaluated yet
CBO_HMC_HD inline void hmc_begin_at(HmcChain &c, int P, const double *x0, int num_samples, int hmc_iters, double stepsize)
{
    c.P = P;
    c.num_samples = num_samples;
    c.hmc_iters = hmc_iters;
    c.stepsize = stepsize;
    c.sample = c.step = c.started = c.done = c.evals = 0;
    c.f = c.f_old = c.h_old = 0.0;
    for (int k = 0; k < kHmcMaxParams; ++k) {
        c.x[k] = (k < P) ? x0[k] : 0.0;
        c.th[k] = (k < P) ? hmc_logexp_f(c.x[k]) : 0.0;
        c.g[k] = c.dl[k] = c.p[k] = 0.0;
        c.x_old[k] = c.th_old[k] = c.g_old[k] = c.dl_old[k] = 0.0;
    }
}

// ... from the parameters theta0, as hmc_sample starts: x0 = Logexp.finv(theta0)
CBO_HMC_HD inline void hmc_begin(HmcChain &c, int P, const double *theta0, int num_samples, int hmc_iters, double stepsize)
{
    double x0[kHmcMaxParams];
    for (int k = 0; k < kHmcMaxParams; ++k) x0[k] = (k < P) ? hmc_logexp_finv(theta0[k]) : 0.0;
    hmc_begin_at(c, P, x0, num_samples, hmc_iters, stepsize);
}

// the parameters the caller evaluates next (P doubles)
CBO_HMC_HD inline const double *hmc_theta(const HmcChain &c) { return c.th; }
CBO_HMC_HD inline bool hmc_done(const HmcChain &c) { return c.done != 0; }

CBO_HMC_HD inline double hmc_hamiltonian(const HmcChain &c)
{
    CBO_HMC_NO_CONTRACT
    double dot = 0.0;
    for (int k = 0; k < c.P; ++k) dot = dot + c.p[k] * c.p[k];
    return c.f + (double)c.P * kLog2Pi / 2.0 + dot / 2.0;
}

CBO_HMC_HD inline void hmc_kick(HmcChain &c)
{
    CBO_HMC_NO_CONTRACT
    const double half = -c.stepsize / 2.0;
    for (int k = 0; k < c.P; ++k) c.p[k] = c.p[k] + half * c.g[k];
}

CBO_HMC_HD inline void hmc_drift(HmcChain &c)
{
    CBO_HMC_NO_CONTRACT
    for (int k = 0; k < c.P; ++k) {
        c.x[k] = c.x[k] + c.stepsize * c.p[k];
        c.th[k] = hmc_logexp_f(c.x[k]);
    }
}

// the end of sample c.sample: accept or reject the proposal the chain stands at
CBO_HMC_HD inline void hmc_close_sample(HmcChain &c, const double *uniforms, double *rows, int *accepts)
{
    CBO_HMC_NO_CONTRACT
    const double h_new = hmc_hamiltonian(c);
    const double k = (c.h_old > h_new) ? 1.0 : exp(c.h_old - h_new);
    const bool accept = uniforms[c.sample] < k;
    if (accept) {
        for (int j = 0; j < c.P; ++j) rows[(long long)c.sample * c.P + j] = c.th[j];
    } else {
        for (int j = 0; j < c.P; ++j) {
            c.x[j] = c.x_old[j];
            c.th[j] = c.th_old[j];
            c.g[j] = c.g_old[j];
            c.dl[j] = c.dl_old[j];
        }
        c.f = c.f_old;
    }
    accepts[c.sample] = accept ? 1 : 0;
    c.sample += 1;
}

// Opens samples until one wants an evaluation (hmc_iters = 0: none does, every sample closes where it opened) or the
// chain is done.  At most num_samples rounds.
CBO_HMC_HD inline void hmc_open_samples(HmcChain &c, const double *momenta, const double *uniforms, double *rows, int *accepts)
{
    while (c.sample < c.num_samples) {
        for (int j = 0; j < c.P; ++j) {
            c.p[j] = momenta[(long long)c.sample * c.P + j];
            c.x_old[j] = c.x[j];
            c.th_old[j] = c.th[j];
            c.g_old[j] = c.g[j];
            c.dl_old[j] = c.dl[j];
            rows[(long long)c.sample * c.P + j] = c.th[j];
        }
        c.f_old = c.f;
        c.h_old = hmc_hamiltonian(c);
        if (c.hmc_iters > 0) {
            c.step = 0;
            hmc_kick(c);
            hmc_drift(c);
            return;
        }
        hmc_close_sample(c, uniforms, rows, accepts);
    }
    c.done = 1;
}

// lml and dlml / dtheta (P doubles) at hmc_theta(c); momenta (num_samples x P), uniforms (num_samples): the chain's draws;
// rows (num_samples x P), accepts (num_samples): its outputs.  Afterwards either hmc_done(c), or hmc_theta(c) is the next
// position to evaluate.
CBO_HMC_HD inline void hmc_feed(HmcChain &c, double lml, const double *dlml, const double *momenta, const double *uniforms,
                                double *rows, int *accepts)
{
    CBO_HMC_NO_CONTRACT
    c.evals += 1;
    c.f = -lml;
    for (int k = 0; k < c.P; ++k) {
        c.dl[k] = dlml[k];
        c.g[k] = -(dlml[k] * hmc_logexp_factor(c.th[k]));
    }
    if (!c.started) {
        c.started = 1;
        hmc_open_samples(c, momenta, uniforms, rows, accepts);
        return;
    }
    hmc_kick(c);
    c.step += 1;
    if (c.step < c.hmc_iters) {
        hmc_kick(c);
        hmc_drift(c);
        return;
    }
    hmc_close_sample(c, uniforms, rows, accepts);
    hmc_open_samples(c, momenta, uniforms, rows, accepts);
}

}  // namespace cbo

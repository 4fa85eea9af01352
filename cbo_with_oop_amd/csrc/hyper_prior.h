// The log prior of a model's hyper-parameters and its gradient: GPy's priors.Gaussian / LogGaussian / Gamma / InverseGamma
// (lnpdf, lnpdf_grad) and, for every parameter that has a prior, the log-Jacobian of its Logexp constraint as GPy's
// Parameterized.log_prior() / _log_prior_gradients() add it.  One entry point, hyper_prior_at, evaluated at theta (the
// constrained parameters: variance, lengthscale(s), noise variance -- the row order of hmc_sets_kernel and mle_sets_kernel).
// Plain C++17, no HIP headers: the same text compiles under hipcc into the kernels (kernels_hmc.hip, kernels_mle.hip,
// kernels_prior.hip) and under g++ into the host simulator of the tests (tests/support/hyper_prior_sim.cpp).
// GPy is not installed where this was written: the four densities and the Jacobian are restated from memory, parity with
// GPy unpinned (utils_functions/priors.py is the same restatement in numpy and is tested against scipy.stats).
//
// The operation order, which the tests hold the device to bit for bit (every operation one IEEE operation, contraction off):
//   lp = 0.0; for k = 0 .. P-1 in index order:
//     kind NONE:          dlp[k] = 0.0 exactly, lp untouched (no + 0.0);
//     otherwise           (dens, g) by the kind's formula below, lp = lp + dens;
//                         (jac, dj) = theta > 36 ? (0.0, 0.0) : (log(e) - theta, 1.0 / e) with e = expm1(theta), lp = lp + jac;
//                         dlp[k] = g + dj.
//   with t = theta, c = constant, (p0, p1) = (mu, sigma) or (a, b), L = log(t), s2 = p1 * p1:
//     GAUSSIAN      u = t - p0;  dens = c - (u * u) / (2.0 * s2);               g = -(u / s2)
//     LOGGAUSSIAN   u = L - p0;  dens = (c - (u * u) / (2.0 * s2)) - L;         g = -((u / s2 + 1.0) / t)
//     GAMMA         dens = (c + (p0 - 1.0) * L) - p1 * t;                       g = (p0 - 1.0) / t - p1
//     INVGAMMA      dens = (c - (p0 + 1.0) * L) - p1 / t;                       g = p1 / (t * t) - (p0 + 1.0) / t
// `constant` comes from the host (lgamma included: the device never calls it):
//     GAUSSIAN, LOGGAUSSIAN   -0.5 * log(2 pi sigma^2);      GAMMA, INVGAMMA   a log(b) - lgamma(a).
// log, expm1 are the compiling side's own: device and host values agree to the libraries' rounding, not bit for bit.
// Floating-point contraction must be off (-ffp-contract=off for g++; the pragma below for clang).
#pragma once

#include <math.h>

#include "cbo_hip.h"

#if defined(__HIPCC__)
#define CBO_PRIOR_HD __host__ __device__
#else
#define CBO_PRIOR_HD
#endif
#if defined(__clang__)
#define CBO_PRIOR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CBO_PRIOR_NO_CONTRACT
#endif

namespace cbo {

constexpr double kPriorLogexpLim = 36.0;            // paramz transformations._lim_val

// one entry's density and its derivative with respect to theta (the kind is not NONE)
CBO_PRIOR_HD inline void hyper_prior_density(const cbo_hyper_prior &pr, double t, double *dens, double *g)
{
    CBO_PRIOR_NO_CONTRACT
    const double c = pr.constant, p0 = pr.p0, p1 = pr.p1;
    if (pr.kind == CBO_PRIOR_GAUSSIAN) {
        const double s2 = p1 * p1, u = t - p0;
        *dens = c - (u * u) / (2.0 * s2);
        *g = -(u / s2);
    } else if (pr.kind == CBO_PRIOR_LOGGAUSSIAN) {
        const double s2 = p1 * p1, L = log(t), u = L - p0;
        *dens = (c - (u * u) / (2.0 * s2)) - L;
        *g = -((u / s2 + 1.0) / t);
    } else if (pr.kind == CBO_PRIOR_GAMMA) {
        const double L = log(t);
        *dens = (c + (p0 - 1.0) * L) - p1 * t;
        *g = (p0 - 1.0) / t - p1;
    } else {                                        // CBO_PRIOR_INVGAMMA (cbo_gp_set_priors admits no other kind)
        const double L = log(t);
        *dens = (c - (p0 + 1.0) * L) - p1 / t;
        *g = p1 / (t * t) - (p0 + 1.0) / t;
    }
}

// log |d theta / d x| of the Logexp constraint at theta and its derivative with respect to theta; both 0 above paramz's limit
CBO_PRIOR_HD inline void hyper_prior_jacobian(double t, double *jac, double *dj)
{
    CBO_PRIOR_NO_CONTRACT
    if (t > kPriorLogexpLim) {
        *jac = 0.0;
        *dj = 0.0;
        return;
    }
    const double e = expm1(t);
    *jac = log(e) - t;
    *dj = 1.0 / e;
}

// *lp = the log prior of theta[0..P) under pr[0..P) (Jacobians included), dlp[k] = its derivative with respect to theta[k];
// an entry without a prior gets dlp[k] = 0.0 exactly and contributes nothing.  The order of operations is the file's head.
CBO_PRIOR_HD inline void hyper_prior_at(const cbo_hyper_prior *pr, int P, const double *theta, double *lp, double *dlp)
{
    CBO_PRIOR_NO_CONTRACT
    double sum = 0.0;
    for (int k = 0; k < P; ++k) {
        if (pr[k].kind == CBO_PRIOR_NONE) {
            dlp[k] = 0.0;
            continue;
        }
        double dens, g, jac, dj;
        hyper_prior_density(pr[k], theta[k], &dens, &g);
        sum = sum + dens;
        hyper_prior_jacobian(theta[k], &jac, &dj);
        sum = sum + jac;
        dlp[k] = g + dj;
    }
    *lp = sum;
}

// how many of pr[0..P) carry a prior
CBO_PRIOR_HD inline int hyper_prior_count(const cbo_hyper_prior *pr, int P)
{
    int n = 0;
    for (int k = 0; k < P; ++k) n += pr[k].kind != CBO_PRIOR_NONE;
    return n;
}

}  // namespace cbo

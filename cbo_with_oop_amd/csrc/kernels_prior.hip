// The hyper-parameters' log prior of many models in one launch for gfx950: log_prior_kernel behind
// cbo_gp_log_prior_batch.  One lane per model evaluates hyper_prior_at (hyper_prior.h) -- the text thread 0 of
// hmc_sets_kernel and mle_sets_kernel runs between two factorisations, compiled by the same compiler against the same
// device log / expm1 -- so what those kernels add to the likelihood can be checked against this call bit for bit.
// A dozen transcendental calls per model: the launch is there for the bits, not for speed.  The items live in pinned,
// device-mapped host memory; every lane touches its own item alone, every loop is bounded by CBO_HMC_MAX_PARAMS.
#include "cbo_internal.h"
#include "hyper_prior.h"

namespace cbo {

__global__ __launch_bounds__(64) void log_prior_kernel(cbo_prior_item *__restrict__ items, int n_models)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_models) return;
    cbo_prior_item &it = items[i];
    const int P = it.n_params < 0 ? 0 : (it.n_params > CBO_HMC_MAX_PARAMS ? CBO_HMC_MAX_PARAMS : it.n_params);
    cbo_hyper_prior pr[CBO_HMC_MAX_PARAMS];
    double theta[CBO_HMC_MAX_PARAMS], dlp[CBO_HMC_MAX_PARAMS], lp = 0.0;
    for (int k = 0; k < CBO_HMC_MAX_PARAMS; ++k) {
        pr[k] = it.priors[k];
        theta[k] = it.theta[k];
        dlp[k] = 0.0;
    }
    hyper_prior_at(pr, P, theta, &lp, dlp);
    it.lp = lp;
    for (int k = 0; k < CBO_HMC_MAX_PARAMS; ++k) it.dlp[k] = k < P ? dlp[k] : 0.0;
    it.done = 1;
}

void launch_log_prior(hipStream_t s, cbo_prior_item *items, int n_models)
{
    hipLaunchKernelGGL(log_prior_kernel, dim3((unsigned)((n_models + 63) / 64)), dim3(64), 0, s, items, n_models);
}

}  // namespace cbo

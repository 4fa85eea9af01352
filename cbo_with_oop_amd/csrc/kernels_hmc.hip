// Every model's HMC chain over its hyper-parameters in one launch for gfx950: hmc_sets_kernel, the sampler
// behind emukit's GPyModelWrapper.generate_hyperparameters_samples for every exploration set of a trial.  One workgroup of
// 256 threads runs one model's whole chain; no workgroup waits for another.  Per position of the chain:
//   thread 0 has left theta(x) in LDS (the chain's state, hmc_chain.h), so every lane works from the same doubles;
//   the model's points are prepared from its RAW coordinates with theta's lengthscales, K(X,X) + (noise + 1e-8) I is
//   assembled and factored inside LDS (hyper_sample_set / hyper_model_points / hyper_factor, as hyper_avg_kernel does for a
//   hyper-parameter sample);
//   the stages behind the factor of small_lml_kernel follow (small_lml_after_factor: L^-1 through the tile solve, alpha,
//   diag(Ky^-1), the gradient sums over the upper tile pairs, the workgroup reduction), the sums staying in LDS -- all of
//   it one device function, small_lml_sums_at (cbo_small_lml_device.h), which mle_sets_kernel calls per evaluation too;
//   thread 0 turns them into the likelihood and its gradients with the host's own arithmetic (lml_outputs.h) and advances
//   the chain (hmc_feed): two multiply-adds per parameter between two evaluations.
// The likelihood at a position is therefore what cbo_gp_lml_gradients answers for the model at those hyper-parameters.
// A chain whose model has priors (cbo_gp_set_priors): thread 0 adds the log prior and its gradient at theta
// (hyper_prior_at, hyper_prior.h) to that pair, one IEEE addition each, before hmc_feed -- the chain samples the posterior.
// A position whose Ky is not positive definite as assembled ends the chain with CBO_HMC_NOT_PD (jitchol's ladder lives on
// the host: the caller repeats the chain there).  Nothing resident is written but the workgroup's scratch slot.
// Every loop is bounded: the positions by 1 + num_samples * hmc_iters, the chain's own loops by num_samples and P.
#include <cstring>

#include "cbo_small_lml_device.h"
#include "hmc_chain.h"
#include "hyper_prior.h"
#include "lml_outputs.h"

namespace cbo {

static_assert(sizeof(SmallShared) + 4 * kSmallLmlTerms * sizeof(double) + sizeof(HmcChain) + kHmcMaxParams * sizeof(double)
                  + kHmcMaxParams * (sizeof(cbo_hyper_prior) + sizeof(double)) <= 163840,
              "the workgroup's static LDS (the reduction's partial sums, the chain's state, the published theta, the priors "
              "and their gradient) beside SmallShared: one CU");
static_assert(kHmcMaxParams == CBO_MAX_DIM + 2, "variance, one lengthscale per dimension, noise variance");

// PRIOR: some run of the launch has a prior (hyper_prior.h).  The instantiation without is the kernel as it
// was before priors existed: a launch without priors runs that code and gives those bits.
template <bool BYVAL, bool PRIOR>
__global__ __launch_bounds__(256) void hmc_sets_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
                                                       const cbo_small_hmc *__restrict__ chains,
                                                       const double *__restrict__ draws, double *scratch, int64_t stride,
                                                       int *__restrict__ info, double *__restrict__ rows_out,
                                                       int *__restrict__ accept_out, double *__restrict__ final_out,
                                                       int *__restrict__ status_out)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    __shared__ double red[4][kSmallLmlTerms];
    __shared__ HmcChain chain;
    __shared__ double theta_row[kHmcMaxParams];
    __shared__ cbo_hyper_prior priors[kHmcMaxParams];             // thread 0's alone, filled when the chain has a prior
    __shared__ double prior_grad[kHmcMaxParams];                       // ... and d log prior / d theta at the evaluated row
    const int b = blockIdx.x;
    const cbo_small_set st = BYVAL ? byval.s[b] : sets[b];
    const cbo_small_hmc &hm = chains[b];
    const int tid = threadIdx.x;
    const int tiles = (st.n + 15) / 16;
    const int n_ls = hm.n_ls, P = hm.n_params, sample_noise = hm.sample_noise;
    const int num_samples = hm.num_samples, hmc_iters = hm.hmc_iters, n_prior = hm.n_prior;
    double *Us = scratch + (int64_t)b * stride, *invs = Us + 128 * kSmallLd, *Vg = Us + kSmallScratch;
    double *alpha_s = sh.sq;                                      // (|x|^2 is the assembly's alone: free behind the factor)
    const double *momenta = draws + hm.draw_off, *uniforms = momenta + (int64_t)num_samples * P;
    double *rows = rows_out + hm.row_off;
    int *accepts = accept_out + hm.acc_off;
    const double rhs = hyper_rhs(st);

    // theta(x) of the chain's position for every lane: a model whose noise is fixed keeps its own in the row's last place
    auto publish = [&]() {
        for (int k = 0; k < kHmcMaxParams; ++k) theta_row[k] = (k < P) ? chain.th[k] : 0.0;
        if (!sample_noise) theta_row[1 + n_ls] = st.noise_var;
    };
    if (tid == 0) {
        hmc_begin(chain, P, hm.theta0, num_samples, hmc_iters, hm.stepsize);
        if (PRIOR && n_prior > 0)
            for (int k = 0; k < P; ++k) priors[k] = hm.priors[k];
        publish();
    }
    __syncthreads();

    const int64_t positions = 1 + (int64_t)num_samples * hmc_iters;
    for (int64_t pos = 0; pos < positions; ++pos) {
        // ---- theta as a hyper-parameter sample's row (variance, lengthscale x n_ls, noise variance): thread 0 left it in LDS
        const double *row = theta_row;
        // not positive definite as assembled: jitchol's business, the chain stops here
        if (!small_lml_sums_at(sh, alpha_s, red, st, row, n_ls, tiles, rhs, Us, invs, Vg, &info[b])) {
            __syncthreads();                                      // (everybody has read the word)
            if (tid == 0) {
                status_out[b] = CBO_HMC_NOT_PD;
                __hip_atomic_store(&info[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        // ---- the likelihood and its gradients by the host's arithmetic, one step of the chain
        if (tid == 0) {
            double lml, dl[kHmcMaxParams], dnoise;
            small_lml_outputs_at(st, row, red, &lml, dl, &dnoise);
            if (sample_noise) dl[1 + n_ls] = dnoise;
            if (PRIOR && n_prior > 0) {                           // (a chain without priors: no stage, no + 0.0)
                double lp;
                hyper_prior_at(priors, P, row, &lp, prior_grad);
                lml = lml + lp;                                   // the log posterior and its gradient: one IEEE addition each
#pragma unroll
                for (int k = 0; k < kHmcMaxParams; ++k)
                    if (k < P) dl[k] = dl[k] + prior_grad[k];
            }
            hmc_feed(chain, lml, dl, momenta, uniforms, rows, accepts);
            publish();
        }
        __syncthreads();
        if (chain.done) break;                                    // (uniform: everybody reads the same word)
    }

    if (tid == 0) {
        double *fin = final_out + (int64_t)b * (2 * kHmcMaxParams + 1);
        for (int k = 0; k < P; ++k) {
            fin[k] = chain.th[k];
            fin[kHmcMaxParams + 1 + k] = chain.dl[k];
        }
        fin[kHmcMaxParams] = -chain.f;
        status_out[b] = CBO_HMC_OK;
    }
}

void launch_hmc_sets(hipStream_t s, const cbo_small_set *sets, const cbo_small_hmc *chains, const double *draws, int n_models,
                     double *scratch, int64_t stride, int *info, double *rows_out, int *accept_out, double *final_out,
                     int *status_out)
{
    static std::atomic<unsigned long long> opted[2][2] = {{{0}, {0}}, {{0}, {0}}};
    const bool byval = n_models <= kSmallByValue;
    bool prior = false;
    for (int j = 0; j < n_models; ++j) prior = prior || chains[j].n_prior > 0;
    SmallSetArgs args{};
    if (byval) std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_models);
    auto launch = [&](auto kernel) {
        small_lds_opt_in(reinterpret_cast<const void *>(kernel), opted[byval][prior]);
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_models), dim3(256), sizeof(SmallShared), s, args,
                           sets, chains, draws, scratch, stride, info, rows_out, accept_out, final_out, status_out);
    };
    if (byval) prior ? launch(hmc_sets_kernel<true, true>) : launch(hmc_sets_kernel<true, false>);
    else prior ? launch(hmc_sets_kernel<false, true>) : launch(hmc_sets_kernel<false, false>);
}

}  // namespace cbo

// Every model's hyper-parameter MLE in one launch for gfx950: mle_sets_kernel, the L-BFGS search behind
// optimize / optimize_restarts for every model of a trial.  One workgroup of 256 threads runs one RUN -- one (model, start)
// pair -- from its start to the search's end; no workgroup waits for another, so a restart is one more workgroup.  Per
// evaluation, exactly what hmc_sets_kernel does per position of a chain (small_lml_sums_at, cbo_small_lml_device.h):
//   thread 0 has left theta(x) of the search's trial point in LDS (mle_search.h), so every lane works from the same doubles;
//   the model's points are prepared from its RAW coordinates with theta's lengthscales, K(X,X) + (noise + 1e-8) I is
//   assembled and factored inside LDS, the stages behind the factor leave the likelihood's sums in LDS;
//   thread 0 turns them into the likelihood and its gradients with the host's own arithmetic (lml_outputs.h) and advances
//   the search (mle_feed).
// The likelihood at a trial point is therefore what cbo_gp_lml_gradients answers for the model at those hyper-parameters.
// A run whose model has priors (cbo_gp_set_priors): thread 0 adds the log prior and its gradient at theta
// (hyper_prior_at, hyper_prior.h) to that pair, one IEEE addition each, before mle_feed -- the search maximises the posterior.
// A TRIAL point whose Ky is not positive definite as assembled is fed as a non-finite value: an Armijo failure, the step
// halves (what _objective's 1e25 does to scipy); the info word is cleared.  At the START it ends the run with
// CBO_MLE_NOT_PD (jitchol's ladder lives on the host: the caller repeats that model there).
// The search's two rings of curvature pairs (2 x 8 x 10 doubles) do not fit beside SmallShared in LDS: they live in the
// run's own slot of a device buffer, read and written by thread 0 alone.  Nothing resident is written but the run's scratch
// slot and ring slot.  Every loop is bounded: the evaluations by 1 + max_rounds, the search's own loops by 8 and P.
#include <cstring>

#include "cbo_small_lml_device.h"
#include "hyper_prior.h"
#include "mle_search.h"

namespace cbo {

static_assert(sizeof(SmallShared) + 4 * kSmallLmlTerms * sizeof(double) + sizeof(MleSearch) + kMleMaxParams * sizeof(double)
                  + kMleMaxParams * (sizeof(cbo_hyper_prior) + sizeof(double)) <= 163840,
              "the workgroup's static LDS (the reduction's partial sums, the search's state, the published theta, the priors "
              "and their gradient) beside SmallShared: one CU");
static_assert(kMleMaxParams == CBO_MAX_DIM + 2, "variance, one lengthscale per dimension, noise variance");
static_assert(kMleRingDoubles == 2 * kRefineHistory * kMleMaxParams, "a run's ring slot holds the search's S and Y");

// PRIOR: some run of the launch has a prior (hyper_prior.h).  The instantiation without is the kernel as it
// was before priors existed: a launch without priors runs that code and gives those bits.
template <bool BYVAL, bool PRIOR>
__global__ __launch_bounds__(256) void mle_sets_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
                                                       const cbo_small_mle *__restrict__ runs, double *scratch, int64_t stride,
                                                       int *__restrict__ info, double *__restrict__ rings,
                                                       double *__restrict__ final_out, int *__restrict__ status_out,
                                                       int *__restrict__ rounds_out)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    __shared__ double red[4][kSmallLmlTerms];
    __shared__ MleSearch search;
    __shared__ double theta_row[kMleMaxParams];
    __shared__ cbo_hyper_prior priors[kMleMaxParams];             // thread 0's alone, filled when the run has a prior
    __shared__ double prior_grad[kMleMaxParams];                       // ... and d log prior / d theta at the evaluated row
    const int b = blockIdx.x;
    const cbo_small_mle &rn = runs[b];
    const cbo_small_set st = BYVAL ? byval.s[rn.model] : sets[rn.model];
    const int tid = threadIdx.x;
    const int tiles = (st.n + 15) / 16;
    const int n_ls = rn.n_ls, P = rn.n_params, fit_noise = rn.fit_noise, max_rounds = rn.max_rounds;
    const int n_prior = rn.n_prior;
    double *Us = scratch + (int64_t)b * stride, *invs = Us + 128 * kSmallLd, *Vg = Us + kSmallScratch;
    double *alpha_s = sh.sq;                                      // (|x|^2 is the assembly's alone: free behind the factor)
    double *ring = rings + (int64_t)b * kMleRingDoubles;
    const double rhs = hyper_rhs(st);

    // theta(x) of the search's trial point for every lane: a model whose noise is fixed keeps its own in the row's last place
    auto publish = [&]() {
        for (int k = 0; k < kMleMaxParams; ++k) theta_row[k] = (k < P) ? search.tht[k] : 0.0;
        if (!fit_noise) theta_row[1 + n_ls] = st.noise_var;
    };
    if (tid == 0) {
        mle_begin(search, P, rn.theta0, ring, ring + kRefineHistory * kMleMaxParams);
        if (PRIOR && n_prior > 0)
            for (int k = 0; k < P; ++k) priors[k] = rn.priors[k];
        publish();
    }
    __syncthreads();

    for (int e = 0; e <= max_rounds; ++e) {
        const double *row = theta_row;
        const bool pd = small_lml_sums_at(sh, alpha_s, red, st, row, n_ls, tiles, rhs, Us, invs, Vg, &info[b]);
        if (!pd) {
            __syncthreads();                                      // (everybody has read the word)
            if (tid == 0) __hip_atomic_store(&info[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (e == 0) {                                         // the start itself: jitchol's business
                if (tid == 0) {
                    status_out[b] = CBO_MLE_NOT_PD;
                    rounds_out[b] = 0;
                }
                return;
            }
        }
        if (tid == 0) {
            double lml = (double)NAN, dl[kMleMaxParams], dnoise = 0.0;
#pragma unroll
            for (int k = 0; k < kMleMaxParams; ++k) dl[k] = 0.0;
            if (pd) {
                small_lml_outputs_at(st, row, red, &lml, dl, &dnoise);
                if (fit_noise) dl[1 + n_ls] = dnoise;
                if (PRIOR && n_prior > 0) {                           // (a run without priors: no stage, no + 0.0)
                    double lp;
                    hyper_prior_at(priors, P, row, &lp, prior_grad);
                    lml = lml + lp;                                   // the log posterior and its gradient: one IEEE addition each
#pragma unroll
                    for (int k = 0; k < kMleMaxParams; ++k)
                        if (k < P) dl[k] = dl[k] + prior_grad[k];
                }
            }
            mle_feed(search, lml, dl, max_rounds);
            publish();
        }
        __syncthreads();
        if (search.status != kRefineRunning) break;               // (uniform: everybody reads the same word)
    }

    if (tid == 0) {
        double *fin = final_out + (int64_t)b * (2 * kMleMaxParams + 1);
        for (int k = 0; k < P; ++k) {
            fin[k] = search.th[k];
            fin[kMleMaxParams + 1 + k] = search.dl[k];
        }
        fin[kMleMaxParams] = -search.f;
        rounds_out[b] = search.rounds;
        status_out[b] = search.status;
    }
}

void launch_mle_sets(hipStream_t s, const cbo_small_set *sets, int n_models, const cbo_small_mle *runs, int n_runs,
                     double *scratch, int64_t stride, int *info, double *rings, double *final_out, int *status_out,
                     int *rounds_out)
{
    static std::atomic<unsigned long long> opted[2][2] = {{{0}, {0}}, {{0}, {0}}};
    const bool byval = n_models <= kSmallByValue;
    bool prior = false;
    for (int j = 0; j < n_runs; ++j) prior = prior || runs[j].n_prior > 0;
    SmallSetArgs args{};
    if (byval) std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_models);
    auto launch = [&](auto kernel) {
        small_lds_opt_in(reinterpret_cast<const void *>(kernel), opted[byval][prior]);
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_runs), dim3(256), sizeof(SmallShared), s, args,
                           sets, runs, scratch, stride, info, rings, final_out, status_out, rounds_out);
    };
    if (byval) prior ? launch(mle_sets_kernel<true, true>) : launch(mle_sets_kernel<true, false>);
    else prior ? launch(mle_sets_kernel<false, true>) : launch(mle_sets_kernel<false, false>);
}

}  // namespace cbo

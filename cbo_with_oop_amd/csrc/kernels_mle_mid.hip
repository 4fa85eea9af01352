// The hyper-parameter MLE of every model of 128 < n <= 256 observations in one launch for gfx950:
// mle_mid_kernel, mle_sets_kernel's search (kernels_mle.hip) around the two-block likelihood.  One workgroup
// of 256 threads runs one RUN -- one (model, start) pair -- from its start to the search's end; no workgroup waits for
// another, so a restart is one more workgroup.  Per evaluation:
//   thread 0 has left theta(x) of the search's trial point in LDS (mle_search.h), so every lane works from the same doubles;
//   mid_lml_sums_at (cbo_mid_lml_device.h) prepares the model's points from its RAW coordinates with theta's lengthscales
//   into the run's slab and runs the five stages small_lml_batch_kernel runs on a model's resident points;
//   thread 0 turns the sums into the likelihood and its gradients with the host's own arithmetic (lml_outputs.h), adds the
//   log prior of a run that has one (hyper_prior.h) and advances the search (mle_feed).
// The likelihood at a trial point is therefore what cbo_gp_lml_gradients_batch answers for the model at those
// hyper-parameters.  A TRIAL point whose Ky is not positive definite as assembled is fed as a non-finite value (the step
// halves) and the info word cleared; at the START it ends the run with CBO_MLE_NOT_PD and 0 rounds.
// The factor and L^-1 live in the run's slab (cbo_mid_lml_device.h), the search's two rings in the run's ring slot, read
// and written by thread 0 alone.  Nothing resident is written but those two.  Every loop is bounded: the evaluations by
// 1 + max_rounds, the search's own loops by 8 and P, the stages' by the padded size.
#include <cstring>

#include "cbo_mid_lml_device.h"
#include "hyper_prior.h"
#include "mle_search.h"

namespace cbo {

static_assert(sizeof(SmallShared) + 4 * kSmallLmlTerms * sizeof(double) + sizeof(MleSearch) + kMleMaxParams * sizeof(double)
                  + kMleMaxParams * (sizeof(cbo_hyper_prior) + sizeof(double)) <= 163840,
              "the workgroup's static LDS beside SmallShared: one CU");
static_assert(kMleMaxParams == CBO_MAX_DIM + 2, "variance, one lengthscale per dimension, noise variance");
static_assert(kMleRingDoubles == 2 * kRefineHistory * kMleMaxParams, "a run's ring slot holds the search's S and Y");

// PRIOR: some run of the launch has a prior.  The instantiation without has no such stage.
template <bool BYVAL, bool PRIOR>
__global__ __launch_bounds__(256) void mle_mid_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
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
    __shared__ double prior_grad[kMleMaxParams];                  // ... and d log prior / d theta at the evaluated row
    const int b = blockIdx.x;
    const cbo_small_mle &rn = runs[b];
    const cbo_small_set st = BYVAL ? byval.s[rn.model] : sets[rn.model];
    const int tid = threadIdx.x;
    const int n_ls = rn.n_ls, P = rn.n_params, fit_noise = rn.fit_noise, max_rounds = rn.max_rounds;
    const int n_prior = rn.n_prior;
    double *slab = scratch + (int64_t)b * stride;
    double *ring = rings + (int64_t)b * kMleRingDoubles;

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
        const bool pd = mid_lml_sums_at(sh, red, st, row, n_ls, slab, &info[b]);
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

size_t mid_mle_scratch_doubles() { return kMidPointScratch; }      // the two-block slab and the point region behind it

void launch_mle_mid(hipStream_t s, const cbo_small_set *sets, int n_models, const cbo_small_mle *runs, int n_runs,
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
    if (byval) prior ? launch(mle_mid_kernel<true, true>) : launch(mle_mid_kernel<true, false>);
    else prior ? launch(mle_mid_kernel<false, true>) : launch(mle_mid_kernel<false, false>);
}

}  // namespace cbo

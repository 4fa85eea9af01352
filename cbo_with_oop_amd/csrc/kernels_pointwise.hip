// Point-wise acquisitions for gfx950: lower confidence bound, probability of improvement and model variance over a cost with
// the arg-max, and the plug-in incumbent of the mean-plug-in Expected Improvement.
//
// Restates emukit 0.4's emukit.bayesian_optimization.acquisitions.NegativeLowerConfidenceBound and ProbabilityOfImprovement
// and emukit.experimental_design.acquisitions.ModelVariance from memory (emukit is not a dependency; parity is unpinned, the
// contract is DESIGN.md §4k):
//   NegativeLowerConfidenceBound.evaluate(x):  mean, variance = model.predict(x); -(mean - beta * sqrt(variance))
//   ProbabilityOfImprovement.evaluate(x):      mean, variance = model.predict(x); mean += jitter; sd = sqrt(variance);
//                                              scipy.stats.norm.cdf((y_minimum - mean) / sd)
//   ModelVariance.evaluate(x):                 model.predict(x)[1]
//   MeanPluginExpectedImprovement:             ExpectedImprovement whose y_minimum is min(model.predict(model.X)[0])
// and emukit.core.acquisition's Quotient (a / b).  Task 'max' mirrors them: mean + beta sd (the upper confidence bound),
// ndtr(-u), max of the means.  Mean and variance come from q = sum V^2, mu = V^T z exactly as acq_kernel forms them
// (kernels_acq.hip, posterior_of with the noise): cbo_gp_predict's bits.
// HBM-bound like the EI pass: 2 doubles in per candidate (4 for a causal model), up to 3 out.
#include "acq_pass.h"

#pragma clang fp contract(off)

namespace cbo {

// (pointwise_of, one candidate's value over the cost, lives in cbo_device.h: the one-launch multi-set sweep shares it.)

// acq_pass (acq_pass.h) scored by pointwise_of<KIND>.
// KIND: CBO_ACQ_LCB, CBO_ACQ_PI or CBO_ACQ_VAR (compile time: one kind's arithmetic per instantiation), or kLogEiKind: the
// pass scored by log_ei_of, log EI - log cost; CAUSAL: the candidates carry a prior mean / variance; MV: mean
// and / or variance are written out.
template <int KIND, bool CAUSAL, bool MV>
__global__ __launch_bounds__(256) void pointwise_acq_kernel(const double *__restrict__ q, const double *__restrict__ mu,
                                                            const double *__restrict__ pm, const double *__restrict__ pv,
                                                            int64_t m, AcqParams p, double *__restrict__ mean_out,
                                                            double *__restrict__ var_out, double *__restrict__ acq_out,
                                                            double *__restrict__ part_val,
                                                            int64_t *__restrict__ part_idx, int64_t index_offset)
{
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    if (!MV) { mean_out = nullptr; var_out = nullptr; }
    [[maybe_unused]] const double log_cost = (KIND == kLogEiKind) ? log(p.cost) : 0.0;      // (uniform: once per launch)
    auto score = [&](d2 mean2, d2 var2) {
        if constexpr (KIND == kLogEiKind)
            return d2{log_ei_of(mean2[0], var2[0], p, log_cost), log_ei_of(mean2[1], var2[1], p, log_cost)};
        else
            return d2{pointwise_of<KIND>(mean2[0], var2[0], p), pointwise_of<KIND>(mean2[1], var2[1], p)};
    };
    acq_pass<CAUSAL>(q, mu, pm, pv, m, p, true, mean_out, var_out, acq_out, index_offset, score, bv, bi);
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

// pointwise_acq_kernel<kLogEiKind> whose incumbent is read from p.y_best_dev, device memory, as acq_kernel reads it: the
// log-EI pass of a batch's further picks under update_incumbent (cbo_acq_sweep_batch_logei), where the
// incumbent moves on the device (BatchState::y_best).  A kernel of its own: routing the read through a shared body moved
// instructions in the arg-max tail of the existing instantiations, which stay the parent's code this way.
template <bool CAUSAL, bool MV>
__global__ __launch_bounds__(256) void logei_moved_incumbent_kernel(const double *__restrict__ q, const double *__restrict__ mu,
                                                                    const double *__restrict__ pm,
                                                                    const double *__restrict__ pv, int64_t m, AcqParams p,
                                                                    double *__restrict__ mean_out,
                                                                    double *__restrict__ var_out, double *__restrict__ acq_out,
                                                                    double *__restrict__ part_val,
                                                                    int64_t *__restrict__ part_idx, int64_t index_offset)
{
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    p.y_best = *p.y_best_dev;                                        // (uniform)
    if (!MV) { mean_out = nullptr; var_out = nullptr; }
    const double log_cost = log(p.cost);                             // (uniform: once per launch)
    auto score = [&](d2 mean2, d2 var2) {
        return d2{log_ei_of(mean2[0], var2[0], p, log_cost), log_ei_of(mean2[1], var2[1], p, log_cost)};
    };
    acq_pass<CAUSAL>(q, mu, pm, pv, m, p, true, mean_out, var_out, acq_out, index_offset, score, bv, bi);
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

template <int KIND>
static void launch_pointwise_kind(hipStream_t s, const double *q, const double *mu, const double *pm, const double *pv,
                                  int64_t m, const AcqParams &p, double *mean_out, double *var_out, double *acq_out,
                                  double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    const bool causal = pv != nullptr, mv = mean_out || var_out;
    auto kernel = causal ? (mv ? pointwise_acq_kernel<KIND, true, true> : pointwise_acq_kernel<KIND, true, false>)
                         : (mv ? pointwise_acq_kernel<KIND, false, true> : pointwise_acq_kernel<KIND, false, false>);
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(256), 0, s, q, mu, pm, pv, m, p, mean_out, var_out, acq_out, part_val,
                       part_idx, index_offset);
}

void launch_pointwise_acq(hipStream_t s, int kind, const double *q, const double *mu, const double *pm, const double *pv,
                          int64_t m, const AcqParams &p, double *mean_out, double *var_out, double *acq_out,
                          double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    if (kind == kLogEiKind && p.y_best_dev) {
        const bool causal = pv != nullptr, mv = mean_out || var_out;
        auto kernel = causal ? (mv ? logei_moved_incumbent_kernel<true, true> : logei_moved_incumbent_kernel<true, false>)
                             : (mv ? logei_moved_incumbent_kernel<false, true> : logei_moved_incumbent_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(256), 0, s, q, mu, pm, pv, m, p, mean_out, var_out, acq_out, part_val,
                           part_idx, index_offset);
        return;
    }
    auto launch = kind == CBO_ACQ_LCB ? launch_pointwise_kind<CBO_ACQ_LCB>
                  : kind == CBO_ACQ_PI ? launch_pointwise_kind<CBO_ACQ_PI>
                  : kind == kLogEiKind ? launch_pointwise_kind<kLogEiKind> : launch_pointwise_kind<CBO_ACQ_VAR>;
    launch(s, q, mu, pm, pv, m, p, mean_out, var_out, acq_out, part_val, part_idx, index_offset, n_blocks);
}

// ---- per-candidate intervention costs ------------------------------------------------------------------
// cost[j] = c(x_j) = sum_k (fix[k] + (variable[k] ? |x_jk| : 0)) from the set's raw AoS points: the refinement kernel's order
// (small_sets_refine_kernel) and the host's one_row_cost -- terms added from 0.0 in column order, no contraction.  A NaN
// coordinate of a variable column gives a NaN cost.
__global__ __launch_bounds__(256) void cands_cost_kernel(const double *__restrict__ raw, int64_t m, int d, const CostTable t,
                                                         double *__restrict__ cost)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k)
            if (k < d) c = c + (t.variable[k] ? t.fix[k] + fabs(raw[j * d + k]) : t.fix[k]);
        cost[j] = c;
    }
}

void launch_cands_cost(hipStream_t s, const double *raw, int64_t m, int d, const CostTable &t, double *cost)
{
    const int64_t want = (m + 255) / 256;
    hipLaunchKernelGGL(cands_cost_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, s, raw, m, d, t, cost);
}

// acq_pass with the cost stream (COST), scored per candidate over its own cost.  LOG false: acquisition_of at cost 1 -- the
// Expected Improvement itself -- then the IEEE quotient by cost[j] (numpy's `/`); true: log_ei_of with log(cost[j]), the
// device library's logarithm.  mean and var are acq_kernel's bits.  p.cost must be 1.
template <bool LOG, bool CAUSAL, bool MV>
__global__ __launch_bounds__(256) void pointcost_acq_kernel(const double *__restrict__ q, const double *__restrict__ mu,
                                                            const double *__restrict__ pm, const double *__restrict__ pv,
                                                            const double *__restrict__ cost, int64_t m, AcqParams p,
                                                            double *__restrict__ mean_out, double *__restrict__ var_out,
                                                            double *__restrict__ acq_out, double *__restrict__ part_val,
                                                            int64_t *__restrict__ part_idx, int64_t index_offset)
{
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    if (!MV) { mean_out = nullptr; var_out = nullptr; }
    auto score = [&](d2 mean2, d2 var2, d2 cost2) {
        if constexpr (LOG)
            return d2{log_ei_of(mean2[0], var2[0], p, log(cost2[0])), log_ei_of(mean2[1], var2[1], p, log(cost2[1]))};
        else
            return d2{acquisition_of(mean2[0], var2[0], p) / cost2[0], acquisition_of(mean2[1], var2[1], p) / cost2[1]};
    };
    acq_pass<CAUSAL, decltype(score), true>(q, mu, pm, pv, m, p, true, mean_out, var_out, acq_out, index_offset, score, bv, bi,
                                            cost);
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

template <bool LOG>
static void launch_pointcost_form(hipStream_t s, const double *q, const double *mu, const double *pm, const double *pv,
                                  const double *cost, int64_t m, const AcqParams &p, double *mean_out, double *var_out,
                                  double *acq_out, double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    const bool causal = pv != nullptr, mv = mean_out || var_out;
    auto kernel = causal ? (mv ? pointcost_acq_kernel<LOG, true, true> : pointcost_acq_kernel<LOG, true, false>)
                         : (mv ? pointcost_acq_kernel<LOG, false, true> : pointcost_acq_kernel<LOG, false, false>);
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(256), 0, s, q, mu, pm, pv, cost, m, p, mean_out, var_out, acq_out,
                       part_val, part_idx, index_offset);
}

void launch_pointcost_acq(hipStream_t s, bool log_form, const double *q, const double *mu, const double *pm, const double *pv,
                          const double *cost, int64_t m, const AcqParams &p, double *mean_out, double *var_out,
                          double *acq_out, double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    auto launch = log_form ? launch_pointcost_form<true> : launch_pointcost_form<false>;
    launch(s, q, mu, pm, pv, cost, m, p, mean_out, var_out, acq_out, part_val, part_idx, index_offset, n_blocks);
}

// out[0] = min (task 'min') or max of mean[0:n), NaN if any of them is (np.min / np.max): one workgroup, each lane a
// strided share, then the waves' and the workgroup's reduction.  n is a model's observation count: next to the prediction
// that produced the means this is nothing.
__global__ __launch_bounds__(256) void plugin_incumbent_kernel(const double *__restrict__ mean, int64_t n, int task,
                                                               double *__restrict__ out)
{
    __shared__ double sv[4];
    __shared__ int sn[4];
    const bool is_min = task == CBO_TASK_MIN;                    // (uniform)
    double acc = is_min ? INFINITY : -INFINITY;
    int nan = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = mean[i];
        nan |= isnan(v) ? 1 : 0;
        if (is_min ? v < acc : v > acc) acc = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(acc, off);
        nan |= __shfl_down(nan, off);
        if (is_min ? ov < acc : ov > acc) acc = ov;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sv[wave] = acc; sn[wave] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            nan |= sn[w];
            if (is_min ? sv[w] < acc : sv[w] > acc) acc = sv[w];
        }
        out[0] = nan ? __builtin_nan("") : acc;
    }
}

void launch_plugin_incumbent(hipStream_t s, const double *mean, int64_t n, int task, double *out)
{
    hipLaunchKernelGGL(plugin_incumbent_kernel, dim3(1), dim3(256), 0, s, mean, n, task, out);
}

}  // namespace cbo

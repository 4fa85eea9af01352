// Constrained acquisition for gfx950: Expected Improvement times probabilities of feasibility over a cost, with the arg-max,
// in one pass over the candidates -- emukit's
//     Quotient(Product(Product(ExpectedImprovement(model), ProbabilityOfFeasibility(c_0)), ProbabilityOfFeasibility(c_1)) ..., Cost)
//
// Restates emukit 0.4's emukit.bayesian_optimization.acquisitions.ProbabilityOfFeasibility from memory (emukit is not a
// dependency; parity is unpinned, the contract is DESIGN.md §4f):
//   evaluate(x):  mean, variance = model.predict(x); mean += jitter; sd = sqrt(variance);
//                 scipy.stats.norm.cdf(max_value, mean, sd)            = ndtr((max_value - mean) / sd)
// and emukit.core.acquisition's Product (a * b) and Quotient (a / b).  A constraint of the other sense, value <= g(x), is the
// complement by symmetry, ndtr(-u).  Every model's mean and variance come from its q = sum V^2, mu = V^T z exactly as
// acq_kernel forms them (kernels_acq.hip); the EI term is that kernel's acquisition_of at cost 1.
// HBM-bound like the EI pass: 2 doubles in per model and candidate (4 for a causal one), nothing out but the workgroup's
// arg-max partial unless per-candidate outputs are asked for.
#include "acq_pass.h"

#pragma clang fp contract(off)

namespace cbo {

// (one constraint's term: feasibility_of, cbo_device.h -- shared with the probability of improvement, kernels_pointwise.hip)

// acq_pass's discipline (acq_pass.h; its comments say why) with its fetch_pair / store_pair, but a loop of its own: a step
// here is ONE model's term of one pair of candidates.  The operands it prefetches are the next model's (the first model's
// of the workgroup's next pair after the last), the result it stores the previous step's -- so the registers hold two
// models' operands whatever the number of models, and the loop over the models has a uniform trip count with the table in
// the kernel arguments (scalar loads).
// CAUSAL: some model's candidates carry a prior mean / variance (the others skip those loads: uniform); OUT: per-candidate
// results are written (acq, and each model's own term where its `out` is set).  The common call asks for neither.
// LOG: the sum of logarithms in the place of the product -- log_ei_of at log cost 0.0 for the objective (the
// mirror for task 'max', not the product form's -EI), log_feasibility_of for a constraint, ((logEI + l_0) + l_1) + ... left to
// right, then one subtraction of log(cost): cbo_acq_sweep_logei's bits with no constraint, for every cost.  The product
// form's instantiations are what they were.
template <bool CAUSAL, bool OUT, bool LOG>
__global__ __launch_bounds__(256) void constrained_acq_kernel(ConParams p, int64_t m, double *__restrict__ acq_out,
                                                              double *__restrict__ part_val,
                                                              int64_t *__restrict__ part_idx, int64_t index_offset)
{
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    if (!OUT) acq_out = nullptr;
    const int nm = p.n_models;
    const int64_t stride = 2 * (int64_t)gridDim.x * kPassThreads;
    int64_t cu = 2 * (int64_t)blockIdx.x * kPassThreads;
    const unsigned lane2 = 2 * threadIdx.x;
    const int64_t span = 2 * kPassThreads;
    // one model's operands; whether it carries a prior is decided per model (uniform)
    auto fetch = [&](const ConModel &md, int64_t base, d2 &q2, d2 &mu2, d2 &pm2, d2 &pv2) __attribute__((always_inline)) {
        fetch_pair(md.q, md.mu, md.pm, md.pv, CAUSAL && md.pv != nullptr, m, base, q2, mu2, pm2, pv2);
    };
    AcqParams ap;                                                // the fields posterior_of / acquisition_of read, per model
    ap.y_best = p.y_best; ap.ei_jitter = p.ei_jitter; ap.cost = 1.0;
    ap.task = p.task; ap.include_noise = 1; ap.want_ei = 1;
    const double log_cost = LOG ? log(p.cost) : 0.0;             // (uniform: once per launch)
    d2 qn = {0.0, 0.0}, mun = {0.0, 0.0}, pmn = {0.0, 0.0}, pvn = {0.0, 0.0};
    // results waiting for the next step's store: one model's term, and the finished product of a pair
    d2 term_done = {0.0, 0.0}, acq_done = {0.0, 0.0};
    double *term_dst = nullptr;
    int64_t term_base = 0, acq_base = -1;
    fetch(p.mdl[0], cu, qn, mun, pmn, pvn);
    for (; cu < m; cu += stride) {
        const bool full = cu + span <= m;                        // uniform
        const int64_t c = cu + lane2;
        const bool one = full || c < m, two = full || c + 1 < m;
        d2 acc = {0.0, 0.0};
        for (int k = 0; k < nm; ++k) {
            const ConModel &md = p.mdl[k];
            d2 q2 = qn, mu2 = mun, pm2 = pmn, pv2 = pvn;
            operand_fence<CAUSAL>(q2, mu2, pm2, pv2);
            if (OUT) {
                store_pair<1>({term_dst}, {term_done}, m, term_base);
                if (acq_base >= 0) store_pair<1>({acq_out}, {acq_done}, m, acq_base);
                acq_base = -1;
            }
            const bool last = k + 1 == nm;
            fetch(p.mdl[last ? 0 : k + 1], last ? cu + stride : cu, qn, mun, pmn, pvn);
            const bool causal = CAUSAL && md.pv != nullptr;      // (uniform)
            ap.variance = md.variance;
            ap.noise_var = md.noise_var;
            d2 mean2, var2, t2;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                double mean, var;
                posterior_of(q2[e], mu2[e], causal ? pm2[e] : 0.0, causal ? pv2[e] : 0.0, causal, ap, mean, var);
                mean2[e] = mean;
                var2[e] = var;
            }
            if (LOG) {
                if (k == 0 && p.has_objective) {                 // (uniform) cbo_acq_sweep_logei's acq at cost 1
                    t2[0] = log_ei_of(mean2[0], var2[0], ap, 0.0);
                    t2[1] = log_ei_of(mean2[1], var2[1], ap, 0.0);
                } else {
                    t2[0] = log_feasibility_of(mean2[0], var2[0], md.value, md.jitter, md.sense);
                    t2[1] = log_feasibility_of(mean2[1], var2[1], md.value, md.jitter, md.sense);
                }
                if (k == 0) acc = t2;
                else acc = acc + t2;
            } else if (k == 0 && p.has_objective) {              // (uniform) cbo_acq_sweep's acq at cost 1
                t2[0] = acquisition_of(mean2[0], var2[0], ap);
                t2[1] = acquisition_of(mean2[1], var2[1], ap);
                acc = t2;
            } else {
                t2[0] = feasibility_of(mean2[0], var2[0], md.value, md.jitter, md.sense);
                t2[1] = feasibility_of(mean2[1], var2[1], md.value, md.jitter, md.sense);
                if (k == 0) acc = t2;
                else acc = acc * t2;
            }
            if (OUT) { term_dst = md.out; term_base = cu; term_done = t2; }
        }
        if (LOG) {
            acc[0] = acc[0] - log_cost;
            acc[1] = acc[1] - log_cost;
        } else if (nm == 1 && p.has_objective) {
            // no constraint: acquisition_of's own quotient (the reciprocal of the cost, corrected by the remainder), so that
            // the result is cbo_acq_sweep's bits for every cost
            const double rc = 1.0 / p.cost;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double qv = acc[e] * rc;
                acc[e] = fma(fma(-qv, p.cost, acc[e]), rc, qv);
            }
        } else {
            acc[0] = acc[0] / p.cost;                            // IEEE division (emukit's Quotient is numpy's)
            acc[1] = acc[1] / p.cost;
        }
        lane_argmax(one, acc[0], c + index_offset, bv, bi);
        lane_argmax(two, acc[1], c + 1 + index_offset, bv, bi);
        if (OUT) { acq_done = acc; acq_base = cu; }
    }
    if (OUT) {
        store_pair<1>({term_dst}, {term_done}, m, term_base);
        if (acq_base >= 0) store_pair<1>({acq_out}, {acq_done}, m, acq_base);
    }
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

void launch_constrained_acq(hipStream_t s, const ConParams &p, int64_t m, double *acq_out, double *part_val,
                            int64_t *part_idx, int64_t index_offset, int n_blocks, bool log_form)
{
    bool causal = false, out = acq_out != nullptr;
    for (int k = 0; k < p.n_models; ++k) {
        causal = causal || p.mdl[k].pv != nullptr;
        out = out || p.mdl[k].out != nullptr;
    }
    auto kernel = causal ? (out ? constrained_acq_kernel<true, true, false> : constrained_acq_kernel<true, false, false>)
                         : (out ? constrained_acq_kernel<false, true, false> : constrained_acq_kernel<false, false, false>);
    if (log_form)
        kernel = causal ? (out ? constrained_acq_kernel<true, true, true> : constrained_acq_kernel<true, false, true>)
                        : (out ? constrained_acq_kernel<false, true, true> : constrained_acq_kernel<false, false, true>);
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(256), 0, s, p, m, acq_out, part_val, part_idx, index_offset);
}

}  // namespace cbo

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
#include "cbo_device.h"

#pragma clang fp contract(off)

namespace cbo {

// (pointwise_of, one candidate's value over the cost, lives in cbo_device.h: the one-launch multi-set sweep shares it.)

// acq_kernel's structure (kernels_acq.hip; its comments say why): two consecutive candidates per lane and iteration (16-byte
// loads and stores), addresses "scalar base + 32-bit lane offset", and every memory operation of an iteration issued in one
// place right behind the iteration's only wait -- the operands of the NEXT iteration and the results of the PREVIOUS one.
// KIND: CBO_ACQ_LCB, CBO_ACQ_PI or CBO_ACQ_VAR (compile time: one kind's arithmetic per instantiation); CAUSAL: the
// candidates carry a prior mean / variance; MV: mean and / or variance are written out.
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
    constexpr bool causal = CAUSAL;
    if (!MV) { mean_out = nullptr; var_out = nullptr; }
    const int64_t stride = 2 * (int64_t)gridDim.x * blockDim.x;
    const int64_t first = 2 * (int64_t)blockIdx.x * blockDim.x;
    int64_t cu = first;
    const unsigned lane2 = 2 * threadIdx.x;
    const int64_t span = 2 * (int64_t)blockDim.x;
    // operands of the pair at base + lane2 (the second of an odd tail: a copy of the first, never stored); nothing is read
    // at or beyond m
    auto fetch = [&](int64_t base, d2 &q2, d2 &mu2, d2 &pm2, d2 &pv2) __attribute__((always_inline)) {
        if (base + span <= m) {                                  // (uniform) every lane has its two candidates
            q2 = *reinterpret_cast<const d2 *>(q + base + lane2);
            mu2 = *reinterpret_cast<const d2 *>(mu + base + lane2);
            if (causal) {
                pm2 = *reinterpret_cast<const d2 *>(pm + base + lane2);
                pv2 = *reinterpret_cast<const d2 *>(pv + base + lane2);
            }
            return;
        }
        const int64_t at = base + lane2;
        if (at + 1 < m) {
            q2 = *reinterpret_cast<const d2 *>(q + at);
            mu2 = *reinterpret_cast<const d2 *>(mu + at);
            if (causal) {
                pm2 = *reinterpret_cast<const d2 *>(pm + at);
                pv2 = *reinterpret_cast<const d2 *>(pv + at);
            }
        } else if (at < m) {
            q2 = d2{q[at], q[at]};
            mu2 = d2{mu[at], mu[at]};
            if (causal) {
                pm2 = d2{pm[at], pm[at]};
                pv2 = d2{pv[at], pv[at]};
            }
        }
    };
    auto store = [&](int64_t base, const d2 &mean2, const d2 &var2, const d2 &acq2) __attribute__((always_inline)) {
        const int64_t c = base + lane2;
        if (base + span <= m) {                                  // (uniform)
            if (mean_out) *reinterpret_cast<d2 *>(mean_out + base + lane2) = mean2;
            if (var_out) *reinterpret_cast<d2 *>(var_out + base + lane2) = var2;
            if (acq_out) *reinterpret_cast<d2 *>(acq_out + base + lane2) = acq2;
        } else if (c + 1 < m) {
            if (mean_out) *reinterpret_cast<d2 *>(mean_out + c) = mean2;
            if (var_out) *reinterpret_cast<d2 *>(var_out + c) = var2;
            if (acq_out) *reinterpret_cast<d2 *>(acq_out + c) = acq2;
        } else if (c < m) {
            if (mean_out) mean_out[c] = mean2[0];
            if (var_out) var_out[c] = var2[0];
            if (acq_out) acq_out[c] = acq2[0];
        }
    };
    d2 qn = {0.0, 0.0}, mun = {0.0, 0.0}, pmn = {0.0, 0.0}, pvn = {0.0, 0.0};
    d2 mean_done = {0.0, 0.0}, var_done = {0.0, 0.0}, acq_done = {0.0, 0.0};
    fetch(cu, qn, mun, pmn, pvn);
    for (int64_t done = -1; cu < m; done = cu, cu += stride) {
        d2 q2 = qn, mu2 = mun, pm2 = pmn, pv2 = pvn;
        // (the operands are in their registers before anything below is issued; nothing memory moves across this line)
        if (CAUSAL) asm volatile("" : "+v"(q2), "+v"(mu2), "+v"(pm2), "+v"(pv2) : : "memory");
        else asm volatile("" : "+v"(q2), "+v"(mu2) : : "memory");
        if (done >= 0) store(done, mean_done, var_done, acq_done);
        fetch(cu + stride, qn, mun, pmn, pvn);
        const bool full = cu + span <= m;                        // uniform
        const int64_t c = cu + lane2;
        const bool one = full || c < m, two = full || c + 1 < m;
        d2 mean2, var2, acq2;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            double mean, var;
            posterior_of(q2[e], mu2[e], causal ? pm2[e] : 0.0, causal ? pv2[e] : 0.0, causal, p, mean, var);
            mean2[e] = mean;
            var2[e] = var;
            acq2[e] = pointwise_of<KIND>(mean, var, p);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double acq = acq2[e];
            const int64_t gi = c + e + index_offset;
            if ((e == 0 ? one : two) && !(acq < bv) && better(acq, gi, bv, bi)) { bv = acq; bi = gi; }
        }
        mean_done = mean2;
        var_done = var2;
        acq_done = acq2;
    }
    // (cu has run past m by whole strides: the last iteration's results, if there was one)
    if (cu - stride >= first) store(cu - stride, mean_done, var_done, acq_done);
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
    auto launch = kind == CBO_ACQ_LCB ? launch_pointwise_kind<CBO_ACQ_LCB>
                  : kind == CBO_ACQ_PI ? launch_pointwise_kind<CBO_ACQ_PI> : launch_pointwise_kind<CBO_ACQ_VAR>;
    launch(s, q, mu, pm, pv, m, p, mean_out, var_out, acq_out, part_val, part_idx, index_offset, n_blocks);
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

// emukit's max-value entropy search (MES, Wang & Jegelka 2017) for gfx950: the scoring pass of a sweep and the Gumbel fit.
//
// Restates emukit 0.4's emukit.bayesian_optimization.acquisitions.MaxValueEntropySearch from memory (emukit is not a
// dependency; parity is unpinned, the contract is DESIGN.md §4e):
//   evaluate(x):          fsd = max(sqrt(var), 1e-10), gamma = (mins - mean) / fsd (M x K),
//                         minus_cdf = clip(1 - ndtr(gamma), 1e-10, 1),
//                         mean_k(-gamma pdf(gamma) / (2 minus_cdf) - log(minus_cdf))
//   update_parameters():  _fit_gumbel's three scipy.optimize.bisect calls on
//                         probf(x) = 1 - exp(sum_i log_ndtr(-(x - fmean_i) / fsd_i))
// mean and variance come from q = sum V^2, mu = V^T z exactly as acq_kernel forms them (kernels_acq.hip).
#include "acq_pass.h"

#pragma clang fp contract(off)

namespace cbo {

// (mes_term / mes_of, the epilogue, are cbo_device.h's: the multi-set sweep of kernels_sets.hip shares them)

// acq_pass (acq_pass.h) scored by mes_of.  Unlike the EI pass this one is bound by fp64 arithmetic (about a hundred vector
// instructions per sample), not by HBM; the two candidates of a lane are scored one after the other (one copy of the sample
// loop).
template <bool CAUSAL, bool MV>
__global__ __launch_bounds__(256) void mes_acq_kernel(const double *__restrict__ q, const double *__restrict__ mu,
                                                      const double *__restrict__ pm, const double *__restrict__ pv,
                                                      int64_t m, MesParams p, double *__restrict__ mean_out,
                                                      double *__restrict__ var_out, double *__restrict__ acq_out,
                                                      double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                      int64_t index_offset)
{
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    if (!MV) { mean_out = nullptr; var_out = nullptr; }
    AcqParams ap;                                                    // the posterior epilogue's fields of the EI pass
    ap.variance = p.variance; ap.noise_var = p.noise_var; ap.y_best = 0.0; ap.ei_jitter = 0.0; ap.cost = 1.0;
    ap.task = CBO_TASK_MIN; ap.include_noise = 1; ap.want_ei = 0;
    auto score = [&](d2 mean2, d2 var2) {
        d2 acq2;
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
            const double v = mes_of(e ? mean2[1] : mean2[0], e ? var2[1] : var2[0], p);
            if (e) acq2[1] = v; else acq2[0] = v;
        }
        return acq2;
    };
    acq_pass<CAUSAL>(q, mu, pm, pv, m, ap, true, mean_out, var_out, acq_out, index_offset, score, bv, bi);
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

void launch_mes_acq(hipStream_t s, const double *q, const double *mu, const double *pm, const double *pv, int64_t m,
                    const MesParams &p, double *mean_out, double *var_out, double *acq_out, double *part_val,
                    int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    const bool causal = pv != nullptr, mv = mean_out || var_out;
    auto kernel = causal ? (mv ? mes_acq_kernel<true, true> : mes_acq_kernel<true, false>)
                         : (mv ? mes_acq_kernel<false, true> : mes_acq_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(256), 0, s, q, mu, pm, pv, m, p, mean_out, var_out, acq_out, part_val,
                       part_idx, index_offset);
}

// ---- the Gumbel fit ------------------------------------------------------------------------------------------------
constexpr int kGumbelThreads = 1024;
constexpr int kGumbelWaves = kGumbelThreads / 64;

// sum_i log_ndtr(-(x - mean_i) / sqrt(var_i)) over the m grid points: thread t sums i = t, t + 1024, ... in order, a
// butterfly sums each wave, every thread sums the 16 wave partials in wave order -- every thread returns the same bits.
// `buf` alternates between two LDS rows from call to call, so one barrier per call suffices.
__device__ double gumbel_log_sum(const double *__restrict__ mean, const double *__restrict__ var, int64_t m, double x,
                                 double (*part)[kGumbelWaves], int &buf)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += kGumbelThreads) s = s + log_ndtr(-(x - mean[i]) / sqrt(var[i]));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s = s + __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) part[buf][threadIdx.x >> 6] = s;
    __syncthreads();
    double t = part[buf][0];
#pragma unroll
    for (int w = 1; w < kGumbelWaves; ++w) t = t + part[buf][w];
    buf ^= 1;
    return t;
}

// One workgroup per quantile (val = 0.25, 0.5, 0.75) and set.  left = min(fmean - 5 fsd), right = max(fmean + 5 fsd), then scipy's
// bisect (scipy/optimize/Zeros/bisect.c) with xtol = 2e-12, rtol = 4 eps, maxiter = 10000, on f(x) = probf(x) - val:
//     fa = f(xa), fb = f(xb); fa fb > 0: error; fa == 0: xa; fb == 0: xb; dm = xb - xa;
//     repeat: dm *= .5; xm = xa + dm; fm = f(xm); if fm fa >= 0: xa = xm; if fm == 0 or |dm| < xtol + rtol |xm|: xm
// Every thread holds the whole state and takes the same decisions from the same sums: the control flow is uniform.
// blockIdx.y is the set: its (mean, var, m) come from table[blockIdx.y] -- or, for the single fit, from the kernel
// arguments -- and its five doubles and three status words lie at out + 5 blockIdx.y, status + 3 blockIdx.y.
__global__ __launch_bounds__(kGumbelThreads) void gumbel_quantiles_kernel(const GumbelSet one,
                                                                          const GumbelSet *__restrict__ table,
                                                                          double *__restrict__ out,
                                                                          int64_t *__restrict__ status)
{
    const GumbelSet gs = table ? table[blockIdx.y] : one;             // (uniform)
    const double *__restrict__ mean = gs.mean;
    const double *__restrict__ var = gs.var;
    const int64_t m = gs.m;
    out += 5 * blockIdx.y;
    status += 3 * blockIdx.y;
    __shared__ double part[2][kGumbelWaves];
    __shared__ double lr[2][kGumbelWaves];
    int buf = 0;
    const double val = 0.25 * (double)(blockIdx.x + 1);
    // bracket: min / max are exact whatever the order; a NaN anywhere makes both NaN (np.min / np.max propagate it)
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = threadIdx.x; i < m; i += kGumbelThreads) {
        const double sd = sqrt(var[i]);
        const double a = mean[i] - 5.0 * sd, b = mean[i] + 5.0 * sd;
        lo = (isnan(a) || a < lo) ? a : lo;
        hi = (isnan(b) || b > hi) ? b : hi;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
        lo = (isnan(ol) || ol < lo) ? ol : lo;
        hi = (isnan(oh) || oh > hi) ? oh : hi;
    }
    if ((threadIdx.x & 63) == 0) { lr[0][threadIdx.x >> 6] = lo; lr[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = lr[0][0];
    hi = lr[1][0];
    for (int w = 1; w < kGumbelWaves; ++w) {
        lo = (isnan(lr[0][w]) || lr[0][w] < lo) ? lr[0][w] : lo;
        hi = (isnan(lr[1][w]) || lr[1][w] > hi) ? lr[1][w] : hi;
    }
    auto f = [&](double x) { return (1.0 - exp(gumbel_log_sum(mean, var, m, x, part, buf))) - val; };
    const double xtol = 2e-12, rtol = 4.0 * 2.220446049250313e-16;
    double xa = lo, result = lo;
    int64_t st = 0;
    const double fa = f(lo);
    const double fb = f(hi);
    if (fa * fb > 0.0) {
        st = 1;
    } else if (fa == 0.0) {
        result = lo;
    } else if (fb == 0.0) {
        result = hi;
    } else {
        double dm = hi - lo;
        st = 2;
        for (int it = 0; it < 10000; ++it) {
            dm *= 0.5;
            const double xm = xa + dm;
            const double fm = f(xm);
            if (fm * fa >= 0.0) xa = xm;
            if (fm == 0.0 || fabs(dm) < xtol + rtol * fabs(xm)) { result = xm; st = 0; break; }
        }
        if (st == 2) result = xa;
    }
    if (threadIdx.x == 0) {
        out[blockIdx.x] = result;
        status[blockIdx.x] = st;
        if (blockIdx.x == 0) { out[3] = lo; out[4] = hi; }
    }
}

void launch_gumbel_quantiles(hipStream_t s, const GumbelSet &one, const GumbelSet *table, int n_sets, double *out,
                             int64_t *status)
{
    hipLaunchKernelGGL(gumbel_quantiles_kernel, dim3(3, (unsigned)(table ? n_sets : 1)), dim3(kGumbelThreads), 0, s, one,
                       table, out, status);
}

}  // namespace cbo

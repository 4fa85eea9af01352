// The device-resident do-calculus prior for gfx950: what cbo_do_prior_create prepares once per handle
// beside the two Gram products (gram_tile_kernel, kernels_joint.hip), and do_prior_eval_kernel, cbo_do_prior_eval's
// launch.
//
//     b_ri = exp(-1/2 sum_{c not in I} ((O_rc - X_g[i,c]) / l_c)^2)      do_prior_rows_kernel, k-major like V: [N_obs_pad][ldb]
//     w_i  = sigma^2 alpha_i mean_r b_ri                                  do_prior_weights_kernel, r ascending
//     (m, v)(x)                                                           do_prior_eval_kernel: do_prior_at, one point per
//                                                                         workgroup and turn
//
// The squared distances are fma chains over differences of scaled coordinates and the exponential is exp_nonpositive, as
// cbo_device.h has them; every sum has one fixed order and nothing is accumulated atomically: two creations and two
// evaluations give the same bits.
#include "do_prior_device.h"

#pragma clang fp contract(off)

namespace cbo {

__global__ __launch_bounds__(256) void do_prior_rows_kernel(DoPriorRowsArgs a)
{
    const int64_t total = a.rows_pad * a.ldb;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / a.ldb, i = e - r * a.ldb;
        double v = 0.0;
        if (r < a.n_obs && i < a.n) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k)
                if (k < a.n_free) {
                    const int c = a.col[k];
                    const double o = a.obs[r * a.d + c];
                    const double dk = (a.ard ? o / a.ls[k] : o) - a.xs[(int64_t)c * a.ldx + i];
                    s = (k == 0) ? __dmul_rn(dk, dk) : __fma_rn(dk, dk, s);
                }
            v = exp_nonpositive(__dmul_rn(-0.5, __dmul_rn(s, a.inv_l2)));
        }
        a.b[e] = v;
    }
}

__global__ __launch_bounds__(256) void do_prior_weights_kernel(const double *__restrict__ b, int64_t ldb, int64_t n_obs,
                                                               const double *__restrict__ alpha, double variance, int n,
                                                               double *__restrict__ w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t r = 0; r < n_obs; ++r) s = __dadd_rn(s, b[r * ldb + i]);
    w[i] = __dmul_rn(__dmul_rn(variance, alpha[i]), __ddiv_rn(s, (double)n_obs));
}

__global__ __launch_bounds__(kDoPriorGroup) void do_prior_eval_kernel(const DoPriorView *__restrict__ view,
                                                                       const double *__restrict__ values, int64_t m,
                                                                       double *scratch, double *__restrict__ mean_out,
                                                                       double *__restrict__ var_out)
{
    __shared__ double red[2 * kDoPriorGroup / 64];
    const DoPriorView pv = *view;
    double *a = scratch + (int64_t)blockIdx.x * kDoPriorMaxN;
    for (int64_t p = blockIdx.x; p < m; p += gridDim.x) {               // (uniform)
        double xv[CBO_MAX_DIM];
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k) xv[k] = (k < pv.n_iv) ? values[p * pv.n_iv + k] : 0.0;
        double mean, var;
        do_prior_at<kDoPriorGroup>(pv, xv, a, red, (int)threadIdx.x, mean, var);
        if (threadIdx.x == 0) {
            mean_out[p] = mean;
            var_out[p] = var;
        }
    }
}

void launch_do_prior_rows(hipStream_t s, const DoPriorRowsArgs &a)
{
    const int64_t total = a.rows_pad * a.ldb;
    const int64_t blocks = (total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096;
    hipLaunchKernelGGL(do_prior_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

void launch_do_prior_weights(hipStream_t s, const double *b, int64_t ldb, int64_t n_obs, const double *alpha, double variance,
                             int n, double *w)
{
    hipLaunchKernelGGL(do_prior_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b, ldb, n_obs, alpha,
                       variance, n, w);
}

int do_prior_eval_blocks(int64_t m) { return (int)(m < 512 ? m : 512); }

void launch_do_prior_eval(hipStream_t s, const DoPriorView *view, const double *values, int64_t m, double *scratch,
                          double *mean_out, double *var_out)
{
    hipLaunchKernelGGL(do_prior_eval_kernel, dim3((unsigned)do_prior_eval_blocks(m)), dim3(kDoPriorGroup), 0, s, view, values,
                       m, scratch, mean_out, var_out);
}

}  // namespace cbo

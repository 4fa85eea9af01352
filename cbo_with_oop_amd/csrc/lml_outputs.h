// The few lines of arithmetic between the reduced sums of a likelihood kernel and what cbo_gp_lml_gradients answers with,
// written once: the host applies it to the record of small_lml_kernel / small_lml_batch_kernel and to the general path's
// sums (cbo_api.hip), hmc_sets_kernel applies it to the same sums inside its launch (kernels_hmc.hip) -- the likelihood an
// HMC chain sees on the device is then the text the host call answers with.  Plain C++17, no HIP headers; contraction off,
// so that the device forms no fused multiply-add where the host has none.
#pragma once

#if defined(__HIPCC__)
#define CBO_LML_HD __host__ __device__
#else
#define CBO_LML_HD
#endif
#if defined(__clang__)
#define CBO_LML_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CBO_LML_NO_CONTRACT
#endif

namespace cbo {

// grad_sums: the variance sum, then the lengthscale sums per dimension; ls: the d lengthscales of an ARD kernel, else the
// one lengthscale; zz = z^T z, logdet = sum log diag(U), aa = alpha^T alpha, tr_w = tr(Ky^-1).  dlengthscale_out: d values
// (ARD) or one.  lml_out may be null.
CBO_LML_HD inline void lml_outputs_of(double variance, bool ard, const double *ls, int d, long long n, const double *grad_sums,
                                      double zz, double logdet, double aa, double tr_w, double *lml_out,
                                      double *dvariance_out, double *dlengthscale_out, double *dnoise_out)
{
    CBO_LML_NO_CONTRACT
    *dvariance_out = 0.5 * grad_sums[0] / variance;
    if (ard) {
        for (int k = 0; k < d; ++k) dlengthscale_out[k] = 0.5 * grad_sums[1 + k] / ls[k];
    } else {
        double sum = 0.0;
        for (int k = 0; k < d; ++k) sum += grad_sums[1 + k];
        dlengthscale_out[0] = 0.5 * sum / ls[0];
    }
    *dnoise_out = 0.5 * (aa - tr_w);
    // GPy: 0.5 * (-n log(2 pi) - W_logdet - sum(alpha * (Y - m))),  W_logdet = 2 sum log L_ii
    if (lml_out) *lml_out = 0.5 * (-(double)n * 1.8378770664093453 - 2.0 * logdet - zz);
}

}  // namespace cbo

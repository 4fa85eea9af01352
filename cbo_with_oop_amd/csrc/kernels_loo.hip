// Leave-one-out cross-validation of a fitted Gaussian process from the one factor the model already holds
// (Rasmussen & Williams, Gaussian Processes for Machine Learning, 5.4.2; what GPy exposes as
// model.inference_method.LOO(kern, X, Y, likelihood, posterior)).  With r = y - m(X), alpha = Ky^-1 r and
// c_i = (Ky^-1)_ii:
//     mean_i = y_i - alpha_i / c_i          the prediction of y_i from the other n - 1 points
//     var_i  = 1 / c_i                      its predictive variance (of y_i: noise and the 1e-8 of Ky included)
//     lpd_i  = -1/2 log 2 pi + 1/2 log c_i - 1/2 alpha_i^2 / c_i
// lpd is GPy's return value (-neg_log_marginal_LOO).  GPy's formula is restated from memory, not from its source: parity
// with GPy is NOT pinned by a recorded GPy output (as for the emukit pieces); the tests pin the closed form against n
// brute-force refits on n - 1 points instead.
//
// Ky^-1 = L^-T L^-1, so c is the vector of squared column norms of L^-1 and alpha = L^-T z.  Two paths:
//   small_loo_batch_kernel   models of at most 128 observations, one workgroup each, not fitted beforehand: K(X,X) + diag,
//                            the factorisation and L^-1 inside LDS with the device functions small_lml_kernel uses
//                            (cbo_small_device.h), then everything above.  One launch for every model of a batch.
//   general path             L V = I by the sweep's own substitution kernels (kernels_trsm.hip), whose q output is c; here
//                            only the right-hand sides (loo_identity_chunk_kernel), the per-point epilogue
//                            (loo_finish_kernel) and the fixed-order sum (loo_sum_kernel).
// Summation orders (all fixed, so two identical calls return the same bits): c_i and alpha_i in the substitution kernels'
// order; the sum of lpd per 256 points as a binary tree over the workgroup, the per-workgroup partials -- and the small
// path's at most 128 terms -- one after the other in index order.
#include <hip/hip_ext.h>
#include <atomic>
#include <cstring>

#include "cbo_small_device.h"

namespace cbo {

// One point's three outputs.  IEEE divisions and the device library's log: a handful of points, nothing to save here.
__device__ __forceinline__ void loo_point(double y, double alpha, double c, double &mean, double &var, double &lpd)
{
#pragma clang fp contract(off)
    mean = y - alpha / c;
    var = 1.0 / c;
    lpd = (-0.91893853320467274178 + 0.5 * log(c)) - 0.5 * ((alpha * alpha) / c);
}

// ---- small path -------------------------------------------------------------------------------------------------------
// Model b reads descriptor b (by value up to kSmallByValue, else from the pinned array), uses scratch slot b (kSmallScratch
// doubles: factor rows and inverses), status word info[b] (zero on entry, zero again afterwards) and writes record out[b]
// (pinned host memory, closed by the call's sequence number).  A model whose Ky is not positive definite as assembled
// reports its first bad pivot in the record's info; its numbers then mean nothing.
template <bool BYVAL>
__global__ __launch_bounds__(256) void small_loo_batch_kernel(const SmallSetArgs byval,
                                                              const cbo_small_set *__restrict__ sets, double *scratch,
                                                              int *__restrict__ info,
                                                              cbo_small_loo_result *__restrict__ out, int seq)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int b = blockIdx.x;
    const cbo_small_set st = BYVAL ? byval.s[b] : sets[b];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int tiles = (st.n + 15) / 16;
    double *Us = scratch + (int64_t)b * kSmallScratch, *invs = Us + 128 * kSmallLd;
    double iv[8][4], zr[8][4];
    small_model_factor(sh, st, tiles, Us, invs, &info[b], iv, zr);
    // this thread's point (the epilogue below): in flight with the factor's way back into LDS
    double yi = 0.0;
    if (tid < st.n) yi = st.y[tid];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // the points' LDS copies are free once Ky is assembled: c, alpha and lpd are staged there
    double *c_s = sh.xs[0], *a_s = sh.xs[1], *l_s = sh.xs[2];
    // ---- V = L^-1: column tile ct of the identity through the tile solve (small_lml_kernel's loop without its stores);
    // c = column sums of V^2, alpha = V^T z
    for (int ct = wave; ct < tiles; ct += 4) {
        d4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = (t == ct && kq + 4 * r == lc) ? 1.0 : 0.0;
        double qacc = 0.0, macc = 0.0;
        panel_solve_tiles(&sh.blk.S[kq][lc], acc, iv, tiles, [&](int s2, const d4 &x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                qacc = fma(x[r], x[r], qacc);
                macc = fma(x[r], zr[s2][r], macc);
            }
        });
        qacc += __shfl_xor(qacc, 16);
        qacc += __shfl_xor(qacc, 32);
        macc += __shfl_xor(macc, 16);
        macc += __shfl_xor(macc, 32);
        const int col = 16 * ct + lc;
        if (kq == 0 && col < st.n) {
            c_s[col] = qacc;
            a_s[col] = macc;
        }
    }
    __syncthreads();
    if (tid < st.n) {
        double mean, var, lpd;
        loo_point(yi, a_s[tid], c_s[tid], mean, var, lpd);
        out[b].mean[tid] = mean;
        out[b].var[tid] = var;
        out[b].lpd[tid] = lpd;
        l_s[tid] = lpd;
        __threadfence_system();
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < st.n; ++i) sum += l_s[i];                  // index order
        out[b].sum = sum;
        out[b].info = atomicAdd(&info[b], 0);
        __threadfence_system();
        *reinterpret_cast<volatile int *>(&out[b].seq) = seq;
        info[b] = 0;
    }
}

size_t small_loo_scratch_doubles() { return (size_t)kSmallScratch; }

void launch_small_loo_batch(hipStream_t s, const cbo_small_set *sets, int n_models, double *scratch, int *info,
                            cbo_small_loo_result *out, int seq)
{
    {
        static std::atomic<unsigned long long> opted[2];
        const bool byval = n_models <= kSmallByValue;
        small_lds_opt_in(byval ? reinterpret_cast<const void *>(small_loo_batch_kernel<true>)
                               : reinterpret_cast<const void *>(small_loo_batch_kernel<false>), opted[byval]);
    }
    SmallSetArgs args{};
    if (n_models <= kSmallByValue) {
        std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_models);
        hipLaunchKernelGGL(small_loo_batch_kernel<true>, dim3((unsigned)n_models), dim3(256), sizeof(SmallShared), s, args,
                           sets, scratch, info, out, seq);
    } else {
        hipLaunchKernelGGL(small_loo_batch_kernel<false>, dim3((unsigned)n_models), dim3(256), sizeof(SmallShared), s,
                           args, sets, scratch, info, out, seq);
    }
}

// ---- general path -----------------------------------------------------------------------------------------------------
// Columns [c0, c0 + cols) of the identity for the trailing system that starts at row r0 <= c0: V[i][j] = 1 where
// r0 + i == c0 + j, 0 elsewhere, for i < rows, j < cols (cols even: two columns per thread, one 16-byte store).
__global__ __launch_bounds__(256) void loo_identity_chunk_kernel(double *__restrict__ V, int64_t ldv, int64_t rows,
                                                                 int64_t cols, int64_t shift /* c0 - r0 */)
{
    const int64_t i = blockIdx.x;
    const int64_t j = 2 * ((int64_t)blockIdx.y * 256 + threadIdx.x);
    if (i >= rows || j >= cols) return;
    d2 v;
    v[0] = (i == j + shift) ? 1.0 : 0.0;
    v[1] = (i == j + 1 + shift) ? 1.0 : 0.0;
    *reinterpret_cast<d2 *>(V + i * ldv + j) = v;
}

void launch_loo_identity_chunk(hipStream_t s, double *V, int64_t ldv, int64_t rows, int64_t cols, int64_t shift)
{
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(loo_identity_chunk_kernel, dim3((unsigned)rows, (unsigned)((cols + 511) / 512)), dim3(256), 0, s, V,
                       ldv, rows, cols, shift);
}

// mean, var, lpd of the points i < n (each output may be null) and partial[block] = the sum of the block's 256 lpd
// values, a binary tree in a fixed order; points i >= n (the padding) contribute nothing.
__global__ __launch_bounds__(256) void loo_finish_kernel(const double *__restrict__ c, const double *__restrict__ alpha,
                                                         const double *__restrict__ y, int64_t n,
                                                         double *__restrict__ mean_out, double *__restrict__ var_out,
                                                         double *__restrict__ lpd_out, double *__restrict__ partial)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    double lpd = 0.0;
    if (i < n) {
        double mean, var;
        loo_point(y[i], alpha[i], c[i], mean, var, lpd);
        if (mean_out) mean_out[i] = mean;
        if (var_out) var_out[i] = var;
        if (lpd_out) lpd_out[i] = lpd;
    }
    red[tid] = lpd;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) red[tid] = red[tid] + red[tid + half];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// out[0] = partial[0] + partial[1] + ... in index order (one workgroup, one lane adds)
__global__ void loo_sum_kernel(const double *__restrict__ partial, int nb, double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sum = 0.0;
    for (int b = 0; b < nb; ++b) sum += partial[b];
    *out = sum;
}

int loo_finish_blocks(int64_t n) { return (int)((n + 255) / 256); }

void launch_loo_finish(hipStream_t s, const double *c, const double *alpha, const double *y, int64_t n, double *mean_out,
                       double *var_out, double *lpd_out, double *partial, double *sum_out)
{
    const int nb = loo_finish_blocks(n);
    hipLaunchKernelGGL(loo_finish_kernel, dim3((unsigned)nb), dim3(256), 0, s, c, alpha, y, n, mean_out, var_out, lpd_out,
                       partial);
    hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(64), 0, s, partial, nb, sum_out);
}

}  // namespace cbo

// Device functions shared by the kernels that factor a small model (at most 128 observations) at hyper-parameters OTHER
// than its own, from its raw coordinates, and by those that turn such a factor into the log marginal likelihood and its
// gradients: hyper_avg_kernel / hyper_sets_kernel (kernels_hyper.hip), small_lml_kernel / small_lml_batch_kernel
// (kernels_chol.hip), hmc_sets_kernel (kernels_hmc.hip) and mle_sets_kernel (kernels_mle.hip).  Each function exists once, so the kernels built from them
// agree bit for bit.
#pragma once

#include "cbo_small_device.h"
#include "lml_outputs.h"

namespace cbo {

// One point from AoS raw coordinates: x[k] = raw[k] / ls[k] (ARD; ls null: unscaled), |x|^2 in prep_points_kernel's order
__device__ __forceinline__ void hyper_point(const double *__restrict__ raw, int64_t i, int d, const double *ls, bool in,
                                            double (&x)[CBO_MAX_DIM], double &sum)
{
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) x[k] = 0.0;
    if (in) {
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k)
            if (k < d) {
                double v = raw[i * d + k];
                if (ls) v = v / ls[k];
                x[k] = v;
            }
    }
    sum = squared_norm(x, d);
}

// The descriptor of sample h: the model's with the sample's variance, lengthscale and noise in the place of its own
__device__ __forceinline__ cbo_small_set hyper_sample_set(const cbo_small_set &st, const double *__restrict__ row, int n_ls)
{
    cbo_small_set sh = st;
    sh.variance = row[0];
    sh.lengthscale = st.ard ? 1.0 : row[1];
    sh.noise_var = row[1 + n_ls];
    sh.diag_add = __dadd_rn(sh.noise_var, kGpyDiagJitter);             // Ky = K + (noise + 1e-8) I
    return sh;
}

// The model's points of sample h into LDS (threads 0..127), as the resident copies of a model with that sample's
// lengthscales hold them.  The caller synchronises.
__device__ __forceinline__ void hyper_model_points(SmallShared &sh, const cbo_small_set &st, const double *ls)
{
    const int tid = threadIdx.x;
    if (tid < 128) {
        const bool in = tid < st.n;
        double x[CBO_MAX_DIM], sum;
        hyper_point(st.raw, tid, st.d, ls, in, x, sum);
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k)
            if (k < st.d) sh.xs[k][tid] = x[k];
        sh.sq[tid] = sum;
        sh.sv[tid] = (in && st.sv) ? sqrt(st.pv[tid]) : 0.0;
    }
}

// K(X,X) + diag and the rhs into the block, the factorisation of the `tiles` real tiles into the scratch slot (Us, invs):
// small_model_factor's steps between its point loads and its read-back, on points that are already in LDS
__device__ __forceinline__ void hyper_factor(SmallShared &sh, const cbo_small_set &st, int tiles, double rhs, double *Us,
                                             double *invs, int *info_word)
{
    const int tid = threadIdx.x;
    CBO_FOR_DIM(st.d, small_assemble<D>(sh, st, tiles));
    const int rows = 16 * tiles;
    for (int r = tid >> 4; r < rows; r += 16)
        for (int c = rows + (tid & 15); c < kDiagLd; c += 16) {
            if (c == 128 && r < st.n) continue;                                                // (the rhs: below)
            sh.blk.S[r][c] = 0.0;
        }
    if (tid < st.n) sh.blk.S[tid][128] = rhs;                                                  // r = y - m(X)
    __syncthreads();
    diag128_factor_in_lds(sh.blk, Us, kSmallLd, 0, 128, invs, info_word, nullptr, tiles, nullptr,
                          (st.n - 16 * (tiles - 1) + 3) / 4);
    // (ends with a barrier.)  Every wave's stores of factor rows / inverses / z are complete before anyone re-reads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// r = y - m(X) of this thread's row: it does not depend on the sample
__device__ __forceinline__ double hyper_rhs(const cbo_small_set &st)
{
    const int tid = threadIdx.x;
    double rhs = 0.0;
    if (tid < st.n) {
        const double yv = st.y[tid];
        rhs = st.pm ? __dadd_rn(yv, -st.pm[tid]) : yv;
    }
    return rhs;
}

// phases 1 of a two-launch form: factor the sample `row` of the model into the scratch slot `fs`, nothing else
__device__ __forceinline__ void hyper_factor_sample(SmallShared &sh, const cbo_small_set &st, const double *__restrict__ row,
                                                    int n_ls, int tiles, double rhs, double *fs, int *info_word)
{
    const cbo_small_set sth = hyper_sample_set(st, row, n_ls);
    hyper_model_points(sh, st, st.ard ? row + 1 : nullptr);
    __syncthreads();
    hyper_factor(sh, sth, tiles, rhs, fs, fs + 128 * kSmallLd, info_word);
}

// ------------------------------------------------------------------------------------------------
// Everything of the likelihood and its gradients that lies behind the factor (the second half of small_lml_body,
// kernels_chol.hip): the factor is in LDS (sh.blk.S) and in the scratch slot (Us; z in its column 128), its tile inverses
// and z in the registers iv / zr, the model's points in sh.xs / sh.sv, and every wave's loads have landed (s_waitcnt
// vmcnt(0) + barrier; alpha_s[0..127] zeroed before that barrier).  V = L^-1 goes to Vg ([128][kSmallLd] doubles);
//   alpha = V^T z, diag(Ky^-1) = column sums of V^2, W = V^T V tile by tile contracted with the kernel and its lengthscale
//   derivatives, then z^T z, sum log diag(U), alpha^T alpha and tr(Ky^-1), all reduced over the workgroup.
// Ends with the four waves' partial sums in red and a barrier: term k is small_lml_term(red, k).
template <int D>
__device__ __forceinline__ void small_lml_after_factor(SmallShared &sh, double *alpha_s, double (*red)[kSmallLmlTerms],
                                                       const cbo_small_set &st, const double *Us, double *Vg,
                                                       const double (&iv)[8][4], const double (&zr)[8][4])
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int tiles = (st.n + 15) / 16, rows = 16 * tiles;

    // ---- V = L^-1: column tile ct of the identity through the tile solve; alpha and diag(Ky^-1) fall out
    double trw = 0.0;
    for (int ct = wave; ct < tiles; ct += 4) {
        d4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = (t == ct && kq + 4 * r == lc) ? 1.0 : 0.0;
        double qacc = 0.0, macc = 0.0;
        double *Vc = Vg + 16 * ct + lc;
        panel_solve_tiles(&sh.blk.S[kq][lc], acc, iv, tiles, [&](int s2, const d4 &x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Vc[(int64_t)(16 * s2 + kq + 4 * r) * kSmallLd] = x[r];
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
            alpha_s[col] = macc;
            trw += qacc;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- gradient sums over the upper tile pairs, one pair per wave at a time
    const double inv_l2 = st.ard ? 1.0 : 1.0 / (st.lengthscale * st.lengthscale);
    double sum[1 + D];
#pragma unroll
    for (int k = 0; k <= D; ++k) sum[k] = 0.0;
    int pair = 0;
    for (int ti = 0; ti < tiles; ++ti)
        for (int tj = ti; tj < tiles; ++tj, ++pair) {
            if ((pair & 3) != wave) continue;                       // uniform per wave
            d4 w = {0.0, 0.0, 0.0, 0.0}, w2 = {0.0, 0.0, 0.0, 0.0};
            const double *Va = Vg + 16 * ti + lc, *Vb = Vg + 16 * tj + lc;
            // V is lower triangular: rows above tile tj contribute nothing to column tile tj
            for (int k0 = 16 * tj; k0 < rows; k0 += 8) {
                w = MFMA_F64(Va[(int64_t)(k0 + kq) * kSmallLd], Vb[(int64_t)(k0 + kq) * kSmallLd], w);
                w2 = MFMA_F64(Va[(int64_t)(k0 + 4 + kq) * kSmallLd], Vb[(int64_t)(k0 + 4 + kq) * kSmallLd], w2);
            }
            w += w2;
            const int gj = 16 * tj + lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = 16 * ti + kq + 4 * r;
                if (gi >= st.n || gj >= st.n || gj < gi) continue;
                double r2 = 0.0, d2k[D];
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double df = sh.xs[k][gi] - sh.xs[k][gj];
                    d2k[k] = df * df * inv_l2;
                    r2 += d2k[k];
                }
                const double kv = st.variance * exp_nonpositive(-0.5 * r2);
                const double m = (gi == gj ? 1.0 : 2.0) * (alpha_s[gi] * alpha_s[gj] - w[r]);
                const double mk = m * kv;
                sum[0] += mk + m * (sh.sv[gi] * sh.sv[gj]);
#pragma unroll
                for (int k = 0; k < D; ++k) sum[1 + k] = fma(mk, d2k[k], sum[1 + k]);
            }
        }
    // ---- z^T z, sum log diag(U), alpha^T alpha, tr(Ky^-1); everything reduced over the workgroup
    double terms[kSmallLmlTerms];
#pragma unroll
    for (int k = 0; k < kSmallLmlTerms; ++k) terms[k] = 0.0;
#pragma unroll
    for (int k = 0; k <= D; ++k) terms[k] = sum[k];
    if (tid < st.n) {
        const double zi = Us[(int64_t)tid * kSmallLd + 128];
        terms[1 + CBO_MAX_DIM + 0] = zi * zi;
        terms[1 + CBO_MAX_DIM + 1] = log(sh.blk.S[tid][tid]);
        terms[1 + CBO_MAX_DIM + 2] = alpha_s[tid] * alpha_s[tid];
    }
    terms[1 + CBO_MAX_DIM + 3] = trw;
#pragma unroll
    for (int k = 0; k < kSmallLmlTerms; ++k) {
        double v = terms[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
}

// term k of the record from the four waves' partial sums
__device__ __forceinline__ double small_lml_term(const double (*red)[kSmallLmlTerms], int k)
{
    return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// the factor of the scratch slot back into LDS (rows of the factored tiles; the solve reads nothing else), its tile
// inverses and z into registers: small_model_factor's closing steps.  Ends with loads in flight: the caller waits.
__device__ __forceinline__ void hmc_factor_to_lds(SmallShared &sh, const double *Us, const double *invs, int tiles,
                                                  double (&iv)[8][4], double (&zr)[8][4])
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const unsigned s0 = lds_byte_address(&sh.blk.S[0][0]);
    const int rows = 16 * tiles;
    for (int p = wave; p < rows; p += 4)
        glds16(Us + (int64_t)p * kSmallLd + lane * 2, __builtin_amdgcn_readfirstlane(s0 + 8u * (unsigned)(p * kDiagLd)));
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            iv[s][kk] = (s < tiles) ? invs[s * 256 + (4 * kk + kq) * 16 + lc] : 0.0;
            zr[s][kk] = (s < tiles) ? Us[(int64_t)(16 * s + kq + 4 * kk) * kSmallLd + 128] : 0.0;
        }
}

// The likelihood of the model st at the hyper-parameter row `row` (variance, lengthscale x n_ls, noise variance; in LDS, the
// same doubles for every lane) from its RAW coordinates, inside one resident workgroup: what hmc_sets_kernel does per
// position of a chain and mle_sets_kernel per evaluation of a search.  The points are prepared with the row's lengthscales,
// K(X,X) + (noise + 1e-8) I is assembled and factored inside LDS into the scratch slot (Us, invs), and the stages behind the
// factor leave the four waves' partial sums in red (small_lml_after_factor), behind a barrier.  Returns false -- to every
// thread alike, with nothing behind the factor done and the info word still set: the caller clears it -- when Ky is not
// positive definite as assembled.  alpha_s: 128 doubles of LDS that are free behind the factor.
__device__ __forceinline__ bool small_lml_sums_at(SmallShared &sh, double *alpha_s, double (*red)[kSmallLmlTerms],
                                                  const cbo_small_set &st, const double *row, int n_ls, int tiles, double rhs,
                                                  double *Us, double *invs, double *Vg, int *info_word)
{
    const int tid = threadIdx.x;
    const cbo_small_set sth = hyper_sample_set(st, row, n_ls);
    hyper_model_points(sh, st, st.ard ? row + 1 : nullptr);
    __syncthreads();
    hyper_factor(sh, sth, tiles, rhs, Us, invs, info_word);
    if (__hip_atomic_load(info_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return false;
    double iv[8][4], zr[8][4];
    hmc_factor_to_lds(sh, Us, invs, tiles, iv, zr);
    if (tid < 128) alpha_s[tid] = 0.0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CBO_FOR_DIM(st.d, small_lml_after_factor<D>(sh, alpha_s, red, sth, Us, Vg, iv, zr));
    return true;
}

// ... and, on ONE thread behind that barrier, the likelihood and its gradients with respect to the row's entries by the
// host's arithmetic (lml_outputs.h): dl[0] variance, dl[1 ..] the lengthscale(s), *dnoise the noise variance
__device__ __forceinline__ void small_lml_outputs_at(const cbo_small_set &st, const double *row,
                                                     const double (*red)[kSmallLmlTerms], double *lml, double *dl,
                                                     double *dnoise)
{
    double t[kSmallLmlTerms];
#pragma unroll
    for (int k = 0; k < kSmallLmlTerms; ++k) t[k] = small_lml_term(red, k);
    lml_outputs_of(row[0], st.ard != 0, row + 1, st.d, st.n, t, t[1 + CBO_MAX_DIM], t[1 + CBO_MAX_DIM + 1],
                   t[1 + CBO_MAX_DIM + 2], t[1 + CBO_MAX_DIM + 3], lml, &dl[0], &dl[1], dnoise);
}

}  // namespace cbo

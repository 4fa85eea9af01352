// Device functions of the two-block likelihood: the log marginal likelihood's sums for a model of 128 < n <= 256
// observations inside ONE workgroup with no fit, shared by small_lml_batch_kernel (kernels_chol.hip: the model at its own
// hyper-parameters, points read from its resident copies) and mle_mid_kernel (kernels_mle_mid.hip: the model at a search's
// trial hyper-parameters, points prepared from its raw coordinates).  Each function exists once, so the two
// kernels agree bit for bit.
//
// The padded size is 256: rows n..255 are identity padding.  The LDS holds one 128-row block at a time, so the factor and
// L^-1 live in the workgroup's global slab (about 1 MB, L2-resident):
//   1. K11 + diag and r1 into LDS, factored there (diag128_factor_in_lds): U11, its tile inverses, z1 to the slab
//   2. U12 = U11^-T K12 and V11 = U11^-T (identity) through the tile solve, U11 back in LDS
//   3. K22 - U12^T U12 (fp64 MFMA, tile by tile) and r2 - U12^T z1 into LDS, factored: U22, inverses, z2
//   4. V21 = U22^-T (-U12^T V11) and V22 = U22^-T (identity), U22 in LDS          (V = L^-1 = U^-T, lower triangular)
//   5. alpha = V^T z, diag(Ky^-1) = column sums of V^2, then W = V^T V tile by tile on the matrix cores, each tile
//      contracted with the kernel and its lengthscale derivatives -- the small kernel's sums, points read from global.
// Every slab word a stage reads was written earlier in the same evaluation (the upper right block of V is neither written
// nor read), and a read of a word that another wave wrote stays behind mid_sync().
#pragma once

#include "cbo_small_lml_device.h"

namespace cbo {

// the slab: [U11 | inverses 1 | U12 | U22 | inverses 2 | V | alpha], then -- for the kernels that prepare the model's points
// themselves -- the point region [xs (CBO_MAX_DIM x 256, SoA) | |x|^2 | sqrt(pv)]
constexpr int kMidLdV = 256 + 8;
constexpr size_t kMidU11 = 0, kMidInv1 = kMidU11 + 128 * kSmallLd, kMidU12 = kMidInv1 + 8 * 256,
                 kMidU22 = kMidU12 + 128 * kSmallLd, kMidInv2 = kMidU22 + 128 * kSmallLd, kMidV = kMidInv2 + 8 * 256,
                 kMidAlpha = kMidV + (size_t)256 * kMidLdV, kMidLmlScratch = kMidAlpha + 256;
constexpr int kMidPointLd = 256;
constexpr size_t kMidPointXs = kMidLmlScratch, kMidPointSq = kMidPointXs + (size_t)CBO_MAX_DIM * kMidPointLd,
                 kMidPointSv = kMidPointSq + kMidPointLd, kMidPointScratch = kMidPointSv + kMidPointLd;

template <int D>
__device__ __forceinline__ double mid_kernel_value(const cbo_small_set &st, int gi, int gj, double inv_l2)
{
    double xi[D], xj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { xi[k] = st.xs[(int64_t)k * st.ld + gi]; xj[k] = st.xs[(int64_t)k * st.ld + gj]; }
    double w = kernel_value<D>(xi, xj, st.sq[gi], st.sq[gj], st.variance, inv_l2, st.zero_diag && gi == gj);
    if (st.sv != nullptr) w = __dadd_rn(w, __dmul_rn(st.sv[gi], st.sv[gj]));
    return w;
}

// Ky block (b, b) (+ diag, identity padding) into LDS, upper tile pairs; for b = 1 minus U12^T U12 (MFMA, k = 0..127)
template <int D>
__device__ __forceinline__ void mid_assemble(SmallShared &sh, const cbo_small_set &st, int b, const double *U12)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    int pair = 0;
    for (int ti = 0; ti < 8; ++ti)
        for (int tj = ti; tj < 8; ++tj, ++pair) {
            if ((pair & 3) != wave) continue;                       // uniform per wave
            d4 w = {0.0, 0.0, 0.0, 0.0};
            if (b == 1) {
                const double *Pa = U12 + 16 * ti + lc, *Pb = U12 + 16 * tj + lc;
                for (int k0 = 0; k0 < 128; k0 += 4)
                    w = MFMA_F64(Pa[(int64_t)(k0 + kq) * kSmallLd], Pb[(int64_t)(k0 + kq) * kSmallLd], w);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = 16 * ti + kq + 4 * r, lj = 16 * tj + lc;
                const int gi = 128 * b + li, gj = 128 * b + lj;
                double v = (gi == gj) ? 1.0 : 0.0;                  // identity padding
                if (gi < st.n && gj < st.n) {
                    v = mid_kernel_value<D>(st, gi, gj, inv_l2);
                    if (gi == gj) v = __dadd_rn(v, st.diag_add);
                    v -= w[r];
                }
                sh.blk.S[li][lj] = v;
            }
        }
}

// the factor rows of a 128-row block from the slab into LDS (what the tile solve reads), the tile inverses to registers
__device__ __forceinline__ void mid_factor_to_lds(SmallShared &sh, const double *U, const double *invs, double (&iv)[8][4])
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int lc = lane & 15, kq = lane >> 4;
    for (int e = tid; e < 128 * 128; e += 256) sh.blk.S[e >> 7][e & 127] = U[(int64_t)(e >> 7) * kSmallLd + (e & 127)];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) iv[t][kk] = invs[t * 256 + (4 * kk + kq) * 16 + lc];
}

__device__ __forceinline__ void mid_sync()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// Stages 1-5 on the descriptor st (its xs / sq / sv are global memory: the model's resident copies, or a slab's point
// region).  Ends with the four waves' partial sums in red behind a barrier: term k is small_lml_term(red, k).
// CHECK: the info word is read behind the barrier that follows each of the two factorisations; a set word -- Ky is not
// positive definite as assembled -- returns false to every thread alike with nothing further done (the caller clears the
// word).  Without CHECK the stages run to their end whatever the word says, and the function returns true.
template <int D, bool CHECK>
__device__ __forceinline__ bool mid_lml_stages(SmallShared &sh, double (*red)[kSmallLmlTerms], const cbo_small_set &st,
                                               double *slab, int *__restrict__ info)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int n = st.n, n2 = st.n - 128;
    double *U11 = slab + kMidU11, *inv1 = slab + kMidInv1, *U12 = slab + kMidU12, *U22 = slab + kMidU22,
           *inv2 = slab + kMidInv2, *V = slab + kMidV, *alpha = slab + kMidAlpha;
    const double inv_l2a = 1.0 / (st.lengthscale * st.lengthscale);
    double iv[8][4];

    // ---- 1. leading block
    mid_assemble<D>(sh, st, 0, nullptr);
    if (tid < 128) {
        const double rhs = st.pm ? __dadd_rn(st.y[tid], -st.pm[tid]) : st.y[tid];       // r = y - m(X)
        sh.blk.S[tid][128] = rhs;
#pragma unroll
        for (int c = 129; c < kDiagLd; ++c) sh.blk.S[tid][c] = 0.0;
    }
    __syncthreads();
    diag128_factor_in_lds(sh.blk, U11, kSmallLd, 0, 128, inv1, info, nullptr, 8);
    mid_sync();
    if (CHECK && __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return false;

    // ---- 2. U12 = U11^-T K12, V11 = U11^-T I
    mid_factor_to_lds(sh, U11, inv1, iv);
    mid_sync();
    for (int ct = wave; ct < 16; ct += 4) {
        const bool ident = ct >= 8;
        const int c0 = 16 * (ct & 7);
        d4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + kq + 4 * r, gj = 128 + c0 + lc;
                if (ident) acc[t][r] = (row == c0 + lc) ? 1.0 : 0.0;
                else acc[t][r] = (gj < n) ? mid_kernel_value<D>(st, row, gj, inv_l2a) : 0.0;
            }
        double *dst = ident ? V + c0 + lc : U12 + c0 + lc;
        const int64_t ld = ident ? kMidLdV : kSmallLd;
        panel_solve_tiles(&sh.blk.S[kq][lc], acc, iv, 8, [&](int s2, const d4 &x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(int64_t)(16 * s2 + kq + 4 * r) * ld] = x[r];
        });
    }
    mid_sync();

    // ---- 3. trailing block: K22 - U12^T U12, r2 - U12^T z1
    mid_assemble<D>(sh, st, 1, U12);
    if (tid < 128) {
        double rhs = 0.0;
        if (tid < n2) {
            double dot = 0.0;
            for (int k = 0; k < 128; ++k) dot = fma(U12[(int64_t)k * kSmallLd + tid], U11[(int64_t)k * kSmallLd + 128], dot);
            const int g = 128 + tid;
            rhs = (st.pm ? __dadd_rn(st.y[g], -st.pm[g]) : st.y[g]) - dot;
        }
        sh.blk.S[tid][128] = rhs;
#pragma unroll
        for (int c = 129; c < kDiagLd; ++c) sh.blk.S[tid][c] = 0.0;
    }
    __syncthreads();
    diag128_factor_in_lds(sh.blk, U22, kSmallLd, 0, 128, inv2, info, nullptr, 8);
    mid_sync();
    if (CHECK && __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return false;

    // ---- 4. V21 = U22^-T (-U12^T V11), V22 = U22^-T I
    mid_factor_to_lds(sh, U22, inv2, iv);
    mid_sync();
    for (int ct = wave; ct < 16; ct += 4) {
        const bool ident = ct >= 8;
        const int c0 = 16 * (ct & 7);
        d4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (ident) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][r] = (16 * t + kq + 4 * r == c0 + lc) ? 1.0 : 0.0;
            } else {
                d4 w = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < 128; k0 += 4)
                    w = MFMA_F64(U12[(int64_t)(k0 + kq) * kSmallLd + 16 * t + lc], V[(int64_t)(k0 + kq) * kMidLdV + c0 + lc], w);
                acc[t] = -w;
            }
        }
        double *dst = V + (int64_t)128 * kMidLdV + (ident ? 128 : 0) + c0 + lc;
        panel_solve_tiles(&sh.blk.S[kq][lc], acc, iv, 8, [&](int s2, const d4 &x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(int64_t)(16 * s2 + kq + 4 * r) * kMidLdV] = x[r];
        });
    }
    mid_sync();

    // ---- 5. alpha = V^T z, tr(Ky^-1), then the gradient sums over the upper tile pairs
    double trw = 0.0;
    {
        const int j = tid;                                          // one column per thread
        double a = 0.0;
        if (j < n) {
            for (int i = j; i < n; ++i) {
                const double v = V[(int64_t)i * kMidLdV + j];
                const double zi = (i < 128) ? U11[(int64_t)i * kSmallLd + 128] : U22[(int64_t)(i - 128) * kSmallLd + 128];
                a = fma(v, zi, a);
                trw = fma(v, v, trw);
            }
        }
        alpha[j] = a;
    }
    mid_sync();
    const int tiles = (n + 15) / 16, rows = 16 * tiles;
    const double inv_l2 = st.ard ? 1.0 : inv_l2a;
    double sum[1 + D];
#pragma unroll
    for (int k = 0; k <= D; ++k) sum[k] = 0.0;
    int pair = 0;
    for (int ti = 0; ti < tiles; ++ti)
        for (int tj = ti; tj < tiles; ++tj, ++pair) {
            if ((pair & 3) != wave) continue;                       // uniform per wave
            d4 w = {0.0, 0.0, 0.0, 0.0}, w2 = {0.0, 0.0, 0.0, 0.0};
            const double *Va = V + 16 * ti + lc, *Vb = V + 16 * tj + lc;
            for (int k0 = 16 * tj; k0 < rows; k0 += 8) {
                w = MFMA_F64(Va[(int64_t)(k0 + kq) * kMidLdV], Vb[(int64_t)(k0 + kq) * kMidLdV], w);
                w2 = MFMA_F64(Va[(int64_t)(k0 + 4 + kq) * kMidLdV], Vb[(int64_t)(k0 + 4 + kq) * kMidLdV], w2);
            }
            w += w2;
            const int gj = 16 * tj + lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = 16 * ti + kq + 4 * r;
                if (gi >= n || gj >= n || gj < gi) continue;
                double r2 = 0.0, d2k[D];
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double df = st.xs[(int64_t)k * st.ld + gi] - st.xs[(int64_t)k * st.ld + gj];
                    d2k[k] = df * df * inv_l2;
                    r2 += d2k[k];
                }
                const double kv = st.variance * exp_nonpositive(-0.5 * r2);
                const double m = (gi == gj ? 1.0 : 2.0) * (alpha[gi] * alpha[gj] - w[r]);
                const double mk = m * kv;
                const double svv = st.sv ? st.sv[gi] * st.sv[gj] : 0.0;
                sum[0] += mk + m * svv;
#pragma unroll
                for (int k = 0; k < D; ++k) sum[1 + k] = fma(mk, d2k[k], sum[1 + k]);
            }
        }
    double terms[kSmallLmlTerms];
#pragma unroll
    for (int k = 0; k < kSmallLmlTerms; ++k) terms[k] = 0.0;
#pragma unroll
    for (int k = 0; k <= D; ++k) terms[k] = sum[k];
    if (tid < n) {
        const double *Ub = (tid < 128) ? U11 : U22;
        const int i = tid & 127;
        const double zi = Ub[(int64_t)i * kSmallLd + 128];
        terms[1 + CBO_MAX_DIM + 0] = zi * zi;
        terms[1 + CBO_MAX_DIM + 1] = log(Ub[(int64_t)i * kSmallLd + i]);
        terms[1 + CBO_MAX_DIM + 2] = alpha[tid] * alpha[tid];
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
    return true;
}

// The likelihood's sums of the model st (128 < n <= 256) at the hyper-parameter row `row` (variance, lengthscale x n_ls,
// noise variance; in LDS, the same doubles for every lane) from its RAW coordinates, inside one resident workgroup of 256
// threads: the counterpart of small_lml_sums_at.  Thread t prepares point t with the row's lengthscales (hyper_point: what
// prep_points_kernel leaves in the resident copies of a model set to that row) into the point region at the end of the
// run's slab; the descriptor is the sample's (hyper_sample_set) with its points there; stages 1-5 run on it.  Returns
// false -- to every thread alike, the info word still set: the caller clears it -- when one of the two blocks is not
// positive definite as assembled.  On true the four waves' partial sums are in red behind a barrier, and ONE thread forms
// the likelihood and its gradients from them with small_lml_outputs_at (lml_outputs_of, the host's arithmetic).
__device__ __forceinline__ bool mid_lml_sums_at(SmallShared &sh, double (*red)[kSmallLmlTerms], const cbo_small_set &st,
                                                const double *row, int n_ls, double *slab, int *info)
{
    const int tid = threadIdx.x;                                    // 0..255: one point each
    cbo_small_set sth = hyper_sample_set(st, row, n_ls);
    double *pxs = slab + kMidPointXs, *psq = slab + kMidPointSq, *psv = slab + kMidPointSv;
    {
        const bool in = tid < st.n;
        double x[CBO_MAX_DIM], sum;
        hyper_point(st.raw, tid, st.d, st.ard ? row + 1 : nullptr, in, x, sum);
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k)
            if (k < st.d) pxs[(int64_t)k * kMidPointLd + tid] = x[k];
        psq[tid] = sum;
        psv[tid] = (in && st.sv) ? sqrt(st.pv[tid]) : 0.0;
    }
    sth.xs = pxs; sth.sq = psq; sth.sv = st.sv ? psv : nullptr; sth.ld = kMidPointLd;
    mid_sync();                                                     // (the points: written by other waves)
    bool pd = false;
    CBO_FOR_DIM(st.d, pd = mid_lml_stages<D, true>(sh, red, sth, slab, info));
    return pd;
}

}  // namespace cbo

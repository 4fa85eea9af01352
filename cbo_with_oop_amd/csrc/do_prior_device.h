// The do-calculus prior of an RBF graph GP at one point, on the device: do_prior_at, shared by
// do_prior_eval_kernel (kernels_do_prior.hip: cbo_do_prior_eval) and small_sets_refine_kernel's causal instantiations
// (kernels_sets_refine.hip), which call it with the same lane group -- what cbo_do_prior_eval returns at a point is, bit
// for bit, what the refinement uses there.
//
// With the graph GP's inputs X_g (n rows), the intervened columns I and a handle's snapshot (w, M; cbo_do_prior_create):
//     a_i(x) = exp(-1/2 sum_{c in I} ((x_c - X_g[i,c]) / l_c)^2)
//     m(x)   = sum_i w_i a_i(x)                 v(x) = (sigma^2 + sigma_n^2) - a(x)^T M a(x)
// -- the mean over the observed rows of the graph GP's predictive mean and variance (src/DoCalculus.py:34-89) without the
// rows: O(n^2) per point.
#pragma once

#include "cbo_device.h"

namespace cbo {

// (m, v) at the point whose value columns are xv[0 .. n_iv), by the G lanes lid = 0 .. G-1 of one workgroup; every lane
// returns both.  a: n doubles of global scratch of the group; red: 2 G / 64 doubles of LDS.  Contains barriers: every
// thread of the workgroup calls it, with the same arguments.
// The order is fixed: lane l takes the rows r = l, l + G, ... in ascending order -- u_r = sum_j M[j][r] a_j over j
// ascending, then t += a_r u_r and s += w_r a_r -- the lanes of a wave meet in a butterfly, the waves in a tree.
template <int G>
__device__ __forceinline__ void do_prior_at(const DoPriorView &pv, const double (&xv)[CBO_MAX_DIM], double *a, double *red,
                                            int lid, double &mean, double &var)
{
#pragma clang fp contract(off)
    static_assert(G == 256, "the waves' tree below is written for four waves");
    constexpr int R = kDoPriorMaxN / G;
    const int n = pv.n;
    double xc[CBO_MAX_DIM];
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) {
        double v = xv[0];
#pragma unroll
        for (int q = 1; q < CBO_MAX_DIM; ++q) v = (pv.src[k] == q) ? xv[q] : v;
        xc[k] = (k < pv.n_col) ? (pv.ard ? v / pv.ls[k] : v) : 0.0;
    }
    for (int i = lid; i < n; i += G) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k)
            if (k < pv.n_col) {
                const double dk = xc[k] - pv.xi[(int64_t)k * pv.ldx + i];
                s = (k == 0) ? __dmul_rn(dk, dk) : __fma_rn(dk, dk, s);
            }
        a[i] = exp_nonpositive(__dmul_rn(-0.5, __dmul_rn(s, pv.inv_l2)));
    }
    __syncthreads();
    // rows beyond n are clamped onto the last row: computed, then left out of the sums
    int rc[R];
    double u[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int r = lid + G * q;
        rc[q] = r < n ? r : n - 1;
        u[q] = 0.0;
    }
    const int chunks = (n + G - 1) / G;                            // (uniform)
    // a_j reaches the lanes 64 at a time (one load per lane, then a lane read per j: no load of its own in the chain of
    // row loads, eight rows of M in flight per lane and chunk)
    const int lane = lid & 63;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const double av = a[(j0 + lane < n) ? j0 + lane : n - 1];
        const int jn = (n - j0 < 64) ? n - j0 : 64;
#pragma unroll 8
        for (int jj = 0; jj < jn; ++jj) {
            const double aj = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(av), jj),
                                               __builtin_amdgcn_readlane(__double2loint(av), jj));
            const double *row = pv.M + (int64_t)(j0 + jj) * pv.ldm;
#pragma unroll
            for (int q = 0; q < R; ++q)
                if (q < chunks) u[q] = __fma_rn(row[rc[q]], aj, u[q]);
        }
    }
    double t = 0.0, s = 0.0;
#pragma unroll
    for (int q = 0; q < R; ++q)
        if (q < chunks) {
            const double ar = (lid + G * q < n) ? a[rc[q]] : 0.0;
            t = __fma_rn(ar, u[q], t);
            s = __fma_rn(pv.w[rc[q]], ar, s);
        }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        t = __dadd_rn(t, __shfl_xor(t, off));
        s = __dadd_rn(s, __shfl_xor(s, off));
    }
    const int wave = lid >> 6;
    if ((lid & 63) == 0) { red[wave] = t; red[4 + wave] = s; }
    __syncthreads();
    t = __dadd_rn(__dadd_rn(red[0], red[1]), __dadd_rn(red[2], red[3]));
    s = __dadd_rn(__dadd_rn(red[4], red[5]), __dadd_rn(red[6], red[7]));
    mean = s;
    var = __dsub_rn(pv.vmax, t);
    __syncthreads();                                               // a and red are free for the next point
}

}  // namespace cbo

// Greedy batch selection (emukit GreedyBatchPointCalculator, the Kriging believer) for gfx950: one further pick of
// cbo_acq_sweep_batch as three launches over the RESIDENT solution V = L^-1 K* (DESIGN.md §4g).
//
// The believed observation is the model's own prediction at a candidate p, so
//   * its column of the factor is column p of V (no forward solve): l = V[:, p], l^T l = q_p, l^T z = mu_p;
//   * its residual is zero: the new entry of z is 0 and every posterior mean stays as it is.  Only q grows:
//       d   = sqrt(max(Kdiag_p - q_p, 1e-15) + noise + 1e-8)
//       c_j = k(x_p, x_j) - sum_{i<n} V_ip V_ij - sum_{s<t} W_sp W_sj,   W_tj = c_j / d,   q_j += W_tj^2
//     (W: the fantasy rows of earlier picks -- the rows V would have gained had the points been appended).
// The pivot is read from device memory (argmax_final_kernel's output of the previous pick): picks queue back to back.
//
//   batch_pivot_kernel    the pivot column into a contiguous n-vector, the pick's scalars into BatchState, the previous
//                         winner into the pinned host arrays
//   batch_partial_kernel  the pass over V: rows sliced over the grid, the slice of the pivot column in LDS, two candidate
//                         columns per lane (16-byte loads), eight rows in flight per lane; n x m x 8 bytes, the traffic
//   batch_final_kernel    slice sums in slice order, the W correction, k(x_p, .), the division, q and the new row of W
#include "cbo_device.h"

#pragma clang fp contract(off)

namespace cbo {

constexpr int kBatchRowsLds = 128;         // rows of the pivot column a workgroup of the pass holds at a time

// block 0 forms the pick's scalars; every block gathers its 256 rows of the pivot column
__global__ __launch_bounds__(256) void batch_pivot_kernel(BatchPivotArgs a)
{
    int64_t p = *a.best_idx - a.index_offset;
    if (p < 0 || p >= a.m) p = 0;                                    // (cannot happen: m >= 1 and an index always wins)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) a.col[i] = a.V[i * a.ldv + p];
    if (blockIdx.x != 0) return;
    BatchState *st = a.state;
    if ((int)threadIdx.x < a.t - 1) st->wp[threadIdx.x] = a.W[(int64_t)threadIdx.x * a.m_pad + p];
    if (threadIdx.x == 64) {
        a.h_vals[a.t - 1] = *a.best_val;
        a.h_idxs[a.t - 1] = *a.best_idx;
    }
    if (threadIdx.x == 65) {
        const bool causal = a.pv != nullptr;
        st->d = batch_believer_sd(a.variance, causal ? a.pv[p] : 0.0, causal, a.q[p], a.noise_var);
        for (int k = 0; k < CBO_MAX_DIM; ++k) st->x[k] = (k < a.dims) ? a.xs[(int64_t)k * a.ldx + p] : 0.0;
        st->sq = a.sq[p];
        st->sv = (causal && a.sv) ? a.sv[p] : 0.0;
        st->p = p;
        if (a.update_incumbent)
            st->y_best = batch_moved_incumbent(st->y_best, a.mu[p], causal ? a.pm[p] : 0.0, causal, a.task);
    }
}

// the last winner to the host arrays (the picks before it went with the next pick's pivot kernel)
__global__ void batch_record_kernel(const double *__restrict__ best_val, const int64_t *__restrict__ best_idx, int slot,
                                    double *__restrict__ h_vals, int64_t *__restrict__ h_idxs)
{
    if (threadIdx.x == 0) {
        h_vals[slot] = *best_val;
        h_idxs[slot] = *best_idx;
    }
}

__global__ void batch_state_init_kernel(BatchState *st, double y_best)
{
    if (threadIdx.x == 0) st->y_best = y_best;
}

// partial[r][j] = sum over the r-th slice of rows i < n of col_i V[i][j]: workgroup (x, r) takes the 512 columns from
// 512 x, lane l the pair 512 x + 2 l.  The rows of a slice are summed in order by ONE chain of FMAs per column (the
// result does not depend on the launch geometry beyond rows_per_slice); eight rows' loads are issued before the first is
// used.  V's leading dimension and m_pad are even and V is 16-byte aligned: every pair is one aligned 16-byte load.
__global__ __launch_bounds__(256) void batch_partial_kernel(const double *__restrict__ V, int64_t ldv, int64_t n,
                                                            int rows_per_slice, const double *__restrict__ col,
                                                            int64_t m_pad, double *__restrict__ partial)
{
    __shared__ double ls[kBatchRowsLds];
    const int64_t j = (int64_t)blockIdx.x * 512 + 2 * threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t i1 = (i0 + rows_per_slice < n) ? i0 + rows_per_slice : n;
    const bool in = j < m_pad;
    d2 s = {0.0, 0.0};
    for (int64_t base = i0; base < i1; base += kBatchRowsLds) {
        __syncthreads();
        if (threadIdx.x < kBatchRowsLds) ls[threadIdx.x] = (base + threadIdx.x < i1) ? col[base + threadIdx.x] : 0.0;
        __syncthreads();
        const int cnt = (int)((i1 - base < kBatchRowsLds) ? i1 - base : kBatchRowsLds);
        if (in) {
            const double *vp = V + base * ldv + j;
            int t = 0;
            for (; t + 8 <= cnt; t += 8) {
                d2 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const d2 *>(vp + (int64_t)(t + u) * ldv);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double l = ls[t + u];
                    s[0] = batch_pass_step(l, v[u][0], s[0]);
                    s[1] = batch_pass_step(l, v[u][1], s[1]);
                }
            }
            for (; t < cnt; ++t) {
                const d2 v = *reinterpret_cast<const d2 *>(vp + (int64_t)t * ldv);
                const double l = ls[t];
                s[0] = batch_pass_step(l, v[0], s[0]);
                s[1] = batch_pass_step(l, v[1], s[1]);
            }
        }
    }
    if (in) *reinterpret_cast<d2 *>(partial + (int64_t)blockIdx.y * m_pad + j) = s;
}

// one candidate per lane: the slice sums in slice order, then the fantasy rows' in pick order, kmat's element for
// (x_p, x_j), the new row of W and q
template <int D>
__global__ __launch_bounds__(256) void batch_final_kernel(BatchFinalArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m_pad) return;
    double *wrow = a.W + (int64_t)(a.t - 1) * a.m_pad;
    if (j >= a.m) { wrow[j] = 0.0; return; }
    const BatchState *st = a.state;
    double xp[D], xj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xp[k] = st->x[k];
        xj[k] = a.xs[(int64_t)k * a.ldx + j];
    }
    const double w = batch_fantasy_weight<D>(
        a.slices, [&](int r) { return a.partial[(int64_t)r * a.m_pad + j]; }, a.t - 1, st->wp,
        [&](int r) { return a.W[(int64_t)r * a.m_pad + j]; }, xp, xj, st->sq, a.sq[j], a.sv != nullptr, st->sv,
        a.sv ? a.sv[j] : 0.0, a.variance, a.inv_l2, st->d);
    wrow[j] = w;
    a.q[j] = batch_q_update(w, a.q[j]);
}

int batch_slices(int64_t n) { return batch_slice_count(n); }

void launch_batch_state_init(hipStream_t s, BatchState *st, double y_best)
{
    hipLaunchKernelGGL(batch_state_init_kernel, dim3(1), dim3(64), 0, s, st, y_best);
}

void launch_batch_record(hipStream_t s, const double *best_val, const int64_t *best_idx, int slot, double *h_vals,
                         int64_t *h_idxs)
{
    hipLaunchKernelGGL(batch_record_kernel, dim3(1), dim3(64), 0, s, best_val, best_idx, slot, h_vals, h_idxs);
}

void launch_batch_pick(hipStream_t s, const BatchPivotArgs &pa, BatchFinalArgs fa, double *col, double *partial)
{
    const int64_t n = pa.n;
    hipLaunchKernelGGL(batch_pivot_kernel, dim3((unsigned)(n > 0 ? (n + 255) / 256 : 1)), dim3(256), 0, s, pa);
    const int slices = batch_slices(n);
    const int rows_per_slice = batch_rows_per_slice(n, slices);
    if (n > 0)
        hipLaunchKernelGGL(batch_partial_kernel, dim3((unsigned)((pa.m_pad + 511) / 512), (unsigned)slices), dim3(256), 0, s,
                           pa.V, pa.ldv, n, rows_per_slice, col, pa.m_pad, partial);
    fa.slices = n > 0 ? slices : 0;
    fa.partial = partial;
    const dim3 grid((unsigned)((pa.m_pad + 255) / 256));
    CBO_FOR_DIM(pa.dims, hipLaunchKernelGGL(batch_final_kernel<D>, grid, dim3(256), 0, s, fa));
}

}  // namespace cbo

// Gradient refinement of every set's constrained acquisition in one launch for gfx950:
// small_sets_refine_con_kernel<LOG, BYVAL>, small_sets_refine_kernel's sibling (kernels_sets_refine.hip) for
//     EI(x) prod_k PoF_k(x) / c(x)                       (LOG = false; constrained.py's AcquisitionProduct / Cost)
//     log EI(x) + sum_k log PoF_k(x) - log c(x)          (LOG = true;  ConstrainedLogExpectedImprovement / Cost)
// The sibling's conventions hold: grid (workgroups per set, sets), 256 threads, SmallShared in dynamic LDS, a start owns
// 1 + d of a wave's 16 columns (column 0 is k*(x), column j its derivative by x_j), one owner lane per start runs the
// start's state machine (refine_search.h, unchanged).
//
// A set is 1 + n_con consecutive descriptors, the objective first -- kernels_sets_con.hip's convention: first(s) rides in
// descriptor s's pad_ word, a constraint's value, jitter and sense ride in its descriptor's y_best, ei_jitter and task.
// The descriptors carry no candidates.  Each descriptor has a record of its model's per-dimension lengthscales beside it
// (cbo_small_refine_pair): every model scales the moving point itself.
//
// Several models, one LDS block.  The prologue factors every model of the set once (small_model_factor, phases = 1) into
// a slot of its own in the workgroup's global scratch; every round walks the models in order and reloads each -- points,
// factor, inverses and z (phases = 2) -- behind a barrier, forms the model's columns at the trial point in the model's own
// scaling, solves, and the owner lane folds the model's term into two running registers, the value and the gradient.
//
// The curvature rings live in the workgroup's global scratch behind its model slots (32 starts x 2 rings x 64 doubles),
// not in the LDS block's lower-left quadrant where the sibling keeps them: the reload writes whole 128-column rows of every
// factored tile and would overwrite that quadrant as soon as a model has more than 64 observations.
//
// Terms.  The values are the sweeps' own device functions (acquisition_of at cost 1, feasibility_of, the IEEE division by
// c(x); log_ei_of at log cost 0, log_feasibility_of, the subtraction of log c(x)): what small_sets_con_kernel returns for a
// one-point grid at x with cost c(x), to the bit.  The gradient is the host classes': the product rule left to right,
// g <- g pof + run dpof with dpof = -phi(u) (d mean + u d sd) / sd, then divided by c(x) (the reference's zero cost
// gradient, §4q); or d logEI + sum_k rho(u_k) du_k, not divided (§4x's rule), rho = phi / Phi from log_ndtr_and_ratio.
#include <cstring>

#include "cbo_small_device.h"
#include "refine_search.h"

#pragma clang fp contract(off)

namespace cbo {

// the lengthscale records of up to kSmallByValue descriptors travel as kernel arguments beside them (SmallSetArgs)
struct SmallRefinePairArgs { cbo_small_refine_pair p[kSmallByValue]; };
static_assert(sizeof(SmallSetArgs) + sizeof(SmallRefinePairArgs) + 256 <= 4096, "the kernel's arguments: one 4 KB segment");

static_assert(sizeof(SmallShared) + 256 <= 163840, "SmallShared and what the resource report shows beside it: one CU");
static_assert(kRefineHistory * CBO_MAX_DIM <= kRefineConRing, "one ring: kRefineHistory pairs of at most CBO_MAX_DIM doubles");

// One model's term and the coefficients of its differential, d term = a d mean + b d sd (d sd = d var / (2 sd)).
// Functions of their own, NOT inlined, for the reason log_ei_value_and_coefficients (kernels_sets_refine.hip) is not: only
// the owner lane calls them, once per model and round, and the kernel sits at 256 VGPRs.
struct ConTerm {
    double value, s, a, b;
};

// the objective: acquisition_of at cost 1 with CausalExpectedImprovement's coefficients, or log_ei_of at log cost 0 with
// CausalLogExpectedImprovement's (log_h_of<true>: the value is log_h_of<false>'s, operation for operation)
template <bool LOG>
__device__ __attribute__((noinline)) ConTerm objective_term(double mean, double var, double y_best, double jitter, int task)
{
    AcqParams p{};
    p.y_best = y_best; p.ei_jitter = jitter; p.task = task; p.cost = 1.0;
    if constexpr (LOG) {
        double s, A, B;
        const double u = log_ei_u(mean, var, p, s);
        const double log_h = log_h_of<true>(u, A, B);
        return ConTerm{(log_h + log(s)) - 0.0, s, ((task == CBO_TASK_MIN) ? -A : A) / s, B / s};
    } else {
        double s, rs;
        bool special;
        sqrt_and_reciprocal(var, s, rs, special);
        const double sign = (task == CBO_TASK_MIN) ? 1.0 : -1.0;
        const double u = (y_best - (mean + jitter)) / s;
        const double e = exp_nonpositive(-(u * u) / 2.0);
        const double pdf = e * 0.3989422804014327;
        const double cdf = ndtr_with_exp(u, e);
        return ConTerm{acquisition_of(mean, var, p), s, sign * -cdf, sign * pdf};
    }
}

// a constraint: feasibility_of with ProbabilityOfFeasibility's coefficients, or log_feasibility_of with rho(u) du
template <bool LOG>
__device__ __attribute__((noinline)) ConTerm constraint_term(double mean, double var, double value, double jitter, int sense)
{
    const double flip = (sense == CBO_CON_LE) ? 1.0 : -1.0;
    if constexpr (LOG) {
        double s, u, rho;
        const double l = log_feasibility_of(mean, var, value, jitter, sense, s, u, rho);
        // du = -flip (d mean + u_le d sd) / sd with u_le = flip u
        return ConTerm{l, s, -(flip * rho) / s, -(rho * u) / s};
    } else {
        double s, rs;
        bool special;
        sqrt_and_reciprocal(var, s, rs, special);
        const double u = (value - (mean + jitter)) / s;
        const double pdf = exp_nonpositive(-(u * u) / 2.0) * 0.3989422804014327;
        return ConTerm{feasibility_of(mean, var, value, jitter, sense), s, flip * (-pdf / s), flip * (-pdf * u / s)};
    }
}

template <bool LOG, bool BYVAL>
__global__ __launch_bounds__(256) void small_sets_refine_con_kernel(
    const SmallSetArgs byval, const SmallRefinePairArgs byval_ls, const cbo_small_set *__restrict__ pairs,
    const cbo_small_refine_pair *__restrict__ pair_ls, int n_pairs, const cbo_small_refine *__restrict__ refs,
    const double *__restrict__ starts, double *scratch, int blocks_per_set, int slots, int *__restrict__ info, int max_rounds,
    double *__restrict__ x_out, double *__restrict__ val_out, double *__restrict__ grad_out, int *__restrict__ rounds_out,
    int *__restrict__ status_out)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int set = blockIdx.y, blk = blockIdx.x;
    const int p0 = BYVAL ? byval.s[set].pad_ : pairs[set].pad_;
    const int p1 = (set + 1 < (int)gridDim.y) ? (BYVAL ? byval.s[set + 1].pad_ : pairs[set + 1].pad_) : n_pairs;
    const cbo_small_refine rf = refs[set];                        // (by value: read across the host link once)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int d = (BYVAL ? byval.s[p0].d : pairs[p0].d), cols = 1 + d;      // (every model of the set has the set's d)
    const int per_wave = 16 / cols, per_block = 4 * per_wave;
    const int k_starts = rf.k;
    if (blk * per_block >= k_starts) return;                      // no start left for this workgroup
    if (p1 - p0 > slots) return;                                  // (the host sized the scratch for `slots` models a set)
    // the workgroup's scratch: `slots` model slots, then the rings of its starts
    double *my = scratch + (int64_t)(set * blocks_per_set + blk) * ((int64_t)slots * kSmallScratch + kRefineConRings);
    double *rings = my + (int64_t)slots * kSmallScratch;

    // this lane's column: start `si` of the wave, role j (0: k*, j >= 1: d k* / d x_(j-1)) -- the sibling's layout
    const int si = lc / cols, j = lc - si * cols;
    const bool valid = si < per_wave;
    const int slot = wave * per_wave + (valid ? si : 0);          // the start's place in the workgroup (its rings)
    const int start = blk * per_block + slot;
    const bool live = valid && start < k_starts;
    const bool owner = live && kq == 0 && j == 0;                 // the one lane that runs the start's search
    const int base = (valid ? si : 0) * cols;                     // lane (and column) of the start's k*
    const int sc = live ? start : k_starts - 1;                   // clamped: the other lanes compute, nobody looks

    double lo[CBO_MAX_DIM], hi[CBO_MAX_DIM], x0[CBO_MAX_DIM];
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) {
        lo[k] = (k < d) ? rf.lo[k] : 0.0;
        hi[k] = (k < d) ? rf.hi[k] : 0.0;
        x0[k] = (k < d) ? starts[rf.row_off + (int64_t)sc * d + k] : 0.0;
    }

    // ---- prologue: every model of the set factored once, each into its own slot
    for (int p = p0; p < p1; ++p) {                               // (uniform)
        const cbo_small_set st = BYVAL ? byval.s[p] : pairs[p];
        small_factor_only(sh, st, my + (int64_t)(p - p0) * kSmallScratch, &info[set]);
        // (ends with every wave's stores complete and a barrier: the next model assembles over this one)
    }
    // a model that is not positive definite as assembled is jitchol's business: the set is declined
    if (__hip_atomic_load(&info[set], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (owner) status_out[rf.out_off + start] = CBO_REFINE_DECLINED;
        return;
    }

    RefineState rs;
    refine_begin(rs, d, x0, lo, hi, rings + (int64_t)(2 * slot) * kRefineConRing, rings + (int64_t)(2 * slot + 1) * kRefineConRing);
    double xt[CBO_MAX_DIM];
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) xt[k] = rs.xt[k];       // (every lane of the start holds the same start)
    const int jm = (j > 0 && j <= d) ? j - 1 : 0;

    for (int it = 0; it <= max_rounds; ++it) {                    // the start's own evaluation, then at most max_rounds rounds
        double run = 0.0, grad[CBO_MAX_DIM];                      // EI, EI pof_0, ... (LOG: logEI, logEI + l_0, ...) and its gradient
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k) grad[k] = 0.0;
        for (int p = p0; p < p1; ++p) {                           // (uniform)
            // the previous model's solve has read the factor, the points and sq in LDS: nobody reloads over them before
            // every wave is through (the round's first model follows the prologue's or the previous round's barrier)
            if (p != p0) __syncthreads();
            const cbo_small_set st = BYVAL ? byval.s[p] : pairs[p];
            const int tiles = (st.n + 15) / 16;
            double *Us = my + (int64_t)(p - p0) * kSmallScratch;
            double iv[8][4], zr[8][4];
            small_model_factor(sh, st, tiles, Us, Us + 128 * kSmallLd, &info[set], iv, zr, 2, true);

            // ---- the moving point as a candidate of THIS model: prep_points_kernel's arithmetic in the model's own scaling
            const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
            double xc[CBO_MAX_DIM], scale_j = 1.0;
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k) {
                const double ls_k = (k < d && st.ard) ? (BYVAL ? byval_ls.p[p].ls[k] : pair_ls[p].ls[k]) : 1.0;
                xc[k] = (k < d) ? (st.ard ? xt[k] / ls_k : xt[k]) : 0.0;
                scale_j = (k == jm) ? ls_k : scale_j;
            }
            const double csq = squared_norm(xc, d);
            double xcj = xc[0];
#pragma unroll
            for (int k = 1; k < CBO_MAX_DIM; ++k) xcj = (k == jm) ? xc[k] : xcj;
            // d r^2-term / d x_j: in scaled coordinates (ARD) one factor 1 / l_j is left, in raw ones 1 / l^2
            const double wj = st.ard ? 1.0 / scale_j : inv_l2;

            // ---- K* and its derivative columns, straight into the MFMA result layout
            d4 acc[8];
            small_kstar_tiles_of(sh, st, tiles, xc, csq, 0.0, inv_l2, kq, acc);
            if (j > 0) {
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * t + kq + 4 * r;
                        acc[t][r] = acc[t][r] * (-(xcj - sh.xs[jm][row]) * wj);
                    }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the factor is in LDS
            __syncthreads();

            // ---- V = L^-1 [k*, dk*]: q and mu per column, and each column's product with the start's column 0
            double qacc, macc, cacc = 0.0;
            solve_q_mu_keep(sh, acc, iv, zr, tiles, kq, lc, qacc, macc, [&](int, const d4 &x) {
#pragma unroll
                for (int r = 0; r < 4; ++r) cacc = fma(__shfl(x[r], (lane & 48) | base), x[r], cacc);
            });
            cacc += __shfl_xor(cacc, 16);
            cacc += __shfl_xor(cacc, 32);
            double dmean[CBO_MAX_DIM], dvar[CBO_MAX_DIM];
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k) {
                const int src = (base + 1 + k) & 15;
                const double m_k = __shfl(macc, src), c_k = __shfl(cacc, src);
                dmean[k] = (k < d) ? m_k : 0.0;
                dvar[k] = (k < d) ? -2.0 * c_k : 0.0;
            }

            // ---- the start's lane: the model's posterior and term, folded into the running value and gradient
            if (owner) {
                AcqParams ap = small_acq_params(st);
                double mean, var;
                posterior_of(qacc, macc, 0.0, 0.0, false, ap, mean, var);
                const ConTerm t = (p == p0) ? objective_term<LOG>(mean, var, st.y_best, st.ei_jitter, st.task)
                                            : constraint_term<LOG>(mean, var, st.y_best, st.ei_jitter, st.task);
#pragma unroll
                for (int k = 0; k < CBO_MAX_DIM; ++k) {
                    const double dt = t.a * dmean[k] + t.b * (dvar[k] / (2.0 * t.s));
                    if (p == p0) grad[k] = dt;
                    else if (LOG) grad[k] = grad[k] + dt;
                    else grad[k] = grad[k] * t.value + run * dt;  // (the host class's order: df g + f dg)
                }
                if (p == p0) run = t.value;
                else if (LOG) run = run + t.value;
                else run = run * t.value;
            }
        }

        // ---- the point's cost closes the value (and the product form's gradient); one step of the search
        if (owner) {
            double cost = 0.0;
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k)
                if (k < d) cost = cost + (rf.variable[k] ? rf.fix[k] + fabs(xt[k]) : rf.fix[k]);
            if (LOG) {
                run = run - log(cost);
            } else {
                run = run / cost;                                 // IEEE division (emukit's Quotient is numpy's)
#pragma unroll
                for (int k = 0; k < CBO_MAX_DIM; ++k) grad[k] = grad[k] / cost;
            }
            refine_feed(rs, lo, hi, run, grad, max_rounds);
        }
        // the next trial point to every lane of the start's columns; the workgroup goes on while one of its searches does
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k) xt[k] = __shfl(rs.xt[k], base);
        if (!__syncthreads_or(owner && !refine_done(rs))) break;
    }

    if (owner) {
        const int64_t row = rf.row_off + (int64_t)start * d;
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k)
            if (k < d) {
                x_out[row + k] = rs.x[k];
                grad_out[row + k] = -rs.g[k];
            }
        val_out[rf.out_off + start] = -rs.f;
        rounds_out[rf.out_off + start] = rs.rounds;
        status_out[rf.out_off + start] = rs.status;
    }
}

template <bool LOG, bool BYVAL>
static void launch_refine_con_as(hipStream_t s, const SmallSetArgs &args, const SmallRefinePairArgs &ls_args,
                                 const cbo_small_set *pairs, const cbo_small_refine_pair *pair_ls, int n_pairs,
                                 const cbo_small_refine *refs, const double *starts, int n_sets, int blocks_per_set, int slots,
                                 double *scratch, int *info, int max_rounds, double *x_out, double *val_out, double *grad_out,
                                 int *rounds_out, int *status_out)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(small_sets_refine_con_kernel<LOG, BYVAL>), opted);
    hipLaunchKernelGGL((small_sets_refine_con_kernel<LOG, BYVAL>), dim3((unsigned)blocks_per_set, (unsigned)n_sets), dim3(256),
                       sizeof(SmallShared), s, args, ls_args, pairs, pair_ls, n_pairs, refs, starts, scratch, blocks_per_set,
                       slots, info, max_rounds, x_out, val_out, grad_out, rounds_out, status_out);
}

size_t small_refine_con_scratch_doubles(int n_sets, int blocks_per_set, int slots)
{
    return (size_t)n_sets * (size_t)blocks_per_set * ((size_t)slots * kSmallScratch + kRefineConRings);
}

void launch_small_sets_refine_con(hipStream_t s, bool log_form, const cbo_small_set *pairs, const cbo_small_refine_pair *pair_ls,
                                  int n_pairs, const cbo_small_refine *refs, const double *starts, int n_sets,
                                  int blocks_per_set, int slots, double *scratch, int *info, int max_rounds, double *x_out,
                                  double *val_out, double *grad_out, int *rounds_out, int *status_out)
{
    SmallSetArgs args{};
    SmallRefinePairArgs ls_args{};
    const bool byval = n_pairs <= kSmallByValue;
    if (byval) {
        std::memcpy(args.s, pairs, sizeof(cbo_small_set) * (size_t)n_pairs);
        std::memcpy(ls_args.p, pair_ls, sizeof(cbo_small_refine_pair) * (size_t)n_pairs);
    }
    auto launch = byval ? (log_form ? launch_refine_con_as<true, true> : launch_refine_con_as<false, true>)
                        : (log_form ? launch_refine_con_as<true, false> : launch_refine_con_as<false, false>);
    launch(s, args, ls_args, pairs, pair_ls, n_pairs, refs, starts, n_sets, blocks_per_set, slots, scratch, info, max_rounds,
           x_out, val_out, grad_out, rounds_out, status_out);
}

}  // namespace cbo

// Gradient refinement of every exploration set's starts in one launch for gfx950: small_sets_refine_kernel<KIND>,
// the second stage of the reference's acquisition optimiser (src/utils_functions/causal_optimizer.py:59-65: L-BFGS from the
// best anchor inside the set's box).  A workgroup factors its set's model inside LDS with the stages of cbo_small_device.h,
// exactly as small_sets_kernel does, and then keeps the factor there for a whole search: every round it evaluates the
// acquisition and its gradient at the current trial point of each of its starts and hands the pair to the start's state
// machine (refine_search.h: lockstep_lbfgs for one start), which answers with the next trial point.
//
// Columns.  A start takes 1 + d of a wave's 16 right-hand sides: column 0 is k*(x), column j the derivative of k* by x_j,
// -k_i (x_j - X_ij) / l_j^2 row by row (no further exponential).  All of them go through the tile solve together; with
// V = L^-1 [k*, dk*]:  q = V_0.V_0 and mu = V_0.z as a sweep forms them, d mu / d x_j = V_j.z (the column's own mu) and
// d var / d x_j = -2 V_0.V_j -- GPy's predictive_gradients.  A wave carries floor(16 / (1 + d)) starts, a workgroup four
// times that; a set with more starts takes more workgroups (grid.x), none of which waits for another.
//
// Column 0 is a candidate's arithmetic to the bit (prep_points_kernel's scaling and |x|^2, small_kstar, the tile solve,
// posterior_of, acquisition_of / pointwise_of<KIND>): the value reported at a point is what the multi-set sweep returns for
// a one-point grid there.
//
// Causal sets (PRIOR).  A set whose model is a CausalRBF GP carries a do-calculus prior (DoPriorView): every
// round, before the columns are formed, the whole workgroup evaluates (m, v) at the trial point of each of its running
// starts with do_prior_at, one start after another (the owners pass their points and take the pair back through the
// workgroup's global scratch, whose factor rows are free once the factor is in LDS).  Column 0 is then the causal k* with
// sqrt(v) -- prep_points_kernel's sv of a candidate --, the derivative columns stay the stationary part's (GPy's
// predictive_gradients differentiates nothing else), posterior_of takes (m, v), and d var / d x_j = -2 V_0.V_j holds with the
// causal V_0.  The plug-in incumbent uses the model's stored priors at its own inputs, as the sweep does.  PRIOR is a
// template flag: the instantiations without it are the kernels they were.
#include <cstring>

#include "cbo_small_device.h"
#include "do_prior_device.h"
#include "refine_search.h"

#pragma clang fp contract(off)

namespace cbo {

static_assert(sizeof(SmallShared) + 128 * sizeof(double) + 4 * sizeof(double) + 4 * sizeof(int) + sizeof(double) +
                      2 * (kDoPriorGroup / 64) * sizeof(double) + 256 <= 163840,
              "the workgroup's static LDS (plug-in means and their reduction, the prior's reduction, and the 256 bytes the "
              "resource report shows for every kind beside them) beside SmallShared: one CU");
// The curvature rings of a workgroup's searches live in the block's lower-left quadrant (rows 64..127, columns 0..63): the
// factor is upper triangular and the tile solve reads nothing below the diagonal tiles.  One row = one ring.
static_assert(2 * 4 * (16 / 2) <= 64 && kRefineHistory * CBO_MAX_DIM <= 64, "one ring per row of the lower-left quadrant");

// The acquisition over the cost and the two coefficients of its gradient, d value = (a d mean + b d sd) / cost, from
// (mean, var) as the host classes form them (CausalExpectedImprovement.evaluate_with_gradients; pointwise_acquisitions.py).
// The value is the sweep's own (acquisition_of / pointwise_of<KIND> / log_ei_of); the coefficients repeat its intermediate steps.
// kLogEiKind: the value is log EI - log cost and (a, b) are the coefficients of d logEI itself -- not over the cost.
// kEiPointKind / kLogEiPointKind: kEiKind's and kLogEiKind's values and coefficients -- the first at cost 1:
// the caller divides by the point's cost itself, as the sweeps of these kinds do -- and the caller adds the cost's own
// derivative, d c / d x_k = variable_k sign(x_k), to the gradient.

// log EI - log cost, s, and the coefficients of d logEI = (-A d mean + B d sd) / s, d mean's sign flipped for 'max'
// (log_h_of<true>).  The value is log_ei_of's, operation for operation.
// A function of its own, NOT inlined: only the one lane that runs a start's search calls it, once per round.  Inlined, its
// three ranges (the device library's log / log1p / expm1 / exp among them) cost the kernel -- which sits at 256 VGPRs --
// 50 spilled VGPRs and 164 bytes of scratch per lane; as a call it costs none (256 VGPRs, 239 AGPRs, no scratch: the figures
// of the LCB and VAR instantiations).
struct LogEiTerms {
    double value, s, a, b;
};
__device__ __attribute__((noinline)) LogEiTerms log_ei_value_and_coefficients(double mean, double var, double y_best,
                                                                              double jitter, int task, double cost)
{
    AcqParams p{};
    p.y_best = y_best; p.ei_jitter = jitter; p.task = task; p.cost = cost;
    double s, A, B;
    const double u = log_ei_u(mean, var, p, s);
    const double log_h = log_h_of<true>(u, A, B);
    return LogEiTerms{(log_h + log(s)) - log(cost), s, ((task == CBO_TASK_MIN) ? -A : A) / s, B / s};
}

template <int KIND>
__device__ __forceinline__ double value_and_coefficients(double mean, double var, const AcqParams &p, double &s, double &a,
                                                         double &b)
{
    double rs;
    bool special;
    sqrt_and_reciprocal(var, s, rs, special);
    const double sign = (p.task == CBO_TASK_MIN) ? 1.0 : -1.0;
    if constexpr (KIND == kEiKind || KIND == CBO_ACQ_MPEI || KIND == CBO_ACQ_PI || KIND == kEiPointKind) {
        const double u = (p.y_best - (mean + p.ei_jitter)) / s;
        const double e = exp_nonpositive(-(u * u) / 2.0);
        const double pdf = e * 0.3989422804014327;
        if constexpr (KIND == CBO_ACQ_PI) {
            a = sign * (-pdf / s);
            b = sign * (-pdf * u / s);
            return pointwise_of<CBO_ACQ_PI>(mean, var, p);
        } else {
            const double cdf = ndtr_with_exp(u, e);
            a = sign * -cdf;
            b = sign * pdf;
            return acquisition_of(mean, var, p);
        }
    } else if constexpr (KIND == kLogEiKind || KIND == kLogEiPointKind) {
        // (the caller does NOT divide this kind by the cost: the cost's gradient is the reference's zero)
        const LogEiTerms t = log_ei_value_and_coefficients(mean, var, p.y_best, p.ei_jitter, p.task, p.cost);
        s = t.s;
        a = t.a;
        b = t.b;
        return t.value;
    } else if constexpr (KIND == CBO_ACQ_LCB) {
        a = -sign;
        b = p.ei_jitter;
        return pointwise_of<CBO_ACQ_LCB>(mean, var, p);
    } else {
        a = 0.0;
        b = 2.0 * s;
        return pointwise_of<CBO_ACQ_VAR>(mean, var, p);
    }
}

// the exchange area of the causal instantiations in the workgroup's scratch: a(x), then per start of the workgroup
// [x (CBO_MAX_DIM) | running | m | v]
constexpr int kPriorSlot = 16;
static_assert(kDoPriorMaxN + 32 * kPriorSlot <= 128 * kSmallLd, "a(x) and the starts' slots fit the scratch factor rows");

template <int KIND, bool BYVAL, bool PRIOR>
__global__ __launch_bounds__(256) void small_sets_refine_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
                                                                const cbo_small_refine *__restrict__ refs,
                                                                const double *__restrict__ starts, double *scratch,
                                                                int blocks_per_set, int *__restrict__ info, int max_rounds,
                                                                double *__restrict__ x_out, double *__restrict__ val_out,
                                                                double *__restrict__ grad_out, int *__restrict__ rounds_out,
                                                                int *__restrict__ status_out)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int set = blockIdx.y, blk = blockIdx.x;
    const cbo_small_set st = BYVAL ? byval.s[set] : sets[set];
    const cbo_small_refine rf = refs[set];                        // (by value: read across the host link once)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int d = st.d, cols = 1 + d;
    const int per_wave = 16 / cols, per_block = 4 * per_wave;
    const int k_starts = rf.k;
    if (blk * per_block >= k_starts) return;                      // no start left for this workgroup
    const int tiles = (st.n + 15) / 16;
    double *my = scratch + (int64_t)(set * blocks_per_set + blk) * kSmallScratch;

    // this lane's column: start `si` of the wave, role j (0: k*, j >= 1: d k* / d x_(j-1))
    const int si = lc / cols, j = lc - si * cols;
    const bool valid = si < per_wave;
    // (the columns beyond the wave's last whole start -- !valid -- take start 0's slot, and with it its ring pointers: they
    // compute along and never call refine_feed, the only writer of a ring, so the alias is never written through)
    const int slot = wave * per_wave + (valid ? si : 0);          // the start's place in the workgroup (its rings)
    const int start = blk * per_block + slot;
    const bool live = valid && start < k_starts;
    const bool owner = live && kq == 0 && j == 0;                 // the one lane that runs the start's search
    const int base = (valid ? si : 0) * cols;                     // lane (and column) of the start's k*
    const int sc = live ? start : k_starts - 1;                   // clamped: the other lanes compute, nobody looks

    double lo[CBO_MAX_DIM], hi[CBO_MAX_DIM], x0[CBO_MAX_DIM], scale[CBO_MAX_DIM];
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) {
        lo[k] = (k < d) ? rf.lo[k] : 0.0;
        hi[k] = (k < d) ? rf.hi[k] : 0.0;
        x0[k] = (k < d) ? starts[rf.row_off + (int64_t)sc * d + k] : 0.0;
        scale[k] = (k < d && rf.ard) ? rf.ls[k] : 1.0;
    }

    double iv[8][4], zr[8][4];
    small_model_factor(sh, st, tiles, my, my + 128 * kSmallLd, &info[set], iv, zr, 3, true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // a model that is not positive definite as assembled is jitchol's business: the set is declined
    if (__hip_atomic_load(&info[set], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (owner) status_out[rf.out_off + start] = CBO_REFINE_DECLINED;
        return;
    }

    AcqParams p = small_acq_params(st);
    if constexpr (KIND == CBO_ACQ_MPEI) {
        __shared__ double plug_mean[128], plug_red[4], plug_out;
        __shared__ int plug_nan[4];
        p.y_best = small_plugin_incumbent(sh, st, tiles, iv, zr, p, false, plug_mean, plug_red, plug_nan, &plug_out);
    }

    RefineState rs;
    refine_begin(rs, d, x0, lo, hi, &sh.blk.S[64 + 2 * slot][0], &sh.blk.S[64 + 2 * slot + 1][0]);
    double xt[CBO_MAX_DIM];
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) xt[k] = rs.xt[k];       // (every lane of the start holds the same start)

    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    const int jm = (j > 0 && j <= d) ? j - 1 : 0;
    // d r^2-term / d x_j: the kernel's exponent is -1/2 sum ((x_k - X_ik) / l_k)^2 -- in scaled coordinates (ARD) one factor
    // 1 / l_j is left, in raw ones (one lengthscale) 1 / l^2
    double scale_j = scale[0];
#pragma unroll
    for (int k = 1; k < CBO_MAX_DIM; ++k) scale_j = (k == jm) ? scale[k] : scale_j;
    const double wj = rf.ard ? 1.0 / scale_j : inv_l2;

    [[maybe_unused]] __shared__ double prior_red[2 * kDoPriorGroup / 64];
    for (int it = 0; it <= max_rounds; ++it) {                    // the start's own evaluation, then at most max_rounds rounds
        // ---- a causal set: (m, v) at the trial point of every running start, the whole workgroup per start
        double pm_c = 0.0, pv_c = 0.0;
        if constexpr (PRIOR) {
            double *pa = my, *px = my + kDoPriorMaxN;
            if (owner) {
#pragma unroll
                for (int k = 0; k < CBO_MAX_DIM; ++k) px[slot * kPriorSlot + k] = xt[k];
                px[slot * kPriorSlot + CBO_MAX_DIM] = refine_done(rs) ? 0.0 : 1.0;
            }
            __syncthreads();
            const int here = (k_starts - blk * per_block < per_block) ? k_starts - blk * per_block : per_block;
            const DoPriorView pview = *rf.prior;
            for (int s = 0; s < here; ++s) {                      // (uniform, as is the flag: every thread reads one word)
                if (px[s * kPriorSlot + CBO_MAX_DIM] == 0.0) continue;
                double xv[CBO_MAX_DIM];
#pragma unroll
                for (int k = 0; k < CBO_MAX_DIM; ++k) xv[k] = (k < d) ? px[s * kPriorSlot + k] : 0.0;
                double m_s, v_s;
                do_prior_at<kDoPriorGroup>(pview, xv, pa, prior_red, tid, m_s, v_s);
                if (tid == 0) {
                    px[s * kPriorSlot + CBO_MAX_DIM + 1] = m_s;
                    px[s * kPriorSlot + CBO_MAX_DIM + 2] = v_s;
                }
            }
            __syncthreads();
            pm_c = px[slot * kPriorSlot + CBO_MAX_DIM + 1];
            pv_c = px[slot * kPriorSlot + CBO_MAX_DIM + 2];
        }
        // ---- the moving point as a candidate: prep_points_kernel's arithmetic
        double xc[CBO_MAX_DIM];
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k) xc[k] = (k < d) ? (rf.ard ? xt[k] / scale[k] : xt[k]) : 0.0;
        const double csq = squared_norm(xc, d);
        double xcj = xc[0];
#pragma unroll
        for (int k = 1; k < CBO_MAX_DIM; ++k) xcj = (k == jm) ? xc[k] : xcj;

        // ---- K* and its derivative columns, straight into the MFMA result layout
        d4 acc[8];
        small_kstar_tiles_of(sh, st, tiles, xc, csq, (PRIOR && j == 0) ? sqrt(pv_c) : 0.0, inv_l2, kq, acc);
        if (j > 0) {
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + kq + 4 * r;
                    acc[t][r] = acc[t][r] * (-(xcj - sh.xs[jm][row]) * wj);
                }
        }

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

        // ---- the start's lane: posterior, acquisition over the point's cost, gradient, one step of the search
        if (owner) {
            double mean, var;
            posterior_of(qacc, macc, pm_c, pv_c, PRIOR, p, mean, var);
            double cost = 0.0;
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k)
                if (k < d) cost = cost + (rf.variable[k] ? rf.fix[k] + fabs(xt[k]) : rf.fix[k]);
            p.cost = (KIND == kEiPointKind) ? 1.0 : cost;
            double s, a, b;
            double value = value_and_coefficients<KIND>(mean, var, p, s, a, b);
            if constexpr (KIND == kEiPointKind) value = value / cost;      // (the sweep's: EI at cost 1, the IEEE quotient)
            double grad[CBO_MAX_DIM];
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k) {
                grad[k] = a * dmean[k] + b * (dvar[k] / (2.0 * s));
                if constexpr (KIND == kEiPointKind || KIND == kLogEiPointKind) {
                    // the quotient rule with the cost's own derivative, sign(0) = 0
                    const double dc = (k < d && rf.variable[k]) ? (xt[k] > 0.0 ? 1.0 : (xt[k] < 0.0 ? -1.0 : 0.0)) : 0.0;
                    if constexpr (KIND == kEiPointKind) grad[k] = (grad[k] - value * dc) / cost;
                    else grad[k] = grad[k] - dc / cost;
                } else if constexpr (KIND != kLogEiKind) {
                    grad[k] = grad[k] / cost;
                }
            }
            refine_feed(rs, lo, hi, value, grad, max_rounds);
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

template <int KIND, bool BYVAL, bool PRIOR>
static void launch_refine_as(hipStream_t s, const SmallSetArgs &args, const cbo_small_set *sets, const cbo_small_refine *refs,
                             const double *starts, int n_sets, int blocks_per_set, double *scratch, int *info, int max_rounds,
                             double *x_out, double *val_out, double *grad_out, int *rounds_out, int *status_out)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(small_sets_refine_kernel<KIND, BYVAL, PRIOR>), opted);
    hipLaunchKernelGGL((small_sets_refine_kernel<KIND, BYVAL, PRIOR>), dim3((unsigned)blocks_per_set, (unsigned)n_sets), dim3(256),
                       sizeof(SmallShared), s, args, sets, refs, starts, scratch, blocks_per_set, info, max_rounds, x_out,
                       val_out, grad_out, rounds_out, status_out);
}

int small_refine_starts_per_block(int d) { return 4 * (16 / (1 + d)); }

void launch_small_sets_refine(hipStream_t s, int kind, bool prior, const cbo_small_set *sets, const cbo_small_refine *refs,
                              const double *starts, int n_sets, int blocks_per_set, double *scratch, int *info, int max_rounds,
                              double *x_out, double *val_out, double *grad_out, int *rounds_out, int *status_out)
{
    SmallSetArgs args{};
    const bool byval = n_sets <= kSmallByValue;
    if (byval) std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_sets);
#define CBO_LAUNCH_AS(K, B, P)                                                                                          \
    launch_refine_as<K, B, P>(s, args, sets, refs, starts, n_sets, blocks_per_set, scratch, info, max_rounds, x_out, val_out, \
                              grad_out, rounds_out, status_out)
#define CBO_LAUNCH_KIND(K)                                                                                              \
    (prior ? (byval ? CBO_LAUNCH_AS(K, true, true) : CBO_LAUNCH_AS(K, false, true))                                     \
           : (byval ? CBO_LAUNCH_AS(K, true, false) : CBO_LAUNCH_AS(K, false, false)))
    switch (kind) {
        case CBO_ACQ_LCB: CBO_LAUNCH_KIND(CBO_ACQ_LCB); break;
        case CBO_ACQ_PI: CBO_LAUNCH_KIND(CBO_ACQ_PI); break;
        case CBO_ACQ_VAR: CBO_LAUNCH_KIND(CBO_ACQ_VAR); break;
        case CBO_ACQ_MPEI: CBO_LAUNCH_KIND(CBO_ACQ_MPEI); break;
        // (log EI: plain sets alone -- the causal instantiation is not built, refine_sets_impl declines such a set)
        case kLogEiKind: byval ? CBO_LAUNCH_AS(kLogEiKind, true, false) : CBO_LAUNCH_AS(kLogEiKind, false, false); break;
        // (the point-cost kinds likewise)
        case kEiPointKind: byval ? CBO_LAUNCH_AS(kEiPointKind, true, false) : CBO_LAUNCH_AS(kEiPointKind, false, false); break;
        case kLogEiPointKind:
            byval ? CBO_LAUNCH_AS(kLogEiPointKind, true, false) : CBO_LAUNCH_AS(kLogEiPointKind, false, false);
            break;
        default: CBO_LAUNCH_KIND(kEiKind); break;
    }
#undef CBO_LAUNCH_KIND
#undef CBO_LAUNCH_AS
}

}  // namespace cbo

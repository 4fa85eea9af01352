// Constrained acquisition in the one-launch multi-set sweep for gfx950: small_sets_kernel's sibling
// (kernels_sets.hip) for EI times the constraints' probabilities of feasibility over a cost.  One workgroup serves (one
// set, 64 candidates) and walks the set's (model, candidate set) pairs in order -- the objective, then the constraints --
// running the stages of cbo_small_device.h, the sibling's sequence, on each pair's own descriptor (every model has its own
// scaled copy of the candidates): small_model_factor, K*, the tile solve, posterior_of with the noise.  The pair's term
// (acquisition_of at cost 1 for the objective, feasibility_of for a constraint) is multiplied into one running register per
// candidate lane, left to right; the closing quotient is constrained_acq_kernel's (kernels_con.hip) in its two forms.  Same
// device functions, same summation orders as the general path: cbo_acq_sweep_constrained's bits.
#include <cstring>

#include "cbo_small_device.h"

#pragma clang fp contract(off)

namespace cbo {

static_assert(sizeof(SmallShared) + sizeof(int) <= 163840, "the workgroup's static LDS (the ticket flag) beside SmallShared: one CU");
// two-launch form: phase 1 factors pair p of a set into scratch slot set * blocks_per_set + p
static_assert(1 + CBO_MAX_CONSTRAINTS <= kSmallTwoPhaseFromBlocks, "a set's pairs each need a scratch slot of their own in the two-launch form");

// Descriptor p of the launch is one (model, candidate set) pair; the pairs of a set are consecutive, the objective first.
// The pair range of set s is [first(s), first(s + 1)): first(s) rides in descriptor s's pad_ word (there are at least as many
// pairs as sets), first(n_sets) is n_pairs.  A constraint's value, jitter and sense ride in its descriptor's y_best,
// ei_jitter and task; the objective's descriptor carries the EI's scalars and the set's cost.
// phases: 1 = workgroup (p, set) factors pair p of the set into its slot, nothing else; 2 = the factors are in the slots;
// 3 = everything in one launch, the workgroup's own slot serving its models one after the other.
// LOG: the running register holds logEI, then (logEI + l_0), then ((logEI + l_0) + l_1), ... -- log_ei_of at
// log cost 0.0 and log_feasibility_of, constrained_acq_kernel<.., true>'s terms and its closing subtraction of log(cost):
// cbo_acq_sweep_constrained_log's bits.
template <bool BYVAL, bool LOG>
__global__ __launch_bounds__(256) void small_sets_con_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
                                                             int n_pairs, double *scratch, int blocks_per_set,
                                                             double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                             int *__restrict__ info, int *__restrict__ ticket,
                                                             cbo_small_result *__restrict__ out, int seq, int phases)
{
    __shared__ int last_flag;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int set = blockIdx.y, blk = blockIdx.x;
    const int p0 = BYVAL ? byval.s[set].pad_ : sets[set].pad_;
    const int p1 = (set + 1 < (int)gridDim.y) ? (BYVAL ? byval.s[set + 1].pad_ : sets[set + 1].pad_) : n_pairs;
    const int slot = set * blocks_per_set + blk;
    if (phases == 1) {                                            // one workgroup per pair: factor it, nothing else
        if (p0 + blk >= p1) return;
        const cbo_small_set st = BYVAL ? byval.s[p0 + blk] : sets[p0 + blk];
        small_factor_only(sh, st, scratch + (int64_t)slot * kSmallScratch, &info[set]);
        return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t c = (int64_t)blk * 64 + wave * 16 + lc;

    double run = 0.0;                                             // EI, then EI * pof_0, then (EI * pof_0) * pof_1, ...
                                                                  // (LOG: logEI, then logEI + l_0, ...)
    double cost = 1.0;
    int64_t m = 0, index_offset = 0;
    for (int p = p0; p < p1; ++p) {                               // (uniform)
        const cbo_small_set st = BYVAL ? byval.s[p] : sets[p];
        if (p == p0) {
            m = st.m; index_offset = st.index_offset; cost = st.cost;
            if ((int64_t)blk * 64 >= m) {                         // no candidates left for this workgroup
                small_set_finish(-INFINITY, INT64_MAX, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq,
                                 &last_flag);
                return;
            }
        } else {
            // the previous model's solve has read the factor, the points and sq / sv in LDS: nobody assembles the next
            // model over them before every wave is through
            __syncthreads();
        }
        const int tiles = (st.n + 15) / 16;
        double *my = scratch + (int64_t)(phases == 2 ? set * blocks_per_set + (p - p0) : slot) * kSmallScratch;
        double *Us = my, *invs = my + 128 * kSmallLd;

        // this wave's 16 candidates in the pair's own scaling
        double xc[CBO_MAX_DIM], csq, csv, cpm_c, cpv_c;
        small_fetch_cand(st, c, xc, csq, csv, cpm_c, cpv_c);

        double iv[8][4], zr[8][4];
        small_model_factor(sh, st, tiles, Us, invs, &info[set], iv, zr, phases, true);

        const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
        d4 acc[8];
        small_kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        double qacc, macc;
        solve_q_mu(sh, acc, iv, zr, tiles, kq, lc, qacc, macc);

        // ---- the pair's term (constrained_acq_kernel's, model by model)
        AcqParams ap = small_acq_params(st);
        ap.cost = 1.0;
        double mean, var;
        if (p == p0) {
            posterior_of(qacc, macc, cpm_c, cpv_c, st.sv != nullptr, ap, mean, var);
            if (LOG) run = log_ei_of(mean, var, ap, 0.0);         // cbo_acq_sweep_logei's acq at cost 1
            else run = acquisition_of(mean, var, ap);             // cbo_acq_sweep's acq at cost 1
        } else {
            ap.y_best = 0.0; ap.ei_jitter = 0.0; ap.task = CBO_TASK_MIN;
            posterior_of(qacc, macc, cpm_c, cpv_c, st.sv != nullptr, ap, mean, var);
            if (LOG) run = run + log_feasibility_of(mean, var, st.y_best, st.ei_jitter, st.task);
            else run = run * feasibility_of(mean, var, st.y_best, st.ei_jitter, st.task);
        }
    }
    if (LOG) {
        run = run - log(cost);
    } else if (p1 - p0 == 1) {
        // no constraint: acquisition_of's own quotient (the reciprocal of the cost, corrected by the remainder)
        const double rc = 1.0 / cost;
        const double qv = run * rc;
        run = fma(fma(-qv, cost, run), rc, qv);
    } else {
        run = run / cost;                                         // IEEE division (emukit's Quotient is numpy's)
    }

    // ---- the workgroup's arg-max
    double bv = -INFINITY;
    int64_t bi = INT64_MAX;
    if (kq == 0 && c < m) { bv = run; bi = c + index_offset; }
    small_block_argmax(sh, lane, wave, bv, bi);
    small_set_finish(bv, bi, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq, &last_flag);
}

template <bool BYVAL, bool LOG>
static void launch_small_sets_con_as(hipStream_t s, const SmallSetArgs &args, const cbo_small_set *pairs, int n_pairs,
                                     int n_sets, int max_pairs, int blocks_per_set, double *scratch, double *part_val,
                                     int64_t *part_idx, int *info, int *ticket, cbo_small_result *out, int seq)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(small_sets_con_kernel<BYVAL, LOG>), opted);
    auto launch = [&](const dim3 &g, int phases) {
        hipLaunchKernelGGL((small_sets_con_kernel<BYVAL, LOG>), g, dim3(256), sizeof(SmallShared), s, args, pairs, n_pairs, scratch,
                           blocks_per_set, part_val, part_idx, info, ticket, out, seq, phases);
    };
    if (blocks_per_set >= kSmallTwoPhaseFromBlocks) {
        launch(dim3((unsigned)max_pairs, (unsigned)n_sets), 1);
        launch(dim3((unsigned)blocks_per_set, (unsigned)n_sets), 2);
    } else {
        launch(dim3((unsigned)blocks_per_set, (unsigned)n_sets), 3);
    }
}

// launch_small_sets for the constrained epilogue (cbo_internal.h)
void launch_small_sets_con(hipStream_t s, const cbo_small_set *pairs, int n_pairs, int n_sets, int max_pairs,
                           int blocks_per_set, const SmallLaunch &L, bool log_form)
{
    SmallSetArgs args{};
    const bool byval = n_pairs <= kSmallByValue;
    if (byval) std::memcpy(args.s, pairs, sizeof(cbo_small_set) * (size_t)n_pairs);
    auto launch = byval ? (log_form ? launch_small_sets_con_as<true, true> : launch_small_sets_con_as<true, false>)
                        : (log_form ? launch_small_sets_con_as<false, true> : launch_small_sets_con_as<false, false>);
    launch(s, args, pairs, n_pairs, n_sets, max_pairs, blocks_per_set, L.scratch, L.part_val, L.part_idx, L.info, L.ticket,
           L.out, L.seq);
}

}  // namespace cbo

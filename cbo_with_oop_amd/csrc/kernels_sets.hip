// The one-launch multi-set sweep for gfx950: small_sets_kernel<KIND>, the causal EI of every exploration
// set of a trial (KIND = kEiKind: cbo_acq_sweep_sets, cbo_trial_step; the reference's operating point) and the point-wise
// acquisitions -- the lower / upper confidence bound, the probability of improvement, the model variance and the mean-
// plug-in Expected Improvement (KIND = CBO_ACQ_*: cbo_acq_sweep_sets_kind).  One workgroup does everything for (one set,
// 64 candidates) inside LDS and registers, from the stages of cbo_small_device.h (its comments say why each is as it is):
// one grid, one one- / two-launch split, one descriptor, one staged form of a trial step, one result record.  The kinds are
// instantiations of one sequence and differ in the epilogue alone: acquisition_of (cbo_acq_sweep's bits) or
// pointwise_of<KIND> (kernels_pointwise.hip's, so cbo_acq_sweep_kind's bits) -- and, for the plug-in EI, in the incumbent
// first: the model's own points run as candidates through the factor the workgroup already holds.
#include <cstring>

#include "cbo_small_device.h"

#pragma clang fp contract(off)

namespace cbo {

static_assert(sizeof(SmallShared) + 128 * sizeof(double) + 4 * sizeof(double) + 4 * sizeof(int) + sizeof(double) +
                      sizeof(int) <= 163840,
              "the workgroup's static LDS (plug-in means, their reduction, the ticket flag) beside SmallShared: one CU");
static_assert(sizeof(SmallShared) + kMesMaxSamples * sizeof(double) + sizeof(int) <= 163840,
              "the workgroup's static LDS (the set's Gumbel samples, the ticket flag) beside SmallShared: one CU");

// KIND: kEiKind, or CBO_ACQ_LCB, _PI, _VAR or _MPEI (compile time: one kind's arithmetic per instantiation).  For a point-wise
// kind the descriptor's ei_jitter carries the kind's parameter (beta; PI's and the plug-in EI's jitter), y_best PI's incumbent.
// kMesKind: max-value entropy search -- the set's Gumbel samples come from aux's table (fetched with the
// candidates, ahead of the factorisation; parked in LDS behind K*'s barrier), the epilogue is mes_of.  kPredictKind: the
// epilogue stores mean and variance at the set's offset in aux's workspace; no arg-max, the record carries the status word.
// kLogEiKind: the epilogue is log_ei_of, log EI - log cost -- cbo_acq_sweep_logei's bits; nothing from aux.
// kEiPointKind / kLogEiPointKind: the lane that holds candidate c reads cost[c] from the set's cost vector
// (aux.cost[set], fetched with the candidate) and scores over it: acquisition_of at cost 1 / cost[c], or log_ei_of with
// log(cost[c]) -- cbo_acq_sweep_pointcost's bits.
// phases 3: every workgroup factors the model itself, into its own scratch slot; 1: one workgroup per set factors it into
// the set's slot 0, nothing else; 2: the set's slot 0 holds the factor.
template <int KIND, bool BYVAL>
__global__ __launch_bounds__(256) void small_sets_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
                                                         double *scratch, int blocks_per_set,
                                                         double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                         int *__restrict__ info, int *__restrict__ ticket,
                                                         cbo_small_result *__restrict__ out, int seq, int phases,
                                                         const SmallAux aux)
{
    __shared__ int last_flag;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int set = blockIdx.y, blk = blockIdx.x;
    const cbo_small_set st = BYVAL ? byval.s[set] : sets[set];
    const int slot = set * blocks_per_set + blk;
    if (phases == 1) {
        small_factor_only(sh, st, scratch + (int64_t)(set * blocks_per_set) * kSmallScratch, &info[set]);
        return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    if ((int64_t)blk * 64 >= st.m) {                              // no candidates left for this workgroup
        small_set_finish(-INFINITY, INT64_MAX, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq,
                         &last_flag);
        return;
    }
    const int tiles = (st.n + 15) / 16;
    double *my = scratch + (int64_t)(phases == 2 ? set * blocks_per_set : slot) * kSmallScratch;
    double *Us = my, *invs = my + 128 * kSmallLd;

    // this wave's 16 candidates
    const int64_t c = (int64_t)blk * 64 + wave * 16 + lc;
    double xc[CBO_MAX_DIM], csq, csv, cpm_c, cpv_c;
    [[maybe_unused]] double cost_c = 1.0;
    if constexpr (KIND == kEiPointKind || KIND == kLogEiPointKind)
        small_fetch_cand(st, c, xc, csq, csv, cpm_c, cpv_c, aux.cost[set], cost_c);
    else
        small_fetch_cand(st, c, xc, csq, csv, cpm_c, cpv_c);
    [[maybe_unused]] cbo_small_aux ax{};
    [[maybe_unused]] double my_min = 0.0;                          // thread t < count: the set's sample t
    if constexpr (KIND == kMesKind || KIND == kPredictKind) ax = aux.per_set[set];
    if constexpr (KIND == kMesKind) {
        if (tid < (int)ax.count) my_min = aux.data[ax.off + tid];
    }

    double iv[8][4], zr[8][4];
    small_model_factor(sh, st, tiles, Us, invs, &info[set], iv, zr, phases, true);

    AcqParams p = small_acq_params(st);
    if constexpr (KIND == CBO_ACQ_MPEI) {
        // the incumbent of every candidate of the set: from the factor, before this workgroup's own candidates
        __shared__ double plug_mean[128], plug_red[4], plug_out;
        __shared__ int plug_nan[4];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        p.y_best = small_plugin_incumbent(sh, st, tiles, iv, zr, p, st.stage != nullptr && (phases & 1), plug_mean, plug_red,
                                          plug_nan, &plug_out);
    }

    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    d4 acc[8];
    small_kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
    [[maybe_unused]] double *mes_mins = nullptr;
    if constexpr (KIND == kMesKind) {
        __shared__ double mins_s[kMesMaxSamples];
        if (tid < kMesMaxSamples) mins_s[tid] = my_min;
        mes_mins = mins_s;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    double qacc, macc;
    solve_q_mu(sh, acc, iv, zr, tiles, kq, lc, qacc, macc);

    // ---- epilogue and the workgroup's arg-max
    double bv = -INFINITY;
    int64_t bi = INT64_MAX;
    if (kq == 0 && c < st.m) {
        double mean, var;
        posterior_of(qacc, macc, cpm_c, cpv_c, st.sv != nullptr, p, mean, var);
        if constexpr (KIND == kPredictKind) {
            aux.mean_out[ax.off + c] = mean;
            aux.var_out[ax.off + c] = var;
        } else {
            if constexpr (KIND == kMesKind) {
                const MesSetParams mp{mes_mins, (int)ax.count, p.cost};
                bv = mes_of(mean, var, mp);
            } else {
                if constexpr (KIND == kLogEiKind)
                    bv = log_ei_of(mean, var, p);
                else if constexpr (KIND == kLogEiPointKind)
                    bv = log_ei_of(mean, var, p, log(cost_c));
                else if constexpr (KIND == kEiPointKind)
                    bv = acquisition_of(mean, var, p) / cost_c;  // (p.cost is 1: the EI itself, then the IEEE quotient)
                else
                    bv = (KIND == kEiKind || KIND == CBO_ACQ_MPEI) ? acquisition_of(mean, var, p)
                                                                   : pointwise_of<KIND>(mean, var, p);
            }
            bi = c + st.index_offset;
        }
    }
    if constexpr (KIND != kPredictKind) small_block_argmax(sh, lane, wave, bv, bi);
    small_set_finish(bv, bi, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq, &last_flag);
}

size_t small_sets_scratch_doubles(int n_sets, int blocks_per_set) { return (size_t)n_sets * blocks_per_set * kSmallScratch; }

template <int KIND, bool BYVAL>
static void launch_small_sets_as(hipStream_t s, const SmallSetArgs &args, const cbo_small_set *sets, int n_sets,
                                 int blocks_per_set, double *scratch, double *part_val, int64_t *part_idx, int *info,
                                 int *ticket, cbo_small_result *out, int seq, const SmallAux &aux)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(small_sets_kernel<KIND, BYVAL>), opted);
    const dim3 grid((unsigned)blocks_per_set, (unsigned)n_sets);
    auto launch = [&](const dim3 &g, int phases) {
        hipLaunchKernelGGL((small_sets_kernel<KIND, BYVAL>), g, dim3(256), sizeof(SmallShared), s, args, sets, scratch,
                           blocks_per_set, part_val, part_idx, info, ticket, out, seq, phases, aux);
    };
    if (blocks_per_set >= kSmallTwoPhaseFromBlocks) {
        launch(dim3(1u, (unsigned)n_sets), 1);
        launch(grid, 2);
    } else {
        launch(grid, 3);
    }
}

void launch_small_sets(hipStream_t s, int kind, const cbo_small_set *sets, int n_sets, int blocks_per_set, const SmallLaunch &L,
                       const SmallAux &aux)
{
    SmallSetArgs args{};
    const bool byval = n_sets <= kSmallByValue;
    if (byval) std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_sets);
#define CBO_LAUNCH_KIND(K)                                                                                              \
    (byval ? launch_small_sets_as<K, true>(s, args, sets, n_sets, blocks_per_set, L.scratch, L.part_val, L.part_idx,     \
                                           L.info, L.ticket, L.out, L.seq, aux)                                         \
           : launch_small_sets_as<K, false>(s, args, sets, n_sets, blocks_per_set, L.scratch, L.part_val, L.part_idx,   \
                                            L.info, L.ticket, L.out, L.seq, aux))
    switch (kind) {
        case CBO_ACQ_LCB: CBO_LAUNCH_KIND(CBO_ACQ_LCB); break;
        case CBO_ACQ_PI: CBO_LAUNCH_KIND(CBO_ACQ_PI); break;
        case CBO_ACQ_VAR: CBO_LAUNCH_KIND(CBO_ACQ_VAR); break;
        case CBO_ACQ_MPEI: CBO_LAUNCH_KIND(CBO_ACQ_MPEI); break;
        case kMesKind: CBO_LAUNCH_KIND(kMesKind); break;
        case kPredictKind: CBO_LAUNCH_KIND(kPredictKind); break;
        case kLogEiKind: CBO_LAUNCH_KIND(kLogEiKind); break;
        case kEiPointKind: CBO_LAUNCH_KIND(kEiPointKind); break;
        case kLogEiPointKind: CBO_LAUNCH_KIND(kLogEiPointKind); break;
        default: CBO_LAUNCH_KIND(kEiKind); break;
    }
#undef CBO_LAUNCH_KIND
}

}  // namespace cbo

// The causal EI marginalised over hyper-parameter samples (emukit IntegratedHyperParameterAcquisition).
//
// hyper_avg_kernel: one workgroup of 256 threads per 64 candidates, small_sets_kernel's layout, for a model of at most 128
// observations.  The workgroup walks the H samples in index order; for sample h it prepares the model's and its own
// candidates' points from their RAW coordinates with sample h's lengthscales (prep_points_kernel's arithmetic), assembles
// and factors K(X,X) + (noise_h + 1e-8) I inside LDS, forms K(X,X*) in the MFMA result registers, solves, and adds
// acquisition_of(...) of its candidates to a per-candidate sum -- all with the device functions of cbo_small_device.h, so
// each term is what cbo_acq_sweep writes for a model with sample h's hyper-parameters.  The sum is s = 0; s = s + acq_h
// (h = 0..H-1), the result s / H: one IEEE division.  Nothing resident is read but the raw points, the targets and the
// prior closures; nothing resident is written.
//   phases 3: every workgroup factors every sample itself (its own scratch slot, reused sample after sample);
//   phases 1: workgroup h factors sample h into scratch slot h and returns;  phases 2: the sweep reads factor h back.
// hyper_sets_kernel: the same for every exploration set of a trial in one launch, from the same device
// functions -- workgroup (block, set) walks its own set's samples.
// The accumulate / finish kernels at the end serve the general path (larger, fp32 or jitter-needing models), whose
// per-sample terms come from cbo_acq_sweep itself.
// LOG: the log-space form, log((1 / H) sum_h EI_h) - log cost.  The term is log_ei_of at log cost 0 --
// cbo_acq_sweep_logei's value at cost 1 -- the per-lane state the streaming log-sum-exp's (M, S) in the place of the sum,
// and the close lse_close in the place of the division (lse_stream.h); everything before the term is the same code.  The
// general path's kernels are hyper_lse_accumulate_kernel / hyper_lse_finish_kernel, from the same header.
#include <cstring>

#include "cbo_small_lml_device.h"
#include "lse_stream.h"

#pragma clang fp contract(off)

namespace cbo {

struct HyperSetArgs { HyperSet s[kSmallByValue]; };             // by value up to kSmallByValue sets, as SmallSetArgs
static_assert(sizeof(HyperSetArgs) <= 3072, "the descriptors by value and the other arguments fit the kernel arguments");

// ---- the prologue, the per-sample body and the close of a marginalised sweep: hyper_avg_kernel (one model, one candidate
// set) and hyper_sets_kernel (every set of a trial) are both built from these, so the arithmetic exists once
// and the two kernels' results are equal by construction.

// This lane's candidate of candidate block `blk` (clamped: lanes beyond the set compute, nobody looks) and the prior
// closures at it, which do not depend on the sample either
struct HyperLane {
    int64_t c, cc;
    double cpm_c, cpv_c, csv;
    bool causal;
};
__device__ __forceinline__ HyperLane hyper_lane(const cbo_small_set &st, int blk, int wave, int lc)
{
    HyperLane L;
    L.c = (int64_t)blk * 64 + wave * 16 + lc;
    L.cc = (L.c < st.m) ? L.c : st.m - 1;
    L.causal = st.sv != nullptr;
    L.cpm_c = st.cpm ? st.cpm[L.cc] : 0.0;
    L.cpv_c = st.cpv ? st.cpv[L.cc] : 0.0;
    L.csv = L.causal ? sqrt(L.cpv_c) : 0.0;
    return L;
}

// The log form's term pushed into the lane's (M, S): log_ei_of at log cost 0 under the sample's scalars, lse_start for the
// first sample, lse_push after it.  Out of line, the state returned in registers: inlined, log_h_of's three ranges and the
// push's exp would share the sweep's 256 VGPRs with the factor's registers (DESIGN.md §4ac has the figures).
struct LseState {
    double M, S;
};
__device__ __attribute__((noinline)) LseState hyper_lse_term(double mean, double var, double y_best, double jitter, int task,
                                                             bool first, double M, double S)
{
    AcqParams p{};
    p.y_best = y_best; p.ei_jitter = jitter; p.task = task; p.cost = 1.0;
    const double l = log_ei_of(mean, var, p, 0.0);
    if (first) lse_start(l, M, S);
    else lse_push(l, M, S);
    return LseState{M, S};
}

// One sample: the points with the sample's lengthscales, the factor (factored here into `slot` when `factor`, else read from
// `slot`, where a first launch left it), K*, the solve, and sum = sum + acquisition_of(...) on the lanes that own a candidate
// (LOG: (sum, S) is the log-sum-exp's (M, S), started by the `first` sample)
template <bool LOG>
__device__ __forceinline__ void hyper_add_sample(SmallShared &sh, const cbo_small_set &st, const double *__restrict__ craw,
                                                 const double *__restrict__ row, int n_ls, int tiles, double rhs, double *slot,
                                                 bool factor, int *info_word, const HyperLane &L, int lane, int wave,
                                                 bool first, double &sum, double &S)
{
    const int lc = lane & 15, kq = lane >> 4;
    const double *ls = st.ard ? row + 1 : nullptr;
    const cbo_small_set sth = hyper_sample_set(st, row, n_ls);
    double *Us = slot, *invs = slot + 128 * kSmallLd;
    double xc[CBO_MAX_DIM], csq;
    hyper_point(craw, L.cc, st.d, ls, true, xc, csq);
    __syncthreads();                                          // the previous sample's solve has read the block and the points
    hyper_model_points(sh, st, ls);
    __syncthreads();
    if (factor) hyper_factor(sh, sth, tiles, rhs, Us, invs, info_word);
    // ---- the factor back into LDS (rows of the factored tiles), inverses and z to registers
    {
        const unsigned s0 = lds_byte_address(&sh.blk.S[0][0]);
        const int rows = 16 * tiles;
        for (int p = wave; p < rows; p += 4)
            glds16(Us + (int64_t)p * kSmallLd + lane * 2, __builtin_amdgcn_readfirstlane(s0 + 8u * (unsigned)(p * kDiagLd)));
    }
    double iv[8][4], zr[8][4];
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            iv[s][kk] = (s < tiles) ? invs[s * 256 + (4 * kk + kq) * 16 + lc] : 0.0;
            zr[s][kk] = (s < tiles) ? Us[(int64_t)(16 * s + kq + 4 * kk) * kSmallLd + 128] : 0.0;
        }
    const double inv_l2 = 1.0 / (sth.lengthscale * sth.lengthscale);
    d4 acc[8];
    small_kstar_tiles_of(sh, sth, tiles, xc, csq, L.csv, inv_l2, kq, acc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    double qacc, macc;
    solve_q_mu(sh, acc, iv, zr, tiles, kq, lc, qacc, macc);

    const AcqParams p = small_acq_params(sth);                // (the sample's variance and noise, the model's EI scalars)
    if (kq == 0 && L.c < st.m) {
        double mean, var;
        posterior_of(qacc, macc, L.cpm_c, L.cpv_c, L.causal, p, mean, var);
        if constexpr (LOG) {
            const LseState t = hyper_lse_term(mean, var, p.y_best, p.ei_jitter, p.task, first, sum, S);
            sum = t.M;
            S = t.S;
        } else {
            sum = __dadd_rn(sum, acquisition_of(mean, var, p));
        }
    }
}

// The mean over the samples (one IEEE division; LOG: lse_close over the lane's (M, S) = (sum, S)) and the workgroup's
// arg-max of it: thread 0's (bv, bi) on return
template <bool LOG>
__device__ __forceinline__ void hyper_mean_argmax(SmallShared &sh, const cbo_small_set &st, double sum, double S, int n_samples,
                                                  double *acq_out, const HyperLane &L, int lane, int wave, double &bv,
                                                  int64_t &bi)
{
    bv = -INFINITY;
    bi = INT64_MAX;
    if ((lane >> 4) == 0 && L.c < st.m) {
        if constexpr (LOG) bv = lse_close(sum, S, n_samples, log(st.cost));
        else bv = __ddiv_rn(sum, (double)n_samples);
        bi = L.c + st.index_offset;
        if (acq_out) acq_out[L.c] = bv;
    }
    small_block_argmax(sh, lane, wave, bv, bi);
}

template <bool LOG>
__global__ __launch_bounds__(256) void hyper_avg_kernel(const HyperArgs a, double *scratch, int blocks,
                                                        double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                        int *__restrict__ info, int *__restrict__ ticket,
                                                        cbo_small_result *__restrict__ out, int seq, int phases)
{
    __shared__ int last_flag;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const cbo_small_set &st = a.st;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = blockIdx.x;
    const int tiles = (st.n + 15) / 16;
    const int row_len = a.n_ls + 2;
    const double rhs = hyper_rhs(st);
    if (phases == 1) {                                            // workgroup h: factor sample h into slot h, nothing else
        hyper_factor_sample(sh, st, a.hyper + (int64_t)blk * row_len, a.n_ls, tiles, rhs,
                            scratch + (int64_t)blk * kSmallScratch, &info[0]);
        return;
    }
    const HyperLane L = hyper_lane(st, blk, wave, lane & 15);
    double sum = 0.0, S = 0.0;
    for (int h = 0; h < a.n_samples; ++h)
        // phases 3: the workgroup's own slot, sample after sample; phases 2: slot h holds sample h's factor
        hyper_add_sample<LOG>(sh, st, a.craw, a.hyper + (int64_t)h * row_len, a.n_ls, tiles, rhs,
                              scratch + (int64_t)(phases == 2 ? h : blk) * kSmallScratch, (phases & 1) != 0, &info[0], L, lane,
                              wave, h == 0, sum, S);
    double bv;
    int64_t bi;
    hyper_mean_argmax<LOG>(sh, st, sum, S, a.n_samples, a.acq_out, L, lane, wave, bv, bi);
    small_set_finish(bv, bi, 0, blk, blocks, part_val, part_idx, info, ticket, out, seq, &last_flag);
}

// The multi-set form (cbo_acq_sweep_sets_hyper): workgroup (blk, set) serves 64 candidates of set `set` and
// walks that set's own samples in index order.
//   phases 3: grid (blocks_per_set, n_sets); every workgroup factors every sample of its set into its own scratch slot
//             set * blocks_per_set + blk, reused sample after sample;
//   phases 1: grid (sum of the sets' n_samples): workgroup first_s + h factors sample h of set s into slot first_s + h;
//   phases 2: grid (blocks_per_set, n_sets): the sweep reads slot first_s + h back.
// A workgroup beyond its set's own candidate blocks (a set narrower than the widest) reads nothing of the set and writes no
// scratch: it only hands in the empty winner, as small_sets_kernel's does, so that the set's ticket counts blocks_per_set.
template <bool BYVAL, bool LOG>
__global__ __launch_bounds__(256) void hyper_sets_kernel(const HyperSetArgs byval, const HyperSet *__restrict__ sets,
                                                         int n_sets, double *scratch, int blocks_per_set,
                                                         double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                         int *__restrict__ info, int *__restrict__ ticket,
                                                         cbo_small_result *__restrict__ out, int seq, int phases)
{
    __shared__ int last_flag;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (phases == 1) {
        // the set whose samples hold slot blockIdx.x: the sets' first slots ascend (uniform scan, at most n_sets - 1 steps)
        const int slot = blockIdx.x;
        int set = 0;
        while (set + 1 < n_sets && (BYVAL ? byval.s[set + 1].first : sets[set + 1].first) <= slot) ++set;
        const HyperSet hs = BYVAL ? byval.s[set] : sets[set];
        const cbo_small_set &st = hs.a.st;
        const int h = slot - hs.first;
        if (h >= hs.a.n_samples) return;
        hyper_factor_sample(sh, st, hs.a.hyper + (int64_t)h * (hs.a.n_ls + 2), hs.a.n_ls, (st.n + 15) / 16, hyper_rhs(st),
                            scratch + (int64_t)slot * kSmallScratch, &info[set]);
        return;
    }
    const int set = blockIdx.y, blk = blockIdx.x;
    const HyperSet hs = BYVAL ? byval.s[set] : sets[set];
    const cbo_small_set &st = hs.a.st;
    const int slot = set * blocks_per_set + blk;
    if ((int64_t)blk * 64 >= st.m) {                              // no candidates left for this workgroup
        small_set_finish(-INFINITY, INT64_MAX, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq,
                         &last_flag);
        return;
    }
    const int tiles = (st.n + 15) / 16;
    const int row_len = hs.a.n_ls + 2;
    const double rhs = hyper_rhs(st);
    const HyperLane L = hyper_lane(st, blk, wave, lane & 15);
    double sum = 0.0, S = 0.0;
    for (int h = 0; h < hs.a.n_samples; ++h)
        hyper_add_sample<LOG>(sh, st, hs.a.craw, hs.a.hyper + (int64_t)h * row_len, hs.a.n_ls, tiles, rhs,
                              scratch + (int64_t)(phases == 2 ? hs.first + h : slot) * kSmallScratch, (phases & 1) != 0,
                              &info[set], L, lane, wave, h == 0, sum, S);
    double bv;
    int64_t bi;
    hyper_mean_argmax<LOG>(sh, st, sum, S, hs.a.n_samples, nullptr, L, lane, wave, bv, bi);
    small_set_finish(bv, bi, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq, &last_flag);
}

size_t hyper_avg_scratch_doubles(int blocks, int n_samples)
{
    return (size_t)(blocks > n_samples ? blocks : n_samples) * kSmallScratch;
}

// schedule 0: from kSmallTwoPhaseFromBlocks candidate blocks on, the samples are factored once by a first launch of n_samples
// workgroups and the sweep reads the factors back (phases 1 + 2); below, every workgroup factors every sample itself (phases 3)
template <bool LOG>
static void launch_hyper_avg_as(hipStream_t s, const cbo_small_set &st, const double *craw, const double *hyper, int n_samples,
                                int n_ls, double *acq_out, int blocks, int schedule, const SmallLaunch &L)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(hyper_avg_kernel<LOG>), opted);
    HyperArgs a{};
    a.st = st; a.craw = craw; a.hyper = hyper; a.n_samples = n_samples; a.n_ls = n_ls; a.acq_out = acq_out;
    const bool two_phase = schedule == 2 || (schedule != 1 && blocks >= kSmallTwoPhaseFromBlocks);
    if (two_phase) {
        hipLaunchKernelGGL(hyper_avg_kernel<LOG>, dim3((unsigned)n_samples), dim3(256), sizeof(SmallShared), s, a, L.scratch,
                           blocks, L.part_val, L.part_idx, L.info, L.ticket, L.out, L.seq, 1);
        hipLaunchKernelGGL(hyper_avg_kernel<LOG>, dim3((unsigned)blocks), dim3(256), sizeof(SmallShared), s, a, L.scratch,
                           blocks, L.part_val, L.part_idx, L.info, L.ticket, L.out, L.seq, 2);
    } else {
        hipLaunchKernelGGL(hyper_avg_kernel<LOG>, dim3((unsigned)blocks), dim3(256), sizeof(SmallShared), s, a, L.scratch,
                           blocks, L.part_val, L.part_idx, L.info, L.ticket, L.out, L.seq, 3);
    }
}

void launch_hyper_avg(hipStream_t s, const cbo_small_set &st, const double *craw, const double *hyper, int n_samples,
                      int n_ls, double *acq_out, int blocks, int schedule, const SmallLaunch &L, bool log_form)
{
    if (log_form) launch_hyper_avg_as<true>(s, st, craw, hyper, n_samples, n_ls, acq_out, blocks, schedule, L);
    else launch_hyper_avg_as<false>(s, st, craw, hyper, n_samples, n_ls, acq_out, blocks, schedule, L);
}

// The two-launch form needs one scratch slot per sample of the call, the single launch one per workgroup
size_t hyper_sets_scratch_doubles(int n_sets, int blocks_per_set, int total_samples, bool two_phase)
{
    return (two_phase ? (size_t)total_samples : (size_t)n_sets * (size_t)blocks_per_set) * kSmallScratch;
}

template <bool BYVAL, bool LOG>
static void launch_hyper_sets_as(hipStream_t s, const HyperSetArgs &args, const HyperSet *sets, int n_sets, int blocks_per_set,
                                 int total_samples, bool two_phase, double *scratch, double *part_val, int64_t *part_idx,
                                 int *info, int *ticket, cbo_small_result *out, int seq)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(hyper_sets_kernel<BYVAL, LOG>), opted);
    const dim3 grid((unsigned)blocks_per_set, (unsigned)n_sets);
    auto launch = [&](const dim3 &g, int phases) {
        hipLaunchKernelGGL((hyper_sets_kernel<BYVAL, LOG>), g, dim3(256), sizeof(SmallShared), s, args, sets, n_sets, scratch,
                           blocks_per_set, part_val, part_idx, info, ticket, out, seq, phases);
    };
    if (two_phase) {
        launch(dim3((unsigned)total_samples), 1);
        launch(grid, 2);
    } else {
        launch(grid, 3);
    }
}

void launch_hyper_sets(hipStream_t s, const HyperSet *sets, int n_sets, int blocks_per_set, int total_samples, bool two_phase,
                       const SmallLaunch &L, bool log_form)
{
    HyperSetArgs args{};
    const bool byval = n_sets <= kSmallByValue;
    if (byval) std::memcpy(args.s, sets, sizeof(HyperSet) * (size_t)n_sets);
    auto launch = byval ? (log_form ? launch_hyper_sets_as<true, true> : launch_hyper_sets_as<true, false>)
                        : (log_form ? launch_hyper_sets_as<false, true> : launch_hyper_sets_as<false, false>);
    launch(s, args, sets, n_sets, blocks_per_set, total_samples, two_phase, L.scratch, L.part_val, L.part_idx, L.info, L.ticket,
           L.out, L.seq);
}

// ---- the general path's two kernels ------------------------------------------------------------------------------------
// sum[i] = (first ? 0 : sum[i]) + acq[i]: the running sum of the per-sample acquisitions, in sample order
__global__ __launch_bounds__(256) void hyper_accumulate_kernel(double *__restrict__ sum, const double *__restrict__ acq,
                                                               int64_t m, int first)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        sum[i] = __dadd_rn(first ? 0.0 : sum[i], acq[i]);
}

// acq[i] = sum[i] / n_samples (acq_out may be null) and the workgroups' arg-max partials for launch_argmax_final
__global__ __launch_bounds__(256) void hyper_finish_kernel(const double *__restrict__ sum, int64_t m, int n_samples,
                                                           double *__restrict__ acq_out, double *__restrict__ part_val,
                                                           int64_t *__restrict__ part_idx, int64_t index_offset)
{
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = __ddiv_rn(sum[i], (double)n_samples);
        if (acq_out) acq_out[i] = v;
        if (better(v, i + index_offset, bv, bi)) { bv = v; bi = i + index_offset; }
    }
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

// The log form's general path: term[i] is sample h's log EI at cost 1 (pointwise_acq_kernel<kLogEiKind>'s
// output); (M[i], S[i]) the streaming log-sum-exp's state, started by the first sample
__global__ __launch_bounds__(256) void hyper_lse_accumulate_kernel(double *__restrict__ M, double *__restrict__ S,
                                                                   const double *__restrict__ term, int64_t m, int first)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        double Mi = 0.0, Si = 0.0;
        if (first) {
            lse_start(term[i], Mi, Si);
        } else {
            Mi = M[i];
            Si = S[i];
            lse_push(term[i], Mi, Si);
        }
        M[i] = Mi;
        S[i] = Si;
    }
}

// acq[i] = lse_close(M[i], S[i], n_samples, log cost) (acq_out may be null) and the workgroups' arg-max partials
__global__ __launch_bounds__(256) void hyper_lse_finish_kernel(const double *__restrict__ M, const double *__restrict__ S,
                                                               int64_t m, int n_samples, double cost,
                                                               double *__restrict__ acq_out, double *__restrict__ part_val,
                                                               int64_t *__restrict__ part_idx, int64_t index_offset)
{
    const double log_cost = log(cost);                            // (uniform: once per launch)
    double bv = -INFINITY;
    int64_t bi = kNoIndex;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = lse_close(M[i], S[i], n_samples, log_cost);
        if (acq_out) acq_out[i] = v;
        if (better(v, i + index_offset, bv, bi)) { bv = v; bi = i + index_offset; }
    }
    block_argmax(bv, bi, &part_val[blockIdx.x], &part_idx[blockIdx.x]);
}

void launch_hyper_lse_accumulate(hipStream_t s, double *M, double *S, const double *term, int64_t m, bool first, int n_blocks)
{
    hipLaunchKernelGGL(hyper_lse_accumulate_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, M, S, term, m, first ? 1 : 0);
}

void launch_hyper_lse_finish(hipStream_t s, const double *M, const double *S, int64_t m, int n_samples, double cost,
                             double *acq_out, double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    hipLaunchKernelGGL(hyper_lse_finish_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, M, S, m, n_samples, cost, acq_out,
                       part_val, part_idx, index_offset);
}

void launch_hyper_accumulate(hipStream_t s, double *sum, const double *acq, int64_t m, bool first, int n_blocks)
{
    hipLaunchKernelGGL(hyper_accumulate_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, sum, acq, m, first ? 1 : 0);
}

void launch_hyper_finish(hipStream_t s, const double *sum, int64_t m, int n_samples, double *acq_out, double *part_val,
                         int64_t *part_idx, int64_t index_offset, int n_blocks)
{
    hipLaunchKernelGGL(hyper_finish_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, sum, m, n_samples, acq_out, part_val,
                       part_idx, index_offset);
}

}  // namespace cbo

// Constrained acquisition in the one-launch multi-set sweep for gfx950: small_sets_kind_kernel's sibling
// (kernels_sets_kind.hip) for EI times the constraints' probabilities of feasibility over a cost.  One workgroup serves (one
// set, 64 candidates) and walks the set's (model, candidate set) pairs in order -- the objective, then the constraints --
// running the sibling's sequence on each pair's own descriptor (every model has its own scaled copy of the candidates):
// small_model_factor, K*, the tile solve, posterior_of with the noise.  The pair's term (acquisition_of at cost 1 for the
// objective, feasibility_of for a constraint) is multiplied into one running register per candidate lane, left to right; the
// closing quotient is constrained_acq_kernel's (kernels_con.hip) in its two forms.  Same device functions, same summation
// orders as the general path: cbo_acq_sweep_constrained's bits.  The kernels of the other sweeps are not touched.
#include <atomic>
#include <cstring>

#include "cbo_small_device.h"

#pragma clang fp contract(off)

namespace cbo {

static_assert(sizeof(SmallShared) + sizeof(int) <= 163840, "the workgroup's static LDS (the ticket flag) beside SmallShared: one CU");
// two-launch form: phase 1 factors pair p of a set into scratch slot set * blocks_per_set + p
constexpr int kTwoPhaseFromBlocks = 12;                           // launch_small_sets' split (kernels_chol.hip)
static_assert(1 + CBO_MAX_CONSTRAINTS <= kTwoPhaseFromBlocks, "a set's pairs each need a scratch slot of their own in the two-launch form");

__device__ __forceinline__ void con_kstar_tiles_of(const SmallShared &sh, const cbo_small_set &st, int tiles, const double *xc,
                                                   double csq, double csv, double inv_l2, int kq, d4 (&acc)[8])
{
    switch (st.d) {
        case 1: small_kstar_tiles<1>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        case 2: small_kstar_tiles<2>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        case 3: small_kstar_tiles<3>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        case 4: small_kstar_tiles<4>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        case 5: small_kstar_tiles<5>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        case 6: small_kstar_tiles<6>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        case 7: small_kstar_tiles<7>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
        default: small_kstar_tiles<8>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc); break;
    }
}

// Descriptor p of the launch is one (model, candidate set) pair; the pairs of a set are consecutive, the objective first.
// The pair range of set s is [first(s), first(s + 1)): first(s) rides in descriptor s's pad_ word (there are at least as many
// pairs as sets), first(n_sets) is n_pairs.  A constraint's value, jitter and sense ride in its descriptor's y_best,
// ei_jitter and task; the objective's descriptor carries the EI's scalars and the set's cost.
// phases: 1 = workgroup (p, set) factors pair p of the set into its slot, nothing else; 2 = the factors are in the slots;
// 3 = everything in one launch, the workgroup's own slot serving its models one after the other.
template <bool BYVAL>
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
        double ivx[8][4], zrx[8][4];
        double *fs = scratch + (int64_t)slot * kSmallScratch;
        small_model_factor(sh, st, (st.n + 15) / 16, fs, fs + 128 * kSmallLd, &info[set], ivx, zrx, 1, true);
        return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t c = (int64_t)blk * 64 + wave * 16 + lc;

    double run = 0.0;                                             // EI, then EI * pof_0, then (EI * pof_0) * pof_1, ...
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

        // this wave's 16 candidates in the pair's own scaling: fetched now, used after the factorisation
        const int64_t cc = (c < st.m) ? c : st.m - 1;             // clamped: lanes beyond the set compute, nobody looks
        double xc[CBO_MAX_DIM];
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k) xc[k] = (k < st.d) ? st.cxs[(int64_t)k * st.cld + cc] : 0.0;
        const double csq = st.csq[cc], csv = st.csv ? st.csv[cc] : 0.0;
        const double cpm_c = st.cpm ? st.cpm[cc] : 0.0, cpv_c = st.cpv ? st.cpv[cc] : 0.0;

        double iv[8][4], zr[8][4];
        small_model_factor(sh, st, tiles, Us, invs, &info[set], iv, zr, phases, true);

        // ---- K(X, X*) of this wave's 16 candidates, straight into the result layout
        const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
        d4 acc[8];
        con_kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        // V = L^-1 K*, q = sum V^2, mu = V^T z: lane partials, then over the four lane groups (the strip kernel's order)
        double qacc = 0.0, macc = 0.0;
        panel_solve_tiles(&sh.blk.S[kq][lc], acc, iv, tiles, [&](int s, const d4 &x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                qacc = fma(x[r], x[r], qacc);
                macc = fma(x[r], zr[s][r], macc);
            }
        });
        qacc += __shfl_xor(qacc, 16);
        qacc += __shfl_xor(qacc, 32);
        macc += __shfl_xor(macc, 16);
        macc += __shfl_xor(macc, 32);

        // ---- the pair's term (constrained_acq_kernel's, model by model)
        AcqParams ap;
        ap.variance = st.variance; ap.noise_var = st.noise_var; ap.cost = 1.0;
        ap.include_noise = 1; ap.want_ei = 1;
        double mean, var;
        if (p == p0) {
            ap.y_best = st.y_best; ap.ei_jitter = st.ei_jitter; ap.task = st.task;
            posterior_of(qacc, macc, cpm_c, cpv_c, st.sv != nullptr, ap, mean, var);
            run = acquisition_of(mean, var, ap);                  // cbo_acq_sweep's acq at cost 1
        } else {
            ap.y_best = 0.0; ap.ei_jitter = 0.0; ap.task = CBO_TASK_MIN;
            posterior_of(qacc, macc, cpm_c, cpv_c, st.sv != nullptr, ap, mean, var);
            run = run * feasibility_of(mean, var, st.y_best, st.ei_jitter, st.task);
        }
    }
    if (p1 - p0 == 1) {
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
    wave_argmax(bv, bi);
    double *red_v = &sh.sq[0];                         // free after the barrier below
    int64_t *red_i = reinterpret_cast<int64_t *>(&sh.sv[0]);
    __syncthreads();
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (better(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
    }
    small_set_finish(bv, bi, set, slot, blocks_per_set, part_val, part_idx, info, ticket, out, seq, &last_flag);
}

template <bool BYVAL>
static void launch_small_sets_con_as(hipStream_t s, const SmallSetArgs &args, const cbo_small_set *pairs, int n_pairs,
                                     int n_sets, int max_pairs, int blocks_per_set, double *scratch, double *part_val,
                                     int64_t *part_idx, int *info, int *ticket, cbo_small_result *out, int seq)
{
    // the whole CU's LDS: once per device and instantiation, as launch_small_sets has it
    {
        static std::atomic<unsigned long long> opted{0};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || !((opted.load(std::memory_order_relaxed) >> (dev & 63)) & 1ull)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(small_sets_con_kernel<BYVAL>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SmallShared)) == hipSuccess)
                opted.fetch_or(1ull << (dev & 63), std::memory_order_relaxed);
        }
    }
    auto launch = [&](const dim3 &g, int phases) {
        hipLaunchKernelGGL((small_sets_con_kernel<BYVAL>), g, dim3(256), sizeof(SmallShared), s, args, pairs, n_pairs, scratch,
                           blocks_per_set, part_val, part_idx, info, ticket, out, seq, phases);
    };
    if (blocks_per_set >= kTwoPhaseFromBlocks) {
        launch(dim3((unsigned)max_pairs, (unsigned)n_sets), 1);
        launch(dim3((unsigned)blocks_per_set, (unsigned)n_sets), 2);
    } else {
        launch(dim3((unsigned)blocks_per_set, (unsigned)n_sets), 3);
    }
}

// launch_small_sets for the constrained epilogue (cbo_internal.h)
void launch_small_sets_con(hipStream_t s, const cbo_small_set *pairs, int n_pairs, int n_sets, int max_pairs,
                           int blocks_per_set, double *scratch, double *part_val, int64_t *part_idx, int *info, int *ticket,
                           cbo_small_result *out, int seq)
{
    SmallSetArgs args{};
    if (n_pairs <= kSmallByValue) {
        std::memcpy(args.s, pairs, sizeof(cbo_small_set) * (size_t)n_pairs);
        launch_small_sets_con_as<true>(s, args, pairs, n_pairs, n_sets, max_pairs, blocks_per_set, scratch, part_val, part_idx,
                                       info, ticket, out, seq);
    } else {
        launch_small_sets_con_as<false>(s, args, pairs, n_pairs, n_sets, max_pairs, blocks_per_set, scratch, part_val,
                                        part_idx, info, ticket, out, seq);
    }
}

}  // namespace cbo

// Greedy batch selection inside the one-launch multi-set sweep for gfx950: small_sets_batch_kernel,
// cbo_acq_sweep_sets_batch -- batch_size Kriging-believer picks (§4g) for every exploration set of a trial in ONE launch.
// small_sets_kernel's grid, one- / two-launch split, descriptor and stage sequence (cbo_small_device.h), with two additions:
//   * a workgroup of 64 candidates also leaves its columns of V = L^-1 K* (the tiles the solve emits), its q and its mu in
//     the set's global scratch, and publishes them with its ticket (agent-scope release);
//   * the set's last workgroup to arrive (agent-scope acquire) does not stop at the reduction of pick 0: it runs picks
//     1 .. batch_size - 1 for the whole set, all 256 threads, one candidate per thread and round -- the pivot column and the
//     pick's scalars in LDS (SmallShared is dead by then), the pass over V, the final stage, EI / cost on the updated q,
//     the arg-max over all m candidates.  The arithmetic of a pick is cbo_device.h's (batch_*), which the general path's
//     three kernels call too: per set the picks are cbo_acq_sweep_batch's, bit for bit.
// Nothing waits for another workgroup: the ticket is the only dependency.
// LOG (cbo_acq_sweep_sets_batch_logei): the same picks scored by log EI - log cost (log_ei_of, st.ei_jitter
// being the log EI's jitter) -- finite and ordered where the EI of every pick is an exact 0.  Only the two epilogues differ.
#include <cstring>

#include "cbo_small_device.h"

#pragma clang fp contract(off)

namespace cbo {

// the last arriver's LDS: lives where SmallShared did
struct SmallBatchShared {
    double col[128];                   // the pivot column V[:, p]
    double wp[CBO_MAX_BATCH];          // W[s][p] of the earlier fantasy rows
    double x[CBO_MAX_DIM], sq, sv;     // the believed point
    double d, y_best;                  // its d; the incumbent (moves with update_incumbent)
    double red_v[4];
    int64_t red_i[4];
    double win_v;                      // the previous pick's winner, for every thread
    int64_t win_i;
    int status;
};
static_assert(sizeof(SmallBatchShared) <= sizeof(SmallShared), "the last arriver's state lives in the dead SmallShared");
static_assert(sizeof(SmallShared) + sizeof(int) <= 163840, "the workgroup's static LDS (the ticket flag) beside SmallShared: one CU");

// The log form's score of one candidate: log_ei_of, kept out of line -- log_h_of's three ranges inlined twice into a kernel
// that already holds the factor's registers would spill.  pointwise_acq_kernel<kLogEiKind>'s bits.
__device__ __attribute__((noinline)) double batch_log_ei(double mean, double var, double y_best, double jitter, int task,
                                                         double log_cost)
{
    AcqParams p{};
    p.y_best = y_best; p.ei_jitter = jitter; p.task = task;
    return log_ei_of(mean, var, p, log_cost);
}

// Picks 1 .. B - 1 of one set by its last workgroup; (bv, bi) = pick 0's winner in every thread on entry.  V, W, q, mu: the
// set's scratch (row stride mp); hv, hi: the set's slots 1.. of the winners array (thread 0 stores).  log_cost: log(st.cost),
// read by the log form alone.
template <int D, bool LOG>
__device__ __forceinline__ void small_batch_picks(SmallBatchShared &bs, const cbo_small_set &st, const SmallBatchArgs &ba,
                                                  const double *V, double *W, double *q, const double *mu, double *hv,
                                                  int64_t *hi, double bv, int64_t bi, [[maybe_unused]] double log_cost)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t mp = ba.m_pad;
    const int n = st.n;
    const int m = (int)st.m;
    const bool causal = st.sv != nullptr;
    const int slices = batch_slice_count(n);
    const int rps = batch_rows_per_slice(n, slices);
    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    AcqParams p = small_acq_params(st);
    for (int t = 1; t < ba.batch_size; ++t) {
        // ---- pivot: column p of V, W_sp of the earlier rows, d, the believed point, the moved incumbent
        int64_t pv_i = bi - st.index_offset;
        if (pv_i < 0 || pv_i >= m) pv_i = 0;                           // (cannot happen: m >= 1 and an index always wins)
        const int pc = (int)pv_i;
        if (tid < n) bs.col[tid] = V[(int64_t)tid * mp + pc];
        if (tid >= 128 && tid - 128 < t - 1) bs.wp[tid - 128] = W[(int64_t)(tid - 128) * mp + pc];
        if (tid == 255) {
            if (t == 1) bs.y_best = st.y_best;
            bs.d = batch_believer_sd(st.variance, causal ? st.cpv[pc] : 0.0, causal, q[pc], st.noise_var);
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k) bs.x[k] = (k < D) ? st.cxs[(int64_t)k * st.cld + pc] : 0.0;
            bs.sq = st.csq[pc];
            bs.sv = (causal && st.csv) ? st.csv[pc] : 0.0;
            if (ba.update_incumbent)
                bs.y_best = batch_moved_incumbent(bs.y_best, mu[pc], causal ? st.cpm[pc] : 0.0, causal, st.task);
        }
        __syncthreads();
        p.y_best = bs.y_best;
        double xp[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xp[k] = bs.x[k];
        const double sqp = bs.sq, svp = bs.sv, dd = bs.d;
        double *wrow = W + (int64_t)(t - 1) * mp;
        bv = -INFINITY;
        bi = INT64_MAX;
        for (int j = tid; j < m; j += 256) {
            // ---- pass: the slices' sums of V_ip V_ij, rows in order on one chain per slice (eight loads ahead of their use)
            auto slice_sum = [&](int i0) {
                const int i1 = (i0 + rps < n) ? i0 + rps : n;
                const double *vp = V + (int64_t)i0 * mp + j;
                double s = 0.0;
                int i = i0;
                for (; i + 8 <= i1; i += 8) {
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = vp[(int64_t)(i - i0 + u) * mp];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s = batch_pass_step(bs.col[i + u], v[u], s);
                }
                for (; i < i1; ++i) s = batch_pass_step(bs.col[i], vp[(int64_t)(i - i0) * mp], s);
                return s;
            };
            const double part0 = slice_sum(0);
            const double part1 = (slices > 1) ? slice_sum(rps) : 0.0;  // (n <= 128: two slices at the most)
            // ---- final stage: the W correction, k(x_p, x_j), the division, q and row t - 1 of W
            double xj[D];
#pragma unroll
            for (int k = 0; k < D; ++k) xj[k] = st.cxs[(int64_t)k * st.cld + j];
            const double w = batch_fantasy_weight<D>(
                slices, [&](int r) { return r == 0 ? part0 : part1; }, t - 1, bs.wp, [&](int r) { return W[(int64_t)r * mp + j]; }, xp, xj,
                sqp, st.csq[j], causal && st.csv != nullptr, svp, (causal && st.csv) ? st.csv[j] : 0.0, st.variance, inv_l2,
                dd);
            wrow[j] = w;
            const double qn = batch_q_update(w, q[j]);
            q[j] = qn;
            // ---- epilogue on the updated q
            double mean, var;
            posterior_of(qn, mu[j], causal ? st.cpm[j] : 0.0, causal ? st.cpv[j] : 0.0, causal, p, mean, var);
            double a;
            if constexpr (LOG) a = batch_log_ei(mean, var, p.y_best, p.ei_jitter, p.task, log_cost);
            else a = acquisition_of(mean, var, p);
            const int64_t aj = (int64_t)j + st.index_offset;
            if (better(a, aj, bv, bi)) { bv = a; bi = aj; }
        }
        // ---- arg-max over the set
        wave_argmax(bv, bi);
        if (lane == 0) { bs.red_v[wave] = bv; bs.red_i[wave] = bi; }
        // q and W of this pick are read by the next one's pivot, through other threads
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (better(bs.red_v[w], bs.red_i[w], bv, bi)) { bv = bs.red_v[w]; bi = bs.red_i[w]; }
            hv[t] = bv;
            hi[t] = bi;
            bs.win_v = bv;
            bs.win_i = bi;
        }
        __syncthreads();
        bv = bs.win_v;
        bi = bs.win_i;
    }
}

// phases as small_sets_kernel's.  ba: the call's scratch, m_pad = 64 blocks_per_set columns per row for every set.
template <bool BYVAL, bool LOG>
__global__ __launch_bounds__(256) void small_sets_batch_kernel(const SmallSetArgs byval, const cbo_small_set *__restrict__ sets,
                                                               double *scratch, int blocks_per_set, double *part_val,
                                                               int64_t *part_idx, int *__restrict__ info,
                                                               int *__restrict__ ticket, cbo_small_result *__restrict__ out,
                                                               int seq, int phases, const SmallBatchArgs ba)
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
    const int64_t mp = ba.m_pad;
    double *Vs = ba.V + (int64_t)set * 128 * mp;
    double *Ws = ba.W + (int64_t)set * (ba.batch_size - 1) * mp;
    double *qs = ba.q + (int64_t)set * mp, *mus = ba.mu + (int64_t)set * mp;

    [[maybe_unused]] const double log_cost = LOG ? log(st.cost) : 0.0;   // (uniform: once per set)
    double bv = -INFINITY;
    int64_t bi = INT64_MAX;
    if ((int64_t)blk * 64 < st.m) {                               // (uniform) a workgroup with candidates
        const int tiles = (st.n + 15) / 16;
        double *my = scratch + (int64_t)(phases == 2 ? set * blocks_per_set : slot) * kSmallScratch;
        double *Us = my, *invs = my + 128 * kSmallLd;
        const int64_t c = (int64_t)blk * 64 + wave * 16 + lc;
        double xc[CBO_MAX_DIM], csq, csv, cpm_c, cpv_c;
        small_fetch_cand(st, c, xc, csq, csv, cpm_c, cpv_c);
        double iv[8][4], zr[8][4];
        small_model_factor(sh, st, tiles, Us, invs, &info[set], iv, zr, phases, true);
        const AcqParams p = small_acq_params(st);
        const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
        d4 acc[8];
        small_kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        double qacc, macc;
        const bool mine = c < st.m;                               // (c < 64 blocks_per_set = mp: every store is inside the row)
        double *vcol = Vs + c;
        const int n = st.n;
        solve_q_mu_keep(sh, acc, iv, zr, tiles, kq, lc, qacc, macc, [&](int s, const d4 &x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * s + kq + 4 * r;
                if (mine && row < n) vcol[(int64_t)row * mp] = x[r];
            }
        });
        if (kq == 0 && mine) {
            qs[c] = qacc;
            mus[c] = macc;
            double mean, var;
            posterior_of(qacc, macc, cpm_c, cpv_c, st.sv != nullptr, p, mean, var);
            if constexpr (LOG) bv = batch_log_ei(mean, var, p.y_best, p.ei_jitter, p.task, log_cost);
            else bv = acquisition_of(mean, var, p);
            bi = c + st.index_offset;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's V, q, mu have left (the barriers follow)
        small_block_argmax(sh, lane, wave, bv, bi);
    }
    if (!small_set_ticket<true>(bv, bi, set, slot, blocks_per_set, part_val, part_idx, ticket, &last_flag)) return;

    // ---- the set's last workgroup: acquire what the others published, reduce pick 0, run the further picks
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    SmallBatchShared &bs = *reinterpret_cast<SmallBatchShared *>(smem_raw);
    double *hv = ba.h_vals + (int64_t)set * ba.batch_size;
    int64_t *hi = ba.h_idxs + (int64_t)set * ba.batch_size;
    int status = 0;
    if (tid < 64) {
        small_set_reduce(set, blocks_per_set, part_val, part_idx, info, bv, bi, status);
        if (tid == 0) {
            bs.win_v = bv;
            bs.win_i = bi;
            bs.status = status;
            hv[0] = bv;
            hi[0] = bi;
        }
    }
    __syncthreads();
    const double v0 = bs.win_v;
    const int64_t i0 = bs.win_i;
    status = bs.status;
    __syncthreads();
    if (status == 0) {                                            // (uniform) else: the general path, from the host
        CBO_FOR_DIM(st.d, (small_batch_picks<D, LOG>(bs, st, ba, Vs, Ws, qs, mus, hv, hi, v0, i0, log_cost)));
    }
    if (tid == 0) small_set_record(v0, i0, status, set, info, ticket, out, seq);   // (after thread 0's winners)
}

size_t small_sets_batch_doubles(int n_sets, int blocks_per_set, int batch_size)
{
    return (size_t)n_sets * (size_t)(128 + (batch_size - 1) + 2) * (size_t)(64 * blocks_per_set);
}

template <bool BYVAL, bool LOG>
static void launch_small_sets_batch_as(hipStream_t s, const SmallSetArgs &args, const cbo_small_set *sets, int n_sets,
                                       int blocks_per_set, double *scratch, double *part_val, int64_t *part_idx, int *info,
                                       int *ticket, cbo_small_result *out, int seq, const SmallBatchArgs &ba)
{
    static std::atomic<unsigned long long> opted{0};
    small_lds_opt_in(reinterpret_cast<const void *>(small_sets_batch_kernel<BYVAL, LOG>), opted);
    const dim3 grid((unsigned)blocks_per_set, (unsigned)n_sets);
    auto launch = [&](const dim3 &g, int phases) {
        hipLaunchKernelGGL((small_sets_batch_kernel<BYVAL, LOG>), g, dim3(256), sizeof(SmallShared), s, args, sets, scratch,
                           blocks_per_set, part_val, part_idx, info, ticket, out, seq, phases, ba);
    };
    if (blocks_per_set >= kSmallTwoPhaseFromBlocks) {
        launch(dim3(1u, (unsigned)n_sets), 1);
        launch(grid, 2);
    } else {
        launch(grid, 3);
    }
}

void launch_small_sets_batch(hipStream_t s, const cbo_small_set *sets, int n_sets, int blocks_per_set, const SmallLaunch &L,
                             double *batch_scratch, int batch_size, int update_incumbent, double *h_vals, int64_t *h_idxs,
                             bool log_form)
{
    SmallBatchArgs ba;
    const size_t mp = (size_t)64 * (size_t)blocks_per_set, ns = (size_t)n_sets;
    ba.m_pad = (int64_t)mp;
    ba.V = batch_scratch;
    ba.W = ba.V + ns * 128 * mp;
    ba.q = ba.W + ns * (size_t)(batch_size - 1) * mp;
    ba.mu = ba.q + ns * mp;
    ba.h_vals = h_vals; ba.h_idxs = h_idxs;
    ba.batch_size = batch_size; ba.update_incumbent = update_incumbent;
    SmallSetArgs args{};
    const bool byval = n_sets <= kSmallByValue;
    if (byval) std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_sets);
    auto launch = byval ? (log_form ? launch_small_sets_batch_as<true, true> : launch_small_sets_batch_as<true, false>)
                        : (log_form ? launch_small_sets_batch_as<false, true> : launch_small_sets_batch_as<false, false>);
    launch(s, args, sets, n_sets, blocks_per_set, L.scratch, L.part_val, L.part_idx, L.info, L.ticket, L.out, L.seq, ba);
}

}  // namespace cbo

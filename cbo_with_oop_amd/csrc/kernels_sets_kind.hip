// Point-wise acquisitions in the one-launch multi-set sweep for gfx950: small_sets_kernel's sibling
// (kernels_chol.hip) for the lower / upper confidence bound, the probability of improvement, the model variance and the
// mean-plug-in Expected Improvement.  One workgroup does everything for (one set, 64 candidates) inside LDS and registers,
// from the same device functions as the EI kernel (cbo_small_device.h, cbo_device.h): the same grid, the same one- / two-
// launch split, the same descriptors, the same staged data of a trial step, the same result record.  Only the epilogue
// differs: pointwise_of<KIND> (kernels_pointwise.hip's, so cbo_acq_sweep_kind's bits) in the place of acquisition_of --
// and, for the plug-in EI, the incumbent first: the model's own points run as candidates through the factor the workgroup
// already holds.  The EI kernel itself is not touched: its code object does not move.
#include <atomic>
#include <cstring>

#include "cbo_small_device.h"

#pragma clang fp contract(off)

namespace cbo {

static_assert(sizeof(SmallShared) + 128 * sizeof(double) + 4 * sizeof(double) + 4 * sizeof(int) + sizeof(double) +
                      sizeof(int) <= 163840,
              "the workgroup's static LDS (plug-in means, their reduction, the ticket flag) beside SmallShared: one CU");

__device__ __forceinline__ void kstar_tiles_of(const SmallShared &sh, const cbo_small_set &st, int tiles, const double *xc,
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

// V = L^-1 K* of one wave's 16 candidates, q = sum V^2, mu = V^T z: lane partials, then over the four lane groups (the strip
// kernel's order, as small_sets_kernel has it)
__device__ __forceinline__ void solve_q_mu(const SmallShared &sh, d4 (&acc)[8], const double (&iv)[8][4],
                                           const double (&zr)[8][4], int tiles, int kq, int lc, double &qacc, double &macc)
{
    qacc = 0.0;
    macc = 0.0;
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
}

// The plug-in incumbent of the workgroup's model: min (task 'min') or max of the posterior means at the model's own n <= 128
// points, NaN if any of them is.  The points are already in LDS in candidate layout (xs, sq, sv); they go through K*, the tile
// solve and posterior_of (noise included) as candidates do, one 16-point tile per wave and round (two rounds at most), and
// the means through plugin_incumbent_kernel's reduction, operation for operation (kernels_pointwise.hip: lane i holds
// point i, the waves' shuffle tree, then thread 0 over the waves), so that even a tie between zeros of either sign falls as it
// does there.  The factor must be in LDS (the caller has waited and synchronised); every thread returns the incumbent.
// `fresh`: the set's new data are still in the staging buffer (a trial step's one-launch form): the prior closures at the
// points are read from there, since the resident copies are being written by the set's first workgroup meanwhile.
__device__ __forceinline__ double small_plugin_incumbent(const SmallShared &sh, const cbo_small_set &st, int tiles,
                                                         const double (&iv)[8][4], const double (&zr)[8][4],
                                                         const AcqParams &p, bool fresh, double *mean_s, double *red_v,
                                                         int *red_n, double *out_s)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    const bool causal = st.sv != nullptr;
    const double *pmsrc = !causal ? nullptr : fresh ? st.stage + (int64_t)st.n * st.d + st.n : st.pm;
    const double *pvsrc = !causal ? nullptr : fresh ? st.stage + (int64_t)st.n * st.d + 2 * (int64_t)st.n : st.pv;
    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    for (int t = wave; t < tiles; t += 4) {                        // (uniform per wave)
        const int row = 16 * t + lc;
        const int rr = (row < st.n) ? row : st.n - 1;              // clamped: lanes beyond the model compute, nobody looks
        double xc[CBO_MAX_DIM];
#pragma unroll
        for (int k = 0; k < CBO_MAX_DIM; ++k) xc[k] = (k < st.d) ? sh.xs[k][rr] : 0.0;
        const double csq = sh.sq[rr], csv = sh.sv[rr];
        const double pm_c = pmsrc ? pmsrc[rr] : 0.0, pv_c = pvsrc ? pvsrc[rr] : 0.0;
        d4 acc[8];
        kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
        double qacc, macc;
        solve_q_mu(sh, acc, iv, zr, tiles, kq, lc, qacc, macc);
        if (kq == 0 && row < st.n) {
            double mean, var;
            posterior_of(qacc, macc, pm_c, pv_c, causal, p, mean, var);
            mean_s[row] = mean;
        }
    }
    __syncthreads();
    const bool is_min = st.task == CBO_TASK_MIN;                   // (uniform)
    double best = is_min ? INFINITY : -INFINITY;
    int nan = 0;
    if (tid < st.n) {
        const double v = mean_s[tid];
        nan |= isnan(v) ? 1 : 0;
        if (is_min ? v < best : v > best) best = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(best, off);
        nan |= __shfl_down(nan, off);
        if (is_min ? ov < best : ov > best) best = ov;
    }
    if (lane == 0) { red_v[wave] = best; red_n[wave] = nan; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            nan |= red_n[w];
            if (is_min ? red_v[w] < best : red_v[w] > best) best = red_v[w];
        }
        *out_s = nan ? __builtin_nan("") : best;
    }
    __syncthreads();
    return *out_s;
}

// KIND: CBO_ACQ_LCB, _PI, _VAR or _MPEI (compile time: one kind's arithmetic per instantiation).  The descriptor's ei_jitter
// carries the kind's parameter (beta; PI's and the plug-in EI's jitter), y_best PI's incumbent.  Everything up to the epilogue
// is small_sets_kernel's sequence (its comments say why).
template <int KIND, bool BYVAL>
__global__ __launch_bounds__(256) void small_sets_kind_kernel(const SmallSetArgs byval,
                                                              const cbo_small_set *__restrict__ sets, double *scratch,
                                                              int blocks_per_set, double *__restrict__ part_val,
                                                              int64_t *__restrict__ part_idx, int *__restrict__ info,
                                                              int *__restrict__ ticket, cbo_small_result *__restrict__ out,
                                                              int seq, int phases)
{
    __shared__ int last_flag;
    __shared__ double plug_mean[128], plug_red[4], plug_out;
    __shared__ int plug_nan[4];
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    const int set = blockIdx.y, blk = blockIdx.x;
    const cbo_small_set st = BYVAL ? byval.s[set] : sets[set];
    const int slot = set * blocks_per_set + blk;
    if (phases == 1) {                                            // one workgroup per set: factor it, nothing else
        double ivx[8][4], zrx[8][4];
        double *fs = scratch + (int64_t)(set * blocks_per_set) * kSmallScratch;
        small_model_factor(sh, st, (st.n + 15) / 16, fs, fs + 128 * kSmallLd, &info[set], ivx, zrx, 1, true);
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

    // this wave's 16 candidates: fetched now, used after the factorisation (their latency is off the chain)
    const int64_t c = (int64_t)blk * 64 + wave * 16 + lc;
    const int64_t cc = (c < st.m) ? c : st.m - 1;                  // clamped: lanes beyond the set compute, nobody looks
    double xc[CBO_MAX_DIM];
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) xc[k] = (k < st.d) ? st.cxs[(int64_t)k * st.cld + cc] : 0.0;
    const double csq = st.csq[cc], csv = st.csv ? st.csv[cc] : 0.0;
    const double cpm_c = st.cpm ? st.cpm[cc] : 0.0, cpv_c = st.cpv ? st.cpv[cc] : 0.0;

    double iv[8][4], zr[8][4];
    small_model_factor(sh, st, tiles, Us, invs, &info[set], iv, zr, phases, true);

    AcqParams p;
    p.variance = st.variance; p.noise_var = st.noise_var; p.y_best = st.y_best; p.ei_jitter = st.ei_jitter;
    p.cost = st.cost; p.task = st.task; p.include_noise = 1; p.want_ei = 1;
    if (KIND == CBO_ACQ_MPEI) {
        // the incumbent of every candidate of the set: from the factor, before this workgroup's own candidates
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        p.y_best = small_plugin_incumbent(sh, st, tiles, iv, zr, p, st.stage != nullptr && (phases & 1), plug_mean, plug_red,
                                          plug_nan, &plug_out);
    }

    // ---- K(X, X*) of this wave's 16 candidates, straight into the result layout
    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    d4 acc[8];
    kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
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
        bv = (KIND == CBO_ACQ_MPEI) ? acquisition_of(mean, var, p) : pointwise_of<KIND>(mean, var, p);
        bi = c + st.index_offset;
    }
    wave_argmax(bv, bi);
    double *red_v = &sh.sq[0];                         // free by now
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

template <int KIND, bool BYVAL>
static void launch_small_sets_kind_as(hipStream_t s, const SmallSetArgs &args, const cbo_small_set *sets, int n_sets,
                                      int blocks_per_set, double *scratch, double *part_val, int64_t *part_idx, int *info,
                                      int *ticket, cbo_small_result *out, int seq)
{
    // the whole CU's LDS: once per device and instantiation, as launch_small_sets has it
    {
        static std::atomic<unsigned long long> opted{0};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || !((opted.load(std::memory_order_relaxed) >> (dev & 63)) & 1ull)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(small_sets_kind_kernel<KIND, BYVAL>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SmallShared)) == hipSuccess)
                opted.fetch_or(1ull << (dev & 63), std::memory_order_relaxed);
        }
    }
    const dim3 grid((unsigned)blocks_per_set, (unsigned)n_sets);
    constexpr int kTwoPhaseFromBlocks = 12;                       // launch_small_sets' split (kernels_chol.hip)
    auto launch = [&](const dim3 &g, int phases) {
        hipLaunchKernelGGL((small_sets_kind_kernel<KIND, BYVAL>), g, dim3(256), sizeof(SmallShared), s, args, sets, scratch,
                           blocks_per_set, part_val, part_idx, info, ticket, out, seq, phases);
    };
    if (blocks_per_set >= kTwoPhaseFromBlocks) {
        launch(dim3(1u, (unsigned)n_sets), 1);
        launch(grid, 2);
    } else {
        launch(grid, 3);
    }
}

// launch_small_sets for the kind's epilogue: the same arguments and conditions (cbo_internal.h)
void launch_small_sets_kind(hipStream_t s, int kind, const cbo_small_set *sets, int n_sets, int blocks_per_set,
                            double *scratch, double *part_val, int64_t *part_idx, int *info, int *ticket,
                            cbo_small_result *out, int seq)
{
    SmallSetArgs args{};
    const bool byval = n_sets <= kSmallByValue;
    if (byval) std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_sets);
#define CBO_LAUNCH_KIND(K)                                                                                              \
    (byval ? launch_small_sets_kind_as<K, true>(s, args, sets, n_sets, blocks_per_set, scratch, part_val, part_idx, info, \
                                                ticket, out, seq)                                                       \
           : launch_small_sets_kind_as<K, false>(s, args, sets, n_sets, blocks_per_set, scratch, part_val, part_idx,    \
                                                 info, ticket, out, seq))
    switch (kind) {
        case CBO_ACQ_LCB: CBO_LAUNCH_KIND(CBO_ACQ_LCB); break;
        case CBO_ACQ_PI: CBO_LAUNCH_KIND(CBO_ACQ_PI); break;
        case CBO_ACQ_VAR: CBO_LAUNCH_KIND(CBO_ACQ_VAR); break;
        default: CBO_LAUNCH_KIND(CBO_ACQ_MPEI); break;
    }
#undef CBO_LAUNCH_KIND
}

}  // namespace cbo

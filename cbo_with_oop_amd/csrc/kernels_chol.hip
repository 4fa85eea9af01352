// Blocked right-looking Cholesky  Ky = U^T U  (upper factor, row-major) for gfx950, with the forward
// solve z = L^-1 (y - m) carried along as an extra right-hand-side column, and the backward solve for
// alpha.
//
// Restates LAPACK dpotrf + dpotrs as reached by GPy's jitchol / dpotrs (GPy ExactGaussianInference;
// the reference builds that model at /root/reference/src/GaussianProcessFactory.py:57-73).  A
// non-positive (or NaN) pivot sets *info (first failing 1-based pivot index), which the host-side
// jitter ladder reads after the factorisation.
//
// Per 128-row panel (rows r0 = 128 k; panels go in pairs, launch_cholesky has the schedule):
//   1. potrf_panel_fused_kernel   diagonal block AND row panel in one launch: workgroup 0 factors the 128x128 block in
//                                 LDS (potrf_diag128_v2's device function: one wave runs the chain of 16x16 register
//                                 Choleskys, three waves solve the block's row panel and update its trailing tiles) and
//                                 publishes finished row tiles; the other workgroups are the panel's 64-column strips
//                                 and follow tile by tile.  Separate launches (CBO_HIP_PANEL_FORM=2):
//                                 potrf_diag128_v2_kernel + panel_trsm_kernel
//   2. syrk_rows_kernel           the next panel's (pair's) own rows  -= P^T P   (the piece of the update on the chain)
//   3. syrk_kernel<64> / trsm_update_kernel   the bulk of  A[below, below] -= P^T P  on a second stream (fp64 MFMA),
//                                 rhs -= P^T z  along with it
// The bulk update carries the n^3/3 flops; steps 1-2 are the serial chain.
// Also here: backsolve / forward-solve steps for single vectors, and the one-workgroup likelihood kernels for small models
// (small_lml_kernel: likelihood and gradients of one MLE iterate).  The one-workgroup sweeps are in kernels_sets.hip.
#include <hip/hip_ext.h>
#include <climits>
#include <atomic>
#include <cstring>
#include <vector>

#include "cbo_mid_lml_device.h"

namespace cbo {

__global__ __launch_bounds__(256) void potrf_diag128_v2_kernel(double *A, int64_t lda, int r0, int rcol,
                                                               double *__restrict__ invDt, int *info,
                                                               double *__restrict__ zvec)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Diag2Shared &sh = *reinterpret_cast<Diag2Shared *>(smem_raw);
    if (__builtin_nontemporal_load(info) != 0) return;      // an earlier block met a non-positive pivot: abandoned
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const unsigned s0 = lds_byte_address(&sh.S[0][0]);
        const double *g = A + (int64_t)(r0 + wave * 32) * lda + r0 + lane * 2;
#pragma unroll 8
        for (int p = 0; p < 32; ++p) {
            // only the upper triangle (by 16-column tiles) is read: lanes left of the row's diagonal tile load nothing
            if (lane >= 8 * ((wave * 32 + p) >> 4))
                glds16(g + (int64_t)p * lda, __builtin_amdgcn_readfirstlane(s0 + 8u * (unsigned)((wave * 32 + p) * kDiagLd)));
        }
    }
    if (tid < 128) {
        sh.S[tid][128] = A[(int64_t)(r0 + tid) * lda + rcol];
#pragma unroll
        for (int c = 129; c < kDiagLd; ++c) sh.S[tid][c] = 0.0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    diag128_factor_in_lds(sh, A, lda, r0, rcol, invDt, info, zvec, 8);
}

// ------------------------------------------------------------------------------------------------
// Row panel of the blocked factorisation, U[r0:r0+128, cols] = U_kk^-T A[r0:r0+128, cols]: the strip kernel's
// arithmetic for ONE 128-row block (same 16x16 diagonal inverses, same tile order), without its three-deep staging
// pipeline -- for 128 rows that pipeline is all prologue.  The whole diagonal block goes to LDS in one burst of
// LDS-DMA, the strip's right-hand sides and the eight inverses go to registers, then the eight tile steps run
// back to back: x_s = inv(L_ss) r_s (two half-sums), tile s+1 brought up to date first, and its own solve chain
// interleaved with the rest of tile s's updates so that the matrix pipe never waits for a dependent result.
// 64 columns per 256-thread workgroup, wave w owns 16 of them (no exchange between waves).
struct PanelShared {
    double U[128][kDiagLd];
};


__global__ __launch_bounds__(256) void panel_trsm_kernel(double *A, int64_t lda, int r0, int col0,
                                                         const double *__restrict__ invDt,
                                                         const int *__restrict__ skip_if)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    PanelShared &sh = *reinterpret_cast<PanelShared *>(smem_raw);
    if (__builtin_nontemporal_load(skip_if) != 0) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    {
        const unsigned s0 = lds_byte_address(&sh.U[0][0]);
        const double *g = A + (int64_t)(r0 + wave * 32) * lda + r0 + lane * 2;
#pragma unroll 8
        for (int p = 0; p < 32; ++p) {
            if (lane >= 8 * ((wave * 32 + p) >> 4))          // upper triangle only (by 16-column tiles)
                glds16(g + (int64_t)p * lda, __builtin_amdgcn_readfirstlane(s0 + 8u * (unsigned)((wave * 32 + p) * kDiagLd)));
        }
    }
    double *Ac = A + (int64_t)r0 * lda + col0 + (int64_t)blockIdx.x * kStrip + wave * 16 + lc;
    d4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = Ac[(int64_t)(16 * t + kq + 4 * r) * lda];
    double iv[8][4];
    const double *inv = invDt + (int64_t)(r0 / 16) * 256 + kq * 16 + lc;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) iv[s][kk] = inv[s * 256 + 64 * kk];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    panel_solve_tiles(&sh.U[kq][lc], acc, iv, 8, [&](int s, const d4 &x) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Ac[(int64_t)(16 * s + kq + 4 * r) * lda] = x[r];
    });
}

// ------------------------------------------------------------------------------------------------
// Diagonal block AND its row panel in one launch (a small cooperative group: nothing waits on a grid-wide barrier).
// Workgroup 0 is the diagonal-block kernel above, publishing: its factor stores are written through to the device's
// coherence point and every worker wave counts itself in at `flag` after its last store of an interval, so row tile s
// of the block (the inverse of its diagonal tile and U[s][s+1..7]) is complete when the count reaches 3 (s + 1).
// Workgroups 1.. are the panel's 64-column strips; each wave owns 16 columns, keeps its 128 x 16 right-hand sides in
// registers and follows the block tile by tile: wait for row tile s, read it (coherent loads, straight into MFMA
// operand registers: no LDS, no barrier, the four waves are independent), x_s = inv(L_ss) r_s, fold it into the
// tiles below.  The panel solve thus hides behind the 128 pivots of the block; what is left after the block's last
// interval is one round trip and a sixteenth of the work.  Same chains as panel_solve_tiles: same bits.
// Ordering.  Producer, per interval: write-through stores (agent-scope atomic stores: global_store sc1, performed at the
// device's coherence point), s_waitcnt vmcnt(0) (they have been performed), [a RELEASE fence at agent scope when built
// with -DCBO_FORMAL_RELEASE], the relaxed increment of the interval's count.  Consumer: relaxed polls of the counts;
// once a count covers what it needs, an ACQUIRE fence at agent scope, then its loads of that data (agent-scope atomic
// loads: never served from a stale line of this XCD's L2).  With the release fence, count increment and poll form the
// synchronises-with edge and the two fences extend it to the data: every store a wave made before counting itself in
// happens-before every load a strip makes after seeing that count -- the language-level argument.  Without it (the
// default, see AGENT_RELEASE above for what the fence costs) the producer side is a hardware-level argument: the
// stores were complete at the coherence point before the increment was issued, and the consumer's loads go to that
// same point, after its acquire.  The count invariant: a worker wave counts itself in once per interval after ALL its
// stores of the interval, and row tile s needs the three workers' interval-s stores, so "count >= 3 (s + 1)" means
// row tile s is complete (the inverse of diagonal tile s is one wave's store: its own count, flag[1]).
// Forward progress rests on an assumption about the hardware, not on the language: a dispatch hands out workgroups in
// order of their index and workgroup 0 never waits for a strip, so workgroup 0 is resident and running before any
// strip can spin.  The spin is bounded all the same (`spin_limit` polls, then the status word reports kFusedTimeout,
// the launch and everything after it in the factorisation drains) and the host then repeats the factorisation with the
// separate-launch kernels (CBO_HIP_PANEL_FORM=2's), same bits: cbo_gp_fit / cbo_gp_fit_sweep.
constexpr int kFusedTimeout = kCholFusedTimeout;

__device__ __forceinline__ double coherent_load(const double *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void potrf_panel_fused_kernel(double *A, int64_t lda, int r0, int rcol,
                                                                double *__restrict__ invDt, int *info,
                                                                double *__restrict__ zvec, int col0, int *flag,
                                                                int spin_limit, int strip_base)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    CHAIN_PRIORITY();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (__builtin_nontemporal_load(info) != 0) return;      // an earlier block met a non-positive pivot: abandoned
    // strip_base == 1: workgroup 0 is the diagonal block, workgroups 1.. the strips (one launch); strip_base == 0: a
    // launch of strips only (no LDS at all), behind a one-workgroup launch of the block (the split form, see launch_panel_fused)
    if (strip_base == 1 && blockIdx.x == 0) {
        Diag2Shared &sh = *reinterpret_cast<Diag2Shared *>(smem_raw);
        {
            const unsigned s0 = lds_byte_address(&sh.S[0][0]);
            const double *g = A + (int64_t)(r0 + wave * 32) * lda + r0 + lane * 2;
#pragma unroll 8
            for (int p = 0; p < 32; ++p) {
                if (lane >= 8 * ((wave * 32 + p) >> 4))
                    glds16(g + (int64_t)p * lda, __builtin_amdgcn_readfirstlane(s0 + 8u * (unsigned)((wave * 32 + p) * kDiagLd)));
            }
        }
        if (tid < 128) {
            sh.S[tid][128] = A[(int64_t)(r0 + tid) * lda + rcol];
#pragma unroll
            for (int c = 129; c < kDiagLd; ++c) sh.S[tid][c] = 0.0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        diag128_factor_in_lds<true>(sh, A, lda, r0, rcol, invDt, info, zvec, 8, flag);
        return;
    }
    // ---- a strip: 16 columns per wave
    const int lc = lane & 15, kq = lane >> 4;
    double *Ac = A + (int64_t)r0 * lda + col0 + (int64_t)((int)blockIdx.x - strip_base) * kStrip + wave * 16 + lc;
    d4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = Ac[(int64_t)(16 * t + kq + 4 * r) * lda];
    const double *inv = invDt + (int64_t)(r0 / 16) * 256 + kq * 16 + lc;
    const double *Ub = A + (int64_t)(r0 + kq) * lda + r0 + lc;           // U[kq][lc] of the block
    // flag[0] / 3 = row tiles of the block that are complete, flag[1] = diagonal-tile inverses that are out (inverse s
    // precedes row tile s by most of an interval: x_s does not wait for the row, and the last step needs no row at all)
    int rows_seen = 0, invs_seen = 0;
    // one poll refreshes both counts (the two words share a cache line: one round trip)
    auto wait_for = [&](bool want_row, int s) -> bool {
        int spins = 0;
        if (spin_limit < 0) {                                            // test hook: every strip gives up at once
            if (lane == 0) atomicCAS(info, 0, kFusedTimeout);
            return false;
        }
        const bool polled = (want_row ? rows_seen : invs_seen) <= s;
        while ((want_row ? rows_seen : invs_seen) <= s) {
            const int f0 = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int f1 = __hip_atomic_load(flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rows_seen = f0 / 3;
            invs_seen = f1;
            if ((want_row ? rows_seen : invs_seen) > s) break;
            if (++spins > spin_limit || __builtin_nontemporal_load(info) != 0) {
                if (spins > spin_limit && lane == 0) atomicCAS(info, 0, kFusedTimeout);
                return false;                                            // uniform: every lane read the same words
            }
            __builtin_amdgcn_s_sleep(2);
        }
        // what the counts cover is visible to the loads that follow (pairs with the producer's release fences)
        if (polled) AGENT_ACQUIRE();
        return true;
    };
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (!wait_for(false, s)) return;
        // a strip that runs behind the block already knows the row is there: its fragments travel with the inverse
        const bool have_row = s < 7 && rows_seen > s;
        double iv[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) iv[kk] = coherent_load(inv + s * 256 + 64 * kk);
        double ub[4][8];
        if (have_row) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int t = s + 1; t < 8; ++t) ub[kk][t] = coherent_load(Ub + (int64_t)(16 * s + 4 * kk) * lda + 16 * t);
        }
        d4 x = {0.0, 0.0, 0.0, 0.0}, x2 = {0.0, 0.0, 0.0, 0.0};
        x = MFMA_F64(iv[0], acc[s][0], x);
        x2 = MFMA_F64(iv[1], acc[s][1], x2);
        x = MFMA_F64(iv[2], acc[s][2], x);
        x2 = MFMA_F64(iv[3], acc[s][3], x2);
        x += x2;
#pragma unroll
        for (int r = 0; r < 4; ++r) Ac[(int64_t)(16 * s + kq + 4 * r) * lda] = x[r];
        if (s == 7) break;
        if (!have_row) {
            if (!wait_for(true, s)) return;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int t = s + 1; t < 8; ++t) ub[kk][t] = coherent_load(Ub + (int64_t)(16 * s + 4 * kk) * lda + 16 * t);
        }
        const d4 nx = -x;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int t = s + 1; t < 8; ++t) acc[t] = MFMA_F64(ub[kk][t], nx[kk], acc[t]);
    }
}

// split: the block as a one-workgroup launch (a whole CU's LDS), then the strips as a launch of their own that needs NO
// LDS: beside a device full of half-LDS update workgroups (the bulk trailing update of a large factorisation, a
// pipelined sweep) a strip workgroup then fits the slot any finishing update workgroup leaves, instead of waiting for
// a CU to drain completely -- 255 strips at 16384 points otherwise wait for the bulk update to end (profiles/r03b_*).
void launch_panel_fused(hipStream_t s, double *A, int64_t lda, int r0, int rcol, double *invDt, int *info, double *zvec,
                        int n_cols, int *flag, int spin_limit, hipEvent_t done = nullptr, bool split = false)
{
    if (!split) {
        hipExtLaunchKernelGGL(potrf_panel_fused_kernel, dim3(1u + (unsigned)(n_cols / kStrip)), dim3(256), sizeof(Diag2Shared),
                              s, nullptr, done, 0, A, lda, r0, rcol, invDt, info, zvec, r0 + 128, flag, spin_limit, 1);
        return;
    }
    hipLaunchKernelGGL(potrf_panel_fused_kernel, dim3(1u), dim3(256), sizeof(Diag2Shared), s, A, lda, r0, rcol, invDt, info,
                       zvec, r0 + 128, flag, spin_limit, 1);
    hipExtLaunchKernelGGL(potrf_panel_fused_kernel, dim3((unsigned)(n_cols / kStrip)), dim3(256), 0, s, nullptr, done, 0, A,
                          lda, r0, rcol, invDt, info, zvec, r0 + 128, flag, spin_limit, 0);
}

void launch_panel_trsm(hipStream_t s, double *A, int64_t lda, int r0, int col0, int n_cols, const double *invDt,
                       const int *skip_if, hipEvent_t done = nullptr)
{
    if (n_cols <= 0) { if (done) hipEventRecord(done, s); return; }
    hipExtLaunchKernelGGL(panel_trsm_kernel, dim3((unsigned)(n_cols / kStrip)), dim3(256), sizeof(PanelShared), s, nullptr,
                          done, 0, A, lda, r0, col0, invDt, skip_if);
}

// ------------------------------------------------------------------------------------------------
// Log marginal likelihood and its analytic gradients for a model of at most 128 observations -- what every iterate
// of the hyper-parameter MLE asks for (src/CBO.py:173 -> GPy model.optimize()) -- in ONE launch of one workgroup, the
// model not fitted beforehand:
//   K(X,X) + diag -> factorisation (as small_sets_kernel)          sum log diag(U), z^T z
//   V = L^-1 (identity right-hand sides through the same tile solve)  alpha = V^T z, diag(Ky^-1) = column sums of V^2
//   W = V^T V tile by tile on the matrix cores (V from the workgroup's scratch), each tile contracted at once with
//   the kernel and its lengthscale derivatives: the sums of lml_grad_tile_kernel (kernels_kmat.hip), GPy's quirk of
//   the causal term in the variance gradient included.
// The record goes to pinned host memory, closed by the call's sequence number (the host polls it).
// The body is shared by the one-model kernel and the batched one (one workgroup per model): same code, same bits.
template <int D>
__device__ __forceinline__ void small_lml_body(SmallShared &sh, double *alpha_s, double (*red)[kSmallLmlTerms],
                                               const cbo_small_set &st, double *scratch, int *__restrict__ info,
                                               cbo_small_lml_result *__restrict__ out, int seq)
{
    const int tid = threadIdx.x;
    const int tiles = (st.n + 15) / 16;
    double *Us = scratch, *invs = scratch + 128 * kSmallLd, *Vg = scratch + kSmallScratch;
    double iv[8][4], zr[8][4];
    small_model_factor(sh, st, tiles, Us, invs, info, iv, zr);
    if (tid < 128) alpha_s[tid] = 0.0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    small_lml_after_factor<D>(sh, alpha_s, red, st, Us, Vg, iv, zr);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kSmallLmlTerms; ++k) out->terms[k] = small_lml_term(red, k);
        out->info = atomicAdd(info, 0);
        __threadfence_system();
        *reinterpret_cast<volatile int *>(&out->seq) = seq;
        *info = 0;
    }
}

template <int D>
__global__ __launch_bounds__(256) void small_lml_kernel(const cbo_small_set st, double *scratch, int *__restrict__ info,
                                                        cbo_small_lml_result *__restrict__ out, int seq)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    __shared__ double alpha_s[128];
    __shared__ double red[4][kSmallLmlTerms];
    small_lml_body<D>(sh, alpha_s, red, st, scratch, info, out, seq);
}

constexpr size_t kSmallLmlScratch = (size_t)kSmallScratch + (size_t)128 * kSmallLd;
size_t small_lml_scratch_doubles() { return kSmallLmlScratch; }

// ------------------------------------------------------------------------------------------------
// The same outputs for a model of 128 < n <= 256 observations, still one workgroup and no fit, in two 128-row blocks: the
// stages of cbo_mid_lml_device.h on the model's resident points, whatever the info word says (the host reads it from the
// record), then the record.
template <int D>
__device__ __forceinline__ void mid_lml_body(SmallShared &sh, double (*red)[kSmallLmlTerms], const cbo_small_set &st,
                                             double *slab, int *__restrict__ info, cbo_small_lml_result *__restrict__ out,
                                             int seq)
{
    const int tid = threadIdx.x;
    mid_lml_stages<D, false>(sh, red, st, slab, info);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kSmallLmlTerms; ++k) out->terms[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        out->info = atomicAdd(info, 0);
        __threadfence_system();
        *reinterpret_cast<volatile int *>(&out->seq) = seq;
        *info = 0;
    }
}
size_t mid_lml_scratch_doubles() { return kMidLmlScratch; }

// Many independent models in ONE launch, one workgroup each (the graph-level GPs of an observe step, every one of them
// at its own L-BFGS iterate): model b reads descriptor b (by value up to kSmallByValue, else from the pinned array),
// uses scratch slot b (`stride` doubles each), status word info[b] and writes record out[b].  Models may differ in n
// (<= 256: above 128 the two-block form), d and ARD.
template <bool BYVAL>
__global__ __launch_bounds__(256) void small_lml_batch_kernel(const SmallSetArgs byval,
                                                              const cbo_small_set *__restrict__ sets, double *scratch,
                                                              int64_t stride, int *__restrict__ info,
                                                              cbo_small_lml_result *__restrict__ out, int seq)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    SmallShared &sh = *reinterpret_cast<SmallShared *>(smem_raw);
    __shared__ double alpha_s[128];
    __shared__ double red[4][kSmallLmlTerms];
    const int b = blockIdx.x;
    const cbo_small_set st = BYVAL ? byval.s[b] : sets[b];
    double *my = scratch + (int64_t)b * stride;
    if (st.n > 128) {                                               // 128 < n <= 256: the two-block form
        CBO_FOR_DIM(st.d, mid_lml_body<D>(sh, red, st, my, &info[b], &out[b], seq));
        return;
    }
    CBO_FOR_DIM(st.d, small_lml_body<D>(sh, alpha_s, red, st, my, &info[b], &out[b], seq));
}

void launch_small_lml_batch(hipStream_t s, const cbo_small_set *sets, int n_models, double *scratch, int64_t stride,
                            int *info, cbo_small_lml_result *out, int seq)
{
    {
        static std::atomic<unsigned long long> opted[2];
        const bool byval = n_models <= kSmallByValue;
        small_lds_opt_in(byval ? reinterpret_cast<const void *>(small_lml_batch_kernel<true>)
                               : reinterpret_cast<const void *>(small_lml_batch_kernel<false>), opted[byval]);
    }
    SmallSetArgs args{};
    if (n_models <= kSmallByValue) {
        std::memcpy(args.s, sets, sizeof(cbo_small_set) * (size_t)n_models);
        hipLaunchKernelGGL(small_lml_batch_kernel<true>, dim3((unsigned)n_models), dim3(256), sizeof(SmallShared), s, args,
                           sets, scratch, stride, info, out, seq);
    } else {
        hipLaunchKernelGGL(small_lml_batch_kernel<false>, dim3((unsigned)n_models), dim3(256), sizeof(SmallShared), s,
                           args, sets, scratch, stride, info, out, seq);
    }
}

void launch_small_lml(hipStream_t s, const cbo_small_set &st, double *scratch, int *info, cbo_small_lml_result *out, int seq)
{
    CBO_FOR_DIM(st.d,
                hipFuncSetAttribute(reinterpret_cast<const void *>(small_lml_kernel<D>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SmallShared));
                hipLaunchKernelGGL(small_lml_kernel<D>, dim3(1), dim3(256), sizeof(SmallShared), s, st, scratch, info, out,
                                   seq));
}

// ------------------------------------------------------------------------------------------------
// SYRK: C[i][j] -= sum_k P[k][i] P[k][j] on the upper tiles of the trailing block, P = the panel rows
// [r0, r0+n1).  TS x TS tile per workgroup, 2x2 waves, each wave (TS/2)^2 via 16x16x4 f64 MFMAs with
// both operand fragments read straight from the panel rows (4 row segments of 128 B per load).
// Extra blocks (blockIdx.x == nt) update the rhs column: r[i] -= sum_k P[k][i] z[k].
template <int TS>
__global__ __launch_bounds__(256) void syrk_kernel(double *A, int64_t lda, int r0, int n1, int c0, int nt, int rcol,
                                                   int ti_begin, const int *__restrict__ skip_if)
{
    if (__builtin_nontemporal_load(skip_if) != 0) return;
    const int tj = blockIdx.x, ti = blockIdx.y + ti_begin;
    const int tid = threadIdx.x;
    const double *P = A + (int64_t)r0 * lda;
    if (tj == nt) {
        // rhs column for the TS rows of tile ti
        constexpr int G = 256 / TS;
        __shared__ double part[256];
        const int i = tid % TS, g = tid / TS;
        const int64_t gi = c0 + (int64_t)ti * TS + i;
        // all loads of a 16-step batch are issued before the first use (L2 latency paid once per batch)
        double s = 0.0;
        for (int k0 = g; k0 < n1; k0 += 16 * G) {
            double pv[16], zv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int k = k0 + u * G;
                const bool ok = k < n1;
                pv[u] = ok ? P[(int64_t)k * lda + gi] : 0.0;
                zv[u] = ok ? P[(int64_t)k * lda + rcol] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) s = fma(pv[u], zv[u], s);
        }
        part[tid] = s;
        __syncthreads();
        if (g == 0) {
            double tot = 0.0;
#pragma unroll
            for (int gg = 0; gg < G; ++gg) tot += part[gg * TS + i];
            A[gi * lda + rcol] -= tot;
        }
        return;
    }
    if (tj < ti) return;
    constexpr int WT = TS / 2, MT = WT / 16;
    static_assert(MT == 2, "the 16-byte interleaved fragment map below is written for 32x32 wave tiles");
    const int lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    if (ti == tj && wr == 1 && wc == 0) return;      // strictly-lower quadrant of a diagonal tile
    const int64_t ib = c0 + (int64_t)ti * TS + wr * WT;
    const int64_t jb = c0 + (int64_t)tj * TS + wc * WT;
    // Interleaved tile map: MFMA tile (m, nn) of the wave's 32x32 block covers rows ib + 2i + m and columns
    // jb + 2j + nn, so one 16-byte load per lane yields the fragments of both m (resp. nn) and every access
    // to C is 16 bytes per lane as well.
    d4 acc[MT][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nn = 0; nn < MT; ++nn) acc[m][nn] = d4{0.0, 0.0, 0.0, 0.0};
    const double *Pa = P + (int64_t)kq * lda + ib + 2 * lc;
    const double *Pb = P + (int64_t)kq * lda + jb + 2 * lc;
    // software pipeline over chunks of CH k-steps: the fragments of chunk c+1 are in flight (L2 latency)
    // while the MFMAs of chunk c issue; n1 is a multiple of 4*CH at every call site (128-row panels)
    constexpr int CH = 4;
    d2 a[2][CH], b[2][CH];
    auto load_chunk = [&](int k0, d2 (&aa)[CH], d2 (&bb)[CH]) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < CH; ++ks) {
            aa[ks] = *reinterpret_cast<const d2 *>(&Pa[(int64_t)(k0 + 4 * ks) * lda]);
            bb[ks] = *reinterpret_cast<const d2 *>(&Pb[(int64_t)(k0 + 4 * ks) * lda]);
        }
    };
    auto mfma_chunk = [&](const d2 (&aa)[CH], const d2 (&bb)[CH]) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < CH; ++ks)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int nn = 0; nn < MT; ++nn) acc[m][nn] = MFMA_F64(aa[ks][m], bb[ks][nn], acc[m][nn]);
    };
    load_chunk(0, a[0], b[0]);
    // the C tile is fetched up front so that its (MALL/HBM) latency hides under the MFMAs
    d2 cv[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            cv[m][r] = *reinterpret_cast<const d2 *>(&A[(ib + 2 * (kq + 4 * r) + m) * lda + jb + 2 * lc]);
    for (int k0 = 0; k0 < n1; k0 += 8 * CH) {
        if (k0 + 4 * CH < n1) load_chunk(k0 + 4 * CH, a[1], b[1]);
        mfma_chunk(a[0], b[0]);
        if (k0 + 8 * CH < n1) load_chunk(k0 + 8 * CH, a[0], b[0]);
        if (k0 + 4 * CH < n1) mfma_chunk(a[1], b[1]);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            d2 o = cv[m][r];
            o[0] -= acc[m][0][r];
            o[1] -= acc[m][1][r];
            *reinterpret_cast<d2 *>(&A[(ib + 2 * (kq + 4 * r) + m) * lda + jb + 2 * lc]) = o;
        }
}

// The trailing update of the NEXT panel's 128 rows only -- the one piece of the update that sits on the chain (the
// next diagonal block and row panel wait for it).  It is bound by the matrix pipe of single waves: a 64x64 tile per
// workgroup means 2x2 MFMA tiles x K/4 steps = 256 dependent-free but serial MFMAs per wave at K = 256 (7.8 us).
// Here a workgroup takes 32 rows x 64 columns (wave w: both 16-row tiles x its 16 columns), which halves the MFMAs
// per wave and doubles the workgroups (256 at N = 4096: every CU busy).  blockIdx.x == nt: the rhs column.
__global__ __launch_bounds__(256) void syrk_rows_kernel(double *A, int64_t lda, int r0, int n1, int c0, int nt, int rcol,
                                                        const int *__restrict__ skip_if)
{
    CHAIN_PRIORITY();
    if (__builtin_nontemporal_load(skip_if) != 0) return;
    const int tj = blockIdx.x, ti = blockIdx.y;                  // 64-column tile, 32-row tile (4 of them)
    const int tid = threadIdx.x;
    const double *P = A + (int64_t)r0 * lda;
    if (tj == nt) {
        __shared__ double part[256];
        const int i = tid & 31, g = tid >> 5;
        const int64_t gi = c0 + (int64_t)ti * 32 + i;
        double s = 0.0;
        for (int k0 = g; k0 < n1; k0 += 16 * 8) {
            double pv[16], zv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int k = k0 + u * 8;
                const bool ok = k < n1;
                pv[u] = ok ? P[(int64_t)k * lda + gi] : 0.0;
                zv[u] = ok ? P[(int64_t)k * lda + rcol] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) s = fma(pv[u], zv[u], s);
        }
        part[tid] = s;
        __syncthreads();
        if (g == 0) {
            double tot = 0.0;
#pragma unroll
            for (int gg = 0; gg < 8; ++gg) tot += part[gg * 32 + i];
            A[gi * lda + rcol] -= tot;
        }
        return;
    }
    const int64_t ib = c0 + (int64_t)ti * 32;                    // first row of the tile (= a column of the panel)
    const int64_t jb0 = c0 + (int64_t)tj * 64;
    if (jb0 + 63 < ib) return;                                   // entirely below the diagonal
    const int lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t jb = jb0 + wave * 16;
    d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
    const double *Pa = P + (int64_t)kq * lda + ib + lc;          // A[i = lc][k = kq] = P[k][ib + i]  (+16: second row tile)
    const double *Pb = P + (int64_t)kq * lda + jb + lc;          // B[k = kq][j = lc] = P[k][jb + j]
    constexpr int CH = 8;                                        // k-steps per software-pipeline chunk (16: more registers, no faster)
    double a0[2][CH], a1[2][CH], b[2][CH];
    auto load_chunk = [&](int k0, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < CH; ++ks) {
            a0[buf][ks] = Pa[(int64_t)(k0 + 4 * ks) * lda];
            a1[buf][ks] = Pa[(int64_t)(k0 + 4 * ks) * lda + 16];
            b[buf][ks] = Pb[(int64_t)(k0 + 4 * ks) * lda];
        }
    };
    load_chunk(0, 0);
    double cv[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) cv[m][r] = A[(ib + 16 * m + kq + 4 * r) * lda + jb + lc];
    // n1 is 128 or 256: a multiple of 2 chunks of 32 rows
    for (int k0 = 0; k0 < n1; k0 += 8 * CH) {
        load_chunk(k0 + 4 * CH, 1);
#pragma unroll
        for (int ks = 0; ks < CH; ++ks) {
            acc[0] = MFMA_F64(a0[0][ks], b[0][ks], acc[0]);
            acc[1] = MFMA_F64(a1[0][ks], b[0][ks], acc[1]);
        }
        if (k0 + 8 * CH < n1) load_chunk(k0 + 8 * CH, 0);
#pragma unroll
        for (int ks = 0; ks < CH; ++ks) {
            acc[0] = MFMA_F64(a0[1][ks], b[1][ks], acc[0]);
            acc[1] = MFMA_F64(a1[1][ks], b[1][ks], acc[1]);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) A[(ib + 16 * m + kq + 4 * r) * lda + jb + lc] = cv[m][r] - acc[m][r];
}

// the first `rows` rows below the n1 panel rows [r0, r0 + n1) against those panel rows: columns from c0 = r0 + n1 on,
// n2 of them (rows: 128 = the next panel, 256 = the next pair of panels)
// `done`: an event that completes with the launch (the launch carries it: no marker packet on the stream)
static void launch_syrk_rows(hipStream_t s, double *A, int64_t lda, int r0, int n1, int n2, int rcol, const int *skip_if,
                             int rows = 128, hipEvent_t done = nullptr)
{
    const int c0 = r0 + n1;
    const int nt = n2 / 64;
    if (nt <= 0) { if (done) hipEventRecord(done, s); return; }
    if (rows > n2) rows = n2;
    hipExtLaunchKernelGGL(syrk_rows_kernel, dim3(nt + 1, rows / 32), dim3(256), 0, s, nullptr, done, 0, A, lda, r0, n1, c0,
                          nt, rcol, skip_if);
}

// tile rows [ti_begin, ti_end) of the trailing update (64-row tiles counted from the first trailing row)
static void launch_syrk(hipStream_t s, double *A, int64_t lda, int r0, int n1, int n2, int rcol, int ti_begin,
                        int ti_end, const int *skip_if)
{
    const int c0 = r0 + n1;
    const int nt = n2 / 64;
    if (ti_end > nt) ti_end = nt;
    if (ti_end <= ti_begin) return;
    hipLaunchKernelGGL(syrk_kernel<64>, dim3(nt + 1, ti_end - ti_begin), dim3(256), 0, s, A, lda, r0, n1, c0, nt, rcol,
                       ti_begin, skip_if);
}

// slot i of an event vector, created on first use
static hipEvent_t event_slot(std::vector<hipEvent_t> &ev, size_t i)
{
    while (ev.size() <= i) {
        hipEvent_t e;
        hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence);
        ev.push_back(e);
    }
    return ev[i];
}

// Rows [r0, r0 + klen) of U (all columns) and of z are final on stream `chain`: hand them to the sweep.
// Two sweep streams with a look-ahead of one panel pair: `stream` solves the pair's rows of V (sd) and folds
// them into the NEXT pair's rows only (first); `bulk` folds them into everything below that (rest).  The
// bulk launches then follow each other without a gap while sd/first of the following pair run beside them:
//   stream: wait chain[p]; sd(p); record sd[p]; wait rest[p-1]; first(p)      (first(p) rewrites rows that
//   bulk  : wait sd[p]; rest(p); record rest[p]                                rest(p-1) also rewrites)
void sweep_pipe_pair(const SweepPipe &pipe, hipStream_t chain, const double *A, int64_t lda, const double *invDt,
                     int64_t n_pad, int p, int r0, int klen)
{
    auto pipe_event = [&](int kind, int pp) {      // kind 0: chain, 1: sd done, 2: rest done
        return event_slot(*pipe.events, (size_t)(3 * pp + kind));
    };
    const int64_t cols = (pipe.lower_tri && r0 + klen < pipe.m_pad) ? (int64_t)(r0 + klen) : pipe.m_pad;
    const double m = (double)cols;
    hipEventRecord(pipe_event(0, p), chain);
    hipStreamWaitEvent(pipe.stream, pipe_event(0, p), 0);
    if (pipe.mark) pipe.mark(pipe.user, pipe.stream, 1, (double)klen * (double)klen * m);
    // (every kernel of the pipeline runs on 16-row, half-LDS stages: two workgroups per CU)
    launch_trsm_strips(pipe.stream, A + (int64_t)r0 * lda + r0, lda, invDt + (int64_t)(r0 / 16) * 256,
                       pipe.V + (int64_t)r0 * pipe.ldv, pipe.ldv, klen, cols, pipe.zvec + r0, pipe.q, pipe.mu, true, true);
    if (pipe.mark) pipe.mark(pipe.user, pipe.stream, 0, 0.0);
    hipEventRecord(pipe_event(1, p), pipe.stream);
    const int below = r0 + klen;
    if (below >= (int)n_pad) return;
    const int first_end = (below + 256 < (int)n_pad) ? below + 256 : (int)n_pad;
    auto update = [&](hipStream_t st, int k0, int kl, int i0, int i1) {
        if (i0 >= i1) return;
        if (pipe.mark) pipe.mark(pipe.user, st, 1, 2.0 * (double)kl * (double)(i1 - i0) * m);
        launch_gemm_update(st, A, lda, pipe.V, pipe.ldv, pipe.V, pipe.ldv, k0, kl, i0, i1, cols, false);
        if (pipe.mark) pipe.mark(pipe.user, st, 0, 0.0);
    };
    // Groups of G pairs, as in launch_cholesky's bulk updates (and for the same reason: the update kernel's rate grows
    // with K -- 0.68 of the fp64 MFMA peak at K = 256, 0.76 at 512, 0.83 at 1024 -- and it accumulates sequentially into
    // C, so one K = 256 G pass has the bits of G passes of K = 256).  Group j = pairs [G j, G j + G), G_g = the rows of
    // group g:
    //   stream: after sd(p), p in group j:  first: rows of pair p+1 -= pair p;
    //                                       near:  the rows from pair p+2 to the end of G_{j+1} -= pair p     (K = 256)
    //           (the first near of a group waits for restA of the group before)
    //   bulk  : [wait sd of the group's last pair]  restA(j): G_{j+2} -= group j;  restB(j): everything below -= group j
    // A pair whose group is not entirely in the pipeline (the remainder of the count, a 128-row remainder) goes alone as
    // before.  The caller decides (pipe.group = G): groups pay where the bulk stream is the pipeline's bottleneck (a
    // round of strips or more per CU); with few strips the pairs schedule starts its updates earlier and wins
    // (profiles/r03_schedule_crossover.txt).
    const int G = pipe.group, lead = pipe.lead;
    const int full_pairs = ((pipe.tail_begin < (int)n_pad) ? pipe.tail_begin : (int)n_pad) / 256;
    // pipe.lead pairs go alone ahead of the first group (round 5: with groups from the first pair on, the bulk stream idled
    // until the SECOND pair was solved -- a fifth of the pipelined phase at C2)
    const bool grouped = G >= 2 && !pipe.lower_tri && klen == 256 && p >= lead && ((p - lead) / G + 1) * G + lead <= full_pairs;
    if (grouped) {
        const int j = (p - lead) / G, i = (p - lead) % G;
        const int g0 = 256 * (lead + G * j);                                                       // the group's first row
        const int next_end = (g0 + 512 * G < (int)n_pad) ? g0 + 512 * G : (int)n_pad;              // end of G_{j+1}
        // the first group behind lead pairs: its rows were last written by the bulk update of the pair before it
        if (i == 0 && j == 0 && lead > 0) hipStreamWaitEvent(pipe.stream, pipe_event(2, lead - 1), 0);
        update(pipe.stream, r0, 256, below, first_end);
        if (i == 0 && j >= 1) hipStreamWaitEvent(pipe.stream, pipe_event(2, lead + G * (j - 1)), 0);   // restA of the group before
        update(pipe.stream, r0, 256, r0 + 512, next_end);
        if (i < G - 1) return;
        hipStreamWaitEvent(pipe.bulk, pipe_event(1, p), 0);
        const int a1 = (g0 + 768 * G < (int)n_pad) ? g0 + 768 * G : (int)n_pad;                    // end of G_{j+2}
        update(pipe.bulk, g0, 256 * G, next_end, a1);
        hipEventRecord(pipe_event(2, lead + G * j), pipe.bulk);                      // restA (the first pair's slot)
        update(pipe.bulk, g0, 256 * G, a1, (int)n_pad);
        hipEventRecord(pipe_event(2, p), pipe.bulk);                                 // restB: what a successor waits for
        return;
    }
    if (p > 0) hipStreamWaitEvent(pipe.stream, pipe_event(2, p - 1), 0);
    update(pipe.stream, r0, klen, below, first_end);
    hipStreamWaitEvent(pipe.bulk, pipe_event(1, p), 0);
    update(pipe.bulk, r0, klen, first_end, (int)n_pad);
    hipEventRecord(pipe_event(2, p), pipe.bulk);
}

// The rows the pairs did not take, [tail_begin, n_pad): every earlier pair has been folded into them (first of the
// last pair on `stream`, rest of the last pair on `bulk`) and the factor is complete on `chain`: one left-looking
// launch of the strip kernel on the sub-problem, on the chain stream itself (every CU, full-LDS variant).
void sweep_pipe_tail(const SweepPipe &pipe, hipStream_t chain, const double *A, int64_t lda, const double *invDt,
                     int64_t n_pad, int pairs_done)
{
    std::vector<hipEvent_t> &ev = *pipe.events;
    const hipEvent_t last = event_slot(ev, (size_t)(3 * pairs_done));
    if (pairs_done > 0) {
        hipEventRecord(last, pipe.stream);                                       // sd and first of the last pair
        hipStreamWaitEvent(chain, last, 0);
        hipStreamWaitEvent(chain, ev[(size_t)(3 * (pairs_done - 1) + 2)], 0);      // rest of the last pair
    }
    const int t0 = pipe.tail_begin;
    const double rows = (double)((int)n_pad - t0);
    if (pipe.mark) pipe.mark(pipe.user, chain, 1, rows * rows * (double)pipe.m_pad);
    launch_trsm_strips(chain, A + (int64_t)t0 * lda + t0, lda, invDt + (int64_t)(t0 / 16) * 256,
                       pipe.V + (int64_t)t0 * pipe.ldv, pipe.ldv, (int64_t)n_pad - t0, pipe.m_pad, pipe.zvec + t0, pipe.q,
                       pipe.mu, true, false);
    if (pipe.mark) pipe.mark(pipe.user, chain, 0, 0.0);
}

__global__ void zero_ints_kernel(int *p, int n)
{
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}

// Look-ahead of one panel pair: the bulk of pair p-1's trailing update (everything below pair p+1's rows) runs on the
// side stream while the main stream factors and solves pair p; the two meet before pair p's own update of pair
// p+1's rows (schedule inside).
void launch_cholesky(hipStream_t s, hipStream_t side, std::vector<hipEvent_t> &events, double *A, int64_t lda,
                     int64_t n_pad, double *invDt, int *info_dev, const CholOptions &opt, const SweepPipe *pipe,
                     bool info_zeroed)
{
    // > 64 KiB of dynamic LDS needs the opt-in on the current device (cheap; done per call so that several
    // devices in one process are all covered)
    hipFuncSetAttribute(reinterpret_cast<const void *>(potrf_diag128_v2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)sizeof(Diag2Shared));
    hipFuncSetAttribute(reinterpret_cast<const void *>(panel_trsm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)sizeof(PanelShared));
    hipFuncSetAttribute(reinterpret_cast<const void *>(potrf_panel_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)sizeof(Diag2Shared));
    // the bulk trailing update takes the LDS-staged GEMM form (trsm_update_kernel<16>, one row block per workgroup) while
    // at least this many rows lie below the pair, the 64x64-tile SYRK from L2 fragments below that (round-2 scan)
    constexpr int syrk_gemm_rows = 6144;
    auto launch_diag = [&](int rr) {
        hipLaunchKernelGGL(potrf_diag128_v2_kernel, dim3(1), dim3(256), sizeof(Diag2Shared), s, A, lda, rr, (int)n_pad,
                           invDt, info_dev, pipe ? pipe->zvec : nullptr);
    };
    const int np = (int)(n_pad / 128);
    // info_dev[0] is the status word; info_dev[1 + 2p], [2 + 2p] the publication counts of panel p's fused launch
    const bool fused = opt.panel_form != 2 && 2 * np <= kCholFlagSlots;
    const bool split = opt.panel_form == 5;
    // (a launch, not hipMemsetAsync: the runtime's fill costs two kernels and ~8 us of marker gaps around each)
    if (!info_zeroed) hipLaunchKernelGGL(zero_ints_kernel, dim3(1), dim3(256), 0, s, info_dev, fused ? 1 + 2 * np : 1);
    int *flags = info_dev + 1;
    const int rcol = (int)n_pad;
    event_slot(events, (size_t)(2 * np + 1));          // (and every slot before it)
    // the side stream starts after everything queued on the main stream so far (K assembly, rhs)
    hipEventRecord(events[2 * np], s);
    hipStreamWaitEvent(side, events[2 * np], 0);
    // Panels are taken in pairs: the second panel of a pair only needs the first one's update of its own 128
    // rows, so the trailing matrix below the pair is updated once with K = 256 (half the read-modify-write
    // passes); the bulk of that update runs on the side stream under the next pair's diagonal/panel work.
    double *zvec = pipe ? pipe->zvec : nullptr;
    // unfused panel solves: the lean panel kernel, or beside a pipelined sweep the half-LDS strip kernel, which fits next
    // to a sweep workgroup
    const bool lean_panel = !pipe;
    int pair = 0;
    auto sweep_rows = [&](int r0, int klen) {
        if (pipe && r0 < pipe->tail_begin) sweep_pipe_pair(*pipe, s, A, lda, invDt, n_pad, pair++, r0, klen);
    };
    // Schedule per pair p (panels A_p, B_p):
    //   chain:  diag A_p, panel A_p, rows B_p -= A_p (K = 128), diag B_p, panel B_p,
    //           [wait bulk(p-1)]  rows A_{p+1}, B_{p+1} -= (A_p, B_p)  (K = 256, 256 rows)
    //   side :  [wait panel B_p]  bulk(p): everything below B_{p+1} -= (A_p, B_p)
    // bulk(p-1) rewrites the rows the K = 256 rows kernel of pair p rewrites, hence the wait; it has the whole chain of
    // pair p to finish, and bulk(p) follows it on the side stream without a gap -- large factorisations are bound by
    // the bulk updates alone, small ones by the chain alone.
    int pending = -1;                      // event index of the bulk update still in flight
    // Large trailing matrices, groups of G pairs (CBO_HIP_BULK_GROUP caps G: 1 = pairs only, 2, 4 = default).  The bulk update is
    // the LDS-staged GEMM kernel, whose rate grows with K (16384 points, all columns: 0.68 / 0.75 / 0.83 of peak at K = 256 /
    // 512 / 1024: profiles/r03_update_kernel_timing.txt), and it accumulates into C sequentially from C's own value, so one K = 256 G
    // pass gives the bits of G passes of K = 256.  Group j = pairs [G j, G j + G); S = 256 G; G_g = the S rows of group g:
    //   chain:  pair p of group j: factor; rows of pair p+1 -= pair p (rows kernel, as ever);
    //           [first pair of the group: wait bigA(j-1)]  near(p): the rows from pair p+2 to the end of G_{j+1} -= pair p (K = 256)
    //   side :  [wait the group's last pair]  bigA(j): G_{j+2} -= group j;  bigB(j): everything below G_{j+2} -= group j   (K = S)
    // -- every row still receives the pairs in order, each through the kernel that applied it before (rows kernel for
    // the pair right above, GEMM kernel otherwise): the factor is bit-identical to the pairs-only schedule
    // (scripts/probes/bulk_group_scan.sh: one digest for G = 1, 2, 4).  The chain only ever waits for bigA (S rows, first on
    // the side stream after the previous bigB), so bigB(j) has the whole chain of group j+1 to finish and bigB(j+1) follows it
    // without a gap.  The near updates (K = 256) are the price: they run on the chain stream beside the bulk update.  Groups
    // are used while every pair's bulk update would take the GEMM form anyway; the last ~6000 rows go pair by pair as before.
    // Groups of four while at least CBO_HIP_BULK_GROUP4_ROWS (10240) rows lie below the group, of two below that: round 5,
    // 16384 points 29.61 (G = 2) -> 29.07 ms on one box (thresholds 4096 / 6144 / 8192: 29.63 / 29.82 / 29.28).
    int group_left = 0;                    // pairs of the open group still to come, this one included
    int group_pairs = 0, group_g0 = 0, group_first_k = 0;
    int pending_big_a = -1;                // event index of the last bigA
    for (int k = 0; k < np; k += 2) {
        const int r0 = 128 * k;
        const int n2 = (int)n_pad - r0 - 128;
        const int n3_pair = (int)n_pad - r0 - 256;                   // rows below this pair
        if (group_left == 0 && opt.bulk_group >= 2 && (fused || lean_panel)) {
            // a group opens here if the rows below it still take the GEMM form for every pair of the group
            int G = 0;
            if (opt.bulk_group >= 4 && n3_pair - 1024 >= opt.group4_rows && n3_pair - 1024 >= syrk_gemm_rows &&
                n3_pair - 1024 >= 1024)
                G = 4;
            else if (n3_pair - 512 >= syrk_gemm_rows && n3_pair - 512 >= 512) G = 2;
            if (G != 0) { group_pairs = G; group_left = G; group_g0 = r0; group_first_k = k; }
        }
        const bool grouped = group_left > 0;
        const bool first_of_group = grouped && group_left == group_pairs;
        const bool last_of_group = grouped && group_left == 1;
        // inside groups, beside a bulk update that fills the device, the strips go as an LDS-free launch of their own
        // (launch_panel_fused)
        const bool split_now = split || grouped;
        // the 128-row panel at r with `cols` columns to its right (none: the diagonal block alone); `done` completes with
        // its last launch (a pipelined sweep's strip solves are never given one: see `carried`)
        auto factor_panel = [&](int r, int cols, hipEvent_t done) {
            if (fused && cols > 0) {
                launch_panel_fused(s, A, lda, r, rcol, invDt, info_dev, zvec, cols, flags + 2 * (r / 128), opt.spin_limit,
                                   done, split_now);
                return;
            }
            launch_diag(r);
            if (cols <= 0) return;
            if (lean_panel) launch_panel_trsm(s, A, lda, r, r + 128, cols, invDt, info_dev, done);
            else
                launch_trsm_strips(s, A + (int64_t)r * lda + r, lda, invDt + (int64_t)(r / 16) * 256,
                                   A + (int64_t)r * lda + r + 128, lda, 128, cols, nullptr, nullptr, nullptr, false, true);
        };
        factor_panel(r0, n2, nullptr);
        if (n2 <= 0) { sweep_rows(r0, 128); break; }
        // rows of the pair's second panel: K = 128 update with the first panel
        launch_syrk_rows(s, A, lda, r0, 128, n2, rcol, info_dev);
        const int r1 = r0 + 128;
        const int n3 = (int)n_pad - r1 - 128;
        const bool bulk = n3 > 256;
        const bool gemm_form = bulk && n3 - 256 >= syrk_gemm_rows;
        // the event the side stream waits for completes WITH the launch it follows (no marker packet on the chain)
        const bool carried = bulk && (fused || lean_panel);
        const hipEvent_t ev_panel = (carried && gemm_form && (!grouped || last_of_group)) ? events[2 * k] : nullptr;
        const hipEvent_t ev_rows = (carried && !gemm_form) ? events[2 * k] : nullptr;
        factor_panel(r1, n3, ev_panel);
        sweep_rows(r0, 256);
        if (n3 <= 0) break;
        if (grouped) {
            const int S = 256 * group_pairs, g0 = group_g0, n = (int)n_pad;
            const int next_end = (g0 + 2 * S < n) ? g0 + 2 * S : n;                   // end of G_{j+1}
            if (last_of_group) {
                // the group's bulk update (K = S) on the side stream, first the rows the chain needs next
                hipStreamWaitEvent(side, events[2 * k], 0);
                const int a_end = (g0 + 3 * S < n) ? g0 + 3 * S : n;                  // end of G_{j+2}
                launch_gemm_update(side, A, lda, A, lda, A, lda, g0, S, next_end, a_end, n_pad + kRhsCols, true, info_dev);
                hipEventRecord(events[2 * group_first_k + 1], side);                  // (the first pair's slot: it has no bulk update of its own)
                pending_big_a = 2 * group_first_k + 1;
                if (a_end < n)
                    launch_gemm_update(side, A, lda, A, lda, A, lda, g0, S, a_end, n, n_pad + kRhsCols, true, info_dev);
                hipEventRecord(events[2 * k + 1], side);
                pending = 2 * k + 1;
            }
            // the next pair's rows on the chain as ever, then the rest of the rows up to the end of the next group
            launch_syrk_rows(s, A, lda, r0, 256, n3, rcol, info_dev, 256, nullptr);
            if (first_of_group && pending_big_a >= 0) hipStreamWaitEvent(s, events[pending_big_a], 0);
            launch_gemm_update(s, A, lda, A, lda, A, lda, r0, 256, r0 + 512, next_end, n_pad + kRhsCols, true, info_dev);
            --group_left;
            continue;
        }
        // both panels against everything below them: the bulk (below the next pair) on the side stream, the next
        // pair's own rows on this stream after the previous pair's bulk update of the same rows.  A large bulk update
        // bounds the factorisation, so it starts as soon as the panels are solved and the rows kernel runs beside its
        // first workgroups; a small one is hidden behind the chain anyway and would only slow the rows kernel (which is
        // ON the chain) down, so it starts after that.
        const int prev = pending;
        auto launch_bulk = [&] {
            if (!carried) hipEventRecord(events[2 * k], s);
            hipStreamWaitEvent(side, events[2 * k], 0);
            // Large trailing blocks go through the LDS-staged GEMM form of the sweep's update kernel (C -= P^T P on
            // 64-column strips x 256-row chunks, upper part only, the rhs strip as one more strip): the 64x64-tile SYRK
            // reads its operands as fragment-shaped loads from L2 and tops out near half the fp64 MFMA rate
            if (gemm_form)
                launch_gemm_update(side, A, lda, A, lda, A, lda, r0, 256, r0 + 256 + 256, (int)n_pad, n_pad + kRhsCols, true,
                                   info_dev);
            else
                launch_syrk(side, A, lda, r0, 256, n3, rcol, 4, n3 / 64, info_dev);
            hipEventRecord(events[2 * k + 1], side);
            pending = 2 * k + 1;
        };
        if (gemm_form) launch_bulk();
        if (prev >= 0) hipStreamWaitEvent(s, events[prev], 0);
        launch_syrk_rows(s, A, lda, r0, 256, n3, rcol, info_dev, 256, ev_rows);
        if (bulk && !gemm_form) launch_bulk();
    }
    // nothing is left on the side stream that the main stream has not waited for (the last bulk update is
    // awaited before the following panel's syrk); make that explicit for robustness
    hipEventRecord(events[2 * np + 1], side);
    hipStreamWaitEvent(s, events[2 * np + 1], 0);
    if (pipe && pipe->tail_begin < (int)n_pad) sweep_pipe_tail(*pipe, s, A, lda, invDt, n_pad, pair);
}

// ------------------------------------------------------------------------------------------------
// Backward solve U alpha = z, 128-row blocks from the bottom, one launch per block.  Every workgroup
// first solves the 128x128 diagonal system redundantly in LDS (16-row sub-blocks: multiply by the
// stored inv(U_bb), then fold into the rows above), then workgroup g folds alpha_blk into the 128 rows
// of block g above it:  zt[g] -= U[g, blk] alpha_blk.  zt is a contiguous working copy of z.
__global__ __launch_bounds__(256) void backsolve_step_kernel(const double *__restrict__ A, int64_t lda,
                                                             const double *__restrict__ invDt, int blk, double *zt,
                                                             double *__restrict__ alpha)
{
    __shared__ double zs[128];
    __shared__ double al[128];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int b0 = blk * 128;
    if (tid < 128) zs[tid] = zt[b0 + tid];
    __syncthreads();
    for (int s = 7; s >= 0; --s) {
        const int o = 16 * s;
        // alpha_s = inv(U_ss) zs_s : 16 outputs, thread (i, part) sums 4 of the 16 terms
        if (tid < 64) {
            const int i = tid >> 2, part = tid & 3;
            const double *Y = invDt + (int64_t)(b0 / 16 + s) * 256;      // Y[i][k] = inv(U_ss)[i][k]
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(Y[i * 16 + 4 * part + k], zs[o + 4 * part + k], acc);
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (part == 0) al[o + i] = acc;
        }
        __syncthreads();
        // rows above inside the block: zs[r] -= sum_c U[b0+r][b0+o+c] al[o+c], r < o
        if (tid < o) {
            const double *row = A + (int64_t)(b0 + tid) * lda + b0 + o;
            double acc = zs[tid];
#pragma unroll
            for (int c = 0; c < 16; ++c) acc = fma(-row[c], al[o + c], acc);
            zs[tid] = acc;
        }
        __syncthreads();
    }
    const int g = blockIdx.x;
    if (g == blk) {
        if (tid < 128) alpha[b0 + tid] = al[tid];
        return;
    }
    // one row per wave iteration: 64 lanes x 2 columns, wave-level reduction
    for (int i = wave; i < 128; i += 4) {
        const d2 u = *reinterpret_cast<const d2 *>(&A[(int64_t)(g * 128 + i) * lda + b0 + 2 * lane]);
        double acc = fma(u[0], al[2 * lane], u[1] * al[2 * lane + 1]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) zt[g * 128 + i] -= acc;
    }
}

__global__ void copy_strided_kernel(const double *__restrict__ src, int64_t stride, int64_t n, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i * stride];
}

// The caller provides alpha with 2*n_pad doubles: [0, n_pad) result, [n_pad, 2 n_pad) working copy of z.
void launch_backsolve(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *alpha)
{
    launch_backsolve_vec(s, A, lda, n_pad, invDt, A + n_pad, lda, alpha + n_pad, alpha);
}

// out = U^-1 src for one strided vector (src is left untouched; work is an n_pad scratch vector).
void launch_backsolve_vec(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt,
                          const double *src, int64_t src_stride, double *work, double *out)
{
    hipLaunchKernelGGL(copy_strided_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, src, src_stride,
                       n_pad, work);
    const int nb = (int)(n_pad / 128);
    for (int blk = nb - 1; blk >= 0; --blk)
        hipLaunchKernelGGL(backsolve_step_kernel, dim3(blk + 1), dim3(256), 0, s, A, lda, invDt, blk, work, out);
}

// ------------------------------------------------------------------------------------------------
// Forward solve U^T l = k (l = L^-1 k) for ONE right-hand side, 128-row blocks from the top, one launch per block:
// the mirror image of backsolve_step_kernel.  Every workgroup first solves the 128x128 diagonal system redundantly
// in LDS (16-row sub-blocks: multiply by the transposed stored inv(U_ss), then fold into the rows below), then
// workgroup g folds l_blk into the 128 entries of block blk + 1 + g:  w[i] -= sum_k U[blk rows k][i] l_k -- a row of
// U is contiguous in i, so the 128 threads of the update read coalesced.  The strip kernel needs 64 columns and a
// workgroup per strip; for a single column this is what fills the device.
__global__ __launch_bounds__(256) void forward_step_kernel(const double *__restrict__ A, int64_t lda,
                                                           const double *__restrict__ invDt, int blk, int nb, double *w,
                                                           double *__restrict__ out)
{
    __shared__ double rs[128];
    __shared__ double ls[128];
    const int tid = threadIdx.x;
    const int b0 = blk * 128;
    if (tid < 128) rs[tid] = w[b0 + tid];
    __syncthreads();
    for (int s = 0; s < 8; ++s) {
        const int o = 16 * s;
        // l_s = inv(U_ss)^T r_s : thread (i, part) sums 4 of the 16 terms; Y[k][i] = inv(U_ss)[k][i]
        if (tid < 64) {
            const int i = tid >> 2, part = tid & 3;
            const double *Y = invDt + (int64_t)(b0 / 16 + s) * 256;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(Y[(4 * part + k) * 16 + i], rs[o + 4 * part + k], acc);
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (part == 0) ls[o + i] = acc;
        }
        __syncthreads();
        // rows below inside the block: rs[c] -= sum_k U[b0+o+k][b0+c] l_{o+k}, c >= o + 16
        if (tid >= o + 16 && tid < 128) {
            double acc = rs[tid];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc = fma(-A[(int64_t)(b0 + o + k) * lda + b0 + tid], ls[o + k], acc);
            rs[tid] = acc;
        }
        __syncthreads();
    }
    const int g = blockIdx.x;
    if (g == 0 && tid < 128) out[b0 + tid] = ls[tid];
    // block blk + 1 + g: two threads per entry, each over 64 of the 128 panel rows
    if (blk + 1 + g >= nb) return;                             // the last block has nothing below it (uniform)
    const int c = tid & 127, half = tid >> 7;
    const int64_t col = (int64_t)(blk + 1 + g) * 128 + c;
    double acc = 0.0;
    for (int k = 64 * half; k < 64 * half + 64; ++k) acc = fma(A[(int64_t)(b0 + k) * lda + col], ls[k], acc);
    __syncthreads();
    if (half == 1) rs[c] = acc;
    __syncthreads();
    if (half == 0) w[col] -= acc + rs[c];
}

// out = L^-1 w for one contiguous vector of n_pad entries (w is used as the work vector and destroyed).
void launch_forward_vec(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *w,
                        double *out)
{
    const int nb = (int)(n_pad / 128);
    for (int blk = 0; blk < nb; ++blk) {
        const int below = nb - 1 - blk;                       // blocks that receive this block's contribution
        hipLaunchKernelGGL(forward_step_kernel, dim3(below > 0 ? below : 1), dim3(256), 0, s, A, lda, invDt, blk, nb, w, out);
    }
}

// ------------------------------------------------------------------------------------------------
// The two single-vector solves as ONE launch each: a chain of workgroups, one per 128-row block.
//
// The per-block launches above cost a launch plus a cold diagonal solve per block (42 us: 5.4 ms for alpha at 16384
// points).  Here workgroup w owns block g and, in the backward solve, folds alpha_blk into its 128 entries for every
// blk > g as those become available (the solved block itself is the signal, see chain_wait), then solves its diagonal
// block and publishes alpha_g.  What the chain waits for per block
// is: the arrival of alpha_{g+1}, one 128 x 128 fold, the diagonal solve, the publication.  Everything that does not
// depend on alpha is in place before it arrives: the diagonal block and its 16 x 16 inverses sit in LDS, the block of U
// for the next fold sits in registers (requested while the previous hand-over is awaited).
// Same operations in the same order as the per-block kernels (each fold is one subtraction of the same wave-reduced
// sum, blocks in the same order; the in-block solve is the same code on LDS copies): same bits.
// Forward progress: block g waits only for blocks solved earlier, and the workgroup index grows in solve order, so under
// in-order dispatch every producer is resident before its consumers (no need for all workgroups to be co-resident).
// The polls are bounded; a give-up lands in the status word and the host repeats the solve with the per-block launches.
constexpr int kVecLd = 129;                      // LDS row stride of the diagonal block: column reads by 128 threads

struct VecChainShared {
    double Ud[128][kVecLd];                      // U[g, g] (row-major)
    double inv[8][256];                          // inverses of its 16 x 16 diagonal tiles
    double zs[128], al[128], ab[128];
    int abort_flag;
};

// The solved block IS the signal: the output vector is pre-filled with a sentinel (a NaN payload no computation
// produces; a computed NaN is stored as the canonical quiet NaN), the producer stores its 128 values as agent-scope
// atomics, and each of the consumer's first 128 threads polls ITS value until it is no longer the sentinel -- one
// round trip to the coherence point per hand-over instead of two (count, then data), and no fence: every element is its
// own atomic object and nothing else is communicated through it.
constexpr unsigned long long kVecSentinel = 0x7ff8dead0000beefull;

__device__ __forceinline__ bool chain_wait(const double *src, int *info, int spin_limit, VecChainShared &sh)
{
    int ok = 1;
    if (threadIdx.x < 128) {
        int spins = 0;
        double v;
        for (;;) {
            v = __hip_atomic_load(src + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned long long)__double_as_longlong(v) != kVecSentinel) break;
            if (spin_limit < 0 || ++spins > spin_limit || ((spins & 63) == 0 && __builtin_nontemporal_load(info) != 0)) { ok = 0; break; }
        }
        sh.ab[threadIdx.x] = v;
    }
    if (!__syncthreads_and(ok)) {
        if (threadIdx.x == 0) atomicCAS(info, 0, kFusedTimeout);
        return false;
    }
    return true;
}

__device__ __forceinline__ void chain_publish(double *dst, const double *vals)
{
    if (threadIdx.x < 128) {
        double v = vals[threadIdx.x];
        if (v != v) v = __longlong_as_double(0x7ff8000000000000ll);
        __hip_atomic_store(dst + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void fill_sentinel_kernel(double *p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = __longlong_as_double((long long)kVecSentinel);
}

__global__ __launch_bounds__(256) void backsolve_chain_kernel(const double *__restrict__ A, int64_t lda,
                                                              const double *__restrict__ invDt, int nb,
                                                              const double *__restrict__ zt, double *alpha, int *info,
                                                              int spin_limit)
{
    extern __shared__ __align__(16) unsigned char vec_smem[];
    VecChainShared &sh = *reinterpret_cast<VecChainShared *>(vec_smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = nb - 1 - (int)blockIdx.x;                       // workgroup 0 owns the last block: solved first
    const int b0 = g * 128;
    if (tid < 128) sh.zs[tid] = zt[b0 + tid];
    for (int i = tid; i < 128 * 128; i += 256) sh.Ud[i >> 7][i & 127] = A[(int64_t)(b0 + (i >> 7)) * lda + b0 + (i & 127)];
    for (int i = tid; i < 8 * 256; i += 256) sh.inv[i >> 8][i & 255] = invDt[(int64_t)(b0 / 16) * 256 + i];
    // The block of the NEXT fold is always in registers before its alpha arrives: U[g, blk] as wave w's rows w, w+4, ...,
    // two columns per lane, requested while the previous hand-over is awaited (32 loads in flight, not 32 round trips).
    d2 un[32];
    auto request_block = [&](int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 32; ++r)
            un[r] = *reinterpret_cast<const d2 *>(&A[(int64_t)(b0 + wave + 4 * r) * lda + blk * 128 + 2 * lane]);
    };
    if (g + 1 < nb) request_block(nb - 1);
    __syncthreads();
    for (int blk = nb - 1; blk > g; --blk) {
        if (!chain_wait(alpha + blk * 128, info, spin_limit, sh)) return;      // alpha_blk is in sh.ab
        const double a0 = sh.ab[2 * lane], a1 = sh.ab[2 * lane + 1];
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            double acc = fma(un[r][0], a0, un[r][1] * a1);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            if (lane == 0) sh.zs[wave + 4 * r] -= acc;
        }
        if (blk - 1 > g) request_block(blk - 1);
        __syncthreads();
    }
    // the diagonal system, bottom tile first (backsolve_step_kernel's arithmetic on the LDS copies)
    for (int s = 7; s >= 0; --s) {
        const int o = 16 * s;
        if (tid < 64) {
            const int i = tid >> 2, part = tid & 3;
            const double *Y = sh.inv[s];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(Y[i * 16 + 4 * part + k], sh.zs[o + 4 * part + k], acc);
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (part == 0) sh.al[o + i] = acc;
        }
        __syncthreads();
        if (tid < o) {
            double acc = sh.zs[tid];
#pragma unroll
            for (int c = 0; c < 16; ++c) acc = fma(-sh.Ud[tid][o + c], sh.al[o + c], acc);
            sh.zs[tid] = acc;
        }
        __syncthreads();
    }
    chain_publish(alpha + b0, sh.al);
}

__global__ __launch_bounds__(256) void forward_chain_kernel(const double *__restrict__ A, int64_t lda,
                                                            const double *__restrict__ invDt, int nb,
                                                            const double *__restrict__ w, double *out, int *info,
                                                            int spin_limit)
{
    extern __shared__ __align__(16) unsigned char vec_smem[];
    VecChainShared &sh = *reinterpret_cast<VecChainShared *>(vec_smem);
    const int tid = threadIdx.x;
    const int g = (int)blockIdx.x;                                // solved in index order
    const int b0 = g * 128;
    const int c = tid & 127, half = tid >> 7;
    if (tid < 128) sh.zs[tid] = w[b0 + tid];
    for (int i = tid; i < 128 * 128; i += 256) sh.Ud[i >> 7][i & 127] = A[(int64_t)(b0 + (i >> 7)) * lda + b0 + (i & 127)];
    for (int i = tid; i < 8 * 256; i += 256) sh.inv[i >> 8][i & 255] = invDt[(int64_t)(b0 / 16) * 256 + i];
    // the block of the NEXT fold, U[blk rows, g columns], in registers before its l_blk arrives: this thread's column,
    // its half of the 128 rows
    double un[64];
    auto request_block = [&](int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 64; ++k) un[k] = A[(int64_t)(blk * 128 + 64 * half + k) * lda + b0 + c];
    };
    if (g > 0) request_block(0);
    __syncthreads();
    for (int blk = 0; blk < g; ++blk) {
        if (!chain_wait(out + blk * 128, info, spin_limit, sh)) return;        // l_blk is in sh.ab
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 64; ++k) acc = fma(un[k], sh.ab[64 * half + k], acc);
        if (blk + 1 < g) request_block(blk + 1);
        if (half == 1) sh.al[c] = acc;                            // (al is free until the diagonal solve)
        __syncthreads();
        if (half == 0) sh.zs[c] -= acc + sh.al[c];
        __syncthreads();
    }
    // the diagonal system, top tile first (forward_step_kernel's arithmetic on the LDS copies)
    for (int s = 0; s < 8; ++s) {
        const int o = 16 * s;
        if (tid < 64) {
            const int i = tid >> 2, part = tid & 3;
            const double *Y = sh.inv[s];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(Y[(4 * part + k) * 16 + i], sh.zs[o + 4 * part + k], acc);
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (part == 0) sh.al[o + i] = acc;
        }
        __syncthreads();
        if (tid >= o + 16 && tid < 128) {
            double acc = sh.zs[tid];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc = fma(-sh.Ud[o + k][tid], sh.al[o + k], acc);
            sh.zs[tid] = acc;
        }
        __syncthreads();
    }
    chain_publish(out + b0, sh.al);
}

// form 1 (CBO_HIP_VEC_SOLVE_FORM=1): the per-block launches.  `info` is the model's status word (0 after a fit).
static bool vec_chain_enabled(int nb, int form) { return form != 1 && nb >= 2; }

// ~151 KB of dynamic LDS needs the opt-in ON THE CURRENT DEVICE: done per call (cheap), as launch_cholesky does, so that
// every device of a process that drives several (cbo_comm_init_all) is covered -- a function-local static would cover
// only the device that was current at the first call.  false: the runtime refused, take the per-block launches.
static bool vec_chain_opt_in()
{
    const hipError_t a = hipFuncSetAttribute(reinterpret_cast<const void *>(backsolve_chain_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(VecChainShared));
    const hipError_t b = hipFuncSetAttribute(reinterpret_cast<const void *>(forward_chain_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(VecChainShared));
    if (a == hipSuccess && b == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

bool launch_backsolve_chain(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt,
                            const double *src, int64_t src_stride, double *work, double *out, int *info, int spin_limit,
                            int form)
{
    const int nb = (int)(n_pad / 128);
    if (!vec_chain_enabled(nb, form)) return false;
    if (!vec_chain_opt_in()) return false;
    hipLaunchKernelGGL(copy_strided_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, src, src_stride,
                       n_pad, work);
    hipLaunchKernelGGL(fill_sentinel_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, out, n_pad);
    hipLaunchKernelGGL(backsolve_chain_kernel, dim3(nb), dim3(256), sizeof(VecChainShared), s, A, lda, invDt, nb, work, out,
                       info, spin_limit);
    // a launch the runtime refused (nothing ran): the caller takes the per-block launches, which fill `out` themselves
    return hipGetLastError() == hipSuccess;
}

bool launch_forward_chain(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, const double *w,
                          double *out, int *info, int spin_limit, int form)
{
    const int nb = (int)(n_pad / 128);
    if (!vec_chain_enabled(nb, form)) return false;
    if (!vec_chain_opt_in()) return false;
    hipLaunchKernelGGL(fill_sentinel_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, out, n_pad);
    hipLaunchKernelGGL(forward_chain_kernel, dim3(nb), dim3(256), sizeof(VecChainShared), s, A, lda, invDt, nb, w, out,
                       info, spin_limit);
    return hipGetLastError() == hipSuccess;          // (forward_chain_kernel leaves `w` untouched: the fallback can still use it)
}

// dst[i] = V[i * ldv] for i < n_pad: one column of a row-major workspace as a contiguous vector
void launch_gather_column(hipStream_t s, const double *V, int64_t ldv, int64_t n_pad, double *dst)
{
    hipLaunchKernelGGL(copy_strided_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, V, ldv, n_pad, dst);
}

}  // namespace cbo

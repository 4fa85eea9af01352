// Device functions of the one-workgroup kernels, shared by the translation units that factor a block inside LDS
// (kernels_chol.hip: the blocked factorisation's diagonal block, small_lml_kernel; kernels_sets.hip: small_sets_kernel;
// kernels_sets_con.hip: small_sets_con_kernel; kernels_sets_batch.hip: small_sets_batch_kernel; kernels_loo.hip:
// small_loo_batch_kernel; kernels_hyper.hip:
// hyper_avg_kernel, hyper_sets_kernel): the register Cholesky of a 16x16 tile, the decoupled-wave factorisation of a 128-row block, the tile
// solve of a 128-row block for one wave's 16 columns, the model side of a small model (points, K(X,X) + diag, factor,
// inverses and z), and the stages of a one-workgroup sweep (a wave's candidates, K*, the solve with q and mu, the
// workgroup's arg-max, the set's reduction).  One definition, so every kernel that factors or sweeps a small model
// produces the same bits.  A function whose own arithmetic the compiler could contract says contract(off) itself, as
// cbo_device.h's do; the translation units that build kernels from the sweep stages say it again for their own text.
#pragma once

#include <atomic>

#include "cbo_device.h"

namespace cbo {

#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// ------------------------------------------------------------------------------------------------
constexpr int kDiagLd = 144;   // LDS row stride (doubles): rows kq and kq+1 of a fragment are 32 banks apart

// ------------------------------------------------------------------------------------------------
// Second form of the diagonal-block kernel: the same arithmetic per tile, decoupled waves.
//
// The block's chain is 8 tile factorisations of 16 dependent pivots each (wave 0); everything else -- the row panel
// X = inv(L_d) S[o:o+16, o+16:] and the rank-16 update of the trailing tiles -- is throughput work.  In the first
// form the four waves alternate between the two kinds of work with two barriers per tile, so the chain waits for
// the row panel and the other waves wait for the chain.  Here wave 0 runs one step ahead and touches nothing the
// other waves produce inside an interval:
//   interval jb:  wave 0     X01 = inv(L_jb) S(jb, jb+1);  S(jb+1, jb+1) -= X01^T X01 (registers);  factor tile jb+1
//                            (factor and inverse stay in LDS: the wave never waits on a global store)
//                 waves 1-3  each solves a third of the row panel X(jb, jb+1..8) (tiles ct with ct % 3 == w), leaves
//                            it in LDS and in global memory (finished factor rows), meets the other two at an LDS
//                            counter, reads the whole panel back into registers and updates its share of the trailing
//                            tiles T(ti, tj) -= X_ti^T X_tj from them (the f64 MFMA result map is both operand maps)
//   ONE workgroup barrier per interval; the rendezvous of waves 1-3 in the middle is theirs alone (an LDS counter), so
//   the chain never waits for it.  A solved tile overwrites its own unsolved image in S (only its owner read that),
//   except tile jb+1, which wave 0 reads in the same interval: that one goes to a spare tile below the diagonal
//   (rows 16..31, columns 0..15 -- the lower triangle of S is never loaded or read).  The diagonal-tile inverse is
//   double-buffered (wave 0 writes tile jb+1's while the others read tile jb's).  The right-hand side rides along as column tile 8 (the 16 spare columns of the LDS row
//   stride: column 128 = r, the rest zero), so z = L^-1 r needs no code of its own.
struct Diag2Shared {
    double S[128][kDiagLd];    // the block, upper triangle; columns 128..143: rhs tile (column 128) 
    double Yt[2][16][16];      // inverse of the diagonal factor of tile jb in Yt[jb & 1]: Yt[k][i] = inv(L_d)[i][k]
    int xcount;                // row-panel tiles published by waves 1-3 (their own rendezvous; wave 0 never waits on it)
    int pad_[3];
};

// Register Cholesky of one 16x16 tile given in the MFMA accumulator layout (d[r] = D[kq + 4r][lc], anything below
// the diagonal ignored); returns the factor in the same layout (zeros below the diagonal), writes the inverse to
// LDS (transposed: the A-operand image of the row-panel product) and to global memory (what the strip TRSM reads).
//
// The tile's 16 pivots are one dependent chain, so what counts is the number of dependent instructions per pivot
// (about 13 cycles each for fp64 VALU work in a lone wave; scripts/probes/tile_factor_probe.hip has the forms tried):
//   * pivots go in blocks of four.  One MFMA with a 0/1 selection operand replicates the block's four rows to every
//     16-lane row (t[r] = D[4b + r][lc] on all lane rows), so no cross-lane shuffle sits between two pivots;
//   * the block's 4x4 diagonal sub-block is factored FIRST, on uniform scalars (its ten entries read once with
//     v_readlane, every lane repeating the same arithmetic): per pivot the chain is rsqrt -> multiply -> fma.  The
//     16-wide row scalings and updates follow from those scalars, off the chain;
//   * rsqrt is ocml's instruction sequence (v_rsq_f64, one third-order correction) without its class-check selects,
//     and the positivity test only records the first bad pivot (reported once, after the tile) -- a non-positive pivot
//     lets NaN / Inf through the rest of the tile, which jitchol's retry discards anyway;
//   * a rank-4 MFMA carries the block into the rows below it.
// Every value goes through the same operations in the same order as the plain right-looking form.
// `blocks` (uniform) < 4: only the tile's first `blocks` blocks of four pivots are factored -- the rows of the others are
// identity padding (a model of fewer rows than its tiles hold), whose factor and inverse are the identity they already
// are; nothing a posterior reads depends on them.
__device__ __forceinline__ d4 factor_tile_regs(d4 din, int lane, int pivot_row0, int *info, double (*Yt)[16],
                                               double *__restrict__ invDt_tile, int blocks = 4)
{
    const int lc = lane & 15, kq = lane >> 4;
    d4 d, e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        d[r] = (kq + 4 * r <= lc) ? din[r] : 0.0;
        e[r] = (kq + 4 * r == lc) ? 1.0 : 0.0;
    }
    const double sel = ((lc >> 2) == kq) ? 1.0 : 0.0;       // A[i = lc][k = kq] = delta(k, i >> 2)
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (b >= blocks) break;
        d4 t = MFMA_F64(sel, d[b], zero);
        d4 s = MFMA_F64(sel, e[b], zero);
        double a[4][4], u[4][4], inv[4], dj[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) a[i][j] = readlane_f64(t[i], 4 * b + j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double pj = a[j][j];
            if (!(pj > 0.0) && bad == 0) bad = 4 * b + j + 1;
            const double y0 = __builtin_amdgcn_rsq(pj);
            const double tt = y0 * -pj;
            const double ee = fma(tt, y0, 1.0);
            const double gg = y0 * ee;
            const double hh = fma(ee, 0.375, 0.5);
            inv[j] = fma(gg, hh, y0);
            dj[j] = pj * inv[j];
#pragma unroll
            for (int k = j + 1; k < 4; ++k) u[j][k] = a[j][k] * inv[j];
#pragma unroll
            for (int i = j + 1; i < 4; ++i)
#pragma unroll
                for (int k = i; k < 4; ++k) a[i][k] = fma(-u[j][i], u[j][k], a[i][k]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int piv = 4 * b + j;
            t[j] = (lc > piv) ? t[j] * inv[j] : ((lc == piv) ? dj[j] : 0.0);
            s[j] *= inv[j];
#pragma unroll
            for (int i = j + 1; i < 4; ++i) {
                t[i] = fma(-u[j][i], t[j], t[i]);
                s[i] = fma(-u[j][i], s[j], s[i]);
            }
        }
        d[b] = (kq == 0) ? t[0] : (kq == 1) ? t[1] : (kq == 2) ? t[2] : t[3];
        e[b] = (kq == 0) ? s[0] : (kq == 1) ? s[1] : (kq == 2) ? s[2] : s[3];
        if (b < 3) {
            const d4 keep = d, keep_e = e;
            const double na = -d[b];
            d = MFMA_F64(na, d[b], d);
            e = MFMA_F64(na, e[b], e);
#pragma unroll
            for (int r = 0; r <= b; ++r) { d[r] = keep[r]; e[r] = keep_e[r]; }
        }
    }
    if (bad != 0 && lane == 0) atomicCAS(info, 0, pivot_row0 + bad);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        Yt[lc][kq + 4 * r] = e[r];
        if (invDt_tile) invDt_tile[lc * 16 + kq + 4 * r] = e[r];
    }
    return d;
}

// The trailing tiles one of waves 1..3 owns: columns {8, 3, 2}, {7, 4, 1}, {6, 5} (12, 12 and 11 tiles, balanced for
// every step since a column loses one tile per step), listed by row so that the tiles still due form a suffix.
template <int W>
struct DiagTiles;
template <>
struct DiagTiles<0> {
    static constexpr int n = 12;
    static constexpr int ti[12] = {1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 6, 7};
    static constexpr int tj[12] = {2, 3, 8, 2, 3, 8, 3, 8, 8, 8, 8, 8};
};
template <>
struct DiagTiles<1> {
    static constexpr int n = 12;
    static constexpr int ti[12] = {1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 7};
    static constexpr int tj[12] = {1, 4, 7, 4, 7, 4, 7, 4, 7, 7, 7, 7};
};
template <>
struct DiagTiles<2> {
    static constexpr int n = 12;      // the last entry repeats a tile and is never written
    static constexpr int ti[12] = {1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6};
    static constexpr int tj[12] = {5, 6, 5, 6, 5, 6, 5, 6, 5, 6, 6, 6};
};

template <int W>
__device__ __forceinline__ void diag_trailing(Diag2Shared &sh, const d4 (&x)[9], const d4 (&nx)[9], int jb, int lane,
                                              int tiles)
{
    using L = DiagTiles<W>;
    const int lc = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int g = 0; g < L::n; g += 4) {
        // the group's last tile has the largest row index: nothing due in the group -> skip it (uniform); its first
        // tile the smallest: a group entirely inside the identity padding of a short block has nothing to do either
        if (L::ti[g + 3] <= jb || L::ti[g] >= tiles) continue;
        d4 acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[k][r] = sh.S[16 * L::ti[g + k] + kq + 4 * r][16 * L::tj[g + k] + lc];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = MFMA_F64(x[L::ti[g + k]][r], nx[L::tj[g + k]][r], acc[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ti = L::ti[g + k], tj = L::tj[g + k];
            const bool dup = (W == 2 && g + k == 11);
            if (!dup && ti > jb && !(ti == tj && ti == jb + 1)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sh.S[16 * ti + kq + 4 * r][16 * tj + lc] = acc[k][r];
            }
        }
    }
}

// A store of the factor that a workgroup of the SAME launch may read (the strips of the fused diagonal + panel launch):
// written through to the coherence point of the device instead of resting in this XCD's L2.
// Fences of the fused diagonal + panel protocol (see potrf_panel_fused_kernel).  The consumer's ACQUIRE is always there
// (1-2 % of the chain).  The producer's RELEASE is a build option: LLVM implements an agent-scope release on gfx950 as
// buffer_wbl2 sc1 -- a write-back of the whole XCD's L2, which at that moment also holds the dirty lines of the bulk
// trailing update running beside the chain -- and it costs 17 % of the factorisation at 4096 points (1.55 -> 1.82 ms;
// 31.9 -> 33.8 ms at 16384; A/B on one box, round 3).  The default producer instead relies on what its stores are on
// this hardware: agent-scope atomic stores (global_store ... sc1, written through to the device's coherence point),
// retired by s_waitcnt vmcnt(0) before the count is incremented.  -DCBO_FORMAL_RELEASE restores the fence.
#ifdef CBO_FORMAL_RELEASE
#define AGENT_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
#else
#define AGENT_RELEASE()
#endif
#define AGENT_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
// The chain's kernels share SIMDs with the bulk update's (and a pipelined sweep's) MFMA waves: their instructions go first.
#ifndef CBO_CHAIN_PRIO
#define CBO_CHAIN_PRIO 3
#endif
#define CHAIN_PRIORITY() __builtin_amdgcn_s_setprio(CBO_CHAIN_PRIO)
template <bool PUBLISH>
__device__ __forceinline__ void gstore(double *p, double v)
{
    if (PUBLISH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// One interval of one of waves 1..3 (W = wave - 1): its third of the row panel, the rendezvous, its trailing tiles.
// The wave with W == jb % 3 also carries tile jb's diagonal factor and inverse from LDS (where wave 0 left them) to
// global memory: the chain wave itself never waits on a global store.  PUBLISH: after its last store of the interval
// the wave counts itself in at `flag` (row tile jb of the factor is complete when the count reaches 3 (jb + 1)).
template <int W, bool PUBLISH>
__device__ __forceinline__ void diag_worker(Diag2Shared &sh, double *A, int64_t lda, int r0, int rcol,
                                            double *__restrict__ invDt, double *__restrict__ zvec, int jb,
                                            const double (&af)[4], int lane, int tiles, int *flag)
{
    const int lc = lane & 15, kq = lane >> 4;
    const int o = 16 * jb;
    constexpr int ct0 = (W == 0) ? 3 : W;                 // own column tiles: ct0, ct0 + 3, ct0 + 6 (<= 8; 8 = rhs)
    constexpr int nown = (ct0 + 6 <= 8) ? 3 : 2;
    // tiles that are not due (ct <= jb) are solved along on whatever S holds there (cheaper than branching around a
    // chain of four MFMAs) and stored nowhere
    if (W == jb % 3) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gstore<PUBLISH>(&A[(int64_t)(r0 + o + kq + 4 * r) * lda + r0 + o + lc], sh.S[o + kq + 4 * r][o + lc]);
            gstore<PUBLISH>(&invDt[(int64_t)(r0 / 16 + jb) * 256 + lc * 16 + kq + 4 * r], sh.Yt[jb & 1][lc][kq + 4 * r]);
        }
    }
    d4 xo[nown];
    {
        double bq[4][nown];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int n = 0; n < nown; ++n) bq[kk][n] = sh.S[o + 4 * kk + kq][16 * (ct0 + 3 * n) + lc];
#pragma unroll
        for (int n = 0; n < nown; ++n) xo[n] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int n = 0; n < nown; ++n) xo[n] = MFMA_F64(af[kk], bq[kk][n], xo[n]);
    }
#pragma unroll
    for (int n = 0; n < nown; ++n) {
        const int ct = ct0 + 3 * n;
        if (ct == jb + 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sh.S[16 + kq + 4 * r][lc] = xo[n][r];
        } else if (ct > jb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sh.S[o + kq + 4 * r][16 * ct + lc] = xo[n][r];
        }
    }
    // publish, then wait for the other two (LDS operations of a wave complete in order; the counter only grows)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_fetch_add(&sh.xcount, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    // rows o .. o+15 of the factor right of the diagonal tile, and z, leave for global memory meanwhile
#pragma unroll
    for (int n = 0; n < nown; ++n) {
        const int ct = ct0 + 3 * n;
        if (ct > jb) {
            if (ct < 8) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    gstore<PUBLISH>(&A[(int64_t)(r0 + o + kq + 4 * r) * lda + r0 + 16 * ct + lc], xo[n][r]);
            } else if (lc == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + o + kq + 4 * r;
                    A[(int64_t)row * lda + rcol] = xo[n][r];
                    if (zvec) zvec[row] = xo[n][r];
                }
            }
        }
    }
    if (PUBLISH && W == jb % 3) {
        // tile jb's inverse (and diagonal factor) are out: flag[1] counts them.  The wait overlaps the rendezvous.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        AGENT_RELEASE();                                       // the count is a release of this wave's stores
        if (lane == 0) __hip_atomic_fetch_add(flag + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    while (__hip_atomic_load(&sh.xcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 3 * (jb + 1))
        __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // the whole panel into registers (tiles <= jb are finished rows whose products nobody stores: zeros)
    d4 x[9], nx[9];
#pragma unroll
    for (int ct = 1; ct <= 8; ++ct) {
        if (ct == jb + 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) x[ct][r] = sh.S[16 + kq + 4 * r][lc];
        } else if (ct > jb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) x[ct][r] = sh.S[o + kq + 4 * r][16 * ct + lc];
        } else {
            x[ct] = d4{0.0, 0.0, 0.0, 0.0};
        }
        nx[ct] = -x[ct];
    }
    // trailing tiles T(ti, tj) -= X_ti^T X_tj, jb < ti <= 7, ti <= tj <= 8, except the next diagonal tile (wave 0's).
    // Ownership is by column (a compile-time list per wave), tiles go four at a time with their accumulation chains
    // interleaved; a tile that is not due (ti <= jb) is computed on stale operands and simply not written back.
    diag_trailing<W>(sh, x, nx, jb, lane, tiles);
    if (PUBLISH) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's write-through stores have arrived
        AGENT_RELEASE();
        if (lane == 0) __hip_atomic_fetch_add(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The factorisation of a block that is already in LDS (S: upper triangle + rhs tile; the caller has synchronised).
// `tiles` = 16-row tiles to factor (8 = the whole block; fewer when the rest is identity padding, which the caller
// then writes out itself).  Factor rows, diagonal inverses and z go to global memory (A, invDt, zvec).
template <bool PUBLISH = false>
__device__ __forceinline__ void diag128_factor_in_lds(Diag2Shared &sh, double *A, int64_t lda, int r0, int rcol,
                                                      double *__restrict__ invDt, int *info,
                                                      double *__restrict__ zvec, int tiles, int *flag = nullptr,
                                                      int last_blocks = 4)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    if (tid == 64) sh.xcount = 0;
    if (wave == 0) {
        d4 t0;
#pragma unroll
        for (int r = 0; r < 4; ++r) t0[r] = sh.S[kq + 4 * r][lc];
        // the factor of the tile stays in LDS, in the tile's own place (nobody else touches it): a worker wave takes
        // it and the inverse to global memory in the tile's interval
        const d4 u = factor_tile_regs(t0, lane, r0, info, sh.Yt[0], nullptr, tiles == 1 ? last_blocks : 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) sh.S[kq + 4 * r][lc] = u[r];
    }
    __syncthreads();

    for (int jb = 0; jb < tiles; ++jb) {
        const int o = 16 * jb;
        double af[4];                                       // A operand of the row-panel product: inv(L_jb)[lc][4 kk + kq]
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) af[kk] = sh.Yt[jb & 1][4 * kk + kq][lc];
        if (wave == 0) {
            if (jb + 1 < tiles) {
                // two half-sums each: a chain of dependent f64 MFMAs runs at about half the issue rate
                d4 x = {0.0, 0.0, 0.0, 0.0}, xb = {0.0, 0.0, 0.0, 0.0}, acc, accb = {0.0, 0.0, 0.0, 0.0};
                double bq[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) bq[kk] = sh.S[o + 4 * kk + kq][o + 16 + lc];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = sh.S[o + 16 + kq + 4 * r][o + 16 + lc];
                x = MFMA_F64(af[0], bq[0], x);
                xb = MFMA_F64(af[1], bq[1], xb);
                x = MFMA_F64(af[2], bq[2], x);
                xb = MFMA_F64(af[3], bq[3], xb);
                x += xb;
                acc = MFMA_F64(x[0], -x[0], acc);
                accb = MFMA_F64(x[1], -x[1], accb);
                acc = MFMA_F64(x[2], -x[2], acc);
                accb = MFMA_F64(x[3], -x[3], accb);
                acc += accb;
                const d4 u = factor_tile_regs(acc, lane, r0 + o + 16, info, sh.Yt[(jb + 1) & 1], nullptr,
                                              jb + 2 == tiles ? last_blocks : 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) sh.S[o + 16 + kq + 4 * r][o + 16 + lc] = u[r];
            }
        } else {
            const int w = wave - 1;
            if (w == 0) diag_worker<0, PUBLISH>(sh, A, lda, r0, rcol, invDt, zvec, jb, af, lane, tiles, flag);
            else if (w == 1) diag_worker<1, PUBLISH>(sh, A, lda, r0, rcol, invDt, zvec, jb, af, lane, tiles, flag);
            else diag_worker<2, PUBLISH>(sh, A, lda, r0, rcol, invDt, zvec, jb, af, lane, tiles, flag);
        }
        __syncthreads();
    }
}

// The eight (or `tiles`) tile steps of a 128-row block solve for one wave's 16 columns: acc[t] = right-hand sides of
// tile t in the MFMA result layout, iv = the diagonal inverses as A operands, ub = &U[kq][lc] of the block in LDS;
// emit(s, x) receives tile s of the solution.  x_s = inv(L_ss) r_s (two half-sums), tile s+1 brought up to date first,
// its solve chain interleaved with the rest of tile s's updates.
template <typename Emit>
__device__ __forceinline__ void panel_solve_tiles(const double *ub, d4 (&acc)[8], const double (&iv)[8][4], int tiles,
                                                  Emit emit)
{
    d4 x = {0.0, 0.0, 0.0, 0.0}, x2 = {0.0, 0.0, 0.0, 0.0};
    x = MFMA_F64(iv[0][0], acc[0][0], x);
    x2 = MFMA_F64(iv[0][1], acc[0][1], x2);
    x = MFMA_F64(iv[0][2], acc[0][2], x);
    x2 = MFMA_F64(iv[0][3], acc[0][3], x2);
    x += x2;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        emit(s, x);
        if (s == 7 || s + 1 >= tiles) break;
        const d4 nx = -x;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            acc[s + 1] = MFMA_F64(ub[(16 * s + 4 * kk) * kDiagLd + 16 * (s + 1)], nx[kk], acc[s + 1]);
            if (s + 2 < 8) acc[s + 2] = MFMA_F64(ub[(16 * s + 4 * kk) * kDiagLd + 16 * (s + 2)], nx[kk], acc[s + 2]);
        }
        d4 y1 = {0.0, 0.0, 0.0, 0.0}, y2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk & 1) y2 = MFMA_F64(iv[s + 1][kk], acc[s + 1][kk], y2);
            else y1 = MFMA_F64(iv[s + 1][kk], acc[s + 1][kk], y1);
#pragma unroll
            for (int t = s + 3; t < 8; ++t) acc[t] = MFMA_F64(ub[(16 * s + 4 * kk) * kDiagLd + 16 * t], nx[kk], acc[t]);
        }
        x = y1 + y2;
    }
}

// ------------------------------------------------------------------------------------------------
// Small models, many sets, ONE launch (the reference's own operating point: N = 10..50 observations per exploration
// set, S = 2..25 sets, /root/reference/src/ArgumentParser.py:18,25, src/CBO.py:237-260).  At that size every kernel of
// the general path is launch latency: K(X,X), eight chain launches, K*, the strip solve, the epilogue, a stream
// synchronisation -- per set.  Here one workgroup does all of it for (one set, 64 candidates) inside LDS and
// registers, with the SAME device functions as the general path (kernel_value, the decoupled-wave block
// factorisation, the tile solve, the EI epilogue), so the numbers are the general path's numbers:
//   K(X,X) + diag  ->  LDS block (identity beyond n)       rhs r = y - m(X)  ->  column tile 8
//   factorisation of the ceil(n/16) tiles that are not padding  (factor rows, inverses, z to a per-workgroup scratch)
//   K(X, X*) of the workgroup's 64 candidates straight into the MFMA result registers
//   V = L^-1 K*,  q = sum V^2,  mu = V^T z,  variance, mean, EI / cost, arg-max over the 64 candidates
// A second, tiny launch reduces the per-workgroup winners of every set.  Every workgroup of a set repeats the
// set's factorisation (no inter-workgroup dependency; it is a few microseconds).
struct SmallShared {
    Diag2Shared blk;           // Ky / factor workspace, later the factor itself for the solve
    double xs[CBO_MAX_DIM][128];
    double sq[128], sv[128];
};
static_assert(sizeof(SmallShared) <= 163840, "one workgroup per CU");

// Opts a kernel whose dynamic LDS is SmallShared in to the whole CU's LDS, once per device: `opted` is the caller's static
// mask of the devices done, one per kernel instantiation (several devices in one process each need it; a failed attempt
// is repeated by the next call; the launch itself reports what is wrong if it never succeeds) -- the call costs a
// microsecond of the forty a reference-scale trial takes.
inline void small_lds_opt_in(const void *kernel, std::atomic<unsigned long long> &opted)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || !((opted.load(std::memory_order_relaxed) >> (dev & 63)) & 1ull)) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SmallShared)) == hipSuccess)
            opted.fetch_or(1ull << (dev & 63), std::memory_order_relaxed);
    }
}

constexpr int kSmallLd = kDiagLd;                              // scratch factor rows: [128][144], z in column 128
constexpr int kSmallScratch = 128 * kSmallLd + 8 * 256;        // doubles per workgroup: factor rows + inverses

template <int D>
__device__ __forceinline__ void small_assemble(SmallShared &sh, const cbo_small_set &st, int tiles)
{
    const int tid = threadIdx.x;
    const int i = tid >> 4, j = tid & 15;
    const double inv_l2 = 1.0 / (st.lengthscale * st.lengthscale);
    const bool causal = st.sv != nullptr;
    // Four tile pairs at a time, no branch around a value: one wave per SIMD has nothing to hide an exp's dependent
    // chain behind but the next value's chain (the points beyond n are zeros in LDS: computed, then replaced).
    int ti = 0, tj = 0;                                                // (uniform)
    while (ti < tiles) {
        int gis[4], gjs[4];
        bool due[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            due[u] = ti < tiles;
            gis[u] = 16 * (due[u] ? ti : 0) + i;
            gjs[u] = 16 * (due[u] ? tj : 0) + j;
            if (++tj >= tiles) { ++ti; tj = ti; }
        }
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int gi = gis[u], gj = gjs[u];
            double xi[D], xj[D];
#pragma unroll
            for (int k = 0; k < D; ++k) { xi[k] = sh.xs[k][gi]; xj[k] = sh.xs[k][gj]; }
            double w = kernel_value<D>(xi, xj, sh.sq[gi], sh.sq[gj], st.variance, inv_l2, st.zero_diag && gi == gj);
            if (causal) w = __dadd_rn(w, __dmul_rn(sh.sv[gi], sh.sv[gj]));
            const double wd = __dadd_rn(w, st.diag_add);               // Ky = K + (noise + 1e-8) I
            w = (gi == gj) ? wd : w;
            const double pad = (gi == gj) ? 1.0 : 0.0;                 // identity padding
            v[u] = (gi < st.n && gj < st.n) ? w : pad;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (due[u]) sh.blk.S[gis[u]][gjs[u]] = v[u];
    }
}

// The model side of the one-workgroup kernels: points -> LDS, K(X,X) + diag and the rhs into the block, the
// factorisation of the `tiles` real tiles (factor rows, inverses, z to the workgroup's scratch), the factor back into
// LDS (what a tile solve reads), the inverses and z into registers.  Ends with loads in flight: the caller waits
// (s_waitcnt vmcnt(0) + barrier) before the solve.
// `phases`: 1 = points + assembly + factorisation only (the factor stays in the scratch), 2 = points + the factor from
// the scratch (somebody factored the model before this launch), 3 = both.
__device__ __forceinline__ void small_model_factor(SmallShared &sh, const cbo_small_set &st, int tiles, double *Us,
                                                   double *invs, int *info_word, double (&iv)[8][4], double (&zr)[8][4],
                                                   int phases = 3, bool skip_padding = false)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, kq = lane >> 4;
    // ---- the model's points and K(X,X) + diag, rhs, zero fill of what the factorisation reads beyond the tiles
    // staged: the model's new data are still in the caller's staging buffer (cbo_trial_step): prepared here, from there, with
    // prep_points_staged_kernel's arithmetic; the set's first workgroup also writes the resident copies
    const bool staged = st.stage != nullptr && (phases & 1);
    const bool writer = staged && blockIdx.x == 0;
    const double *ysrc = staged ? st.stage + (int64_t)st.n * st.d : st.y;
    const double *pmsrc = staged ? (st.sv ? st.stage + (int64_t)st.n * st.d + st.n : nullptr) : st.pm;
    double staged_y = 0.0, staged_pm = 0.0;
    if (tid < 128) {
        const bool in = tid < st.n;
        if (staged) {
            double x[CBO_MAX_DIM];
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k) x[k] = 0.0;
            double pvi = 0.0;
            if (in) {
                // (y and the prior mean are fetched with the points: one trip across the host link, not two)
                staged_y = ysrc[tid];
                if (pmsrc) staged_pm = pmsrc[tid];
#pragma unroll
                for (int k = 0; k < CBO_MAX_DIM; ++k)
                    if (k < st.d) {
                        double v = st.stage[(int64_t)tid * st.d + k];
                        if (writer) st.raw[(int64_t)tid * st.d + k] = v;
                        if (st.stage_ls) v = v / st.stage_ls[k];
                        x[k] = v;
                    }
                if (st.sv) pvi = st.stage[(int64_t)st.n * st.d + 2 * st.n + tid];
            }
            const double sum = squared_norm(x, st.d);
            const double svi = (in && st.sv) ? sqrt(pvi) : 0.0;
#pragma unroll
            for (int k = 0; k < CBO_MAX_DIM; ++k)
                if (k < st.d) sh.xs[k][tid] = x[k];
            sh.sq[tid] = sum;
            sh.sv[tid] = svi;
            if (writer) {
#pragma unroll
                for (int k = 0; k < CBO_MAX_DIM; ++k)
                    if (k < st.d) const_cast<double *>(st.xs)[(int64_t)k * st.ld + tid] = x[k];
                const_cast<double *>(st.sq)[tid] = sum;
                if (st.sv) const_cast<double *>(st.sv)[tid] = svi;
                if (in) {
                    const_cast<double *>(st.y)[tid] = staged_y;
                    if (st.sv) {
                        const_cast<double *>(st.pm)[tid] = staged_pm;
                        st.pv[tid] = pvi;
                    }
                }
            }
        } else {
            if (in && (phases & 1)) {                     // (with the points: the rhs does not wait for a second trip)
                staged_y = ysrc[tid];
                if (pmsrc) staged_pm = pmsrc[tid];
            }
            for (int k = 0; k < st.d; ++k) sh.xs[k][tid] = in ? st.xs[(int64_t)k * st.ld + tid] : 0.0;
            sh.sq[tid] = in ? st.sq[tid] : 0.0;
            sh.sv[tid] = (in && st.sv) ? st.sv[tid] : 0.0;
        }
    }
    __syncthreads();
    if (phases & 1) {
    CBO_FOR_DIM(st.d, small_assemble<D>(sh, st, tiles));
    {
        const int rows = 16 * tiles;
        for (int r = tid >> 4; r < rows; r += 16)
            for (int c = rows + (tid & 15); c < kDiagLd; c += 16) {
                if (c == 128 && r < st.n) continue;                                            // (the rhs: below)
                sh.blk.S[r][c] = 0.0;
            }
        if (tid < st.n) sh.blk.S[tid][128] = pmsrc ? __dadd_rn(staged_y, -staged_pm) : staged_y;   // r = y - m(X)
    }
    __syncthreads();
    diag128_factor_in_lds(sh.blk, Us, kSmallLd, 0, 128, invs, info_word, nullptr, tiles, nullptr,
                          skip_padding ? (st.n - 16 * (tiles - 1) + 3) / 4 : 4);
    // (ends with a barrier.)  Every wave's stores of factor rows / inverses / z are complete before anyone re-reads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    }
    if (!(phases & 2)) return;

    // ---- the factor back into LDS (rows of the factored tiles; the solve reads nothing else), inverses and z to registers
    {
        const unsigned s0 = lds_byte_address(&sh.blk.S[0][0]);
        const int rows = 16 * tiles;
        for (int p = wave; p < rows; p += 4)
            glds16(Us + (int64_t)p * kSmallLd + lane * 2, __builtin_amdgcn_readfirstlane(s0 + 8u * (unsigned)(p * kDiagLd)));
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            iv[s][kk] = (s < tiles) ? invs[s * 256 + (4 * kk + kq) * 16 + lc] : 0.0;
            zr[s][kk] = (s < tiles) ? Us[(int64_t)(16 * s + kq + 4 * kk) * kSmallLd + 128] : 0.0;
        }
}

template <int D>
__device__ __forceinline__ double small_kstar(const SmallShared &sh, const cbo_small_set &st, int row, const double *xc,
                                              double csq, double csv, double inv_l2)
{
    // (no branch around the value -- the four of a tile interleave; rows beyond n are zeros in LDS)
    double xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = sh.xs[k][row];
    double v = kernel_value<D>(xi, xc, sh.sq[row], csq, st.variance, inv_l2, false);
    const double vc = __dadd_rn(v, __dmul_rn(sh.sv[row], csv));
    v = (st.sv != nullptr) ? vc : v;
    return (row < st.n) ? v : 0.0;
}

template <int D>
__device__ __forceinline__ void small_kstar_tiles(const SmallShared &sh, const cbo_small_set &st, int tiles,
                                                  const double *xc, double csq, double csv, double inv_l2, int kq,
                                                  d4 (&acc)[8])
{
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < tiles) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = small_kstar<D>(sh, st, 16 * t + kq + 4 * r, xc, csq, csv, inv_l2);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
        }
    }
}

// ---- the stages of a one-workgroup sweep, in the order a kernel runs them ---------------------------------------------
// phases == 1 of a two-launch form: factor the model into the slot `fs`, nothing else
__device__ __forceinline__ void small_factor_only(SmallShared &sh, const cbo_small_set &st, double *fs, int *info_word)
{
    double ivx[8][4], zrx[8][4];
    small_model_factor(sh, st, (st.n + 15) / 16, fs, fs + 128 * kSmallLd, info_word, ivx, zrx, 1, true);
}

// Candidate c of the set as this lane's column: scaled coordinates, |x|^2, sqrt(v) and the prior closures (zeros for a
// non-causal set).  Clamped: lanes beyond the set compute, nobody looks.  Fetched before the factorisation, used after it
// (their latency is off the chain).
__device__ __forceinline__ void small_fetch_cand(const cbo_small_set &st, int64_t c, double (&xc)[CBO_MAX_DIM], double &csq,
                                                 double &csv, double &cpm_c, double &cpv_c)
{
    const int64_t cc = (c < st.m) ? c : st.m - 1;
#pragma unroll
    for (int k = 0; k < CBO_MAX_DIM; ++k) xc[k] = (k < st.d) ? st.cxs[(int64_t)k * st.cld + cc] : 0.0;
    csq = st.csq[cc];
    csv = st.csv ? st.csv[cc] : 0.0;
    cpm_c = st.cpm ? st.cpm[cc] : 0.0;
    cpv_c = st.cpv ? st.cpv[cc] : 0.0;
}

// ... and its own cost from the set's cost vector, under the same clamp
__device__ __forceinline__ void small_fetch_cand(const cbo_small_set &st, int64_t c, double (&xc)[CBO_MAX_DIM], double &csq,
                                                 double &csv, double &cpm_c, double &cpv_c, const double *__restrict__ cost,
                                                 double &cost_c)
{
    small_fetch_cand(st, c, xc, csq, csv, cpm_c, cpv_c);
    cost_c = cost[(c < st.m) ? c : st.m - 1];
}

// K(X, X*) of one wave's 16 candidates, straight into the MFMA result layout: small_kstar_tiles<d> (d uniform)
__device__ __forceinline__ void small_kstar_tiles_of(const SmallShared &sh, const cbo_small_set &st, int tiles,
                                                     const double *xc, double csq, double csv, double inv_l2, int kq,
                                                     d4 (&acc)[8])
{
    CBO_FOR_DIM(st.d, small_kstar_tiles<D>(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc));
}

// V = L^-1 K* of one wave's 16 candidates, q = sum V^2, mu = V^T z: lane partials, then over the four lane groups (the strip
// kernel's order).  The factor must be in LDS: the caller has waited (s_waitcnt vmcnt(0)) and synchronised.
// keep(s, x): tile s of V as panel_solve_tiles emits it (x[r] = V[16 s + kq + 4 r][this lane's candidate]), for a caller
// that stores V (small_sets_batch_kernel); it takes no part in q and mu.
template <class Keep>
__device__ __forceinline__ void solve_q_mu_keep(const SmallShared &sh, d4 (&acc)[8], const double (&iv)[8][4],
                                                const double (&zr)[8][4], int tiles, int kq, int lc, double &qacc,
                                                double &macc, Keep keep)
{
#pragma clang fp contract(off)
    qacc = 0.0;
    macc = 0.0;
    panel_solve_tiles(&sh.blk.S[kq][lc], acc, iv, tiles, [&](int s, const d4 &x) {
        keep(s, x);
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
__device__ __forceinline__ void solve_q_mu(const SmallShared &sh, d4 (&acc)[8], const double (&iv)[8][4],
                                           const double (&zr)[8][4], int tiles, int kq, int lc, double &qacc, double &macc)
{
    solve_q_mu_keep(sh, acc, iv, zr, tiles, kq, lc, qacc, macc, [](int, const d4 &) {});
}

// posterior_of's and the epilogues' scalars from a descriptor (the predictive variance includes the noise)
__device__ __forceinline__ AcqParams small_acq_params(const cbo_small_set &st)
{
    AcqParams p;
    p.variance = st.variance; p.noise_var = st.noise_var; p.y_best = st.y_best; p.ei_jitter = st.ei_jitter;
    p.cost = st.cost; p.task = st.task; p.include_noise = 1; p.want_ei = 1;
    return p;
}

// The plug-in incumbent of the workgroup's model (small_sets_kernel<CBO_ACQ_MPEI>, small_sets_refine_kernel<CBO_ACQ_MPEI>): min (task 'min') or max of the posterior means at the model's own n <= 128
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
#pragma clang fp contract(off)
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
        small_kstar_tiles_of(sh, st, tiles, xc, csq, csv, inv_l2, kq, acc);
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

// The workgroup's arg-max of the lanes' (bv, bi): the waves' shuffle trees, then thread 0 over the four waves -- whose
// (bv, bi) are the workgroup's winner on return, which is where small_set_finish begins.  The waves' winners pass
// through sh.sq / sh.sv.  Precondition: sh.sq and sh.sv are dead -- no wave reads the model's |x|^2 and sqrt(v) again
// once it is here (their last readers are K* and the plug-in incumbent, before the solve); the first barrier below is
// what keeps a fast wave from writing while a slow one is still at those reads.
// (lane, wave: the caller's -- a second readfirstlane here cost the constrained kernel 3 % more instructions.)
__device__ __forceinline__ void small_block_argmax(SmallShared &sh, int lane, int wave, double &bv, int64_t &bi)
{
    wave_argmax(bv, bi);
    double *red_v = &sh.sq[0];
    int64_t *red_i = reinterpret_cast<int64_t *>(&sh.sv[0]);
    __syncthreads();
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (better(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
    }
}

// The last workgroup of a set to finish (an atomic ticket) reduces the set's per-workgroup winners, hands the result
// record to the host (pinned, device-mapped memory; `seq` is stored last, after a system-scope fence, so that the host
// can poll it) and re-arms the set's status word and ticket for the next call.  Three steps, so that a kernel whose last
// arriver goes on working for the set (small_sets_batch_kernel) takes them one by one:
// the workgroup's winner to its slot and the ticket; true (every thread) in the set's last workgroup to arrive.
// PUBLISH: the workgroup has stored more than its winner for the last arriver to read (every storing wave has drained
// vmcnt(0) ahead of a barrier): the ticket is an agent-scope release of all of it -- the fence, its own wait, the add.
template <bool PUBLISH = false>
__device__ __forceinline__ bool small_set_ticket(double bv, int64_t bi, int set, int slot, int blocks_per_set,
                                                 double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                 int *__restrict__ ticket, int *last_flag)
{
    if (threadIdx.x == 0) {
        part_val[slot] = bv;
        part_idx[slot] = bi;
        if (PUBLISH) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            __threadfence();
        }
        *last_flag = (atomicAdd(&ticket[set], 1) == blocks_per_set - 1) ? 1 : 0;
    }
    __syncthreads();
    return *last_flag != 0;
}
// wave 0 of the last arriver: the set's winner and status word (thread 0's on return)
__device__ __forceinline__ void small_set_reduce(int set, int blocks_per_set, const double *__restrict__ part_val,
                                                 const int64_t *__restrict__ part_idx, int *__restrict__ info, double &bv,
                                                 int64_t &bi, int &status)
{
    const int tid = threadIdx.x;
    status = (tid == 0) ? atomicAdd(&info[set], 0) : 0;                 // (in flight with the loads below)
    bv = -INFINITY;
    bi = INT64_MAX;
    for (int b = tid; b < blocks_per_set; b += 64) {
        const double v = __builtin_nontemporal_load(&part_val[set * blocks_per_set + b]);
        const int64_t i = __builtin_nontemporal_load(&part_idx[set * blocks_per_set + b]);
        if (better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    wave_argmax(bv, bi);
}
// thread 0 of the last arriver: the record, then the set's words re-armed
__device__ __forceinline__ void small_set_record(double bv, int64_t bi, int status, int set, int *__restrict__ info,
                                                 int *__restrict__ ticket, cbo_small_result *__restrict__ out, int seq)
{
    out[set].best_val = bv;
    out[set].best_idx = bi;
    out[set].info = status;
    __threadfence_system();
    *reinterpret_cast<volatile int *>(&out[set].seq) = seq;
    info[set] = 0;
    ticket[set] = 0;
}
__device__ __forceinline__ void small_set_finish(double bv, int64_t bi, int set, int slot, int blocks_per_set,
                                                 double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                 int *__restrict__ info, int *__restrict__ ticket,
                                                 cbo_small_result *__restrict__ out, int seq, int *last_flag)
{
    if (!small_set_ticket(bv, bi, set, slot, blocks_per_set, part_val, part_idx, ticket, last_flag) || threadIdx.x >= 64)
        return;
    __threadfence();
    int status;
    small_set_reduce(set, blocks_per_set, part_val, part_idx, info, bv, bi, status);
    if (threadIdx.x == 0) small_set_record(bv, bi, status, set, info, ticket, out, seq);
}

// Up to kSmallByValue descriptors travel as kernel arguments (no read across the host link before the first
// instruction that needs them); longer lists are read from the pinned array.
constexpr int kSmallByValue = 8;
struct SmallSetArgs { cbo_small_set s[kSmallByValue]; };

}  // namespace cbo

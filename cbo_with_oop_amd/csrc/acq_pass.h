// The candidate pass of the single-model acquisition epilogues: acq_kernel (kernels_acq.hip), pointwise_acq_kernel
// (kernels_pointwise.hip) and mes_acq_kernel (kernels_mes.hip) are acq_pass with their scoring; constrained_acq_kernel
// (kernels_con.hip), whose step is one model's term, keeps its own loop around fetch_pair / store_pair.  DESIGN.md §4t.
#pragma once
#include "cbo_device.h"

namespace cbo {

// The pass's workgroup: block_argmax's 256 threads (the kernels' __launch_bounds__ and their launchers' block size).  A
// constant, not blockDim.x: read inside a device function the workgroup size comes through a vector load and a wait in
// front of the first fetch (the kernels' own reads of it are scalar loads).
constexpr int kPassThreads = 256;

// Operands of the pair of candidates at base + 2 tid of one workgroup (the second of an odd tail: a copy of the first,
// never stored); nothing is read at or beyond m, and where there is nothing to read the registers keep their values.
// The workgroup's first candidate, base, is uniform (scalar registers) and the lane's share of the address a constant 16 tid
// bytes: every access is "scalar base + 32-bit lane offset".  causal: pm and pv are read too (uniform; a constant where the
// kernel knows it at compile time).  COST (compile time): a fifth stream, the candidates' own costs, into
// *c2 -- fetched beside the others under the same tail decision; without it cost and c2 are not looked at.
template <bool COST = false>
__device__ __forceinline__ void fetch_pair(const double *__restrict__ q, const double *__restrict__ mu,
                                           const double *__restrict__ pm, const double *__restrict__ pv, bool causal,
                                           int64_t m, int64_t base, d2 &q2, d2 &mu2, d2 &pm2, d2 &pv2,
                                           const double *__restrict__ cost = nullptr, d2 *c2 = nullptr)
{
    const unsigned lane2 = 2 * threadIdx.x;
    constexpr int64_t span = 2 * kPassThreads;
    if (base + span <= m) {                                      // (uniform) every lane has its two candidates
        q2 = *reinterpret_cast<const d2 *>(q + base + lane2);
        mu2 = *reinterpret_cast<const d2 *>(mu + base + lane2);
        if (causal) {
            pm2 = *reinterpret_cast<const d2 *>(pm + base + lane2);
            pv2 = *reinterpret_cast<const d2 *>(pv + base + lane2);
        }
        if constexpr (COST) *c2 = *reinterpret_cast<const d2 *>(cost + base + lane2);
        return;
    }
    const int64_t at = base + lane2;
    if (at + 1 < m) {
        q2 = *reinterpret_cast<const d2 *>(q + at);
        mu2 = *reinterpret_cast<const d2 *>(mu + at);
        if (causal) {
            pm2 = *reinterpret_cast<const d2 *>(pm + at);
            pv2 = *reinterpret_cast<const d2 *>(pv + at);
        }
        if constexpr (COST) *c2 = *reinterpret_cast<const d2 *>(cost + at);
    } else if (at < m) {
        q2 = d2{q[at], q[at]};
        mu2 = d2{mu[at], mu[at]};
        if (causal) {
            pm2 = d2{pm[at], pm[at]};
            pv2 = d2{pv[at], pv[at]};
        }
        if constexpr (COST) *c2 = d2{cost[at], cost[at]};
    }
}

// N results of that pair, v[k] to dst[k], under ONE tail decision; a null dst[k] (uniform) is skipped; nothing is written
// at or beyond m.
template <int N>
__device__ __forceinline__ void store_pair(double *const (&dst)[N], const d2 (&v)[N], int64_t m, int64_t base)
{
    const unsigned lane2 = 2 * threadIdx.x;
    constexpr int64_t span = 2 * kPassThreads;
    const int64_t c = base + lane2;
    if (base + span <= m) {                                      // (uniform)
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (dst[k]) *reinterpret_cast<d2 *>(dst[k] + base + lane2) = v[k];
    } else if (c + 1 < m) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (dst[k]) *reinterpret_cast<d2 *>(dst[k] + c) = v[k];
    } else if (c < m) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (dst[k]) dst[k][c] = v[k][0];
    }
}

// The operands of a step are in their registers before anything behind this line is issued; nothing memory moves across it.
// Only what was loaded is named: a model without a prior has no pm2 / pv2 to hold back, a pass without COST no c2.
template <bool CAUSAL, bool COST = false>
__device__ __forceinline__ void operand_fence(d2 &q2, d2 &mu2, d2 &pm2, d2 &pv2, d2 *c2 = nullptr)
{
    if constexpr (COST) {
        if (CAUSAL) asm volatile("" : "+v"(q2), "+v"(mu2), "+v"(pm2), "+v"(pv2), "+v"(*c2) : : "memory");
        else asm volatile("" : "+v"(q2), "+v"(mu2), "+v"(*c2) : : "memory");
        return;
    }
    if (CAUSAL) asm volatile("" : "+v"(q2), "+v"(mu2), "+v"(pm2), "+v"(pv2) : : "memory");
    else asm volatile("" : "+v"(q2), "+v"(mu2) : : "memory");
}

// A candidate joins the lane's arg-max (bv, bi).  One below the lane's best cannot win: better() is only asked when it is
// not -- one compare on the usual path instead of better()'s NaN classification of both sides.
__device__ __forceinline__ void lane_argmax(bool valid, double acq, int64_t gi, double &bv, int64_t &bi)
{
    if (valid && !(acq < bv) && better(acq, gi, bv, bi)) { bv = acq; bi = gi; }
}

// The pass: the workgroup's share of the m candidates, grid-strided, into mean_out / var_out / acq_out (each may be null)
// and the lane's arg-max (bv, bi), which the caller hands to block_argmax.
//
// Two consecutive candidates per lane and iteration (16-byte loads and stores), the next iteration's operands requested
// before this one's arithmetic: with one candidate per lane and the load at the top of the loop body the pass was bound by
// memory LATENCY -- 32 KB in flight per CU -- and ran at 0.29 of the HBM roofline whatever the arithmetic cost (round 5: halving
// the transcendental work changed nothing until the loads were decoupled).
//
// Every memory operation of an iteration is issued in one place, right behind the iteration's only wait: the operands of
// the NEXT iteration and the results of the PREVIOUS one.  Loads and stores share one counter on gfx9 and the compiler
// waits for zero whenever both kinds are pending -- with the stores at the end of the body and the loads at its top (the
// form this loop had until round 5) that wait sat right behind the freshly issued prefetch and took its whole latency,
// every iteration, plus the stores': the pass ran at "memory floor + arithmetic" (77 + 48 us at 2^24 candidates) instead
// of the larger of the two.  Now whatever the wait covers was issued a whole iteration of arithmetic earlier.
//
// CAUSAL: the candidates carry a prior mean / variance.  p: what posterior_of reads.  scored (uniform; a constant in every
// kernel but acq_kernel): false leaves the posterior alone -- no scoring, no arg-max, acq_out ignored.  score: the
// epilogue's own part, (d2 mean2, d2 var2) -> the pair's acquisition values; it takes the pair BY VALUE (see `store` below).
// COST (compile time): `cost` holds one cost per candidate, the pair's travels with the other operands and
// score is (d2 mean2, d2 var2, d2 cost2).  Without it the pass is what it was: cost is not looked at.
template <bool CAUSAL, class Score, bool COST = false>
__device__ __forceinline__ void acq_pass(const double *__restrict__ q, const double *__restrict__ mu,
                                         const double *__restrict__ pm, const double *__restrict__ pv, int64_t m,
                                         const AcqParams &p, bool scored, double *__restrict__ mean_out,
                                         double *__restrict__ var_out, double *__restrict__ acq_out, int64_t index_offset,
                                         Score score, double &bv, int64_t &bi, const double *__restrict__ cost = nullptr)
{
    if (!scored) acq_out = nullptr;
    const int64_t stride = 2 * (int64_t)gridDim.x * kPassThreads, span = 2 * (int64_t)kPassThreads;
    const int64_t first = 2 * (int64_t)blockIdx.x * kPassThreads;
    const unsigned lane2 = 2 * threadIdx.x;
    int64_t cu = first;
    // (two forms kept for the register allocator, DESIGN.md §4t: the results reach store_pair by reference through this
    // lambda, and score takes its pair by value -- with either the other way round pointwise_acq_kernel<*, false, true>
    // took 4 more registers and its PI form, 69 -> 73, lost a wave per SIMD)
    auto store = [&](int64_t base, const d2 &mean2, const d2 &var2, const d2 &acq2) __attribute__((always_inline)) {
        store_pair<3>({mean_out, var_out, acq_out}, {mean2, var2, acq2}, m, base);
    };
    d2 qn = {0.0, 0.0}, mun = {0.0, 0.0}, pmn = {0.0, 0.0}, pvn = {0.0, 0.0};
    d2 mean_done = {0.0, 0.0}, var_done = {0.0, 0.0}, acq_done = {0.0, 0.0};
    [[maybe_unused]] d2 cn = {0.0, 0.0};
    fetch_pair<COST>(q, mu, pm, pv, CAUSAL, m, cu, qn, mun, pmn, pvn, cost, &cn);
    for (int64_t done = -1; cu < m; done = cu, cu += stride) {
        d2 q2 = qn, mu2 = mun, pm2 = pmn, pv2 = pvn;
        [[maybe_unused]] d2 c2 = cn;
        operand_fence<CAUSAL, COST>(q2, mu2, pm2, pv2, &c2);
        if (done >= 0) store(done, mean_done, var_done, acq_done);
        fetch_pair<COST>(q, mu, pm, pv, CAUSAL, m, cu + stride, qn, mun, pmn, pvn, cost, &cn);
        const bool full = cu + span <= m;                        // uniform
        const int64_t c = cu + lane2;
        d2 mean2, var2, acq2 = {0.0, 0.0};                       // (acq2: dead wherever scored is a constant)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            double mean, var;
            posterior_of(q2[e], mu2[e], CAUSAL ? pm2[e] : 0.0, CAUSAL ? pv2[e] : 0.0, CAUSAL, p, mean, var);
            mean2[e] = mean;
            var2[e] = var;
        }
        if (scored) {
            if constexpr (COST) acq2 = score(mean2, var2, c2);
            else acq2 = score(mean2, var2);
            lane_argmax(full || c < m, acq2[0], c + index_offset, bv, bi);
            lane_argmax(full || c + 1 < m, acq2[1], c + 1 + index_offset, bv, bi);
        }
        mean_done = mean2;
        var_done = var2;
        acq_done = acq2;
    }
    // (cu has run past m by whole strides: the last iteration's results, if there was one)
    if (cu - stride >= first) store(cu - stride, mean_done, var_done, acq_done);
}

}  // namespace cbo

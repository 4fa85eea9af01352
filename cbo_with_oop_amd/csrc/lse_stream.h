// The streaming log-sum-exp of the log-space marginalised EI: log((1 / H) sum_h exp(l_h)) - log cost over
// terms that arrive one at a time, in sample order.  hyper_avg_kernel<true>, hyper_sets_kernel<*, true> and the general
// path's hyper_lse_accumulate_kernel / hyper_lse_finish_kernel (kernels_hyper.hip) are all built from these three
// functions, so every path returns the others' bits.
//   state: M, the largest term so far, and S = sum exp(l - M) over the terms so far (1 <= S <= their number).
//   NaN propagates: a NaN term fails both comparisons and reaches S through exp; a NaN M makes every later S NaN.
//   -inf is an ordinary value: equal to a -inf maximum it counts 1, below a finite one exp gives 0; all terms -inf close
//   to -inf.  With H = 1 the close is (l_0 + 0) - 0 - log_cost: the single term minus the log cost.
// One rounding per operation (no contraction); the device library's exp and log.
#pragma once
#include <hip/hip_runtime.h>

namespace cbo {

__device__ __forceinline__ void lse_start(double l, double &M, double &S)
{
    M = l;
    S = 1.0;
}

__device__ __forceinline__ void lse_push(double l, double &M, double &S)
{
#pragma clang fp contract(off)
    if (l > M) {
        S = S * exp(M - l) + 1.0;
        M = l;
    } else if (l == M) {
        S = S + 1.0;
    } else {
        S = S + exp(l - M);
    }
}

// log_cost = log(cost): uniform, formed once by the caller
__device__ __forceinline__ double lse_close(double M, double S, int n_terms, double log_cost)
{
#pragma clang fp contract(off)
    return ((M + log(S)) - log((double)n_terms)) - log_cost;
}

}  // namespace cbo

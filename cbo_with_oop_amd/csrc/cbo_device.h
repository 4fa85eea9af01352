// Device functions shared by several kernel translation units: one kernel-matrix element in GPy's operation order,
// the causal Expected Improvement of one candidate, the arg-max comparator.  Every function pins its own
// floating-point contraction (no FMA fusion beyond what is written): the callers' results must not depend on
// which translation unit inlined them.
#pragma once

#include "cbo_internal.h"

namespace cbo {

// c ? a : b through the VOP3 encoding of v_cndmask_b32.  gfx950 issues the VOP2 encoding (mask implicitly in vcc) once per
// ~22 cycles and SIMD, the VOP3 encoding (mask in any scalar pair, vcc included) once per 4.6 like every other full-rate
// instruction (scripts/probes/valu_rate_probe.hip, profiles/r05_valu_rate_probe.txt) -- and the compiler shrinks a select
// to VOP2 wherever its mask lands in vcc.  The EI pass executed ~10 such selects per candidate.
__device__ __forceinline__ unsigned select_u32(unsigned long long mask, unsigned a, unsigned b)
{
    unsigned r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(mask));
    return r;
}
__device__ __forceinline__ double select_f64(bool c, double a, double b)
{
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(c);
    return __hiloint2double((int)select_u32(mask, (unsigned)__double2hiint(a), (unsigned)__double2hiint(b)),
                            (int)select_u32(mask, (unsigned)__double2loint(a), (unsigned)__double2loint(b)));
}
// s = sqrt(x) (IEEE, round to nearest) and rs ~ 1 / s from ONE hardware estimate of 1/sqrt(x): the coupled Newton steps of the
// compiler's own sqrt expansion -- without that expansion's scaling of arguments below 2^-767 (three VOP2 selects and two
// v_ldexp per call; a predictive variance is clipped at 1e-15) -- whose second variable h converges to 1 / (2 s).  rs is good
// to an ulp or two: a quotient a / s formed as q = a rs, q += (a - q s) rs is within half an ulp and a bit of the IEEE one
// (4 instructions where the IEEE division is 14).  x = 0 and x = +inf: s = x, rs is not meaningful (`special` says so).
// Negative and NaN arguments give NaN in both.
__device__ __forceinline__ void sqrt_and_reciprocal(double x, double &s, double &rs, bool &special)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    g = fma(fma(-g, g, x), h, g);
    g = fma(fma(-g, g, x), h, g);
    special = __builtin_amdgcn_class(x, 0x260);                      // +-0, +inf
    s = select_f64(special, x, g);
    rs = h + h;
}

// scipy.special.ndtr is cephes ndtr.c: Phi(a) = 0.5 + 0.5 erf(x) for |x| < sqrt(1/2), x = a / sqrt 2, and 0.5 erfc(|x|)
// (reflected for x > 0) beyond, with cephes' own erf / erfc: erf(x) = x T(x^2) / U(x^2) for |x| <= 1; erfc(x) = 1 - erf(x)
// below 1, exp(-x^2) P(x) / Q(x) on [1, 8), exp(-x^2) R(x) / S(x) from 8 on, 0 once x^2 > MAXLOG.  The same rational
// functions here, coefficient for coefficient (checked against scipy.special.erf / erfc on the host: erf bit for bit, erfc to
// 5e-16), Horner steps as FMAs -- and ONE exponential for the candidate: erfc's exp(-x^2) is the density's exp(-a^2 / 2) up
// to the rounding of the argument (|x^2| ulps of the tail: 2e-13 of Phi at a = -35, nothing at the |a| <= 6 an acquisition
// that matters lives at).  The quotients of the rational functions go through recip_plain, the exponential through
// exp_nonpositive: each within an ulp or two of the IEEE division / the library exponential they stand for, as the FMA
// Horner steps are of scipy's -- an Expected Improvement good to a few 1e-16 (times u^2 in the lower tail) either way.
// Round 4 called the device library's erf / erfc / exp per candidate: 485 vector instructions, the exponential
// evaluated twice; the pass ran at 0.29 of the HBM roofline it is priced against.
// One Horner step p z + C with the coefficient in a scalar register pair: left to itself the compiler emits the two-operand
// v_fmac_f64, whose addend is its destination, behind two v_mov_b32 that put the 64-bit constant there -- three vector
// instructions per step (122 of the pass's 431 were such moves); gfx950 has no 64-bit literal operands.
__device__ __forceinline__ double horner(double p, double z, double coefficient)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(p), "v"(z), "s"(coefficient));
    return r;
}
// 1 / q to the last bit or two for a q of moderate size (the denominators of the rational functions below: no scaling,
// no special cases): the hardware estimate and two Newton steps -- 6 instructions where an IEEE division is 14
__device__ __forceinline__ double recip_plain(double q)
{
    double r = __builtin_amdgcn_rcp(q);
    r = fma(fma(-q, r, 1.0), r, r);
    r = fma(fma(-q, r, 1.0), r, r);
    return r;
}
// exp(x) for x <= 0 (the density's -u^2 / 2): 2^k exp(r), k = rint(x log2 e), r = x - k ln 2 in two parts (|r| <= 0.35),
// exp(r) by its Taylor polynomial of degree 12 (truncation 1.7e-16); 4.7e-16 relative against the host's exp over [-745, 0].
// No range checks beyond the underflow: 18 instructions where the device library's exp is ~45.
__device__ __forceinline__ double exp_nonpositive(double x)
{
    const double k = rint(x * 1.4426950408889634);
    const double r = fma(-k, 1.90821492927058770002e-10, fma(-k, 6.93147180369123816490e-01, x));
    double p = 1.0 / 479001600.0;
    p = horner(p, r, 1.0 / 39916800.0);
    p = horner(p, r, 1.0 / 3628800.0);
    p = horner(p, r, 1.0 / 362880.0);
    p = horner(p, r, 1.0 / 40320.0);
    p = horner(p, r, 1.0 / 5040.0);
    p = horner(p, r, 1.0 / 720.0);
    p = horner(p, r, 1.0 / 120.0);
    p = horner(p, r, 1.0 / 24.0);
    p = horner(p, r, 1.0 / 6.0);
    p = horner(p, r, 0.5);
    p = horner(p, r, 1.0);
    p = horner(p, r, 1.0);
    return select_f64(x <= -745.2, 0.0, ldexp(p, (int)k));           // underflow; a NaN argument has made p NaN
}
// |x|^2 of one point of d coordinates (x[k] = 0 for k >= d), the squared norm every kernel-matrix element's r^2 is formed
// from.  d < 8: the chain rn(x0^2), then fma(xk, xk, s) -- the chain kernel_value's dot product takes, so r^2(x, x) is an
// exact zero.  d = 8: numpy's 8-way pairwise tree, ((p01 + p23) + (p45 + p67)), over the pairs p01 = fma(x1, x1, rn(x0^2)),
// p23 = fma(x3, x3, rn(x2^2)), ...  Every fused step is WRITTEN as an fma: __dmul_rn and __dadd_rn are plain * and + to the
// compiler, and a product next to a sum is contracted or not, and on either operand, as the compiler sees fit; a product
// that feeds an explicit fma, and a sum of two fmas, leave it nothing to choose.  tests/test_dims_gpu.py pins the order: two
// live coordinates in the slots (2k, 2k + 1) of an 8-column problem give the two-column problem's bits, in slots of two
// different pairs rn(rn(a^2) + rn(b^2)).
__device__ __forceinline__ double squared_norm(const double (&x)[CBO_MAX_DIM], int d)
{
    if (d == 8) {
        const double p01 = __fma_rn(x[1], x[1], __dmul_rn(x[0], x[0]));
        const double p23 = __fma_rn(x[3], x[3], __dmul_rn(x[2], x[2]));
        const double p45 = __fma_rn(x[5], x[5], __dmul_rn(x[4], x[4]));
        const double p67 = __fma_rn(x[7], x[7], __dmul_rn(x[6], x[6]));
        return __dadd_rn(__dadd_rn(p01, p23), __dadd_rn(p45, p67));
    }
    double s = __dmul_rn(x[0], x[0]);
#pragma unroll
    for (int k = 1; k < CBO_MAX_DIM; ++k)
        if (k < d) s = __fma_rn(x[k], x[k], s);
    return s;
}

// CBO_FOR_DIM(d, statement): the one place a runtime dimension d picks its instantiation of a `template <int D>` kernel or
// device function.  The statement is compiled once per dimension with D a constant, e.g.
//     CBO_FOR_DIM(st.d, small_assemble<D>(sh, st, tiles));
// Every case comes from CBO_FOR_DIM_CASE(N, ...), which writes N once, as the label and as D, so a label cannot launch
// another dimension's code.  d is validated to [1, CBO_MAX_DIM] where it enters (cbo_gp_create, cbo_cands_create), so
// `default:` can only mean CBO_MAX_DIM.
// A macro and not a generic lambda (for_dim(d, [&](auto D) { ... })): the macro expands to the plain switch, and the device
// code is the hand-written switch's line for line.  The lambda's by-reference capture costs stack in device code --
// hmc_sets_kernel went from 32 to 64 bytes of private segment, from 4 to 14 spilled VGPRs, the file from 8 to 28 scratch
// instructions.
static_assert(CBO_MAX_DIM == 8, "CBO_FOR_DIM lists the cases 1..7 and the default: extend the list with the limit");
#define CBO_FOR_DIM_CASE(N, ...) case N: { constexpr int D = N; __VA_ARGS__; } break;
#define CBO_FOR_DIM(d, ...)                                                                                             \
    switch (d) {                                                                                                        \
        CBO_FOR_DIM_CASE(1, __VA_ARGS__)                                                                                \
        CBO_FOR_DIM_CASE(2, __VA_ARGS__)                                                                                \
        CBO_FOR_DIM_CASE(3, __VA_ARGS__)                                                                                \
        CBO_FOR_DIM_CASE(4, __VA_ARGS__)                                                                                \
        CBO_FOR_DIM_CASE(5, __VA_ARGS__)                                                                                \
        CBO_FOR_DIM_CASE(6, __VA_ARGS__)                                                                                \
        CBO_FOR_DIM_CASE(7, __VA_ARGS__)                                                                                \
        default: { constexpr int D = CBO_MAX_DIM; __VA_ARGS__; } break;                                                 \
    }

// One kernel-matrix element, GPy operation order (Stationary._unscaled_dist: GEMM-trick squared distance from the
// same |x|^2 sums, clip at 0; RBF.K_of_r), restating /root/reference/src/utils_functions/causal_kernels.py:45-62
// without the rank-1 causal term (added by the caller).
template <int D>
__device__ __forceinline__ double kernel_value(const double *xi, const double *xj, double sqi, double sqj,
                                               double variance, double inv_l2, bool force_zero)
{
#pragma clang fp contract(off)
    // np.dot(X, X2.T): BLAS accumulates a_k*b_k with FMAs from a zero accumulator.
    double dot = __dmul_rn(xi[0], xj[0]);
#pragma unroll
    for (int k = 1; k < D; ++k) dot = __fma_rn(xi[k], xj[k], dot);
    double r2 = __dadd_rn(__dmul_rn(-2.0, dot), __dadd_rn(sqi, sqj));
    if (force_zero) r2 = 0.0;
    r2 = select_f64(r2 < 0.0, 0.0, r2);               // np.clip(r2, 0, inf) (NaN stays NaN)
    // GPy goes r = sqrt(r2) / lengthscale, then r*r.  The round trip through the square root costs ~40 fp64
    // instructions per element and changes r^2 by at most a couple of ulp (far below the 1e-16-level
    // differences between exp() implementations), so the squared scaled distance is formed directly;
    // inv_l2 = 1 / lengthscale^2 is exactly 1 for the reference's lengthscale = 1 (and for ARD, whose inputs
    // are pre-scaled).
    // (exp_nonpositive, not the device library's exp: 24 vector instructions where that one is ~60 with 20 32-bit moves and
    // four VOP2 selects -- a kernel-matrix element cost ~300 cycles of a SIMD, two thirds of them the exponential; 4.7e-16
    // against the library's 2e-16, both far inside what separates two hosts' exp())
    return __dmul_rn(variance, exp_nonpositive(__dmul_rn(-0.5, __dmul_rn(r2, inv_l2))));
}

__device__ __forceinline__ double cephes_erf_small(double x)       // |x| <= 1
{
    const double z = x * x;
    double p = 9.60497373987051638749E0;
    p = horner(p, z, 9.00260197203842689217E1);
    p = horner(p, z, 2.23200534594684319226E3);
    p = horner(p, z, 7.00332514112805075473E3);
    p = horner(p, z, 5.55923013010394962768E4);
    double q = z + 3.35617141647503099647E1;
    q = horner(q, z, 5.21357949780152679795E2);
    q = horner(q, z, 4.59432382970980127987E3);
    q = horner(q, z, 2.26290000613890934246E4);
    q = horner(q, z, 4.92673942608635921086E4);
    return x * p * recip_plain(q);
}
// cephes erfc's rational functions without their exp(-x^2) factor, p / q ~ exp(x^2) erfc(x) = erfcx(x): P / Q on [1, 8),
// R / S from 8 on (numerator and denominator apart: the callers divide as they need)
__device__ __forceinline__ void cephes_erfc_pq(double z, double &p, double &q)
{
    p = 2.46196981473530512524E-10;
    p = horner(p, z, 5.64189564831068821977E-1);
    p = horner(p, z, 7.46321056442269912687E0);
    p = horner(p, z, 4.86371970985681366614E1);
    p = horner(p, z, 1.96520832956077098242E2);
    p = horner(p, z, 5.26445194995477358631E2);
    p = horner(p, z, 9.34528527171957607540E2);
    p = horner(p, z, 1.02755188689515710272E3);
    p = horner(p, z, 5.57535335369399327526E2);
    q = z + 1.32281951154744992508E1;
    q = horner(q, z, 8.67072140885989742329E1);
    q = horner(q, z, 3.54937778887819891062E2);
    q = horner(q, z, 9.75708501743205489753E2);
    q = horner(q, z, 1.82390916687909736289E3);
    q = horner(q, z, 2.24633760818710981792E3);
    q = horner(q, z, 1.65666309194161350182E3);
    q = horner(q, z, 5.57535340817727675546E2);
}
__device__ __forceinline__ void cephes_erfc_rs(double z, double &p, double &q)
{
    p = 5.64189583547755073984E-1;
    p = horner(p, z, 1.27536670759978104416E0);
    p = horner(p, z, 5.01905042251180477414E0);
    p = horner(p, z, 6.16021097993053585195E0);
    p = horner(p, z, 7.40974269950448939160E0);
    p = horner(p, z, 2.97886665372100240670E0);
    q = z + 2.26052863220117276590E0;
    q = horner(q, z, 9.39603524938001434673E0);
    q = horner(q, z, 1.20489539808096656605E1);
    q = horner(q, z, 1.70814450747565897222E1);
    q = horner(q, z, 9.60896809063285878198E0);
    q = horner(q, z, 3.36907645100081516050E0);
}
// e = exp(-a^2 / 2), computed by the caller (who needs it for the density)
__device__ __forceinline__ double ndtr_with_exp(double a, double e)
{
    const double SQRTH = 7.07106781186547524401E-1, MAXLOG = 7.09782712893383996843E2;
    if (isnan(a)) return a;
    const double x = a * SQRTH;
    const double z = fabs(x);
    double c;
    if (z < 1.0) {
        // one evaluation for both of cephes' branches below 1: erf(x) = x T / U is odd to the bit, so erf(|x|) = |erf(x)|
        const double erf_x = cephes_erf_small(x);
        if (z < SQRTH) return 0.5 + 0.5 * erf_x;
        c = 1.0 - fabs(erf_x);
    } else if (z * z > MAXLOG) {
        c = 0.0;                                       // cephes: underflow
    } else {
        double p, q;
        if (z < 8.0) cephes_erfc_pq(z, p, q);
        else cephes_erfc_rs(z, p, q);
        c = (e * p) * recip_plain(q);
    }
    const double y = 0.5 * c;
    return select_f64(x > 0, 1.0 - y, y);
}

// scipy.special.log_ndtr(a) (scipy 1.15, real argument): t = a / sqrt 2 (as a * SQRT1_2), then
//     a < -1:  log(erfcx(-t) / 2) - t^2          else:  log1p(-erfc(t) / 2)
// with cephes' erf / erfc as in ndtr_with_exp.  scipy's erfcx is the Faddeeva package's; here erfcx(y) for y > 1 / sqrt 2 is
// cephes erfc's rational function without its exponential (P / Q below 8, R / S beyond: the same relative accuracy as
// erfc itself) and exp(y^2) (1 - erf(y)) below 1.  The Gumbel fit of max-value entropy search calls it (a few hundred
// thousand evaluations per fit), and log_feasibility_of below, once per constraint and candidate: IEEE divisions and the
// device library's exp / log / log1p throughout.
__device__ __forceinline__ double log_ndtr(double a)
{
#pragma clang fp contract(off)
    const double SQRTH = 7.07106781186547524401E-1, MAXLOG = 7.09782712893383996843E2;
    const double t = a * SQRTH;
    double p, q;
    if (a < -1.0) {
        const double y = -t;                           // > 1 / sqrt 2
        double erfcx;
        if (y < 1.0) {
            erfcx = exp(y * y) * (1.0 - cephes_erf_small(y));
        } else {
            if (y < 8.0) cephes_erfc_pq(y, p, q);
            else cephes_erfc_rs(y, p, q);
            erfcx = p / q;
        }
        return log(erfcx / 2.0) - t * t;
    }
    const double z = fabs(t);
    double c;
    if (z < 1.0) {
        c = 1.0 - cephes_erf_small(t);
    } else if (z * z > MAXLOG) {
        c = 0.0;                                       // (t >= 1 here: erfc underflows)
    } else {
        if (z < 8.0) cephes_erfc_pq(z, p, q);
        else cephes_erfc_rs(z, p, q);
        c = (exp(-(z * z)) * p) / q;
    }
    return log1p(-(c / 2.0));
}

// log_ndtr(a) and the hazard ratio rho(a) = phi(a) / Phi(a) = d log_ndtr / d a beside it (the gradient of a
// log feasibility).  The value is log_ndtr's, operation for operation.  rho is never an underflowed density over an
// underflowed distribution: above -1 it is the plain ratio (the density's exponential shared with cephes ndtr, as
// acquisition_of has it; Phi >= 0.158 there), below it is sqrt(2 / pi) / erfcx(-a / sqrt 2) from the erfcx the value forms
// anyway -- exp(-a^2 / 2) cancels analytically.  A NaN argument gives NaN twice.
// Inlined here; its one caller in a kernel (constraint_term of kernels_sets_refine_con.hip) is the function that is NOT
// inlined, for log_ei_value_and_coefficients' reason (kernels_sets_refine.hip) -- a second call level below that one would
// make it a non-leaf function, whose saved return address costs 16 bytes of scratch memory per lane.
struct LogNdtrRatio {
    double value, rho;
};
__device__ __forceinline__ LogNdtrRatio log_ndtr_and_ratio(double a)
{
#pragma clang fp contract(off)
    const double SQRTH = 7.07106781186547524401E-1, MAXLOG = 7.09782712893383996843E2, SQRT_2_OVER_PI = 0.797884560802865355880;
    const double t = a * SQRTH;
    double p, q;
    if (a < -1.0) {
        const double y = -t;                           // > 1 / sqrt 2
        double erfcx;
        if (y < 1.0) {
            erfcx = exp(y * y) * (1.0 - cephes_erf_small(y));
        } else {
            if (y < 8.0) cephes_erfc_pq(y, p, q);
            else cephes_erfc_rs(y, p, q);
            erfcx = p / q;
        }
        return LogNdtrRatio{log(erfcx / 2.0) - t * t, SQRT_2_OVER_PI / erfcx};
    }
    const double e = exp_nonpositive(-(a * a) / 2.0);
    const double rho = (e * 0.3989422804014327) / ndtr_with_exp(a, e);
    const double z = fabs(t);
    double c;
    if (z < 1.0) {
        c = 1.0 - cephes_erf_small(t);
    } else if (z * z > MAXLOG) {
        c = 0.0;                                       // (t >= 1 here: erfc underflows)
    } else {
        if (z < 8.0) cephes_erfc_pq(z, p, q);
        else cephes_erfc_rs(z, p, q);
        c = (exp(-(z * z)) * p) / q;
    }
    return LogNdtrRatio{log1p(-(c / 2.0)), rho};
}

// (va, ia) beats (vb, ib): larger value, NaN maximal (numpy.argmax), lowest index on ties
__device__ __forceinline__ bool better(double va, int64_t ia, double vb, int64_t ib)
{
    const bool na = isnan(va), nb = isnan(vb);
    if (na != nb) return na;
    if (na || va == vb) return ia < ib;
    return va > vb;
}

__device__ __forceinline__ void wave_argmax(double &v, int64_t &i)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int64_t oi = __shfl_down(i, off);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// arg-max of a 256-thread workgroup into *out_v / *out_i (written by thread 0)
__device__ __forceinline__ void block_argmax(double v, int64_t i, double *out_v, int64_t *out_i)
{
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    wave_argmax(v, i);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sv[wave] = v; si[wave] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bv = sv[0];
        int64_t bi = si[0];
        for (int w = 1; w < 4; ++w)
            if (better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        *out_v = bv;
        *out_i = bi;
    }
}

constexpr int64_t kNoIndex = INT64_MAX;

// Posterior epilogue of one candidate (GPy Posterior._raw_predict / GP.predict + CausalRBF.Kdiag,
// causal_kernels.py:64-79): var = clip(Kdiag - q, 1e-15) (+ noise), mean = mu + m(x*).
__device__ __forceinline__ void posterior_of(double q, double mu, double pm, double pv, bool causal, const AcqParams &p,
                                             double &mean, double &var)
{
#pragma clang fp contract(off)
    const double kss = causal ? (p.variance + pv) : p.variance;
    var = kss - q;
    var = select_f64(var < kGpyVarClip, kGpyVarClip, var);          // np.clip(var, 1e-15, inf); NaN stays NaN
    if (p.include_noise) var = var + p.noise_var;                   // Gaussian likelihood predictive_values
    mean = mu;
    if (causal) mean = mean + pm;                                   // GP._raw_predict: mu += mean_function.f(Xnew)
}

// CausalExpectedImprovement.evaluate (causal_acquisition_functions.py:27-43, 77-88) / Cost (emukit Quotient):
// s (u Phi(u) + phi(u)) / cost, task 'max' returns -EI with the same u (reference quirk).
__device__ __forceinline__ double acquisition_of(double mean, double var, const AcqParams &p)
{
#pragma clang fp contract(off)
    double s, rs;
    bool special;
    sqrt_and_reciprocal(var, s, rs, special);
    const double mj = mean + p.ei_jitter;
    const double a = p.y_best - mj;
    double u = a * rs;
    u = fma(fma(-u, s, a), rs, u);
    if (__builtin_expect(special, 0)) u = a / s;                    // (a zero or infinite variance: the IEEE quotient)
    const double e = exp_nonpositive(-(u * u) / 2.0);
    const double pdf = e * 0.3989422804014327;                     // scipy _norm_pdf: exp(-x**2/2)/sqrt(2 pi), to an ulp
    const double cdf = ndtr_with_exp(u, e);
    double imp = s * (u * cdf + pdf);
    if (p.task != CBO_TASK_MIN) imp = -imp;
    // imp / cost, correctly rounded, in three instructions: the cost is the same for every candidate of the launch, so its
    // reciprocal is computed once (hoisted out of the candidate loop) and the quotient corrected by its own remainder
    // (Markstein: RN(q + r rem) with r = RN(1 / c) and q within an ulp is the IEEE quotient for every cost whose significand
    // is not all ones -- the reference's costs are small integers; only the sign of a zero acquisition can differ)
    const double rc = 1.0 / p.cost;
    const double qv = imp * rc;
    return fma(fma(-qv, p.cost, imp), rc, qv);
}

// emukit ProbabilityOfFeasibility / ProbabilityOfImprovement of one candidate: ndtr(+-(value - (mean + jitter)) / sd).  sd and the quotient as acquisition_of has them (one hardware estimate, the
// quotient corrected by its own remainder: within half an ulp and a bit of the IEEE one), the density's exponential shared
// with cephes ndtr (ndtr_with_exp).  A NaN mean or variance gives NaN.
__device__ __forceinline__ double feasibility_of(double mean, double var, double value, double jitter, int sense)
{
#pragma clang fp contract(off)
    double s, rs;
    bool special;
    sqrt_and_reciprocal(var, s, rs, special);
    const double a = value - (mean + jitter);
    double u = a * rs;
    u = fma(fma(-u, s, a), rs, u);
    if (__builtin_expect(special, 0)) u = a / s;                    // (a zero or infinite variance: the IEEE quotient)
    if (sense != CBO_CON_LE) u = -u;                                // (uniform)
    const double e = exp_nonpositive(-(u * u) / 2.0);
    return ndtr_with_exp(u, e);
}

// One candidate's value over the cost.  p.ei_jitter carries the kind's parameter: beta (LCB), the jitter (PI).
//   LCB: the compiler's IEEE square root (np.sqrt's bits), then the operations as numpy applies them, one rounding each
//   PI:  feasibility_of (cbo_device.h) with the incumbent as the bound: the PoF pass's bits
//   VAR: the predictive variance itself
// then acquisition_of's quotient: the reciprocal of the cost (uniform, hoisted out of the loop) corrected by the remainder
// -- the IEEE quotient for every cost whose significand is not all ones; only the sign of a zero can differ.
template <int KIND>
__device__ __forceinline__ double pointwise_of(double mean, double var, const AcqParams &p)
{
#pragma clang fp contract(off)
    double v;
    if (KIND == CBO_ACQ_LCB) {
        const double bs = p.ei_jitter * __dsqrt_rn(var);
        v = p.task == CBO_TASK_MIN ? -(mean - bs) : mean + bs;     // (uniform)
    } else if (KIND == CBO_ACQ_PI) {
        v = feasibility_of(mean, var, p.y_best, p.ei_jitter, p.task == CBO_TASK_MIN ? CBO_CON_LE : CBO_CON_GE);
    } else {
        v = var;
    }
    const double rc = 1.0 / p.cost;
    const double qv = v * rc;
    return fma(fma(-qv, p.cost, v), rc, qv);
}

// ---- log Expected Improvement (Ament et al. 2023, "Unexpected improvements to expected improvement"):
// the epilogue of pointwise_acq_kernel<kLogEiKind>, small_sets_kernel<kLogEiKind> and small_sets_refine_kernel<kLogEiKind>
// -- one definition, so the three return each other's bits.
// log h(u), h(u) = phi(u) + u Phi(u), without underflow, in three ranges (w = sqrt(pi / 2) |u| erfcx(-u / sqrt 2) = 1 - h / phi):
//   u > -1            log(phi + u Phi), the density's exponential shared with cephes ndtr (ndtr_with_exp)
//   -30 < u <= -1     -u^2 / 2 - log sqrt(2 pi) + log1mexp(log w),  log1mexp(x) = log(-expm1(x)) above -ln 2, else log1p(-exp(x));
//                     erfcx from cephes erfc's rational functions without their exponential (P / Q below 8, R / S beyond;
//                     exp(y^2) (1 - erf y) below 1, as log_ndtr has it)
//   u <= -30          -u^2 / 2 - log sqrt(2 pi) - 2 log|u| + log1p(S),  S = -3 / u^2 + 15 / u^4 - 105 / u^6 + ... (eight terms:
//                     the ninth is 2e-18 at |u| = 30) -- 1 - w cancels to nothing from |u| ~ 1e3 on, the series does not
// GRAD: the gradient's coefficients too, A = Phi / h and B = phi / h (d log h / du = A, and d logEI = (-A d mean + B d sd) / sd):
// the plain ratios above -1; below, B = 1 / (1 - w) or u^2 / (1 + S) -- exp(-u^2 / 2) cancels analytically -- and
// A = sqrt(pi / 2) erfcx(-u / sqrt 2) B.
// A NaN argument takes the last range and comes out NaN.  IEEE divisions and the device library's log / log1p / expm1 / exp.
template <bool GRAD>
__device__ __forceinline__ double log_h_of(double u, double &A, double &B)
{
#pragma clang fp contract(off)
    const double SQRTH = 7.07106781186547524401E-1, LOG_SQRT_2PI = 0.918938533204672741780, SQRT_HALF_PI = 1.25331413731550025121,
                 LOG_SQRT_HALF_PI = 0.225791352644727432363, LN2 = 0.693147180559945309417;
    double r;
    if (u > -1.0) {
        const double e = exp_nonpositive(-(u * u) / 2.0);
        const double pdf = e * 0.3989422804014327;
        const double cdf = ndtr_with_exp(u, e);
        const double h = fma(u, cdf, pdf);
        r = log(h);
        if (GRAD) { A = cdf / h; B = pdf / h; }
    } else {
        const double y = -u * SQRTH;                                   // >= 1 / sqrt 2 (or NaN)
        double erfcx;
        if (y < 1.0) {
            erfcx = exp(y * y) * (1.0 - cephes_erf_small(y));
        } else {
            double p, q;
            if (y < 8.0) cephes_erfc_pq(y, p, q);
            else cephes_erfc_rs(y, p, q);
            erfcx = p / q;
        }
        const double head = -(u * u) / 2.0 - LOG_SQRT_2PI;
        if (u > -30.0) {
            const double x = log(erfcx * -u) + LOG_SQRT_HALF_PI;        // log w < 0
            const bool near = x > -LN2;
            const double w = exp(x);
            const double one_minus_w = near ? -expm1(x) : 1.0 - w;
            r = head + (near ? log(one_minus_w) : log1p(-w));
            if (GRAD) B = 1.0 / one_minus_w;
        } else {
            const double u2 = u * u, t = 1.0 / u2;
            double S = 34459425.0;
            S = fma(S, t, -2027025.0);
            S = fma(S, t, 135135.0);
            S = fma(S, t, -10395.0);
            S = fma(S, t, 945.0);
            S = fma(S, t, -105.0);
            S = fma(S, t, 15.0);
            S = fma(S, t, -3.0);
            S = S * t;
            r = (head - 2.0 * log(-u)) + log1p(S);
            if (GRAD) B = u2 / (1.0 + S);
        }
        if (GRAD) A = SQRT_HALF_PI * erfcx * B;
    }
    return r;
}
// The standardised improvement of one candidate, s and the quotient formed as acquisition_of forms them.  Task 'max' is the
// MIRROR, u = ((mean - jitter) - y_best) / s: not the logarithm of acquisition_of's -EI (the reference's quirk), which has none.
__device__ __forceinline__ double log_ei_u(double mean, double var, const AcqParams &p, double &s)
{
#pragma clang fp contract(off)
    double rs;
    bool special;
    sqrt_and_reciprocal(var, s, rs, special);
    const double a = (p.task == CBO_TASK_MIN) ? p.y_best - (mean + p.ei_jitter) : (mean - p.ei_jitter) - p.y_best;   // (uniform)
    double u = a * rs;
    u = fma(fma(-u, s, a), rs, u);
    if (__builtin_expect(special, 0)) u = a / s;                    // (a zero or infinite variance: the IEEE quotient)
    return u;
}
// log EI - log cost of one candidate: log h(u) + log s - log_cost.  log_cost = log(p.cost) is uniform: the callers form it
// once, ahead of their candidate loop.  A NaN mean or variance gives NaN.
__device__ __forceinline__ double log_ei_of(double mean, double var, const AcqParams &p, double log_cost)
{
#pragma clang fp contract(off)
    double s, A, B;
    const double u = log_ei_u(mean, var, p, s);
    return (log_h_of<false>(u, A, B) + log(s)) - log_cost;
}
__device__ __forceinline__ double log_ei_of(double mean, double var, const AcqParams &p)
{
    return log_ei_of(mean, var, p, log(p.cost));
}

// log of feasibility_of: the same u -- the same operations, the same special case, the sign flipped for
// CBO_CON_GE: feasibility_of's bits -- then log_ndtr(u), finite where ndtr(u) itself underflows to 0 (u below about -38).
// A NaN mean or variance gives NaN.
__device__ __forceinline__ double log_feasibility_of(double mean, double var, double value, double jitter, int sense)
{
#pragma clang fp contract(off)
    double s, rs;
    bool special;
    sqrt_and_reciprocal(var, s, rs, special);
    const double a = value - (mean + jitter);
    double u = a * rs;
    u = fma(fma(-u, s, a), rs, u);
    if (__builtin_expect(special, 0)) u = a / s;                    // (a zero or infinite variance: the IEEE quotient)
    if (sense != CBO_CON_LE) u = -u;                                // (uniform)
    return log_ndtr(u);
}
// ... with what its gradient needs: sd, the oriented u and rho(u) = phi(u) / Phi(u) -- d log PoF =
// rho(u) du, du = -+(d mean + u_le d sd) / sd.  The value is log_feasibility_of's to the bit.
__device__ __forceinline__ double log_feasibility_of(double mean, double var, double value, double jitter, int sense,
                                                     double &s, double &u, double &rho)
{
#pragma clang fp contract(off)
    double rs;
    bool special;
    sqrt_and_reciprocal(var, s, rs, special);
    const double a = value - (mean + jitter);
    u = a * rs;
    u = fma(fma(-u, s, a), rs, u);
    if (__builtin_expect(special, 0)) u = a / s;                    // (a zero or infinite variance: the IEEE quotient)
    if (sense != CBO_CON_LE) u = -u;                                // (uniform)
    const LogNdtrRatio r = log_ndtr_and_ratio(u);
    rho = r.rho;
    return r.value;
}

// ---- max-value entropy search: the epilogue of mes_acq_kernel (kernels_mes.hip) and of small_sets_kernel<kMesKind>
// (kernels_sets.hip) -- one definition, so the multi-set sweep returns cbo_acq_sweep_mes' bits.
// One sample's term of emukit's evaluate: -gamma pdf(gamma) / (2 minus_cdf) - log(minus_cdf).  The density and cephes ndtr
// share one exponential (ndtr_with_exp); 1 - ndtr(gamma) is formed as written, not as ndtr(-gamma).
__device__ __forceinline__ double mes_term(double min_k, double mean, double fsd)
{
#pragma clang fp contract(off)
    const double g = (min_k - mean) / fsd;                           // IEEE division, as numpy
    const double e = exp_nonpositive(-(g * g) / 2.0);
    const double pdf = e * 0.3989422804014327;                      // scipy _norm_pdf: exp(-x**2/2)/sqrt(2 pi), to an ulp
    double mc = 1.0 - ndtr_with_exp(g, e);
    mc = select_f64(mc < 1e-10, 1e-10, mc);                         // np.clip(minus_cdf, 1e-10, 1) (NaN stays NaN; mc <= 1)
    return ((-g) * pdf) / (2.0 * mc) - log(mc);
}

// mean over the k samples in numpy's order for a row of an (M, K) array reduced along its last axis (np.mean(axis=1):
// pairwise_sum): below 8 terms one running sum from 0; from 8 on, eight accumulators over the leading multiple of 8, combined
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the rest one by one; then / K
// P: mins (an array or a pointer to the samples, wherever they live), k (uniform) and cost -- MesParams, or MesSetParams
template <class P>
__device__ __forceinline__ double mes_of(double mean, double var, const P &p)
{
#pragma clang fp contract(off)
    double fsd = sqrt(var);                                          // IEEE square root (np.sqrt)
    fsd = select_f64(fsd < 1e-10, 1e-10, fsd);                      // np.maximum(fsd, 1e-10); NaN stays NaN
    const int full = p.k - p.k % 8;
    double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = 0;
    for (; k < full; k += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + mes_term(p.mins[k + j], mean, fsd);
    }
    double s = (p.k < 8) ? 0.0 : ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; k < p.k; ++k) s = s + mes_term(p.mins[k], mean, fsd);
    return (s / (double)p.k) / p.cost;
}
// the samples of one set of the multi-set sweep: in LDS, copied there from the call's table
struct MesSetParams {
    const double *mins;
    int k;
    double cost;
};

// ---- greedy batch selection: the arithmetic of one further pick, shared by batch_pivot_kernel,
// batch_partial_kernel and batch_final_kernel (kernels_batch.hip: cbo_acq_sweep_batch) and small_sets_batch_kernel
// (kernels_sets_batch.hip: cbo_acq_sweep_sets_batch) -- one definition, so the one-launch form returns
// cbo_acq_sweep_batch's bits.
// d of the believed point p: cbo_gp_predict's clipped latent variance (posterior_of without the noise) plus Ky's diagonal term
__device__ __forceinline__ double batch_believer_sd(double variance, double pv_p, bool causal, double q_p, double noise_var)
{
#pragma clang fp contract(off)
    const double kss = causal ? (variance + pv_p) : variance;
    double lat = kss - q_p;
    lat = (lat < kGpyVarClip) ? kGpyVarClip : lat;
    const double s2 = (lat + noise_var) + kGpyDiagJitter;
    return sqrt(s2);
}
// min(model.Y) once the believed point is in the data (max for the 'max' task); a NaN mean leaves it alone
__device__ __forceinline__ double batch_moved_incumbent(double yb, double mu_p, double pm_p, bool causal, int task)
{
#pragma clang fp contract(off)
    double mean = mu_p;
    if (causal) mean = mean + pm_p;
    return (task == CBO_TASK_MIN ? (mean < yb) : (mean > yb)) ? mean : yb;
}
// one row of the pass over V: the column's chain s += V_ip V_ij
__device__ __forceinline__ double batch_pass_step(double l, double v, double s) { return __fma_rn(l, v, s); }
// W_tj of candidate j: slice(r) = the r-th slice sum of the pass, wrow(r) = W_rj of the earlier fantasy rows, wp[r] = W_rp
template <int D, class Slice, class Wrow>
__device__ __forceinline__ double batch_fantasy_weight(int slices, Slice slice, int rows, const double *wp, Wrow wrow,
                                                       const double *xp, const double *xj, double sqp, double sqj,
                                                       bool causal, double svp, double svj, double variance, double inv_l2,
                                                       double d)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int r = 0; r < slices; ++r) s = __dadd_rn(s, slice(r));
    double ws = 0.0;
    for (int r = 0; r < rows; ++r) ws = __fma_rn(wp[r], wrow(r), ws);
    double kv = kernel_value<D>(xp, xj, sqp, sqj, variance, inv_l2, false);
    if (causal) kv = __dadd_rn(kv, __dmul_rn(svp, svj));
    const double c = __dadd_rn(__dadd_rn(kv, -s), -ws);
    return c / d;
}
__device__ __forceinline__ double batch_q_update(double w, double q) { return __fma_rn(w, w, q); }
// row slices of the pass over V: one per 64 rows, kBatchMaxSlices at the most
__host__ __device__ inline int batch_slice_count(int64_t n)
{
    const int64_t s = (n + 63) / 64;
    return (int)(s < 1 ? 1 : (s > kBatchMaxSlices ? kBatchMaxSlices : s));
}
// rows of one slice of the pass: ceil(ceil(n / slices) / 8) * 8
__host__ __device__ inline int batch_rows_per_slice(int64_t n, int slices) { return (int)(((n + slices - 1) / slices + 7) / 8 * 8); }

}  // namespace cbo

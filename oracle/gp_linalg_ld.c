/* Extended-precision (x87 80-bit long double) linear algebra on GIVEN fp64 matrices.  TEST INFRASTRUCTURE ONLY
 * (see oracle/gp_oracle.py header).  gp_truth_ld.c factors its own Ky; the routines here take the device's own
 * factor L (and alpha) instead, so that a test measures one kernel stage at a time: the factorisation through its
 * backward error, the substitution of the sweep, the likelihood gradients, the prediction gradients.
 *
 * Every accumulation is in long double; results are returned in long double (numpy.longdouble on the Python side).
 * Matrices are row-major n x n (numpy C order); only the lower triangle of L is read.
 *
 *   ld_backward_error_rows   max over sampled rows i and all j of |(L L^T - A)_ij| / sqrt(A_ii A_jj)     O(n^2 |rows|)
 *   ld_solve_many            v_k = L^-1 b_k per column: q_k = sum v^2, mu_k = v^T z (kernels_trsm.hip's q and mu)
 *   ld_lml_gradients         log marginal likelihood and its gradients with W = (L L^T)^-1 from the given L     O(n^3)
 *   ld_prediction_gradients  d mean / d x*, d var / d x* with the solves on the given L and the given alpha
 *
 * The kernel entries inside the gradients use direct coordinate differences in long double (the exact quantity
 * GPy's |x|^2 + |x'|^2 - 2 x.x' approximates).  The maths restated is gp_oracle.log_marginal_likelihood_gradients
 * and gp_oracle.predict_gradients (GPy RBF / Stationary, CausalRBF's variance-gradient quirk included).
 *
 * Build: oracle/Makefile (gcc -O2 -fopenmp -shared -fPIC).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef long double ld;

#define MAXD 16

static const ld LOG_2PI = 1.837877066409345483560659472811235279722794947275566825634L;

/* r_k = (a_k - b_k) / l_k in long double; returns sum r_k^2 and leaves the per-dimension (a_k - b_k)^2 / l_k^3 factors
 * of the lengthscale gradient in g (scalar lengthscale: their sum in g[0]) */
static ld sqdist(const double *a, const double *b, int d, const double *ls, int ard, ld *g)
{
    ld r2 = 0;
    if (g) memset(g, 0, sizeof(ld) * (size_t)(ard ? d : 1));
    for (int k = 0; k < d; k++) {
        ld l = ard ? (ld)ls[k] : (ld)ls[0];
        ld diff = (ld)a[k] - (ld)b[k];
        ld t = diff / l;
        r2 += t * t;
        if (g) g[ard ? k : 0] += diff * diff / (l * l * l);
    }
    return r2;
}

static void backward_error_rows(long n, const double *L, const double *A, const long *rows, long nrows,
                                   ld *out_max, long *out_row, long *out_col)
{
    ld best = -1;
    long bi = -1, bj = -1;
    for (long t = 0; t < nrows; t++) {
        const long i = rows[t];
        const double *Li = L + i * n;
        const ld aii = (ld)A[i * n + i];
#pragma omp parallel
        {
            ld tb = -1;
            long tj = -1;
#pragma omp for schedule(static)
            for (long j = 0; j < n; j++) {
                const double *Lj = L + j * n;
                const long kmax = i < j ? i : j;
                ld s = 0;
                for (long k = 0; k <= kmax; k++) s += (ld)Li[k] * (ld)Lj[k];
                ld e = fabsl(s - (ld)A[i * n + j]) / sqrtl(aii * (ld)A[j * n + j]);
                if (e > tb) { tb = e; tj = j; }
            }
#pragma omp critical
            {
                if (tb > best) { best = tb; bi = i; bj = tj; }
            }
        }
    }
    *out_max = best;
    if (out_row) *out_row = bi;
    if (out_col) *out_col = bj;
}

/* returns 0, or i+1 if L_ii is not positive */
int ld_backward_error_rows(long n, const double *L, const double *A, const long *rows, long nrows, ld *out_max,
                           long *out_row, long *out_col)
{
    for (long t = 0; t < nrows; t++) {
        if (rows[t] < 0 || rows[t] >= n) return -1;
        if (!(A[rows[t] * n + rows[t]] > 0)) return (int)(rows[t] + 1);
    }
    for (long i = 0; i < n; i++) if (!(A[i * n + i] > 0)) return (int)(i + 1);
    backward_error_rows(n, L, A, rows, nrows, out_max, out_row, out_col);
    return 0;
}

/* forward substitution L v = b in long double (b given in long double) */
static void fwd(long n, const double *L, const ld *b, ld *v)
{
    for (long i = 0; i < n; i++) {
        const double *Li = L + i * n;
        ld s = b[i];
        for (long k = 0; k < i; k++) s -= (ld)Li[k] * v[k];
        v[i] = s / (ld)Li[i];
    }
}

/* back substitution L^T x = z */
static void bwd(long n, const double *L, const ld *z, ld *x)
{
    for (long i = 0; i < n; i++) x[i] = z[i];
    for (long i = n - 1; i >= 0; i--) {
        x[i] /= (ld)L[i * n + i];
        const double *Li = L + i * n;
        const ld xi = x[i];
        for (long k = 0; k < i; k++) x[k] -= (ld)Li[k] * xi;
    }
}

/* B is n x m row-major.  z: z_in (fp64) if given, else L^-1 r_in in long double if r_in is given, else none (mu_out
 * untouched).  V_out (n x m row-major, fp64-rounded) is optional. */
int ld_solve_many(long n, const double *L, long m, const double *B, const double *z_in, const double *r_in,
                  ld *q_out, ld *mu_out, ld *z_out, double *V_out)
{
    for (long i = 0; i < n; i++) if (!(L[i * n + i] > 0)) return (int)(i + 1);
    ld *z = NULL;
    if (z_in || r_in) {
        z = (ld *)malloc(sizeof(ld) * (size_t)(n ? n : 1));
        if (!z) return -1;
        if (z_in) for (long i = 0; i < n; i++) z[i] = (ld)z_in[i];
        else {
            ld *r = (ld *)calloc((size_t)(n ? n : 1), sizeof(ld));
            if (!r) { free(z); return -1; }
            for (long i = 0; i < n; i++) r[i] = (ld)r_in[i];
            fwd(n, L, r, z);
            free(r);
        }
        if (z_out) for (long i = 0; i < n; i++) z_out[i] = z[i];
    }
    int fail = 0;
#pragma omp parallel
    {
        ld *b = (ld *)malloc(sizeof(ld) * (size_t)(n ? n : 1));
        ld *v = (ld *)malloc(sizeof(ld) * (size_t)(n ? n : 1));
        if (!b || !v) {
#pragma omp atomic write
            fail = 1;
        }
#pragma omp for schedule(dynamic, 1)
        for (long c = 0; c < m; c++) {
            if (!b || !v) continue;
            for (long i = 0; i < n; i++) b[i] = (ld)B[i * m + c];
            fwd(n, L, b, v);
            ld q = 0, mu = 0;
            for (long i = 0; i < n; i++) {
                q += v[i] * v[i];
                if (z) mu += v[i] * z[i];
                if (V_out) V_out[i * m + c] = (double)v[i];
            }
            q_out[c] = q;
            if (z && mu_out) mu_out[c] = mu;
        }
        free(b);
        free(v);
    }
    free(z);
    return fail ? -1 : 0;
}

/* out: [lml, d_variance, d_noise, d_ls[0..nl)] (nl = ard ? d : 1); mag: the same slots with every term of the
 * contraction taken in absolute value (|alpha_i alpha_j| + |W_ij| in the place of alpha_i alpha_j - W_ij; for the lml
 * n log 2pi + 2 sum |log L_ii| + sum |r_i alpha_i|, halved) -- the scale an fp64 evaluation's rounding is relative to.
 * r = y - m(X); vX optional (causal rank-1 term).  alpha_out (optional) = (L L^T)^-1 r. */
int ld_lml_gradients(long n, int d, const double *L, const double *X, const double *r, const double *vX,
                     double variance, const double *ls, int ard, ld *out, ld *mag, ld *alpha_out)
{
    if (d < 1 || d > MAXD) return -1;
    for (long i = 0; i < n; i++) if (!(L[i * n + i] > 0)) return (int)(i + 1);
    const int nl = ard ? d : 1;
    ld *U = (ld *)calloc((size_t)n * (size_t)n, sizeof(ld));   /* U = L^-T: row j = column j of L^-1 (entries k >= j) */
    ld *rr = (ld *)calloc((size_t)(n ? n : 1), sizeof(ld));
    ld *z = (ld *)malloc(sizeof(ld) * (size_t)n);
    ld *al = (ld *)malloc(sizeof(ld) * (size_t)n);
    ld *sv = (ld *)malloc(sizeof(ld) * (size_t)n);
    if (!U || !rr || !z || !al || !sv) { free(U); free(rr); free(z); free(al); free(sv); return -1; }
    for (long i = 0; i < n; i++) {
        rr[i] = (ld)r[i];
        sv[i] = vX ? sqrtl((ld)vX[i]) : 0;
    }
    fwd(n, L, rr, z);
    bwd(n, L, z, al);
    if (alpha_out) for (long i = 0; i < n; i++) alpha_out[i] = al[i];
    ld logdet = 0, logdet_mag = 0, fit = 0, fit_mag = 0;
    for (long i = 0; i < n; i++) {
        ld lg = logl((ld)L[i * n + i]);
        logdet += lg;
        logdet_mag += fabsl(lg);
        fit += rr[i] * al[i];
        fit_mag += fabsl(rr[i] * al[i]);
    }
    out[0] = -0.5L * ((ld)n * LOG_2PI + 2 * logdet + fit);
    mag[0] = 0.5L * ((ld)n * LOG_2PI + 2 * logdet_mag + fit_mag);
    /* columns of L^-1 */
#pragma omp parallel for schedule(dynamic, 8)
    for (long j = 0; j < n; j++) {
        ld *x = U + j * n;
        for (long i = j; i < n; i++) {
            const double *Li = L + i * n;
            ld s = (i == j) ? 1 : 0;
            for (long k = j; k < i; k++) s -= (ld)Li[k] * x[k];
            x[i] = s / (ld)Li[i];
        }
    }
    const ld s2 = (ld)variance;
    ld acc[3 + MAXD], accm[3 + MAXD];
    for (int t = 0; t < 3 + MAXD; t++) acc[t] = accm[t] = 0;
#pragma omp parallel
    {
        ld a[3 + MAXD], am[3 + MAXD], g[MAXD];
        for (int t = 0; t < 3 + MAXD; t++) a[t] = am[t] = 0;
#pragma omp for schedule(dynamic, 8)
        for (long i = 0; i < n; i++) {
            const ld *Ui = U + i * n;
            for (long j = 0; j <= i; j++) {
                /* W_ij = sum_{k >= i} L^-1_ki L^-1_kj  (i >= j) */
                const ld *Uj = U + j * n;
                ld w = 0;
                for (long k = i; k < n; k++) w += Ui[k] * Uj[k];
                const ld aa = al[i] * al[j];
                const ld dk = 0.5L * (aa - w), dkm = 0.5L * (fabsl(aa) + fabsl(w));
                const ld mult = (i == j) ? 1 : 2;
                const ld r2 = sqdist(X + i * d, X + j * d, d, ls, ard, g);
                const ld krbf = s2 * expl(-0.5L * r2);
                const ld kfull = krbf + sv[i] * sv[j];
                a[0] += mult * dk * kfull;
                am[0] += mult * dkm * fabsl(kfull);
                if (i == j) { a[1] += dk; am[1] += dkm; }
                for (int t = 0; t < nl; t++) {
                    a[2 + t] += mult * dk * krbf * g[t];
                    am[2 + t] += mult * dkm * krbf * g[t];
                }
            }
        }
#pragma omp critical
        for (int t = 0; t < 2 + nl; t++) { acc[t] += a[t]; accm[t] += am[t]; }
    }
    out[1] = acc[0] / s2;
    mag[1] = accm[0] / s2;
    out[2] = acc[1];
    mag[2] = accm[1];
    for (int t = 0; t < nl; t++) { out[3 + t] = acc[2 + t]; mag[3 + t] = accm[2 + t]; }
    free(U); free(rr); free(z); free(al); free(sv);
    return 0;
}

/* dmean / dvar (m x d row-major) of GPy predictive_gradients: dmean_k = sum_i alpha_i Krbf_i (x_ik - x*_k) / l_k^2,
 * dvar_k = -2 sum_i w_i Krbf_i (x_ik - x*_k) / l_k^2 with w = (L L^T)^-1 k(X, x*) (causal rank-1 term included in k,
 * not differentiated).  mag_*: the same sums over absolute values. */
int ld_prediction_gradients(long n, int d, const double *L, const double *alpha, const double *X, long m,
                            const double *Xs, const double *vX, const double *vXs, double variance, const double *ls,
                            int ard, ld *dmean, ld *dvar, ld *mag_mean, ld *mag_var)
{
    if (d < 1 || d > MAXD) return -1;
    for (long i = 0; i < n; i++) if (!(L[i * n + i] > 0)) return (int)(i + 1);
    const ld s2 = (ld)variance;
    int fail = 0;
#pragma omp parallel
    {
        ld *kx = (ld *)malloc(sizeof(ld) * (size_t)n);
        ld *kr = (ld *)malloc(sizeof(ld) * (size_t)n);
        ld *v = (ld *)malloc(sizeof(ld) * (size_t)n);
        ld *w = (ld *)malloc(sizeof(ld) * (size_t)n);
        if (!kx || !kr || !v || !w) {
#pragma omp atomic write
            fail = 1;
        }
#pragma omp for schedule(dynamic, 1)
        for (long c = 0; c < m; c++) {
            if (!kx || !kr || !v || !w) continue;
            const double *xs = Xs + c * d;
            const ld svs = (vX && vXs) ? sqrtl((ld)vXs[c]) : 0;
            for (long i = 0; i < n; i++) {
                kr[i] = s2 * expl(-0.5L * sqdist(X + i * d, xs, d, ls, ard, NULL));
                kx[i] = kr[i] + ((vX && vXs) ? sqrtl((ld)vX[i]) * svs : 0);
            }
            fwd(n, L, kx, v);
            bwd(n, L, v, w);
            for (int k = 0; k < d; k++) {
                const ld l = ard ? (ld)ls[k] : (ld)ls[0];
                ld sm = 0, sv = 0, am = 0, av = 0;
                for (long i = 0; i < n; i++) {
                    const ld t = kr[i] * ((ld)X[i * d + k] - (ld)xs[k]) / (l * l);
                    sm += (ld)alpha[i] * t;
                    am += fabsl((ld)alpha[i] * t);
                    sv += w[i] * t;
                    av += fabsl(w[i] * t);
                }
                dmean[c * d + k] = sm;
                dvar[c * d + k] = -2 * sv;
                mag_mean[c * d + k] = am;
                mag_var[c * d + k] = 2 * av;
            }
        }
        free(kx); free(kr); free(v); free(w);
    }
    return fail ? -1 : 0;
}

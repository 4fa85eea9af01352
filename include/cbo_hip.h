/* cbo_hip.h -- C-ABI of libcbo_hip.so: MI355X (gfx950) GP posterior update + causal acquisition sweep.
 *
 * The reference (ChampiB/CBO_with_OOP, pure Python) has no FFI layer; its operator API for this path
 * is a Python duck type.  Each entry point below names the reference interface it
 * replaces (paths relative to /root/reference/).  The Python host side in cbo_with_oop_amd/ binds
 * exactly these symbols with ctypes (cbo_with_oop_amd/_lib.py); INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only; all host arrays are C-contiguous float64 (row-major
 * (n,d) for points); the caller owns every host buffer and it is only touched during the call; every
 * function returns 0 (CBO_OK) or a negative cbo_status and records a message for cbo_last_error();
 * a handle is bound to one HIP device + one stream and is not thread-safe (distinct handles are).
 * There is no CPU fallback anywhere behind this interface.
 */
#ifndef CBO_HIP_H
#define CBO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cbo_timers gained ms_f32_convert (the library writes sizeof(cbo_timers) bytes into the caller's struct),
 *    cbo_gp_create accepts CBO_DTYPE_F32, cbo_synchronize is device-wide.
 * cbo_abi_version() returns this value. */
#define CBO_HIP_ABI_VERSION 5
#define CBO_MAX_DIM 8

typedef enum cbo_status {
    CBO_OK = 0,
    CBO_ERR_INVALID = -1,     /* bad argument (shape, NULL, dtype) */
    CBO_ERR_HIP = -2,         /* a HIP runtime call failed; see cbo_last_error() */
    CBO_ERR_NOT_PD = -3,      /* jitchol exhausted its 5 retries (numpy.linalg.LinAlgError in GPy) */
    CBO_ERR_NONPOS_DIAG = -4, /* jitchol: "not pd: non-positive diagonal elements" */
    CBO_ERR_NOT_FITTED = -5,
    CBO_ERR_UNSUPPORTED = -6, /* a request this build cannot serve (e.g. a workspace cap too small for the call) */
    CBO_ERR_NO_DEVICE = -7,
    CBO_ERR_COMM = -8
} cbo_status;

enum { CBO_DTYPE_F64 = 0, CBO_DTYPE_F32 = 1 };
enum { CBO_TASK_MIN = 0, CBO_TASK_MAX = 1 };

typedef struct cbo_ctx cbo_ctx;     /* one HIP device + stream + workspaces */
typedef struct cbo_gp cbo_gp;       /* one GP posterior resident on a ctx */
typedef struct cbo_cands cbo_cands; /* one candidate-intervention set resident on a ctx */

/* Per-phase device time of the calls made since cbo_reset_timers(), from hipEvents recorded on the
 * ctx stream (only while profiling is enabled with cbo_set_profiling).  ms_* are sums, n_* counts. */
typedef struct cbo_timers {
    double ms_kxx;     /* K(X,X) assembly (+ diagonal)                       */
    double ms_chol;    /* jittered Cholesky incl. forward solve z = L^-1 r   */
    double ms_alpha;   /* backward solve alpha = L^-T z                      */
    double ms_kstar;   /* K(X,X*) assembly                                   */
    double ms_trsm;    /* V = L^-1 K*, fused sum(V^2) and V^T z  (dominant)  */
    double ms_acq;     /* variance/EI/cost/argmax epilogue                   */
    int64_t n_fit;     /* number of fits timed                               */
    int64_t n_sweep;   /* number of sweeps / predicts timed                  */
    int64_t n_trsm_launches;
    double trsm_flops; /* algorithmic flops of the timed trsm launches: sum n_pad^2 * m_pad */
    double ms_f32_convert; /* CBO_DTYPE_F32 models: factor / diagonal inverses / z down-converted after a fit */
} cbo_timers;

/* ---- context ---------------------------------------------------------------------------------- */
int cbo_abi_version(void);
const char *cbo_last_error(void);
int cbo_device_count(int *count_out);
/* Bind device `device_id`; fails with CBO_ERR_NO_DEVICE when no gfx950-class GPU is visible. */
int cbo_init(int device_id, cbo_ctx **out);
/* Releases everything the context owns.  Contexts still open when the process exits are shut down by an atexit
 * handler the first cbo_init registers (it runs before the HIP runtime's own exit handlers: a context's CU-masked
 * streams must not outlive the runtime -- tools that hook finalisation crash otherwise); a handle that was already
 * shut down is ignored.  Models, candidate sets and communicators of a context must be destroyed before it. */
void cbo_shutdown(cbo_ctx *ctx);
int cbo_synchronize(cbo_ctx *ctx);
int cbo_set_profiling(cbo_ctx *ctx, int enabled);
int cbo_reset_timers(cbo_ctx *ctx);
int cbo_get_timers(cbo_ctx *ctx, cbo_timers *out);
int cbo_device_name(cbo_ctx *ctx, char *buf, int buflen);
/* Device time (hipEvents on the ctx stream) of everything enqueued between the two calls; the work of the
 * other streams a call uses joins the ctx stream before the call returns, so it is covered. */
int cbo_region_begin(cbo_ctx *ctx);
int cbo_region_end(cbo_ctx *ctx, double *ms_out);

/* ---- GP model ----------------------------------------------------------------------------------
 * Replaces GaussianProcessFactory.create / create_non_causal_gp / create_causal_gp / create_graph_gp
 * (src/GaussianProcessFactory.py:24-73) + GPy GPRegression construction.  prior_mean_X / prior_var_X
 * are the reference's mean_function(X) / variance_adjustment(X) closures (DoCalculus.py:34-66)
 * already evaluated on X (NULL, NULL = non-causal kernel, zero mean).  zero_diag selects GPy's
 * X2=None distance shortcut (plain RBF) vs CausalRBF's explicit-X2 path (causal_kernels.py:53-55).
 * Uploads X, y, priors; does not fit. */
/* dtype (BASELINE.json configs[4], "fp32 path with MFMA"): CBO_DTYPE_F64 -- everything fp64; CBO_DTYPE_F32 -- the
 * FIT stays fp64 (Ky carries a 1e-8 jitter fp32 cannot represent) and every sweep / predict of the model runs its
 * substitution V = L^-1 K* on the f32 MFMA (157 TFLOP/s dense against 78.6 for fp64) from a once-per-fit fp32 copy of
 * the factor; K* is evaluated in fp64 and rounded to fp32, q = sum V^2 and mu = V^T z accumulate in fp64.  Accuracy is
 * that of an fp32 triangular solve: about 6e-8 * sqrt(cond(Ky)) relative in V (tests/test_f32_gpu.py states what it
 * meets on the coral ranges); cbo_gp_append and cbo_cands_keep_solution do not apply (the caller refits). */
int cbo_gp_create(cbo_ctx *ctx, int dtype, int64_t n, int d, const double *X, const double *y,
                  const double *prior_mean_X, const double *prior_var_X, double variance,
                  const double *lengthscale /* 1 value, or d values if ard */, int ard,
                  double noise_var, int zero_diag, cbo_gp **out);
void cbo_gp_destroy(cbo_gp *gp);

/* GPy ExactGaussianInference.inference + util.linalg.jitchol: K(X,X) assembly, Ky = K+(noise+1e-8)I,
 * jittered Cholesky (retry ladder mean(diag)*1e-6 x10, <= 5 retries) with the forward solve
 * z = L^-1 (y - m) carried through the factorisation.  GPy's alpha = L^-T z is materialised on first use
 * (cbo_gp_get_posterior): predict and the sweep form the mean as (L^-1 k*)^T z.  Everything runs on the
 * device from the resident X, y.  jitter_tries_out / jitter_out may be NULL. */
int cbo_gp_fit(cbo_gp *gp, int *jitter_tries_out, double *jitter_out);

/* emukit GPyModelWrapper.set_data -> GPy set_XY (called from src/Monitor.py:160): replace the data
 * and refit. */
int cbo_gp_set_data(cbo_gp *gp, int64_t n, const double *X, const double *y,
                    const double *prior_mean_X, const double *prior_var_X);

/* The upload half of cbo_gp_set_data: replace the data and leave the model unfitted, for a caller that refits
 * together with the next sweep (cbo_gp_fit_sweep).  Any call that needs the posterior returns
 * CBO_ERR_NOT_FITTED until then. */
int cbo_gp_upload_data(cbo_gp *gp, int64_t n, const double *X, const double *y,
                       const double *prior_mean_X, const double *prior_var_X);

/* One more observation for a fitted model -- what every CBO trial does to the set it intervened on
 * (src/Monitor.py:148-160 appends to data_x/data_y, src/CBO.py:224-235 rebuilds the model from them).  Appending
 * row/column n to Ky leaves the first n rows of its factor unchanged: the new column is one forward solve, done as
 * an ordinary one-candidate sweep.  *appended_out = 1: the model is fitted on n+1 points; 0: nothing changed, the
 * shortcut does not apply (jitter in the current factor, padded size exhausted, non-positive pivot) and the caller
 * refits with cbo_gp_set_data.  Same results as a full refit up to rounding. */
int cbo_gp_append(cbo_gp *gp, const double *x_new, double y_new, double prior_mean_new, double prior_var_new,
                  int *appended_out);

/* k more observations for a fitted model in one device step -- the results of a batch picked by cbo_acq_sweep_batch
 * coming back together (src/Monitor.py:148-160 appends once per result).  With L the current factor, z = L^-1 (y - m),
 * Xb the k new points and sigma = noise_var + 1e-8:
 *     B   = L^-1 K(X, Xb)                          (n x k)
 *     S   = K(Xb, Xb) + sigma I - B^T B            (k x k; the diagonal prior term is variance + v(x), as cbo_gp_append's;
 *                                                   off-diagonal entries with X2 explicit, + sqrt(v) sqrt(v) when causal)
 *     L22 = chol(S),   zb = L22^-1 ((yb - m(Xb)) - B^T z)
 *     U[0:n, n:n+k] = B,  U[n:n+k, n:n+k] = L22^T,  z[n:n+k] = zb   (the rhs column of the factor's buffer carries z too)
 * The resident data (y, coordinates, prior closures) grow by k rows and the diagonal-tile inverses gain the columns of
 * the new rows.  *appended_out = 1: the model is fitted on n + k points, same results as a full refit up to rounding.
 * *appended_out = 0: nothing at all changed and the caller refits with cbo_gp_set_data -- under cbo_gp_append's rules:
 * jitter in the current factor, n + k beyond the padded size (n + k equal to it is allowed), an fp32 model, or a pivot
 * of S that is not positive and finite (decided on the device before anything is committed).  k = 1 is cbo_gp_append
 * itself.  A candidate set that keeps its solution (cbo_cands_keep_solution) and was swept on the model just before
 * the block gains the k new rows of V in one pass at its next sweep:  C = K(Xb, X*) - B^T V[0:n, :],  W = L22^-1 C,
 * V[n:n+k, :] = W,  q += sum_r W_r^2,  mu += sum_r W_r zb_r (r in row order); every other set takes the substitution.
 * Every sum has a fixed order: two identical call sequences give the same bits.
 * X_new: k * d row-major; prior_mean_new / prior_var_new: k values each for a causal model, NULL otherwise.
 * CBO_ERR_INVALID: k outside 1..CBO_MAX_APPEND, NULL gp, X_new, y_new or appended_out, a causal model without both prior
 * arrays; CBO_ERR_NOT_FITTED: the model is not fitted. */
#define CBO_MAX_APPEND 64
int cbo_gp_append_block(cbo_gp *gp, int k, const double *X_new, const double *y_new, const double *prior_mean_new,
                        const double *prior_var_new, int *appended_out);

/* GPyModelWrapper.predict -> GP.predict -> Posterior._raw_predict (called from
 * src/utils_functions/causal_acquisition_functions.py:33 and src/DoCalculus.py:77):
 * mean = K*^T Ky^-1 (y-m) + m(X*), var = clip(Kdiag - |L^-1 K*|^2, 1e-15) (+ noise). */
int cbo_gp_predict(cbo_gp *gp, int64_t m, const double *Xs, const double *prior_mean_s,
                   const double *prior_var_s, int include_noise, double *mean_out, double *var_out);

/* Joint posterior (emukit GPyModelWrapper.predict_with_full_covariance / predict_covariance /
 * get_covariance_between_points / calculate_variance_reduction, the methods emukit's multipoint, variance-reduction and
 * entropy acquisitions call next to src/utils_functions/causal_acquisition_functions.py).
 *
 * cbo_gp_predict_cov: GPy GP.predict(X, full_cov=True) -> PosteriorExact._raw_predict, full_cov branch,
 * Kxx - (L^-1 Kx)^T (L^-1 Kx) (+ mean function, + Gaussian.predictive_values: noise_var on the diagonal when
 * include_noise).  mean_out (m, may be NULL) is what cbo_gp_predict returns; cov_out is m*m row-major, exactly symmetric.
 * cbo_gp_cov_between: GPy posterior_covariance_between_points(X1, X2) (include_likelihood=False):
 * K(X1,X2) - (L^-1 K(X,X1))^T (L^-1 K(X,X2)); cov_out m1*m2 row-major; noise-free.
 *
 * The prior term follows the kernel GPy evaluates, in kmat's operation order (GEMM-trick squared distance, clip at 0,
 * scale, exp, causal term):
 *  - non-causal models (GPy RBF): Kxx = K(X) with X2 = None, so the squared distance on the diagonal of
 *    cbo_gp_predict_cov is exactly 0 (the model's zero_diag rule, as for K(X,X)); cbo_gp_cov_between passes X2.
 *  - causal models (CausalRBF.K, src/utils_functions/causal_kernels.py:53-61): X2 is always passed explicitly, no
 *    diagonal shortcut, and sqrt(v(X1)) sqrt(v(X2))^T is added everywhere.  The diagonal of the full covariance is
 *    therefore NOT Kdiag (variance + v, causal_kernels.py:64-79) but variance * exp(-r2_ii / 2) + v, r2_ii the rounding
 *    residue of the GEMM-trick distance of a point to itself: GPy's quirk, kept.
 * The full covariance is not clipped (the 1e-15 clip of cbo_gp_predict belongs to the diagonal branch).  Causal models
 * need prior_var_* (and prior_mean_s when mean_out is requested): CBO_ERR_INVALID otherwise.  Unfitted model:
 * CBO_ERR_NOT_FITTED; NULL arguments or m <= 0: CBO_ERR_INVALID; a failed device allocation: CBO_ERR_HIP.  fp32 models
 * answer from the fp64 factor (the fp64 model's result).  Every call solves L^-1 K* afresh; the solution of all points
 * must fit the context's workspace at once. */
int cbo_gp_predict_cov(cbo_gp *gp, int64_t m, const double *Xs, const double *prior_mean_s,
                       const double *prior_var_s, int include_noise, double *mean_out, double *cov_out);
int cbo_gp_cov_between(cbo_gp *gp, int64_t m1, const double *X1, const double *prior_var_1,
                       int64_t m2, const double *X2, const double *prior_var_2, double *cov_out);

/* Joint posterior samples (GPy GP.posterior_samples_f(X, size), which draws np.random.multivariate_normal(mean, cov,
 * size) from the full_cov prediction): samples_out[i][j] = mean_i + sum_k L[i][k] normals[j][k], with L L^T = Sigma +
 * jitter I.  Sigma is exactly cbo_gp_predict_cov(..., include_noise = 0, ...) (the causal diagonal quirk and the
 * zero-distance rule included) and the mean is cbo_gp_predict's, bit for bit.  normals: n_samples * m row-major, one
 * draw per row (the caller's standard normals: the library has no generator of its own); samples_out: m * n_samples
 * row-major, point i, sample j.  GPy factors Sigma by SVD, this call by Cholesky: same distribution, other draws.
 *
 * Jitter ladder: a plain attempt, then 1e-6 * mean(Kdiag(X*)) on the diagonal, x10 per retry, at most 5 retries; Kdiag
 * is the PRIOR diagonal, variance + v(x), which is always positive.  This differs on purpose from jitchol (cbo_gp_fit),
 * whose base is the mean of the matrix's own diagonal: a posterior diagonal can be ~1e-12 or slightly negative at
 * training points, where jitchol would give up with "non-positive diagonal".  *jitter_tries_out (retries taken) and
 * *jitter_out (the jitter of the factor used) may be NULL.
 *
 * Unfitted model: CBO_ERR_NOT_FITTED; NULL arguments, m <= 0, n_samples <= 0, or a causal model without prior_var_s or
 * prior_mean_s: CBO_ERR_INVALID; the ladder runs out: CBO_ERR_NOT_PD; a failed device allocation: CBO_ERR_HIP.  fp32
 * models answer from the fp64 factor.  The solution L^-1 K* of all points must fit the context's workspace at once, as
 * for cbo_gp_predict_cov.  The model is left untouched (factor, z, alpha, fitted state, candidate sets). */
int cbo_gp_posterior_samples(cbo_gp *gp, int64_t m, const double *Xs, const double *prior_mean_s,
                             const double *prior_var_s, int64_t n_samples, const double *normals, double *samples_out,
                             int *jitter_tries_out, double *jitter_out);

/* Integrated variance reduction (emukit IntegratedVarianceReduction.evaluate, which averages
 * GPyModelWrapper.calculate_variance_reduction(x_i, Xint) = cov(x_i, Xint)^2 / predict(x_i)[1] over the integration
 * points), for m candidates at once and divided by a cost, as emukit's Quotient with a Cost has it:
 *     ivr_out[i] = ((sum_j C(x_i, xint_j)^2 / var_i) / p) / cost,
 * C = cbo_gp_cov_between(Xs, Xint) element for element (same prior term, same rounding), var_i = cbo_gp_predict's
 * variance with the noise (include_noise = 1), bit for bit.  No m x p matrix is stored: the squares are summed in the
 * product's epilogue, one partial per candidate and 128-column tile, and the partials in a fixed order, so two calls give
 * the same bits.  best_val / best_idx: the arg-max of ivr_out (lowest index on ties, NaN maximal).  ivr_out (m),
 * best_val and best_idx may each be NULL, but not all three.
 *
 * The solution of the m candidates must fit the context's workspace (CBO_HIP_WORKSPACE_MB) together with one
 * 128-column tile of integration points; the integration points need not fit: they are solved in chunks of whole tiles
 * in the workspace that remains, and the result is the same bits for any number of chunks.  The candidates are solved
 * once per call.
 *
 * Unfitted model: CBO_ERR_NOT_FITTED; NULL arguments, m <= 0, p <= 0, cost <= 0 (or NaN), a causal model without
 * prior_var_s or prior_var_int, or candidates whose solution does not fit: CBO_ERR_INVALID; a failed device allocation:
 * CBO_ERR_HIP.  fp32 models answer from the fp64 factor (the fp64 model's result).  The model is left untouched
 * (factor, z, alpha, fitted state, candidate sets). */
int cbo_gp_integrated_variance_reduction(cbo_gp *gp, int64_t m, const double *Xs, const double *prior_var_s,
                                         int64_t p, const double *Xint, const double *prior_var_int, double cost,
                                         double *ivr_out, double *best_val, int64_t *best_idx);

/* Max-value entropy search (emukit MaxValueEntropySearch, Wang & Jegelka 2017; emukit 0.4 restated from memory, parity
 * unpinned: DESIGN.md §4e), the entropy acquisition emukit users reach for after EI, in two calls.
 *
 * cbo_gp_mes_gumbel: MaxValueEntropySearch.update_parameters' model.predict(grid) (noise included) and _fit_gumbel's three
 * scipy.optimize.bisect(lambda x: probf(x) - val, left, right, maxiter=10000) calls, val = 0.25, 0.5, 0.75, with
 *     probf(x) = 1 - exp(sum_i log_ndtr(-(x - fmean_i) / fsd_i)),  fsd = sqrt(fvar),
 *     left = min(fmean - 5 fsd), right = max(fmean + 5 fsd),
 * scipy's xtol = 2e-12 and rtol = 4 eps, and scipy's loop (Zeros/bisect.c); quantiles3 = (q25, q50, q75),
 * b = (q25 - q75) / (log(log(4/3)) - log(log(4))), a = q50 - b log(log(2)).  The m grid points Xg (emukit stacks model.X
 * on top of its uniform grid; the caller does) are predicted as cbo_gp_predict predicts them and the bisections run on the
 * device from that mean and variance: nothing comes back in between.  mean_out / var_out (m, may be NULL): the grid's
 * mean and variance, bit for bit cbo_gp_predict's.  The sums over the grid run in a fixed order (two calls give the same
 * bits), not numpy's: a decision of the bisection can differ from scipy's where probf(x) - val is at rounding level.
 * A bracket whose ends do not change sign (scipy's ValueError) or a bisection that does not converge: CBO_ERR_INVALID
 * with a message.  Unfitted model: CBO_ERR_NOT_FITTED; NULL arguments, m <= 0, a causal model without prior_mean_g and
 * prior_var_g: CBO_ERR_INVALID.  The model is only read.
 *
 * cbo_acq_sweep_mes: MaxValueEntropySearch.evaluate / Cost over a candidate set, with the arg-max:
 *     acq = mean_k(-g_k pdf(g_k) / (2 c_k) - log(c_k)) / cost,  g_k = (mins[k] - mean) / max(sqrt(var), 1e-10),
 *     c_k = clip(1 - ndtr(g_k), 1e-10, 1),
 * mean / var as cbo_acq_sweep forms them (same path: the candidates' cached q, mu when the fit stamp matches, one appended
 * row, the fp32 strip of fp32 models), so mean_out / var_out are bit for bit cbo_acq_sweep's.  The mean over the samples
 * is summed in numpy's order (np.mean(axis=1)).  best_idx: lowest index on ties, NaN maximal, offset by the set's
 * index_offset.  acq_out / mean_out / var_out (m doubles each) may be NULL.  n_samples is at most 64 (the samples travel
 * in the kernel's arguments).  n_samples <= 0 or > 64, NULL or non-finite mins, cost <= 0 or NaN, a causal model whose
 * candidates carry no prior: CBO_ERR_INVALID; unfitted model: CBO_ERR_NOT_FITTED.  The model is only read. */
int cbo_gp_mes_gumbel(cbo_gp *gp, int64_t m, const double *Xg, const double *prior_mean_g, const double *prior_var_g,
                      double *quantiles3, double *a, double *b, double *mean_out, double *var_out);
int cbo_acq_sweep_mes(cbo_gp *gp, cbo_cands *cands, int n_samples, const double *mins, double cost, double *acq_out,
                      double *mean_out, double *var_out, double *best_val, int64_t *best_idx);

/* Constrained acquisition: Expected Improvement times the probability that up to CBO_MAX_CONSTRAINTS other nodes of the
 * graph stay inside their range, over a cost -- emukit's
 *     Quotient(Product(Product(ExpectedImprovement, ProbabilityOfFeasibility_0), ProbabilityOfFeasibility_1) ..., Cost):
 *     acq_i = (((EI_i * pof_0i) * pof_1i) * ...) / cost        (multiplications left to right, one IEEE division last)
 * in ONE pass over the m candidates with the arg-max, from the q = sum V^2, mu = V^T z of n_con + 1 (model, candidate set)
 * pairs.  emukit's ProbabilityOfFeasibility is restated from memory (emukit is not a dependency; parity is unpinned, the
 * contract is DESIGN.md §4f).
 *  - EI_i: what cbo_acq_sweep(gp, cands, y_best, task, ei_jitter, 1.0, ...) writes to acq_out[i], bit for bit (the 'max'
 *    task's sign quirk included); ei_out (m, may be NULL).
 *  - pof_ki = ndtr(u) for con_sense[k] = CBO_CON_LE (scipy.stats.norm.cdf(con_value, mean, sd)), ndtr(-u) for
 *    CBO_CON_GE, u = (con_value[k] - (mean_ki + con_jitter[k])) / sqrt(var_ki); mean / var: constraint model k's
 *    cbo_gp_predict(..., include_noise = 1) at candidate i of con_cands[k], bit for bit; ndtr is the cephes restatement
 *    the EI pass uses, the quotient is within an ulp of the IEEE one.  pof_out (n_con * m, constraint-major, may be NULL).
 *  - gp == NULL and cands == NULL: no objective, acq = (pof_0 * pof_1 * ...) / cost (ProbabilityOfFeasibility.evaluate on
 *    its own, or a product of them); n_con >= 1, ei_out must be NULL, y_best / task / ei_jitter are not read.
 *  - n_con = 0 (with an objective): cbo_acq_sweep's acq_out, best_val and best_idx with the same cost (only the sign of a
 *    zero can differ).
 *  - best_idx: lowest index on ties, NaN maximal, offset by the index_offset of the objective's set (of the first
 *    constraint's without an objective).  acq_out (m) may be NULL.
 * Every pair reaches its q, mu exactly as cbo_acq_sweep would (the candidates' cached copies when the fit stamp matches,
 * one appended row after cbo_gp_append, the fp32 strip of fp32 models, the chunked substitution otherwise), one pair after
 * the other; the vectors stay in the candidates' own buffers, also with CBO_HIP_SWEEP_CACHE=0 (same bits either way).
 * Every set has the same m, candidate i of every set is the same intervention; a set may serve several pairs only with
 * the same model.  Out of scope: refitting in the same call (cbo_gp_fit_sweep).  The single launch of small sets is
 * cbo_acq_sweep_sets_constrained, below.  The models are only read.
 * CBO_ERR_INVALID: n_con outside 0..CBO_MAX_CONSTRAINTS (or 0 without an objective), only one of gp / cands NULL, a NULL
 * among the first n_con entries or a NULL array with n_con > 0, pairs on different contexts, sets whose m differ,
 * gp->d != cands->d in a pair, a causal model whose set carries no prior, one set with two models, a non-finite con_value
 * or con_jitter, a sense other than the two, cost <= 0 or NaN, a bad task with an objective, ei_out without one.
 * An unfitted model: CBO_ERR_NOT_FITTED. */
#define CBO_MAX_CONSTRAINTS 8
enum { CBO_CON_LE = 0, CBO_CON_GE = 1 };
int cbo_acq_sweep_constrained(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double ei_jitter, double cost,
                              int n_con, cbo_gp *const *con_gps, cbo_cands *const *con_cands,
                              const double *con_value, const double *con_jitter, const int *con_sense,
                              double *acq_out, double *ei_out, double *pof_out /* n_con * m, constraint-major */,
                              double *best_val, int64_t *best_idx);

/* The constrained acquisition in log space: cbo_acq_sweep_constrained's argument list, ei_out and pof_out
 * becoming logei_out and logpof_out, ei_jitter the log EI's jitter:
 *     acq_out[i] = (((logEI_i + l_0i) + l_1i) + ...) - log(cost)                    (additions left to right, log(cost) once)
 * logEI_i is what cbo_acq_sweep_logei(gp, cands, y_best, task, ei_jitter, 1.0, ...) writes to acq_out[i] -- task 'max' its
 * mirror, the improvement of a maximiser, not the product form's -EI -- and l_ki = log_ndtr(u_ki) with u_ki the very
 * argument whose ndtr cbo_acq_sweep_constrained multiplies in.  Finite and ordered where EI, a probability or their
 * product is an exact 0.  Contracts: n_con = 0 gives cbo_acq_sweep_logei's acq_out, best_val and best_idx bit for bit for
 * every cost; logei_out is its acq_out at cost 1; per-candidate outputs do not change the values; the arg-max is
 * numpy.argmax(acq_out) + index_offset (lowest index on ties, NaN maximal, -inf an ordinary value).
 * Errors are cbo_acq_sweep_constrained's, and with an objective a non-finite ei_jitter or y_best. */
int cbo_acq_sweep_constrained_log(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double ei_jitter, double cost,
                                  int n_con, cbo_gp *const *con_gps, cbo_cands *const *con_cands,
                                  const double *con_value, const double *con_jitter, const int *con_sense,
                                  double *acq_out, double *logei_out, double *logpof_out /* n_con * m, constraint-major */,
                                  double *best_val, int64_t *best_idx);

/* The causal EI over a cost, marginalised over hyper-parameter samples, with the arg-max -- emukit's
 * IntegratedHyperParameterAcquisition(model, acquisition_generator, n_samples) around ExpectedImprovement / Cost, whose
 * evaluate() is `for sample in samples: model.fix_model_hyperparameters(sample); acquisition_value += acquisition.evaluate(x)`
 * and `return acquisition_value / n_samples` (emukit 0.4 restated from memory; emukit is not a dependency, parity is
 * unpinned, the contract is DESIGN.md §4j):
 *     acq_out[i] = ((((0 + a_0i) + a_1i) + ...) + a_(H-1)i) / H       (additions in sample order, one IEEE division last)
 * where a_hi is what cbo_acq_sweep(gp_h, cands, y_best, task, ei_jitter, cost, ...) writes to acq_out[i] for a model gp_h
 * with the data of gp and the hyper-parameters of sample h -- the 'max' task's sign quirk and the causal priors included;
 * m(.) and v(.) at X and X* do not depend on the sample.  Two identical calls return the same bits.
 * hyper: n_samples rows of (variance, lengthscale x L, noise_var), L = d if the model is ard else 1: GPy's parameter order
 * for GPRegression with an RBF kernel (rbf.variance, rbf.lengthscale, Gaussian_noise.variance).
 * best_idx: lowest index on ties, NaN maximal, offset by the set's index_offset.  acq_out (m) may be NULL; best_val and
 * best_idx may be NULL when acq_out is not.
 *  - An fp64 model of at most 128 observations (unless CBO_HIP_SMALL_SETS=0, or above 65535 candidate blocks of 64) is
 *    answered by one launch (two from 12 candidate blocks on) that factors every sample's Ky inside LDS from the model's
 *    and the set's RAW coordinates.  The model need not be fitted, and NOTHING of the model or the candidate set is touched:
 *    factor, z, fit stamp, hyper-parameters, the scaled point sets, cached q / mu, kept solutions.  A cbo_acq_sweep before
 *    and after the call returns the same bits.
 *  - Larger and fp32 models, and a small model one of whose samples is not positive definite as assembled, take the general
 *    path: for h in order cbo_gp_set_hyper, cbo_gp_fit (the jitchol ladder) and cbo_acq_sweep with the acquisition kept on
 *    the device and added in by a small kernel; one closing kernel divides and takes the arg-max.  Afterwards the model's
 *    hyper-parameters are restored and, if it was fitted on entry, it is refitted: the same factor (the fit is
 *    deterministic) under a NEW fit stamp, so the caches of every candidate set swept with this model are recomputed at
 *    their next sweep, and a kept solution no longer extends by an append.  A sample whose ladder runs out: CBO_ERR_NOT_PD
 *    (CBO_ERR_NONPOS_DIAG), after restoring.
 * CBO_ERR_INVALID: cbo_acq_sweep's argument checks, n_samples outside 1..CBO_MAX_HYPER_SAMPLES, NULL hyper, NULL best_val
 * or best_idx together with NULL acq_out, cost <= 0 or NaN, a non-finite or non-positive variance or lengthscale or a
 * negative or non-finite noise_var in any row.  There is no CBO_ERR_NOT_FITTED: neither path needs a fit. */
#define CBO_MAX_HYPER_SAMPLES 256
int cbo_acq_sweep_hyper(cbo_gp *gp, cbo_cands *cands, int n_samples,
                        const double *hyper /* n_samples rows of (variance, lengthscale x L, noise_var) */,
                        double y_best, int task, double ei_jitter, double cost, double *acq_out /* m, may be NULL */,
                        double *best_val, int64_t *best_idx);

/* The point-wise acquisitions a GPy / emukit user reaches for next to EI, over a cost, with the arg-max: emukit's
 * NegativeLowerConfidenceBound, ProbabilityOfImprovement, MeanPluginExpectedImprovement and (experimental design)
 * ModelVariance under a Quotient with a Cost (emukit 0.4 restated from memory; emukit is not a dependency, parity is
 * unpinned, the contract is DESIGN.md §4k).  mean / var: cbo_gp_predict(..., include_noise = 1) at the candidate, bit for
 * bit -- what cbo_acq_sweep writes to mean_out / var_out; s = sqrt(var), the IEEE square root.
 *  - CBO_ACQ_LCB:  acq = -(mean - param * s) / cost for task 'min', (mean + param * s) / cost for 'max'; param = beta,
 *    finite and >= 0; y_best is not read.  One rounding per operation, as numpy applies them.  The value can be negative,
 *    and it is divided by the cost all the same, as emukit's Quotient does: a negative bound then FAVOURS the costly
 *    intervention.
 *  - CBO_ACQ_PI:   acq = ndtr(u) / cost for 'min', ndtr(-u) / cost for 'max', u = (y_best - (mean + param)) / s; param = the
 *    jitter.  At cost 1 bit for bit the pof_out of cbo_acq_sweep_constrained(NULL, NULL, ..., n_con = 1, the same model and
 *    set, con_value = y_best, con_jitter = param, CBO_CON_LE for 'min', CBO_CON_GE for 'max').
 *  - CBO_ACQ_VAR:  acq = var / cost; y_best, task and param are not read.
 *  - CBO_ACQ_MPEI: cbo_acq_sweep(gp, cands, cbo_gp_plugin_incumbent(gp, task), task, param, cost, ...) bit for bit -- acq_out,
 *    best_val and best_idx -- with the incumbent kept on the device (no host round trip); param = EI's jitter, y_best is not
 *    read.  A NaN incumbent (a NaN prior mean at a training point) gives cbo_acq_sweep's result for y_best = NaN.
 * The quotient by the cost is cbo_acq_sweep's: the IEEE one for every cost whose significand is not all ones; only the sign
 * of a zero can differ.  best_idx: lowest index on ties, NaN maximal, offset by the set's index_offset.  acq_out / mean_out
 * / var_out (m doubles each), best_val and best_idx may be NULL.  q, mu are reached exactly as cbo_acq_sweep reaches them
 * (the candidates' cached copies when the fit stamp matches, one appended row or block after cbo_gp_append /
 * cbo_gp_append_block, the fp32 strip of fp32 models, the chunked substitution otherwise), and the model and the set are
 * left as cbo_acq_sweep leaves them.  Out of scope: refitting in the same call (cbo_gp_fit_sweep), the batch,
 * hyper-marginalised and constrained calls, the multi-GPU exchange.  (The single launch of small sets has the kinds through
 * cbo_acq_sweep_sets_kind and cbo_trial_step_kind, below.)
 * CBO_ERR_INVALID: cbo_acq_sweep's argument checks, a kind outside 1..4, a non-finite param, beta < 0, a non-finite y_best
 * for CBO_ACQ_PI, cost <= 0 or NaN, a bad task for every kind but CBO_ACQ_VAR.  Unfitted model: CBO_ERR_NOT_FITTED.
 *
 * cbo_gp_plugin_incumbent: the incumbent CBO_ACQ_MPEI uses -- min (task 'min') or max ('max') over the n posterior means
 * at the model's own inputs, cbo_gp_predict(gp, n, X, prior closures at X, include_noise = 1)'s bits (computed as that
 * prediction, from the device copies of the data), NaN if any of them is (np.min / np.max).  NULL argument, bad task:
 * CBO_ERR_INVALID; unfitted model: CBO_ERR_NOT_FITTED.  The model is only read. */
enum { CBO_ACQ_LCB = 1, CBO_ACQ_PI = 2, CBO_ACQ_VAR = 3, CBO_ACQ_MPEI = 4 };
int cbo_acq_sweep_kind(cbo_gp *gp, cbo_cands *cands, int kind, double y_best, int task, double param, double cost,
                       double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx);
int cbo_gp_plugin_incumbent(cbo_gp *gp, int task, double *incumbent_out);

/* log Expected Improvement over a cost (Ament et al. 2023, "Unexpected improvements to expected
 * improvement"): cbo_acq_sweep_kind's argument list without kind, param being the jitter.
 *     acq = log h(u) + log s - log cost,   h(u) = phi(u) + u Phi(u),   s = sqrt(var),
 *     u = (y_best - (mean + jitter)) / s for task 'min',   u = ((mean - jitter) - y_best) / s for task 'max'
 * computed without underflow (three ranges of u; finite and correct down to u = -3e7), so that candidates whose EI is an
 * exact 0.0 in double precision -- u < -38.6: most of a grid once a model with noise 1e-10 has a few dozen observations --
 * keep a strict order and a gradient.  Wherever EI is representable the arg-max is cbo_acq_sweep's.  Task 'max' is the MIRROR
 * of 'min' (the improvement of a maximiser): it is NOT the logarithm of cbo_acq_sweep's 'max' value, which is the reference's
 * negative -EI and has none.  mean_out / var_out are cbo_acq_sweep_kind's bits; s and the quotient u are formed as
 * cbo_acq_sweep forms them; the tie rule, the outputs that may be NULL and the route to q, mu are cbo_acq_sweep_kind's.  A NaN
 * mean or variance gives NaN.  The multi-set and refinement forms are cbo_acq_sweep_sets_logei and cbo_acq_refine_sets_logei,
 * below; a one-call trial step, the constrained, hyper-marginalised, plug-in and batch forms are out of scope.  (Since built:
 * the constrained form, cbo_acq_sweep_constrained_log, and the hyper-marginalised one, cbo_acq_sweep_hyper_log.)
 * CBO_ERR_INVALID, scalars first: a bad task, a non-finite jitter or y_best, cost <= 0 or NaN; then cbo_acq_sweep's argument
 * checks.  Unfitted model: CBO_ERR_NOT_FITTED. */
int cbo_acq_sweep_logei(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double jitter, double cost,
                        double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx);

/* The Expected Improvement, or its logarithm, of every candidate over the candidate's OWN cost: what the CBO
 * papers write as EI(x) / c(x).  cands must carry a cost vector (cbo_cands_set_cost).
 *     log_form 0:  acq[j] = EI_j / cost[j]  -- cbo_acq_sweep's value at cost 1, then the IEEE quotient (numpy's `/`)
 *     log_form 1:  acq[j] = cbo_acq_sweep_logei's value at cost 1 with log(cost[j]) in the place of log cost
 * mean_out / var_out are cbo_acq_sweep's bits; the tie rule (lowest index, NaN maximal, index_offset applied), the outputs that
 * may be NULL and the route to q, mu (cached copies, a kept solution, an appended row, else the substitution) are
 * cbo_acq_sweep's.  A NaN cost gives a NaN acquisition.  The candidate pass reads the costs as a fifth 8-byte stream.
 * CBO_ERR_INVALID, scalars first: log_form other than 0 / 1, a bad task, a non-finite jitter or y_best; then cbo_acq_sweep's
 * argument checks; then a set without a cost vector.  Unfitted model: CBO_ERR_NOT_FITTED.
 * Out of scope: point-wise costs for the other acquisitions, constraints, hyper-marginalisation, batches, a one-call trial
 * step. */
int cbo_acq_sweep_pointcost(cbo_gp *gp, cbo_cands *cands, int log_form, double y_best, int task, double jitter,
                            double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx);

/* Hyper-parameter MLE support (GPy model.optimize() reached from src/CBO.py:173 and
 * src/utils_functions/utils.py:44).  cbo_gp_set_hyper replaces kernel variance, lengthscale(s) and noise
 * variance (the model must be refitted with cbo_gp_fit); cbo_gp_log_marginal returns GPy's
 * log_marginal_likelihood of the fitted model, 0.5*(-n log 2pi - logdet Ky - r^T Ky^-1 r), computed on the
 * device from the factor's diagonal and z = L^-1 r.  The optimiser loop itself is host logic. */
int cbo_gp_set_hyper(cbo_gp *gp, double variance, const double *lengthscale, double noise_var);
int cbo_gp_log_marginal(cbo_gp *gp, double *lml_out);
/* The gradients GPy hands its optimiser (ExactGaussianInference dL_dK -> kern.update_gradients_full, dL_dthetaL):
 * d log p(y) / d variance, / d lengthscale (1 value, or d values if ard), / d noise_var, of the fitted model, all on
 * the device (Ky^-1 = L^-T L^-1 through the sweep and GEMM kernels, then one contraction pass).  lml_out may be NULL.
 * An fp64 model of at most 128 observations -- every model the reference builds, and what its per-trial optimize()
 * iterates on -- need not be fitted: one launch goes from the data and the current hyper-parameters to all outputs and
 * leaves the model as it was (if Ky is not positive definite as assembled, the model is fitted with the jitchol
 * ladder and the general path answers).  Larger models: CBO_ERR_NOT_FITTED until fitted. */
int cbo_gp_lml_gradients(cbo_gp *gp, double *lml_out, double *dvariance_out, double *dlengthscale_out,
                         double *dnoise_out);
/* The same for many independent models in one call: the graph-level GPs an observe step fits
 * (src/graphs/impl/CompleteGraph.py:114-137, CoralGraph.py:186-212, SimplifiedCoralGraph.py:194-220: one
 * src/utils_functions/utils.py:40-45 fit_gaussian_process, i.e. one GPy gp.optimize(), per fit dependency), each at its
 * own optimiser iterate.  Every model cbo_gp_lml_gradients would answer in one launch (fp64, at most 128 observations)
 * is answered inside ONE launch for all of them, with the same bits; the others -- larger models (fitted beforehand, as
 * for cbo_gp_lml_gradients), and models whose Ky is not positive definite as assembled (fitted here with the jitchol
 * ladder) -- by the general path, one by one, without touching the rest.  All models live on one context.  Outputs per
 * model i: lml[i], dvar[i], dls[i * CBO_MAX_DIM + k] (k < 1, or < d if ard), dnoise[i], status[i] = CBO_OK or the
 * error cbo_gp_lml_gradients would have returned for that model alone (its outputs are then undefined).  The call
 * itself fails only on bad arguments or a device error. */
int cbo_gp_lml_gradients_batch(int n_models, cbo_gp *const *gps, double *lml, double *dvar, double *dls,
                               double *dnoise, int *status);

/* Leave-one-out cross-validation of the fitted model, all on the device (Rasmussen & Williams 5.4.2; what GPy exposes as
 * model.inference_method.LOO -- restated from memory, parity with GPy is not pinned by a recorded GPy output).  With
 * r = y - m(X), alpha = Ky^-1 r and c_i = (Ky^-1)_ii, for every observation i < n:
 *     mean_out[i] = y_i - alpha_i / c_i       the prediction of y_i from the other n - 1 observations
 *     var_out[i]  = 1 / c_i                   its predictive variance, of y_i: the noise and the 1e-8 of Ky included
 *     lpd_out[i]  = -1/2 log 2 pi + 1/2 log c_i - 1/2 alpha_i^2 / c_i      (GPy's return value and sign)
 * and *sum_lpd_out = sum_i lpd_out[i], the LOO pseudo-likelihood, summed on the device in a fixed order (two identical
 * calls return the same bits).  Each of the four outputs may be NULL, not all of them (CBO_ERR_INVALID; a NULL gp too).
 * Unfitted model: CBO_ERR_NOT_FITTED.  The model is only read: factor, z, fitted state, candidate sets with their
 * cached vectors and kept solutions stay as they are (alpha is materialised as by cbo_gp_get_posterior).  A factor that
 * carries jitchol jitter is used as it is -- the result is the LOO of the jittered Ky; cbo_gp_jitter tells.  fp32
 * models answer from the fp64 factor.  After cbo_gp_append / cbo_gp_append_block the n + k observations are covered.
 * Causal models need nothing extra: m(X) and v(X) are in z and in the factor. */
int cbo_gp_loo(cbo_gp *gp, double *mean_out, double *var_out, double *lpd_out, double *sum_lpd_out);
/* The same for many models in one call (every exploration set of a trial, with and without the causal prior).  Every
 * fp64 model of at most 128 observations need not be fitted: all of them are answered inside ONE launch, from the data
 * and the current hyper-parameters, and are left as they were -- with the same bits whatever else the batch holds.
 * Larger models must be fitted beforehand and are answered one by one as by cbo_gp_loo; a small model whose Ky is not
 * positive definite as assembled is fitted here with the jitchol ladder and answered that way too.  All models live on
 * one context.  Outputs per model i: sum_lpd[i]; lpd_cat (may be NULL) takes the per-point lpd of all models one after
 * the other in model order (n_0 + n_1 + ... doubles); status[i] = CBO_OK or the error cbo_gp_loo would have returned for
 * that model alone (its outputs are then undefined).  The call itself fails only on bad arguments (n_models <= 0, NULL
 * gps, sum_lpd or status, a NULL model, models of different contexts: CBO_ERR_INVALID) or a device error. */
int cbo_gp_loo_batch(int n_models, cbo_gp *const *gps, double *sum_lpd, double *lpd_cat, int *status);

/* Prediction gradients: emukit GPyModelWrapper.get_prediction_gradients -> GPy
 * predictive_gradients, called from CausalExpectedImprovement.evaluate_with_gradients
 * (src/utils_functions/causal_acquisition_functions.py:54) inside the L-BFGS refinement of
 * src/utils_functions/causal_optimizer.py:59-65.  dmean_out / dvar_out: m*d row-major,
 * d mean / d x and d var / d x.  For the causal kernel GPy differentiates the stationary part only, but the
 * solve Ky^-1 k*(x) behind the variance gradient uses the full kernel, hence prior_var_s = variance_adjustment(Xs)
 * (NULL for the non-causal kernel).  Any number of points: the variance gradient's Ky^-1 k*(x) is a forward and a
 * backward substitution of the whole batch, both by the sweep's strip kernel (the backward one on the factor read
 * in reversed index order, which is lower triangular again), chunked like a sweep. */
int cbo_gp_predict_gradients(cbo_gp *gp, int64_t m, const double *Xs, const double *prior_var_s,
                             double *dmean_out, double *dvar_out);

/* Do-calculus prior (src/DoCalculus.py:34-89): predict at m_groups * group points and
 * average the predictive mean and variance over each consecutive run of `group` rows -- one run per
 * candidate intervention, its rows being the observed inputs with the intervened columns overwritten
 * (DoCalculus.compute_do / get_intervened_inputs, then np.mean over the rows, :59-60).  The reduction runs
 * on the device; only m_groups values per output come back. */
int cbo_gp_predict_grouped(cbo_gp *gp, int64_t m_groups, int64_t group, const double *Xs,
                           const double *prior_mean_s, const double *prior_var_s, int include_noise,
                           double *mean_out /* m_groups */, double *var_out /* m_groups */);

/* The same reduction with the prediction points built on the device: candidate c's rows are the n_obs rows of
 * `observed` (n_obs x d, the graph-level GP's inputs) with column j replaced by values[c * n_iv + iv_index[j]] wherever
 * iv_index[j] >= 0 (DoCalculus.get_intervened_inputs, src/DoCalculus.py:80-89).  Only observed and values cross the
 * host link -- the m * n_obs points (16384 candidates x 1000 rows = 393 MB for d = 3) never exist on the host.
 * Non-causal (graph-level) models only. */
int cbo_gp_predict_do(cbo_gp *gp, int64_t m, int64_t n_obs, const double *observed, int n_iv, const double *values,
                      const int *iv_index /* d */, int include_noise, double *mean_out /* m */, double *var_out /* m */);

/* Posterior state for inspection / tests (GPy posterior.woodbury_chol, .woodbury_vector).
 * L_out: n*n row-major lower triangle (upper part zero); alpha_out: n. Either may be NULL. */
int cbo_gp_get_posterior(cbo_gp *gp, double *L_out, double *alpha_out);
/* Assembled Ky (before factorisation) of the last fit attempt is not kept; this re-assembles
 * K(X,X) + diag into K_out (n*n row-major, symmetric) for tests of the assembly kernel. */
int cbo_gp_assemble_kxx(cbo_gp *gp, double *K_out);
int64_t cbo_gp_n(const cbo_gp *gp);
int cbo_gp_dtype(const cbo_gp *gp);
/* Outcome of the jitchol ladder of the last fit: retries used (0 = none) and jitter added. */
int cbo_gp_jitter(const cbo_gp *gp, int *jitter_tries_out, double *jitter_out);

/* ---- candidate sets ---------------------------------------------------------------------------
 * A candidate-intervention grid resident in HBM (the generalisation of the 100 random anchors of
 * src/utils_functions/causal_optimizer.py:52-55).  index_offset is added to local
 * row numbers when reporting the arg-max (candidate shards of a global grid). */
int cbo_cands_create(cbo_ctx *ctx, int64_t m, int d, const double *Xs, const double *prior_mean_s,
                     const double *prior_var_s, int64_t index_offset, cbo_cands **out);
void cbo_cands_destroy(cbo_cands *c);
/* Keep V = L^-1 K* of this candidate set resident after a sweep (n_pad * m_pad doubles): when the model is then
 * extended with cbo_gp_append, the next sweep adds ONE row to V (O(n m)) instead of redoing the substitution
 * (O(n^2 m)).  Off by default. */
int cbo_cands_keep_solution(cbo_cands *c, int on);
/* Per-candidate intervention costs.  cbo_cands_set_cost gives the set a cost vector,
 *     cost[j] = c(x_j) = sum_k (fix[k] + (variable[k] ? |x_jk| : 0)),   k < d,
 * formed on the device from the set's raw points in cbo_acq_refine_sets' order (terms added from 0.0 in column order, no
 * contraction): the reference's variable-cost table, priced per candidate and not over the batch column.  fix and variable
 * hold d entries each.  The vector stays with the set (m doubles), whose points never change; cbo_cands_get_cost copies it to
 * out[0..m), cbo_cands_clear_cost drops it.  A NaN coordinate of a variable column gives a NaN cost.
 * CBO_ERR_INVALID: NULL arguments, a non-finite fixed cost, a flag other than 0 / 1, a fixed-cost sum that is not positive
 * (so c(x) > 0 everywhere); cbo_cands_get_cost on a set without a cost vector. */
int cbo_cands_set_cost(cbo_cands *c, const double *fix, const int *variable);
int cbo_cands_get_cost(const cbo_cands *c, double *out);
int cbo_cands_clear_cost(cbo_cands *c);

/* ---- acquisition sweep -------------------------------------------------------------------------
 * Replaces the batched `acquisition.evaluate(X)` of the anchor scoring step
 * (causal_optimizer.py:52-55) = CausalExpectedImprovement.evaluate
 * (causal_acquisition_functions.py:27-43) / Cost.evaluate (cost_functions.py:11-17), followed by the
 * top-1 selection.  acq = sign * s (u Phi(u) + phi(u)) / cost, u = (y_best - (mean + ei_jitter))/s;
 * task max returns -EI with the same u (reference quirk).  best_idx is the lowest index attaining
 * the maximum (NaN counts as maximal, like numpy.argmax), offset by the set's index_offset.
 * Outputs stay on the device unless asked for: acq_out / mean_out / var_out (m doubles each) may be
 * NULL. */
int cbo_acq_sweep(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double ei_jitter,
                  double cost, double *acq_out, double *mean_out, double *var_out, double *best_val,
                  int64_t *best_idx);

/* Greedy batch selection: emukit's GreedyBatchPointCalculator (the Kriging believer) over a candidate set.  Pick the
 * arg-max, add it to the model as a fake observation whose y is the model's own prediction there, pick again,
 * batch_size times in all -- without touching the model.
 *  - Pick 0 is cbo_acq_sweep(gp, cands, y_best, task, ei_jitter, cost, ...): best_vals[0] / best_idxs[0] are its bits and,
 *    with batch_size == 1, so are acq_out / mean_out / var_out.  q, mu are reached as cbo_acq_sweep reaches them (the
 *    candidates' cached copies, a kept solution whose stamp matches, one appended row, else the substitution); fp32
 *    models answer from the fp64 factor (the fp64 model's result).
 *  - Pick t >= 1, with p the local index of pick t - 1 (read on the device; one synchronisation for the whole batch):
 *        s2  = max(Kdiag_p - q_p, 1e-15) + noise_var + 1e-8      (cbo_gp_predict's clipped latent variance + what
 *        d   = sqrt(s2)                                            cbo_gp_fit puts on Ky's diagonal; Kdiag_p = variance + v(x_p))
 *        c_j = k(x_p, x_j) - sum_{i<n} V_ip V_ij - sum_{s<t} W_sp W_sj
 *        W_tj = c_j / d,   q_j <- q_j + W_tj^2,   mu_j unchanged (the believed residual is zero)
 *    with V = L^-1 K* and k in the kernel-matrix kernel's operation order (X2 explicit), then the EI / cost / arg-max pass
 *    of cbo_acq_sweep on the updated q: lowest index on ties, NaN maximal, index_offset added, task max's sign quirk.
 *  - update_incumbent = 0: y_best stays fixed (the reference's CausalExpectedImprovement, whose incumbent is a constructor
 *    argument); 1: after each pick y_best <- min(y_best, mean_p) (max for CBO_TASK_MAX) on the device -- what emukit's
 *    ExpectedImprovement sees through min(model.Y) once the believed point is in the data.
 *  - acq_out / mean_out / var_out (m doubles each, may be NULL): the state at the LAST pick.
 *  - The model (factor, z, alpha, fitted state) and the candidates (cached q, mu, kept V, stamps) are left as they were:
 *    the fantasy rows W and the working copy of q live in the context's scratch.  A cbo_acq_sweep after the call returns
 *    the bits it returned before; two identical calls return the same bits (fixed summation orders).
 *  - batch_size > 1 needs V of ALL candidates resident at once: the candidates' own buffer (cbo_cands_keep_solution) or
 *    one chunk of the workspace; CBO_ERR_UNSUPPORTED (naming CBO_HIP_WORKSPACE_MB) when the workspace holds fewer columns.
 * CBO_ERR_INVALID: cbo_acq_sweep's argument checks; batch_size outside 1..CBO_MAX_BATCH or above the candidate count; NULL
 * best_vals / best_idxs; cost <= 0 or NaN; update_incumbent other than 0 or 1.  Unfitted model: CBO_ERR_NOT_FITTED. */
#define CBO_MAX_BATCH 64
int cbo_acq_sweep_batch(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double ei_jitter, double cost,
                        int batch_size, int update_incumbent, double *best_vals, int64_t *best_idxs, double *acq_out,
                        double *mean_out, double *var_out);

/* cbo_acq_sweep_batch on the log Expected Improvement: the same believer -- pivot column, fantasy rows W,
 * the update of q, update_incumbent's moved incumbent -- with every pick scored by cbo_acq_sweep_logei's pass,
 *     acq_j = log EI_j - log cost    on the updated q (jitter: the log EI's jitter; task 'max' is LOGEI's mirror),
 * and the same arg-max.  The EI of a pick is an exact 0.0 over the whole grid wherever the incumbent lies well below the
 * model's data (every exploration set but the best one, in CBO): cbo_acq_sweep_batch then returns candidate 0 for that and
 * every later pick; the log form stays finite and ordered there.  Where the EI is representable the two calls pick the same
 * indices (ties and near-ties apart).
 *  - batch_size == 1 on an fp64 model is cbo_acq_sweep_logei(gp, cands, y_best, task, jitter, cost, ...): its bits.
 *  - acq_out / mean_out / var_out: the state at the LAST pick; best_vals[t] is acq[best_idxs[t]] of pick t's state.
 *  - An fp32 model answers from its fp64 factor.  Model and candidates are left as they were.
 * CBO_ERR_INVALID, scalars first (as cbo_acq_sweep_logei checks them): a bad task; a non-finite jitter or y_best; cost <= 0 or
 * NaN; batch_size outside 1..CBO_MAX_BATCH; update_incumbent other than 0 or 1; then cbo_acq_sweep_batch's checks of the
 * handles, batch_size above the candidate count and NULL best_vals / best_idxs.  CBO_ERR_UNSUPPORTED and CBO_ERR_NOT_FITTED
 * as cbo_acq_sweep_batch. */
int cbo_acq_sweep_batch_logei(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double jitter, double cost,
                              int batch_size, int update_incumbent, double *best_vals, int64_t *best_idxs, double *acq_out,
                              double *mean_out, double *var_out);

/* Refit (as cbo_gp_fit, jitchol ladder included) and sweep (as cbo_acq_sweep) in one call, overlapped: the
 * sweep's substitution advances panel by panel on a second stream while the factorisation's chain of short
 * kernels runs.  This is the pair of calls CBO.intervene() makes for the set it has just intervened on
 * (src/Monitor.py:160 set_data -> refit; src/CBO.py:250-257 find_next_y_point).  Same outputs as the two calls
 * in sequence, also on failure: on a non-OK return (CBO_ERR_NOT_PD once jitchol's ladder is exhausted) acq_out /
 * mean_out / var_out / best_val / best_idx are left untouched.  tries_out / jitter_out as in cbo_gp_fit (may be NULL). */
int cbo_gp_fit_sweep(cbo_gp *gp, cbo_cands *cands, double y_best, int task, double ei_jitter, double cost,
                     double *acq_out, double *mean_out, double *var_out, double *best_val,
                     int64_t *best_idx, int *tries_out, double *jitter_out);

/* Every exploration set of a trial in one call: CBO.compute_best_acquisition_values (src/CBO.py:237-260) loops
 * find_next_y_point over the S sets (S = 2 toy, 6 complete, 25 coral).  Pair i is (gps[i], cands[i]) with its own
 * incumbent y_best[i] and batch cost costs[i]; best_vals / best_idxs receive S winners.  Sets whose model has at most
 * 128 observations (every model the reference builds: 10 + <= 40 points) are factored AND swept by one launch inside
 * LDS -- no per-set launch chain, no per-set synchronisation, one copy back; such a model need not be fitted
 * (cbo_gp_upload_data suffices) and its fitted state is left alone.  Larger models, fp32 models and sets whose
 * factorisation needs jitchol's jitter take the general path (cbo_gp_fit_sweep if unfitted, else cbo_acq_sweep).
 * Same numbers as the per-set calls (same device functions, same summation orders).  All pairs on one context. */
int cbo_acq_sweep_sets(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                       double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs);

/* The schedule of cbo_gp_fit_sweep is measured, not tabulated: per shape (padded rows, padded candidates) the context
 * times the calls it is given anyway -- the plain sequence first (factorisation alone, sweep alone), then neighbouring
 * splits of the sweep between the pipeline under the factorisation and the closing launch -- and keeps the fastest
 * (cbo_api.hip, schedule_choose / schedule_report; results are the same bits whatever the schedule).  This call writes
 * what was measured and chosen, one text line per shape, into buf (NUL-terminated, truncated to cap; buf may be NULL)
 * and returns the number of shapes still exploring (0 = all settled), or a CBO_ERR_* code (negative as they are).  Every
 * line also says what the shape's last call ran ("last call ran pairs P group G", P = -1: the plain sequence).
 * No reference counterpart: the reference's loop (src/CBO.py:143-173) has no device schedule to choose. */
int cbo_schedule_report(cbo_ctx *ctx, char *buf, int64_t cap);

/* jitchol's ladder walked by the ranks of a communicator side by side (cbo_with_oop_amd/sharding.py, fit_over_ranks).
 * GPy's util.linalg.jitchol (reached from src/GaussianProcessFactory.py:57-73 through GPRegression) tries the plain
 * factorisation, then mean(diag)*1e-6 of jitter, x10 per retry, five retries at most, and keeps the FIRST level that
 * goes through.  With the posterior replicated on G ranks every rank repeats that walk (at config 4: a failed 26 ms
 * attempt, then the 31 ms one, on all eight GPUs).  Instead rank r tries ONE level: the levels below the one expected
 * to succeed get one rank each, all other ranks try the expected level; one small all-gather later every rank knows
 * the lowest level that went through -- the same answer as the sequential walk -- and the ranks that tried a failing
 * level receive the factor from the ones that hold it.
 *   cbo_gp_fit_level: one level (0 = plain, k = the k-th retry's jitter).  *status = 1: factored, the model is fitted
 *     with tries = level; 0: not positive definite at this level; -1: non-positive diagonal entries (jitchol's
 *     "not pd: non-positive diagonal elements", raised before its first retry).  level > 5: CBO_ERR_NOT_PD.
 *   cbo_comm_gather_i64: one integer from every rank, in rank order (out[world]).
 *   cbo_comm_share_factor: called by every rank with the same lists; the needers receive the factor at `level` in
 *     |owners| row slices, one from each owner (ncclSend / ncclRecv in one group), and adopt it. */
int cbo_gp_fit_level(cbo_gp *gp, int level, int *status, double *jitter_out);
/* (cbo_comm_gather_i64 and cbo_comm_share_factor are declared with the communicator, below) */

/* One whole trial of the reference's loop in one call -- what CBO.intervene() (src/CBO.py:143-173) does between two
 * observations, for callers whose models are small enough that three calls' worth of host glue would cost as much as
 * the device work: (1) the model of the set intervened on last takes its new data, as src/CBO.py:224-235
 * (update_gaussian_process_of_last_intervention) / src/Monitor.py:160 (set_data) give it: gps[refit_set] <- (n, X, y,
 * prior mean / variance at X or NULL), left unfitted; refit_set < 0 skips this; (2) cbo_acq_sweep_sets over all pairs
 * (src/CBO.py:237-260); (3) cbo_argmax_sets over the S winners (src/CBO.py:269-277) into *chosen_out.  Errors as those
 * calls; on an error the outputs are unspecified and the model may already hold the new data. */
int cbo_trial_step(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int refit_set, int64_t n,
                   const double *X, const double *y, const double *prior_mean_X, const double *prior_var_X,
                   const double *y_best, int task, double ei_jitter, const double *costs, double *best_vals,
                   int64_t *best_idxs, int *chosen_out);

/* cbo_acq_sweep_sets and cbo_trial_step for the point-wise acquisitions of cbo_acq_sweep_kind: kind is one
 * of CBO_ACQ_LCB | _PI | _VAR | _MPEI, param its parameter (beta; PI's jitter; not read; EI's jitter), y_best[i] is read by
 * CBO_ACQ_PI only (the array itself must be given).  Routing is cbo_acq_sweep_sets': fp64 models of at most 128 observations
 * are factored AND swept by one launch inside LDS (small_sets_kernel<kind>: the EI launch's sequence with the kind's
 * epilogue; for CBO_ACQ_MPEI the workgroup first runs the model's own points through its factor for the plug-in incumbent)
 * -- they need no fit, and their fitted state and caches are left alone; larger models, fp32 models and sets whose
 * factorisation needs jitchol's jitter take the general path inside the same call: cbo_gp_fit if unfitted, then
 * cbo_acq_sweep_kind.
 * Contract: for every set, best_vals[i] and best_idxs[i] are bit for bit what cbo_acq_sweep_kind(gps[i], cands[i], kind,
 * y_best[i], task, param, costs[i], ...) returns on a fitted twin of the model -- the same tie rule: lowest index wins, NaN
 * is maximal, the set's index_offset is applied.  cbo_trial_step_kind is bit for bit cbo_gp_upload_data +
 * cbo_acq_sweep_sets_kind + cbo_argmax_sets.
 * CBO_ERR_INVALID, before any model is touched: cbo_acq_sweep_sets' (cbo_trial_step's) argument checks, a kind outside 1..4,
 * a non-finite param, beta < 0, a non-finite y_best[i] for CBO_ACQ_PI, costs[i] <= 0 or NaN, a bad task for every kind but
 * CBO_ACQ_VAR.  The other epilogues of the one launch are calls of their own, below: the constrained one is
 * cbo_acq_sweep_sets_constrained, the hyper-marginalised one cbo_acq_sweep_sets_hyper, max-value entropy search
 * cbo_acq_sweep_sets_mes, greedy batch selection cbo_acq_sweep_sets_batch. */
int cbo_acq_sweep_sets_kind(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int kind, const double *y_best,
                            int task, double param, const double *costs, double *best_vals, int64_t *best_idxs);
int cbo_trial_step_kind(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int refit_set, int64_t n,
                        const double *X, const double *y, const double *prior_mean_X, const double *prior_var_X,
                        int kind, const double *y_best, int task, double param, const double *costs, double *best_vals,
                        int64_t *best_idxs, int *chosen_out);

/* cbo_acq_sweep_sets_kind for the log Expected Improvement of cbo_acq_sweep_logei: its argument list without
 * kind, param being the jitter; y_best[i] is set i's incumbent.  Routing is cbo_acq_sweep_sets_kind's (small_sets_kernel with
 * log_ei_of's epilogue; larger and fp32 models: cbo_gp_fit if unfitted, then cbo_acq_sweep_logei, inside the same call), and
 * so is the contract: per set, bit for bit, what cbo_acq_sweep_logei returns on a fitted twin; models the one launch takes are
 * left untouched.  CBO_ERR_INVALID, before any model is touched: a bad task, a non-finite jitter or y_best[i], costs[i] <= 0
 * or NaN, and cbo_acq_sweep_sets' argument checks. */
int cbo_acq_sweep_sets_logei(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                             double jitter, const double *costs, double *best_vals, int64_t *best_idxs);

/* cbo_acq_sweep_sets with every candidate priced at its own cost: cbo_acq_sweep_sets_logei's argument list
 * with log_form in front of y_best and without costs -- every cands[i] carries its cost vector.  Routing is
 * cbo_acq_sweep_sets' (one launch of small_sets_kernel for fp64 models of at most 128 observations; larger and fp32 models:
 * cbo_gp_fit if unfitted, then cbo_acq_sweep_pointcost, inside the same call); per set, bit for bit, what
 * cbo_acq_sweep_pointcost returns on a fitted twin; models the launch takes are left untouched.
 * CBO_ERR_INVALID, before any model is touched: cbo_acq_sweep_pointcost's scalar checks, cbo_acq_sweep_sets' argument checks,
 * a set without a cost vector. */
int cbo_acq_sweep_sets_pointcost(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int log_form, const double *y_best,
                                 int task, double jitter, double *best_vals, int64_t *best_idxs);

/* cbo_acq_sweep_sets for the constrained acquisition of cbo_acq_sweep_constrained: set i is an objective pair
 * (gps[i], cands[i]) and n_con[i] constraint pairs, whose five con_* entries lie set-major in arrays of sum(n_con) entries
 * (set 0's constraints, then set 1's, ...); the arrays may be NULL when every n_con[i] is 0.  Sets of one call may have
 * different n_con.
 * Routing, per set: when every one of its 1 + n_con[i] models is fp64 with at most 128 observations (and CBO_HIP_SMALL_SETS is
 * on, and the call's widest such set has at most 65535 blocks of 64 candidates), the set is factored AND swept by one launch
 * inside LDS (small_sets_con_kernel): a workgroup serves 64 candidates and walks the set's models in order, the running
 * product in a register.  Those models need no fit (cbo_gp_upload_data suffices), and nothing of them or of their candidate
 * sets is touched: not the factor, not the fitted flag, not the cached q / mu, not the kept solutions.  Every other set -- a
 * larger or fp32 model anywhere in it, or a non-positive pivot in any of its models (jitchol's ladder) -- takes the general
 * path inside the same call: cbo_gp_fit on each unfitted model, the objective first, then the constraints in order, then
 * cbo_acq_sweep_constrained.
 * Contract: for every set, best_vals[i] and best_idxs[i] are bit for bit what cbo_acq_sweep_constrained(gps[i], cands[i],
 * y_best[i], task, ei_jitter, costs[i], n_con[i], <set i's slices>, NULL, NULL, NULL, &v, &idx) returns on freshly fitted
 * twins of the models: the same tie rule (lowest index, NaN maximal, the objective set's index_offset), n_con[i] = 0 closing
 * with cbo_acq_sweep's quotient, n_con[i] >= 1 multiplying left to right and closing with one IEEE division.
 * CBO_ERR_INVALID, before any model is touched (what needs no handle is checked first): n_sets <= 0; a NULL y_best, costs,
 * n_con, best_vals or best_idxs; a bad task; costs[i] <= 0 or NaN; an n_con[i] outside 0..CBO_MAX_CONSTRAINTS; a NULL con_*
 * array while some n_con[i] > 0; a non-finite con_value or con_jitter; a sense other than CBO_CON_LE / CBO_CON_GE; then a
 * NULL handle array or handle; models of different contexts; a model without data; within a set, candidate sets whose m
 * differ, gp->d != cands->d in a pair, a causal model whose candidate set carries no prior, one candidate set used with two
 * different models.  An objective is required (cbo_acq_sweep_constrained's form without one is not offered here). */
int cbo_acq_sweep_sets_constrained(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                                   double ei_jitter, const double *costs, const int *n_con, cbo_gp *const *con_gps,
                                   cbo_cands *const *con_cands, const double *con_value, const double *con_jitter,
                                   const int *con_sense, double *best_vals, int64_t *best_idxs);

/* cbo_acq_sweep_sets_constrained in log space: the same argument list, the same routing (the one launch is
 * small_sets_con_kernel's log instantiation, the running sum in a register; the general path ends in
 * cbo_acq_sweep_constrained_log), the same untouched models.  Contract: for every set, best_vals[i] and best_idxs[i] are
 * bit for bit what cbo_acq_sweep_constrained_log returns for the set on freshly fitted twins.  Errors are the sibling's,
 * and a non-finite ei_jitter or y_best[i], refused with the other scalars before any handle is looked at. */
int cbo_acq_sweep_sets_constrained_log(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best,
                                       int task, double ei_jitter, const double *costs, const int *n_con,
                                       cbo_gp *const *con_gps, cbo_cands *const *con_cands, const double *con_value,
                                       const double *con_jitter, const int *con_sense, double *best_vals,
                                       int64_t *best_idxs);

/* cbo_acq_sweep_sets for the marginalised EI of cbo_acq_sweep_hyper: set i is (gps[i], cands[i]) with its
 * own n_samples[i] in 1..CBO_MAX_HYPER_SAMPLES rows hyper[i] of (variance, lengthscale x L_i, noise_var), cbo_acq_sweep_hyper's
 * row format (L_i = d if gps[i] is ard else 1).  Sets of one call may differ in n_samples, d, ARD and causal / plain.
 * Contract: for every set, best_vals[i] and best_idxs[i] are bit for bit what cbo_acq_sweep_hyper(gps[i], cands[i],
 * n_samples[i], hyper[i], y_best[i], task, ei_jitter, costs[i], NULL, &v, &idx) returns: the same sum in sample order, the
 * same division, the same tie rule (lowest index, NaN maximal, index_offset applied).
 * Routing is cbo_acq_sweep_sets': the fp64 models of at most 128 observations (CBO_HIP_SMALL_SETS on, the call's widest such
 * set at most 65535 blocks of 64 candidates) are answered by ONE launch whose workgroups serve (one set, 64 candidates) and
 * walk that set's samples (hyper_sets_kernel) -- two launches from 12 candidate blocks per set on when one scratch slot per
 * sample of the call fits the workspace limit (CBO_HIP_WORKSPACE_MB); CBO_HIP_HYPER_SCHEDULE=1 / =2 forces the schedule,
 * same bits either way.  Those models need no fit, nothing resident of them or of their candidate sets is read beyond raw
 * points, targets and prior closures, and nothing is written: factor, fit stamp, cached q / mu and kept solutions stay, an
 * unfitted model stays unfitted.  A larger or fp32 model, and a set one of whose samples met a non-positive pivot in the
 * launch, takes cbo_acq_sweep_hyper's general path inside the same call, which restores the model as described there,
 * without disturbing the other sets.
 * CBO_ERR_INVALID, before any model is touched (what needs no handle is checked first): n_sets <= 0; a NULL n_samples, hyper,
 * y_best, costs, best_vals or best_idxs; a bad task; an n_samples[i] out of range; a NULL hyper[i]; costs[i] <= 0 or NaN;
 * then a NULL handle array or handle; models of different contexts; a model without data; gp->d != cands->d; a causal model
 * whose candidate set carries no prior; a variance or lengthscale that is not finite and positive, a noise that is negative
 * or not finite, in any row.  There is no CBO_ERR_NOT_FITTED. */
int cbo_acq_sweep_sets_hyper(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const int *n_samples,
                             const double *const *hyper, const double *y_best, int task, double ei_jitter,
                             const double *costs, double *best_vals, int64_t *best_idxs);

/* The marginalised EI in log space, for the models whose EI is an exact 0.0 over most of a grid under every
 * sample (noise 1e-10, a few dozen observations), where cbo_acq_sweep_hyper's average is 0.0 too and orders nothing:
 *     acq_i = log((1 / H) sum_h EI_h,i) - log cost = LSE_h(l_h,i) - log H - log cost
 * l_h,i being, bit for bit, what cbo_acq_sweep_logei(gp_h, cands, y_best, task, jitter, 1.0, ...) writes to acq_out[i] on a
 * fitted twin gp_h carrying sample h's hyper-parameters; task 'max' is cbo_acq_sweep_logei's mirror, not cbo_acq_sweep_hyper's
 * -EI.  This is the LOGARITHM OF THE AVERAGE that cbo_acq_sweep_hyper forms, not the average of the logarithms (what emukit's
 * IntegratedHyperParameterAcquisition would form from a generator of log acquisitions).  The reduction is one stated sequence,
 * in sample order, one rounding per operation, the device library's exp and log:
 *     M = l_0, S = 1;   for h = 1..H-1:  l > M: S = S exp(M - l) + 1, M = l;   l == M: S = S + 1;   else S = S + exp(l - M);
 *     acq = ((M + log S) - log (double)H) - log cost
 * so that NaN propagates (and is maximal in the arg-max), -inf is an ordinary value (all samples at -inf give -inf), and H = 1
 * gives cbo_acq_sweep_logei's acq_out, best_val and best_idx bit for bit.  Error against the exact log-sum-exp of the same
 * terms: at most 4 * 2^-53 * (H + |acq|).
 * cbo_acq_sweep_hyper_log: cbo_acq_sweep_hyper's argument list (ei_jitter being the log EI's jitter), its routing -- one
 * launch for an fp64 model of at most 128 observations, which touches nothing; the general path otherwise, per sample
 * cbo_acq_sweep_logei's steps at cost 1 with the term kept on the device, restoring the model as described there -- and its
 * error returns, plus cbo_acq_sweep_logei's scalar ones (checked first): a non-finite jitter or y_best.
 * cbo_acq_sweep_sets_hyper_log: cbo_acq_sweep_sets_hyper's list, routing and two-launch rule; per set, bit for bit, what
 * cbo_acq_sweep_hyper_log returns.  Its error returns, plus a non-finite jitter or y_best[i].
 * cbo_lse_rows: the reduction alone, over terms the caller hands in -- out[i] = the sequence above over terms[0][i], ...,
 * terms[n_rows - 1][i] with the cost given, by the kernels of the general path (and, by construction, the bits of the
 * one-launch path): what the sweeps compute from their terms can be pinned without restating the device's exp and log on
 * the host.  n_rows in 1..CBO_MAX_HYPER_SAMPLES, m >= 1, cost > 0; terms is n_rows x m, row-major, host memory; out m doubles.
 * Out of scope: constraints, batches, the plug-in EI, MES and per-candidate costs under marginalisation, refinement, a
 * one-call trial step, several ranks. */
int cbo_acq_sweep_hyper_log(cbo_gp *gp, cbo_cands *cands, int n_samples,
                            const double *hyper /* n_samples rows of (variance, lengthscale x L, noise_var) */,
                            double y_best, int task, double jitter, double cost, double *acq_out /* m, may be NULL */,
                            double *best_val, int64_t *best_idx);
int cbo_acq_sweep_sets_hyper_log(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const int *n_samples,
                                 const double *const *hyper, const double *y_best, int task, double jitter,
                                 const double *costs, double *best_vals, int64_t *best_idxs);
int cbo_lse_rows(cbo_ctx *ctx, int n_rows, int64_t m, const double *terms /* n_rows x m, host */, double cost,
                 double *out /* m */);

/* Max-value entropy search for every exploration set of a trial, in two calls with the host's draw of the
 * Gumbel samples between them (mins = log(-log(1 - u)) * b + a, u from the caller's generator).
 *
 * cbo_acq_sweep_sets_mes, the scoring half: set i is (gps[i], cands[i]) scored against its own n_samples[i] (1..64) Gumbel
 * samples mins[i] over costs[i].  Sets of one call may differ in n_samples, d, ARD and causal / plain.
 * Contract: for every set, best_vals[i] and best_idxs[i] are bit for bit what cbo_acq_sweep_mes(gps[i], cands[i],
 * n_samples[i], mins[i], costs[i], NULL, NULL, NULL, &v, &idx) returns on a fitted twin of the model: the same sum over the
 * samples in numpy's order, the same tie rule (lowest index, NaN maximal, index_offset applied).
 * Routing is cbo_acq_sweep_sets': fp64 models of at most 128 observations (CBO_HIP_SMALL_SETS on) are factored AND swept by
 * one launch inside LDS (small_sets_kernel with cbo_acq_sweep_mes' epilogue; the sets' samples travel in one pinned table
 * with an offset and a count per set) -- two launches from 12 candidate blocks per set on; they need no fit, and their
 * fitted state and caches are left alone.  Larger models, fp32 models and sets whose factorisation needs jitchol's jitter
 * take the general path inside the same call: cbo_gp_fit if unfitted, then cbo_acq_sweep_mes.
 * CBO_ERR_INVALID, before any model is touched: n_sets <= 0; a NULL n_samples, mins, costs, best_vals or best_idxs; an
 * n_samples[i] outside 1..64; a NULL or non-finite mins[i]; costs[i] <= 0 or NaN; then cbo_acq_sweep_sets' checks of the
 * handles (NULL, contexts, a model without data, dimensions, a causal model whose candidates carry no prior).
 *
 * cbo_gp_mes_gumbel_sets, the Gumbel fit of every set in one call: grids[i] is a candidate set over set i's Gumbel grid
 * (emukit stacks model.X on top of its uniform grid; the caller does; for a causal model the set carries the prior closures
 * at the grid).  quantiles (n_sets x 3), a and b (n_sets each): for every set bit for bit what cbo_gp_mes_gumbel returns
 * on a fitted twin for the same points.
 * Two launches for all sets and one synchronisation: (1) the grids of the fp64 models of at most 128 observations are
 * predicted, noise included, by the one-workgroup sweep's stages (small_sets_kernel storing mean and variance in the place of
 * an acquisition; its factor-once first launch from 12 blocks per set on belongs to this step) into one device workspace of
 * 2 sum(m_i) doubles -- those models need no fit and are only read; every other model is fitted if need be and predicted by
 * the general path into the same workspace; (2) the bisections of all sets, three workgroups per set.  A small model that
 * met a non-positive pivot is fitted (jitchol's ladder) and answered as cbo_gp_mes_gumbel answers, inside the same call.
 * A set fails as the single call does (a bracket without a sign change, a bisection that does not converge): CBO_ERR_INVALID,
 * the single call's message behind "set <i>: " for the first such set; the outputs are then unspecified.
 * CBO_ERR_INVALID, before any model is touched: n_sets outside 1..65535, NULL arguments or handles, models of different
 * contexts, a model without data, an empty grid, gp->d != grid->d, a causal model whose grid carries no prior.
 * CBO_ERR_UNSUPPORTED (naming CBO_HIP_WORKSPACE_MB): the mean / variance workspace exceeds the workspace limit. */
int cbo_acq_sweep_sets_mes(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const int *n_samples,
                           const double *const *mins, const double *costs, double *best_vals, int64_t *best_idxs);
int cbo_gp_mes_gumbel_sets(int n_sets, cbo_gp *const *gps, cbo_cands *const *grids, double *quantiles, double *a, double *b);

/* cbo_acq_sweep_sets for greedy batch selection: batch_size Kriging-believer picks (cbo_acq_sweep_batch,
 * §4g) for every exploration set of a trial.  best_vals and best_idxs hold n_sets x batch_size entries, set-major: pick t of
 * set i is at [i * batch_size + t].
 * Contract: for every set i the batch_size (value, index) pairs are bit for bit those of cbo_acq_sweep_batch(gps[i],
 * cands[i], y_best[i], task, ei_jitter, costs[i], batch_size, update_incumbent, ...) on a fitted twin of the model: its
 * formulas, clip, tie rule (lowest index, NaN maximal, index_offset applied), 'max'-task sign and update_incumbent
 * semantics; a pick may repeat a point.  Pick 0 is cbo_acq_sweep_sets' result; batch_size == 1 IS cbo_acq_sweep_sets.
 * Routing is cbo_acq_sweep_sets' plus one cap: an fp64 model of at most 128 observations (CBO_HIP_SMALL_SETS on) whose set
 * has at most 1024 candidates is answered by ONE launch (small_sets_batch_kernel; two from 12 candidate blocks per set on):
 * the workgroups of a set leave V = L^-1 K*, q and mu in global scratch and the last of them to arrive runs the further
 * picks.  Those models need no fit, and nothing of them or of their candidate sets is touched: fitted flag, factor, cached
 * q / mu, kept V and stamps stay; an unfitted model is still unfitted afterwards.  Every other set -- a larger or fp32 model,
 * more than 1024 candidates, a non-positive pivot in the launch -- takes cbo_gp_fit if unfitted, then cbo_acq_sweep_batch,
 * inside the same call.
 * CBO_ERR_INVALID, before any model is touched (what needs no handle is checked first): n_sets <= 0; a NULL y_best, costs,
 * best_vals or best_idxs; a bad task; batch_size outside 1..CBO_MAX_BATCH; update_incumbent other than 0 / 1; costs[i] <= 0
 * or NaN; a non-finite y_best[i]; then cbo_acq_sweep_sets' checks of the handles and batch_size above a set's number of
 * candidates. */
int cbo_acq_sweep_sets_batch(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                             double ei_jitter, const double *costs, int batch_size, int update_incumbent,
                             double *best_vals, int64_t *best_idxs);

/* cbo_acq_sweep_sets_batch on the log Expected Improvement.  Contract: for every set i the batch_size
 * (value, index) pairs are bit for bit those of cbo_acq_sweep_batch_logei(gps[i], cands[i], y_best[i], task, jitter, costs[i],
 * batch_size, update_incumbent, ...) on a fitted twin.  Routing, scratch, the untouched models and the general path inside
 * the call are cbo_acq_sweep_sets_batch's (the launch is small_sets_batch_kernel's log instantiation; the general path is
 * cbo_gp_fit if unfitted, then cbo_acq_sweep_batch_logei); batch_size == 1 IS cbo_acq_sweep_sets_logei.
 * CBO_ERR_INVALID: cbo_acq_sweep_sets_batch's checks, and a non-finite jitter. */
int cbo_acq_sweep_sets_batch_logei(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                                   double jitter, const double *costs, int batch_size, int update_incumbent,
                                   double *best_vals, int64_t *best_idxs);

/* The second stage of the reference's optimiser for every exploration set of a trial: from each of set
 * i's k starts a box-constrained L-BFGS ascent of acquisition / cost -- lockstep_lbfgs of utils_functions/causal_optimizer.py,
 * restated in csrc/refine_search.h -- and every search of every set advances inside ONE launch (small_sets_refine_kernel):
 * the set's model is factored in LDS once per workgroup and stays there for all rounds.
 * kind: 0 = the causal Expected Improvement (y_best[i] the incumbent, param the jitter), or CBO_ACQ_LCB | _PI | _VAR | _MPEI
 * with param as for cbo_acq_sweep_sets_kind.  The cost of a point is c(x) = (fix_0 + variable_0 |x_0|) + (fix_1 + ...) + ...
 * accumulated from 0 in that order; value = acquisition / c(x), gradient = d acquisition / c(x) (the reference's zero cost
 * gradient).  The value reported at a point is, bit for bit, what cbo_acq_sweep_sets (_kind) returns for a one-point grid
 * at that point with costs[i] = c(x).
 * Outputs, concatenated in set order: x_out and grad_out sum(k) rows, row-major with each set's own d; val_out, rounds_out
 * and status_out sum(k) entries.  status_out: why the search ended (CBO_REFINE_*).  max_rounds = 0 evaluates value and
 * gradient at the starts (clipped to the box) and returns them.
 * A set whose model has a prior (a causal model), more than 128 observations, or fp32 data, or whose factorisation meets a
 * non-positive pivot in the launch, is DECLINED: status_out = CBO_REFINE_DECLINED for all its starts, its other output
 * rows are not written.  Models are only read: fitted state, caches and kept solutions stay as they were; no fit needed.
 * CBO_ERR_INVALID before any launch: n_sets <= 0, NULL arguments, k outside 1..CBO_REFINE_MAX_STARTS, lo > hi, non-finite
 * bounds or starts, a fixed-cost sum that is not positive, a variable flag other than 0 / 1, an unknown kind (and
 * cbo_acq_sweep_sets_kind's checks of param and y_best), a bad task, max_rounds outside 0..CBO_REFINE_ROUNDS_LIMIT (emukit's maxfun). */
#define CBO_REFINE_MAX_STARTS 64
#define CBO_REFINE_ROUNDS_LIMIT 1000
enum { CBO_REFINE_PGTOL = 0, CBO_REFINE_FTOL = 1, CBO_REFINE_STEP = 2, CBO_REFINE_MAX_ROUNDS = 3,
       CBO_REFINE_NAN_START = 4, CBO_REFINE_DECLINED = 5 };
typedef struct cbo_refine_set {
    int k; const double *starts;                        /* k x d, row-major */
    const double *lo, *hi;                              /* d */
    const double *cost_fix; const int *cost_variable;   /* d */
} cbo_refine_set;
int cbo_acq_refine_sets(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, int kind, const double *y_best,
                        int task, double param, int max_rounds, double *x_out, double *val_out, double *grad_out,
                        int *rounds_out, int *status_out);
/* cbo_acq_refine_sets for the log Expected Improvement: its argument list without kind, param being the
 * jitter.  value = log EI(x) - log c(x) and gradient = d log EI(x) -- NOT divided by the cost: the logarithm of a quotient with
 * the reference's zero cost gradient.  The value reported at a point is, bit for bit, what cbo_acq_sweep_sets_logei returns
 * for a one-point grid there with costs[i] = c(x).  A start where the EI and its gradient are exact zeros (kind 0 ends there
 * with CBO_REFINE_PGTOL after 0 rounds) has a finite value and a gradient here.  A causal set is DECLINED, as it is by
 * cbo_acq_refine_sets (the causal instantiation of this kind is out of scope), as are larger and fp32 models.
 * CBO_ERR_INVALID: cbo_acq_refine_sets' checks, a non-finite jitter or y_best[i]. */
int cbo_acq_refine_sets_logei(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, const double *y_best, int task,
                              double jitter, int max_rounds, double *x_out, double *val_out, double *grad_out,
                              int *rounds_out, int *status_out);

/* cbo_acq_refine_sets / _logei with the TRUE gradient of the quotient: the values are theirs -- at a point,
 * bit for bit, what cbo_acq_sweep_sets_pointcost returns for a one-point grid there -- and the gradient carries the cost's
 * own derivative, d c / d x_k = variable[k] sign(x_k) with sign(0) = 0:
 *     log_form 0:  (d EI_k - (EI / c) d c_k) / c          log_form 1:  d logEI_k - d c_k / c
 * so the search climbs the function the point-cost sweeps score.  cbo_refine_set is used as it is.  Causal sets, larger and
 * fp32 models are DECLINED.  CBO_ERR_INVALID: cbo_acq_sweep_pointcost's scalar checks, then cbo_acq_refine_sets' checks. */
int cbo_acq_refine_sets_pointcost(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, int log_form,
                                  const double *y_best, int task, double jitter, int max_rounds, double *x_out,
                                  double *val_out, double *grad_out, int *rounds_out, int *status_out);

/* The second stage under constraints: cbo_acq_refine_sets for
 *     log_form 0:  EI(x) prod_k PoF_k(x) / c(x)                 log_form 1:  log EI(x) + sum_k log PoF_k(x) - log c(x)
 * -- the functions cbo_acq_sweep_sets_constrained / _constrained_log score.  Set i has n_con[i] (0..CBO_MAX_CONSTRAINTS)
 * constraints; con_gps, con_value, con_jitter and con_sense are set-major with sum(n_con) entries, as in
 * cbo_acq_sweep_sets_constrained, and may be NULL when every n_con[i] is 0.  Output layout and status codes are
 * cbo_acq_refine_sets'.  The value reported at a point is, bit for bit, what the constrained multi-set sweep of the same form
 * returns for a one-point grid there with costs[i] = c(x).  The gradient is the host classes' (AcquisitionProduct,
 * ConstrainedLogExpectedImprovement): the product rule left to right, then over c(x) -- the reference's zero cost gradient --
 * or d logEI + sum_k rho(u_k) d u_k, rho = pdf / cdf formed without underflow, not divided by the cost.
 * Routing: the sets with n_con[i] = 0 take cbo_acq_refine_sets' (kind 0) or cbo_acq_refine_sets_logei's launch and return
 * their bits; the sets with constraints go to one launch of their own on the same stream: every model of the set factored
 * once, reloaded every round.  A set is DECLINED when one of its models is causal, has more than 128 observations or is fp32,
 * or meets a non-positive pivot as assembled.  The models are only read: fit state, caches and kept solutions stay.
 * CBO_ERR_INVALID, before any launch: cbo_acq_refine_sets' checks; log_form other than 0 / 1; a non-finite ei_jitter or
 * y_best[i]; n_con[i] outside 0..CBO_MAX_CONSTRAINTS; a NULL con_* array with some n_con[i] > 0; a NULL constraint handle; a
 * constraint model without data, on another context, or whose d differs from the set's; a non-finite con_value /
 * con_jitter; a sense that is neither CBO_CON_LE nor CBO_CON_GE. */
int cbo_acq_refine_sets_constrained(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, int log_form,
                                    const double *y_best, int task, double ei_jitter, const int *n_con,
                                    cbo_gp *const *con_gps, const double *con_value, const double *con_jitter,
                                    const int *con_sense, int max_rounds, double *x_out, double *val_out,
                                    double *grad_out, int *rounds_out, int *status_out);

/* The do-calculus prior of an RBF graph GP as a device-resident handle (src/DoCalculus.py:34-89).  With the
 * graph GP's inputs X_g, the observed rows O (n_obs x d_in) and the intervened columns I,
 *     a_i(x) = exp(-1/2 sum_{c in I} ((x_c - X_g[i,c]) / l_c)^2),      b_ri = the same over c not in I at O_rc,
 *     m(x) = sum_i w_i a_i(x),  w_i = sigma^2 alpha_i mean_r b_ri;      v(x) = (sigma^2 + sigma_n^2) - a(x)^T M a(x),
 *     M = sigma^4 (Ky^-1 o b^T b / n_obs)
 * are cbo_gp_predict_do's row means (noise included) at O(n_g^2) per point instead of O(n_obs n_g^2).
 * cbo_do_prior_create snapshots w, M, the intervened columns of X_g (scaled as the kernels scale points), their lengthscales
 * and sigma^2 + sigma_n^2 from the fitted model: the handle owns its device memory and does not refer to the model
 * afterwards -- rebuild it when the graph GP changes.  intervened_index: cbo_gp_predict_do's iv_index (d_in entries, -1 = not
 * intervened, else the column of `values`).  The model is only read (its alpha is materialised as a prediction would).
 * Every element of w and M is one fixed-order sum: two creations give the same bits.
 * CBO_ERR_UNSUPPORTED, the reason in cbo_last_error(): an fp32 graph GP; a causal graph GP (it has a prior of its own); more
 * than CBO_DO_PRIOR_MAX_N rows; a graph GP that needed jitchol's jitter; a model whose latent variance the factored form cannot
 * keep above GPy's 1e-15 clip with margin -- sn / (n_g sigma^2 + sn) < 2^-26 with sn = sigma_n^2 + 1e-8 (the factored form has
 * no per-row clip; the bound is the least latent variance over sigma^2, kept above sqrt(eps)).
 * CBO_ERR_INVALID: NULL arguments, n_obs <= 0, n_iv outside 1..CBO_MAX_DIM, an index >= n_iv, no intervened column;
 * CBO_ERR_NOT_FITTED: the model is not fitted.
 * cbo_do_prior_eval: m(x) and v(x) at the m rows of `values` (m x n_iv); what it returns at a point is, bit for bit, what
 * cbo_acq_refine_sets_prior uses there (one device function, the same lane group). */
#define CBO_DO_PRIOR_MAX_N 1024
typedef struct cbo_do_prior cbo_do_prior;
int cbo_do_prior_create(cbo_gp *graph_gp, int64_t n_obs, const double *observed /* n_obs x d_in */, int n_iv,
                        const int *intervened_index /* d_in */, cbo_do_prior **out);
void cbo_do_prior_destroy(cbo_do_prior *prior);
int cbo_do_prior_eval(const cbo_do_prior *prior, int64_t m, const double *values /* m x n_iv */, double *mean_out /* m */,
                      double *var_out /* m */);

/* cbo_acq_refine_sets with causal sets inside the launch: priors[i] is NULL or the do-calculus prior of set
 * i's causal model (priors itself may be NULL: cbo_acq_refine_sets, which is this call with every prior NULL).  Every round
 * the workgroup evaluates (m, v) at the trial point of each of its running starts (do_prior_at); column 0 is the causal k*
 * with sqrt(v), the derivative columns are the stationary part's (GPy's predictive_gradients differentiates nothing else)
 * and the posterior takes (m, v).  The value at a point is, bit for bit, cbo_acq_sweep_sets (_kind) on a one-point grid there
 * whose prior arrays are cbo_do_prior_eval's.  A causal model with a NULL prior is DECLINED as before.  Sets with and without
 * a prior go to two launches on the call's stream.
 * CBO_ERR_INVALID before any launch, beside cbo_acq_refine_sets': a prior given for a model without one of its own; a prior
 * whose n_iv differs from the model's d; a prior of another context. */
int cbo_acq_refine_sets_prior(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, const cbo_do_prior *const *priors,
                              int kind, const double *y_best, int task, double param, int max_rounds, double *x_out,
                              double *val_out, double *grad_out, int *rounds_out, int *status_out);

/* Hyper-parameter posterior samples of every model by HMC in ONE launch: GPy's inference.mcmc.HMC with the
 * unit mass matrix over the Logexp-transformed parameters -- integrated_hyper.hmc_sample, restated in csrc/hmc_chain.h -- one
 * chain per model, every chain inside hmc_sets_kernel: a workgroup factors its model at each position of its chain from
 * the raw coordinates and evaluates the log marginal likelihood and its gradients there, with cbo_gp_lml_gradients'
 * arithmetic.  The random numbers are the caller's: per sample one momentum (n_params standard normals) and one uniform.
 * Per model: theta0 (n_params positive values: variance, the lengthscale(s), and the noise variance when sample_noise = 1; a
 * model whose noise is fixed has sample_noise = 0 and keeps its own), num_samples, hmc_iters leapfrog steps of stepsize.
 * Outputs per model: rows_out (num_samples x n_params, theta at each sample's start, overwritten by the proposal when it
 * is accepted), accept_out (num_samples flags), and the chain's last state: final_theta, final_lml, final_grad (n_params;
 * d lml / d theta) -- the likelihood and gradients cbo_gp_lml_gradients returns for the model at final_theta, bit for bit.
 * status_out[i]: CBO_HMC_OK; CBO_HMC_NOT_PD -- a position's Ky was not positive definite as assembled (the launch cannot
 * walk jitchol's ladder): the chain stopped, its outputs mean nothing, the caller repeats it on the host with the same draws;
 * CBO_HMC_DECLINED -- the model is not one the launch takes (more than 128 observations, fp32 data, CBO_HIP_SMALL_SETS=0):
 * nothing else is written for it.  Models are only read: hyper-parameters, fitted state, caches and kept solutions stay as
 * they were; no fit needed.
 * CBO_ERR_INVALID before any device work: n_models <= 0, NULL arguments or handles, models of different contexts,
 * num_samples outside 1..CBO_HMC_MAX_SAMPLES, hmc_iters < 0, num_samples * hmc_iters above CBO_HMC_MAX_EVALS, a stepsize or
 * theta0 that is not finite and positive, sample_noise other than 0 / 1, n_params other than 1 + (ARD ? d : 1) +
 * sample_noise, non-finite draws.
 * CBO_HMC_MAX_SAMPLES: 4096 samples of 10 parameters are 320 KiB of draws and as much of rows per model, in pinned memory --
 * twenty times emukit's default chain (100 burn-in + 10 x 10).  CBO_HMC_MAX_EVALS: one launch evaluates the likelihood
 * 1 + num_samples * hmc_iters times per model, one after the other, at tens of microseconds each: 2^18 keeps the longest
 * launch to some seconds (emukit's default chain has 4000). */
#define CBO_HMC_MAX_PARAMS (CBO_MAX_DIM + 2)
#define CBO_HMC_MAX_SAMPLES 4096
#define CBO_HMC_MAX_EVALS 262144
enum { CBO_HMC_OK = 0, CBO_HMC_NOT_PD = 1, CBO_HMC_DECLINED = 2 };
typedef struct cbo_hmc_chain {
    int n_params, sample_noise, num_samples, hmc_iters;
    double stepsize;
    const double *theta0;                               /* n_params */
    const double *momenta, *uniforms;                   /* num_samples x n_params, num_samples */
    double *rows_out; int *accept_out;                  /* num_samples x n_params, num_samples */
    double *final_theta, *final_lml, *final_grad;       /* n_params, 1, n_params */
} cbo_hmc_chain;
int cbo_gp_hmc_sets(int n_models, cbo_gp *const *gps, const cbo_hmc_chain *chains, int *status_out);

/* Hyper-parameter MLE of every model by L-BFGS in ONE launch: causal_optimizer.lockstep_lbfgs without a box
 * over the Logexp-transformed parameters -- restated in csrc/mle_search.h -- one search per RUN, a run being one (model,
 * start) pair, every run inside mle_sets_kernel: a workgroup factors its model at each trial point of its search from the
 * raw coordinates and evaluates the log marginal likelihood and its gradients there, with cbo_gp_lml_gradients' arithmetic.
 * The iteration is lockstep_lbfgs', not scipy's L-BFGS-B (setulb): same stationary points, another path to them.
 * Per model: n_starts rows of theta0 (n_params positive values each: variance, the lengthscale(s), and the noise variance
 * when fit_noise = 1; a model whose noise is fixed has fit_noise = 0 and keeps its own), at most max_rounds rounds per run
 * (max_rounds = 0 evaluates the starts and moves nothing).  Outputs per run s of the model: status_out[s] -- why the search
 * ended, CBO_REFINE_PGTOL / FTOL / STEP / MAX_ROUNDS / NAN_START, or CBO_MLE_NOT_PD: the START's Ky was not positive definite
 * as assembled (the launch cannot walk jitchol's ladder), nothing else of the run means anything and the caller repeats the
 * model on the host; a TRIAL point of that kind counts as a failed step, as a non-finite value does --, rounds_out[s],
 * theta_out (row s: the end point), lml_out[s] and grad_out (row s: d lml / d theta) there -- the likelihood and gradients
 * cbo_gp_lml_gradients returns for the model at that theta, bit for bit.  The call does not choose among a model's runs.
 * model_status_out[i]: CBO_OK, or CBO_MLE_DECLINED -- the model is not one the launch takes (more than 128 observations,
 * fp32 data, CBO_HIP_SMALL_SETS=0): nothing else is written for it.  Models are only read: hyper-parameters, fitted state,
 * caches and kept solutions stay as they were; no fit needed.
 * CBO_ERR_INVALID before any device work: n_models <= 0, NULL arguments, handles or per-model pointers, models of different
 * contexts, fit_noise other than 0 / 1, n_params other than 1 + (ARD ? d : 1) + fit_noise, n_starts outside
 * 1..CBO_MLE_MAX_STARTS, max_rounds outside 0..CBO_MLE_MAX_ROUNDS, a theta0 entry that is not finite and positive, more than
 * 65535 runs in all. */
#define CBO_MLE_MAX_STARTS 16
#define CBO_MLE_MAX_ROUNDS 4096
#define CBO_MLE_DECLINED CBO_REFINE_DECLINED
#define CBO_MLE_NOT_PD 6
typedef struct cbo_mle_run {            /* one model: n_starts runs */
    int n_params, fit_noise, n_starts, max_rounds;
    const double *theta0;               /* n_starts x n_params, row 0 = the model's own start */
    double *theta_out, *lml_out, *grad_out;   /* n_starts x n_params, n_starts, n_starts x n_params */
    int *status_out, *rounds_out;       /* n_starts */
} cbo_mle_run;
int cbo_gp_mle_sets(int n_models, cbo_gp *const *gps, const cbo_mle_run *runs, int *model_status_out);
/* The same call with the band of models the launch takes chosen by the caller: max_rows = 128 IS
 * cbo_gp_mle_sets.  max_rows = 256: the models of at most 128 observations go into the mle_sets_kernel launch exactly as
 * above, with the same bits; the fp64 models of 129..256 observations (CBO_HIP_SMALL_SETS not 0) go into one mle_mid_kernel
 * launch on the same stream -- the same search around the two-block likelihood, one workgroup per run with about 1 MB of
 * scratch -- and one synchronisation waits for both; everything else is CBO_MLE_DECLINED.  For such a run lml_out and
 * grad_out are, bit for bit, what cbo_gp_lml_gradients_batch answers for the model at theta_out (cbo_gp_lml_gradients
 * alone refits a model of that size and takes the general path: the same values to rounding).
 * CBO_ERR_INVALID before any device work, beside the cases above: max_rows other than 128 or 256; more than 256 runs of
 * models of 129..256 observations in one call (one workgroup per compute unit, about 256 MB of scratch). */
int cbo_gp_mle_sets_rows(int n_models, cbo_gp *const *gps, const cbo_mle_run *runs, int max_rows, int *model_status_out);

/* Priors on the hyper-parameters: GPy's set_prior with priors.Gaussian / LogGaussian / Gamma /
 * InverseGamma, restated in csrc/hyper_prior.h (from memory, parity with GPy unpinned).  Priors are state of the model
 * handle: cbo_gp_set_data / _upload_data / _append / _append_block / _set_hyper and every fit keep them.  One descriptor per
 * parameter in the row order of cbo_gp_hmc_sets and cbo_gp_mle_sets: variance, the lengthscale(s) (ARD ? d : 1), the noise
 * variance; n_params = 2 + (ARD ? d : 1), the noise slot always present.  kind CBO_PRIOR_NONE: the parameter has no prior.
 * (p0, p1) = (mu, sigma) for GAUSSIAN and LOGGAUSSIAN, (a, b) for GAMMA and INVGAMMA (b the rate, resp. the scale);
 * `constant` is the density's constant, computed by the caller: -log(2 pi sigma^2) / 2, resp. a log(b) - lgamma(a) (the
 * device never calls lgamma).  The log prior is the sum of the densities at theta plus, for every parameter that has a
 * prior, the log-Jacobian of its Logexp constraint, log(expm1(theta)) - theta (0 above 36), as GPy's log_prior() adds it.
 * cbo_gp_set_priors: priors == NULL, or every kind NONE, clears the priors.  CBO_ERR_INVALID, before any device work and
 * with the reason in cbo_last_error(): a NULL handle, n_params other than 2 + (ARD ? d : 1), an unknown kind, a parameter
 * or constant that is not finite, sigma <= 0, a <= 0 or b <= 0.  cbo_gp_get_priors writes the n_params descriptors (all
 * NONE for a model without priors).
 * With priors set, cbo_gp_hmc_sets and cbo_gp_mle_sets sample and maximise the log POSTERIOR: at every position / trial
 * point the log prior and its gradient (hyper_prior_at over the run's n_params entries -- a prior on the noise variance
 * takes part only when the noise is sampled / fitted) are added to the likelihood and its gradients, one IEEE addition each,
 * before the chain / search sees them; final_lml, final_grad, lml_out and grad_out then hold the log posterior and its
 * gradient with respect to theta (the negated objective, GPy's -f_opt): fl(lml + lp), fl(dl[k] + dlp[k]) with lml, dl what
 * cbo_gp_lml_gradients and lp, dlp what cbo_gp_log_prior_batch answer there, bit for bit.  A model without priors skips the
 * stage (no + 0.0) and gives the bits it gave before priors existed; a call in which no model has priors launches the
 * kernel without the stage. */
enum { CBO_PRIOR_NONE = 0, CBO_PRIOR_GAUSSIAN = 1, CBO_PRIOR_LOGGAUSSIAN = 2, CBO_PRIOR_GAMMA = 3, CBO_PRIOR_INVGAMMA = 4 };
typedef struct cbo_hyper_prior {
    int kind, pad_;
    double p0, p1, constant;
} cbo_hyper_prior;
int cbo_gp_set_priors(cbo_gp *gp, int n_params, const cbo_hyper_prior *priors);
int cbo_gp_get_priors(const cbo_gp *gp, int n_params, cbo_hyper_prior *priors_out);
/* The log prior and its gradient with respect to theta of many models in ONE tiny launch, one lane per model, by
 * hyper_prior_at ON THE DEVICE (its log / expm1 are the ones the searches use, so what they add can be checked bit for
 * bit).  thetas[i]: 2 + (ARD ? d : 1) values (variance, lengthscale(s), noise variance), or NULL -- the model's own
 * parameters; thetas == NULL: every model's own.  lp_out: n_models; grad_out: n_models x CBO_HMC_MAX_PARAMS, zeros behind
 * the model's entries; status[i] = CBO_OK.  A model without priors answers 0 and zeros.  The models are only read.
 * CBO_ERR_INVALID: n_models <= 0, NULL arguments or handles, models of different contexts, a theta that is not finite. */
int cbo_gp_log_prior_batch(int n_models, cbo_gp *const *gps, const double *const *thetas, double *lp_out, double *grad_out,
                           int *status);

/* Host-buffer convenience form of the same call (uploads Xs first). */
int cbo_acq_sweep_host(cbo_gp *gp, int64_t m, const double *Xs, const double *prior_mean_s,
                       const double *prior_var_s, double y_best, int task, double ei_jitter,
                       double cost, double *acq_out, double *best_val, int64_t *best_idx);

/* src/CBO.py:269-277 select_next_intervention: first index of the maximum over exploration sets.
 * Host-side (S <= 25). */
int cbo_argmax_sets(const double *ys, int s, int *idx_out);

/* Reduce (best_val, best_idx) pairs gathered from all candidate shards (one per GPU) to the global
 * winner with the same tie rule; pure host arithmetic on 16 B per rank (cbo_comm_argmax gathers and calls it). */
int cbo_argmax_pairs(const double *vals, const int64_t *idxs, int n, double *best_val,
                     int64_t *best_idx);

/* ---- arg-max exchange across GPUs ------------------------------------------------------
 * The candidate grid shards over the GPUs of a node (contiguous blocks, index_offset of cbo_cands_create), the
 * posterior is replicated, and the one exchange step is 16 bytes per rank: (best acquisition value, best GLOBAL
 * candidate index), all-gathered over RCCL (xGMI) and reduced identically on every rank with the tie rule of
 * cbo_argmax_pairs -- RCCL has no MAXLOC.  The reference is a single process (src/CBO.py:269-277 picks over sets);
 * this is the cross-GPU counterpart of that pick.  librccl.so.1 is dlopen'ed on first use (CBO_HIP_RCCL_LIB
 * overrides the name); no PyTorch involved.  Every RCCL failure returns CBO_ERR_COMM with RCCL's message.
 *
 * One process per GPU: rank 0 calls cbo_comm_unique_id (128 bytes), the launcher's side channel (a file, MPI_Bcast,
 * a TCP store) hands the bytes to the other ranks, every rank calls cbo_comm_init_rank on its own context.
 * One process driving G devices: cbo_comm_init_all fills out[0..n) (rank i on ctxs[i]); use cbo_comm_argmax_all,
 * which issues the G collectives as one group. */
typedef struct cbo_comm cbo_comm;
#define CBO_COMM_ID_BYTES 128
int cbo_comm_unique_id(void *id_out /* CBO_COMM_ID_BYTES */);
int cbo_comm_init_rank(cbo_ctx *ctx, int world, int rank, const void *id /* CBO_COMM_ID_BYTES */, cbo_comm **out);
int cbo_comm_init_all(int n, cbo_ctx *const *ctxs, cbo_comm **out /* n handles */);
void cbo_comm_destroy(cbo_comm *comm);
int cbo_comm_size(const cbo_comm *comm, int *world_out, int *rank_out);
/* This rank's (val, global idx) in, the global winner out (identical on every rank).  A rank whose shard is empty
 * passes idx = INT64_MAX.  Blocking (the exchange runs on the communicator's own stream). */
int cbo_comm_argmax(cbo_comm *comm, double val, int64_t idx, double *best_val, int64_t *best_idx);
int cbo_comm_argmax_all(int n, cbo_comm *const *comms, const double *vals, const int64_t *idxs, double *best_val,
                        int64_t *best_idx);
/* max over the ranks of one double (the slowest rank's time of a benchmark); doubles as a barrier */
int cbo_comm_max_f64(cbo_comm *comm, double value, double *max_out);
int cbo_comm_barrier(cbo_comm *comm);
/* the ladder walked side by side: see cbo_gp_fit_level above */
int cbo_comm_gather_i64(cbo_comm *comm, int64_t value, int64_t *out);
int cbo_comm_share_factor(cbo_comm *comm, cbo_gp *gp, int level, const int *owners, int n_owners,
                          const int *needers, int n_needers);
/* The needer's side of cbo_comm_share_factor with device copies in the place of ncclRecv: dst (same data and
 * hyper-parameters as src, same context) takes src's factor at `level` in the n_owners row slices the owners would send
 * and adopts it (fitted, tries = level).  For tests on a one-GPU box, where the transfer between ranks cannot run; no
 * reference counterpart (the reference's jitchol, reached from src/GaussianProcessFactory.py:57-73, is one process). */
int cbo_gp_take_factor_slices(cbo_gp *dst, cbo_gp *src, int level, int n_owners);

/* ---- Monte-Carlo interventional target -----------------------------------------
 * Replaces compute_interventions (src/utils_functions/graph_functions.py:48-77): the mean of the target node
 * over num_samples draws of sample_from_model (:8-27) on the mutilated model of intervene_dict (:30-45).
 *
 * The model is an additive structural equation model listed in evaluation order (the reference's
 * OrderedDict order): node k takes
 *     value_k = sum_t  c_t * g_t(a_t * value[parent_t])   [ + eps[eps_index_k] ]
 * terms added left to right and the noise last, g in {x, x^2, exp, cos, sin}.  The closed-form SEM the
 * reference ships has this shape (src/graphs/impl/CompleteGraph.py:57-97).  An intervened node takes its
 * intervention value instead.  The noise matrix eps (n_samples x n_eps, row-major: one row per draw, exactly
 * the `randn(len(model))` vectors the reference draws after np.random.seed(seed)) is generated by the caller
 * with numpy's legacy stream and stays resident on the device, so every call sees the reference's draws. */
#define CBO_SEM_MAX_NODES 16
#define CBO_SEM_MAX_TERMS 64
enum cbo_sem_fn { CBO_FN_ID = 0, CBO_FN_SQUARE = 1, CBO_FN_EXP = 2, CBO_FN_COS = 3, CBO_FN_SIN = 4 };
typedef struct cbo_sem_spec {
    int n_nodes;
    int eps_index[CBO_SEM_MAX_NODES];       /* column of eps added to node k, or -1 */
    int term_begin[CBO_SEM_MAX_NODES + 1];  /* terms of node k are [term_begin[k], term_begin[k+1]) */
    int term_parent[CBO_SEM_MAX_TERMS];     /* index of an EARLIER node */
    int term_fn[CBO_SEM_MAX_TERMS];         /* enum cbo_sem_fn */
    double term_a[CBO_SEM_MAX_TERMS];
    double term_c[CBO_SEM_MAX_TERMS];
} cbo_sem_spec;
typedef struct cbo_sem cbo_sem;

int cbo_sem_create(cbo_ctx *ctx, const cbo_sem_spec *spec, int64_t n_samples, int n_eps,
                   const double *eps /* n_samples * n_eps, row-major */, cbo_sem **out);
void cbo_sem_destroy(cbo_sem *sem);
/* mean_out[i] = mean over the draws of node `target` under do(iv_nodes[j] = values[i*n_iv + j], j < n_iv).
 * n_iv may be 0 (observational mean); m interventions are evaluated in one launch. */
int cbo_sem_target(cbo_sem *sem, int target, int64_t m, int n_iv, const int *iv_nodes,
                   const double *values /* m * n_iv */, double *mean_out /* m */);

/* ---- hardware self-test ------------------------------------------------------------------------
 * Runs the fp64 MFMA lane-layout check (asymmetric operands) used by tests; returns CBO_OK when the
 * v_mfma_f64_16x16x4_f64 A/B/C maps this library assumes hold on the device. */
int cbo_selftest_mfma(cbo_ctx *ctx, double *max_abs_err_out);

#ifdef __cplusplus
}
#endif
#endif /* CBO_HIP_H */

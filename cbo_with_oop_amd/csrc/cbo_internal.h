// Internal declarations shared by the kernel translation units and the C-ABI host code.
// gfx950 (MI355X / CDNA4) only: 64-lane wavefronts, v_mfma_f64_16x16x4_f64, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "cbo_hip.h"

namespace cbo {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
typedef __attribute__((address_space(3))) void *lds_ptr_t;
// LDS-DMA (global_load_lds_dwordx4): 64 lanes x 16 B land at (wave-uniform LDS byte address) + lane * 16;
// the global address is per lane.  Issued through inline asm with M0 written in the same statement
// (cdna_hip_programming.md 5.7) so that hipcc does not track it: with the builtin next to ds_reads every
// LDS-read wait degrades to lgkmcnt(0).  The caller counts completion by hand (s_waitcnt vmcnt + barrier).
__device__ __forceinline__ void glds16(const double *gsrc, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}
__device__ __forceinline__ unsigned lds_byte_address(const void *p)
{
    return (unsigned)(unsigned long)(lds_ptr_t)p;
}
#endif

// ---- data layout in HBM ------------------------------------------------------
// * Points: SoA, coordinate k of point i at xs[k * ld + i]; squared norms sq[i]; sqrt(v(x_i)) sv[i].
// * Ky and its Cholesky factor share one row-major buffer A[n_pad][lda].  Only the UPPER triangle is
//   meaningful: Ky = U^T U, U[k][i] = L[i][k].  A right-hand-side strip of 64 columns sits at column
//   n_pad; its first column carries r = y - m(X) and is overwritten by z = L^-1 r during the
//   factorisation.  n_pad = round_up(n, 128); padded rows/cols form an identity block.
// * invDt[b] (b = 16-row block index) holds inv(U_bb) row-major, i.e. invDt[b][k][i] = inv(L_bb)[i][k].
// * V workspace [n_pad][ldv]: K(X, X*) for a chunk of candidates, overwritten by L^-1 K*.
constexpr int kPadN = 128;       // n_pad granularity
constexpr int kStrip = 64;       // candidate columns per workgroup strip
constexpr int kRhsCols = 64;     // width of the right-hand-side strip appended to A
constexpr int kLdExtra = 16;     // extra doubles per row so consecutive rows fall in different channels

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// shared with cbo_comm.hip (the context is defined in cbo_api.hip)
int set_error(int code, const std::string &msg);          // records the message for cbo_last_error(), returns code
hipStream_t ctx_stream(cbo_ctx *c);
int ctx_device(cbo_ctx *c);
// the factor of a model for cbo_comm_share_factor: where it lives; whether this rank holds it at `level` of the ladder;
// its adoption by a rank that has received it
int gp_factor_view(cbo_gp *g, double **A, int64_t *lda, int64_t *n_pad, double **invDt, cbo_ctx **ctx);
bool gp_is_fitted_at(const cbo_gp *g, int level);
int gp_adopt_received_factor(cbo_gp *g, int level);

// GPy constants (GPy 1.10.0 exact_gaussian_inference.py / posterior.py); see oracle/gp_oracle.py.
constexpr double kGpyDiagJitter = 1e-8;
constexpr double kGpyVarClip = 1e-15;

struct PointSet {            // device-resident SoA point set
    double *xs = nullptr;    // [d][ld]
    double *sq = nullptr;    // [ld]
    double *sv = nullptr;    // [ld] sqrt(prior variance) or nullptr
    double *pm = nullptr;    // [ld] prior mean or nullptr
    double *pv = nullptr;    // [ld] prior variance (raw) or nullptr
    int64_t n = 0, ld = 0;
    int d = 0;
};

struct KernelHyper {
    double variance;
    double lengthscale;      // isotropic lengthscale (distance divided after sqrt); 1.0 when ard
    int ard;                 // inputs were pre-scaled per dimension
    int zero_diag;           // GPy X2=None shortcut: r2[i][i] = 0
};

// ---- kernel launchers (kernels_*.hip) -----------------------------------------------------------
// AoS (n,d) raw -> SoA (optionally divided by per-dim lengthscale), squared norms, sqrt(v).
void launch_prep_points(hipStream_t s, const double *raw_aos, int64_t n, int d, const double *ls_dev /*d or null*/,
                        const double *pv_raw /*n or null*/, double *xs, int64_t ld, double *sq, double *sv);

void launch_prep_points_staged(hipStream_t s, const double *stage, int64_t n, int d, const double *ls_dev, bool has_prior,
                               double *raw, double *y, double *pm, double *pv, double *xs, int64_t ld, double *sq,
                               double *sv);

// K(X,X) + diag into the upper 64x64 tiles of A (identity on the padding), and the rhs strip.
void launch_kxx(hipStream_t s, const PointSet &X, const KernelHyper &h, double diag_add, double jitter,
                double *A, int64_t lda, int64_t n_pad);
void launch_zero_pair(hipStream_t s, double *a, double *b, int64_t n);       // a[0:n] = b[0:n] = 0
// (zero, zero_count: ints the launch clears on the way -- the factorisation's status word and counters, cholesky_info_ints())
void launch_rhs(hipStream_t s, const double *y, const double *pm, int64_t n, double *A, int64_t lda, int64_t n_pad,
                int *zero = nullptr, int zero_count = 0);
// K(X, X*) for candidate columns [c_begin, c_begin + m_pad) into V (rows >= n are zero).
void launch_kstar(hipStream_t s, const PointSet &X, const PointSet &C, int64_t c_begin, int64_t m_pad,
                  const KernelHyper &h, double *V, int64_t ldv, int64_t n_pad);

// ---- joint posterior (kernels_joint.hip) ----------------------------------------------------------------
// Covariance: C[i][j] = K(X1_i, X2_j) - sum_{k < n_k} V[k][a_off + i] V[k][b_off + j] for i < m1, j < m2 into C
// (row-major, ldc).  V is the resident solution L^-1 K* of a candidate set holding both point sets (rows >= n are
// zero); xs / sq / sv the scaled SoA points (ld = ldx) of X1 and X2 (sv: sqrt of the prior variance, null =
// non-causal).  sym: X1 = X2, upper tiles only, mirrored stores, zero-distance rule (zero_diag) and noise on the
// diagonal.  Columns of V are read below v_cols only.
struct CovArgs {
    const double *V; int64_t ldv;
    int64_t a_off, b_off, v_cols;
    int n_k;
    const double *xs1, *sq1, *sv1, *xs2, *sq2, *sv2; int64_t ldx;
    int64_t m1, m2;
    double *C; int64_t ldc;
    double variance, inv_l2, noise;
    int zero_diag, tiles;
};
void launch_cov_tiles(hipStream_t s, int d, bool sym, CovArgs a);
// Samples: F[i][j] = mean[i] + sum_{k <= i} U[k][i] Z[k][j] for i < m, j < s into F (row-major, ldf).  U is the upper
// factor launch_cholesky leaves in [m_pad][ldu] (only k <= i is read as the factor), Z the transposed normals
// [m_pad][ldz] (ldz >= round_up(s, 128), rows >= m zero).  tiles_* are set by the launcher.
struct SampArgs {
    const double *U; int64_t ldu;
    const double *Z; int64_t ldz;
    const double *mean;
    int64_t m, s;
    double *F; int64_t ldf;
    int tiles_i, tiles_j;
};
void launch_samples_tiles(hipStream_t st, SampArgs a);
// Z[k][j] = normals[j][k] (normals: s rows of m) over [m_pad][ldz], zero outside k < m, j < s
void launch_normals_transpose(hipStream_t st, const double *normals, int64_t m, int64_t s, double *Z, int64_t m_pad,
                              int64_t ldz);
// padding of a factorisation buffer [m_pad][lda] holding an m x m matrix: identity rows >= m, zero columns >= m above
void launch_factor_padding(hipStream_t st, double *A, int64_t lda, int64_t m, int64_t m_pad);
// Integrated variance reduction, one chunk of integration points: for i < m and the chunk's tile columns T,
// part[i * ldp + tile0 + T] = sum over j < p of tile T of C_ij^2, C = K(Xc_i, Xint_j) - sum_{k < n_k} Vc[k][i] Vi[k][j]
// (cov_tile_kernel's cross element, squared).  Vc / Vi: the candidates' and the chunk's solutions L^-1 K* (leading
// dimension ldv, rows >= n zero), read below c_cols / i_cols columns only; xs / sq / sv as for CovArgs (1: candidates,
// 2: the chunk's points).  The chunk starts on global tile column tile0 (its first point is 128 tile0).
constexpr int kJointTile = 128;                    // output tile side of kernels_joint.hip
struct IvrArgs {
    const double *Vc, *Vi; int64_t ldv, c_cols, i_cols;
    int n_k;
    const double *xs1, *sq1, *sv1, *xs2, *sq2, *sv2; int64_t ldx;
    int64_t m, p;
    double *part; int64_t ldp; int64_t tile0;
    double variance, inv_l2;
};
void launch_ivr_tiles(hipStream_t s, int d, IvrArgs a);
// the closing launch (kernels_acq.hip): ivr[i] = ((sum_t part[i * ldp + t] / var[i]) / p) / cost, t < tiles in order, for
// i < m (ivr may be null); arg-max partials of ivr per workgroup (n_blocks <= 2048) for launch_argmax_final
void launch_ivr_finish(hipStream_t s, const double *part, int64_t ldp, int tiles, const double *var, int64_t m, double p,
                       double cost, double *ivr, double *part_val, int64_t *part_idx, int n_blocks);
int ivr_finish_blocks_for(int64_t m);
// ---- fp32 sweep (kernels_f32.hip; BASELINE.json configs[4]) -----------------------------------------------
// The fit stays fp64; factor, diagonal inverses and z are down-converted once per fit into a layout whose 16-row
// groups are row-permuted (physical row 4 (k & 3) + (k >> 2) = logical row k) and padded to n32 = round_up(n_pad, 256).
constexpr int kPadN32 = 256;
void launch_factor_to_f32(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, float *Uf,
                          int64_t ldu, float *invF, int64_t n32);
// K(X, X*) in fp64 arithmetic, stored as fp32; the posterior mean's kernel part mu = K*^T alpha (GPy's own formula)
// is formed on the way from the unrounded values: mu_part is (n32 / 64) * m_pad doubles of workspace
void launch_kstar_f32(hipStream_t s, const PointSet &X, const PointSet &C, int64_t c_begin, int64_t m_pad,
                      const KernelHyper &h, float *V, int64_t ldv, int64_t n32, const double *alpha, double *mu_part,
                      double *mu);
// V <- L^-1 V in fp32 (64-column strips), q[c] = sum V^2 accumulated in fp64
void launch_trsm_strips_f32(hipStream_t s, const float *U, int64_t ldu, const float *invDt, float *V, int64_t ldv,
                            int64_t n32, int64_t m_pad, double *q);
int run_mfma_f32_selftest(hipStream_t s, double *max_err);

// Recursive blocked Cholesky (upper) of A[0:n_pad, 0:n_pad] incl. forward solve of the rhs strip.
// Sweep pipelined with the factorisation: as soon as a pair of 128-row panels of U is final, the strip kernel
// solves those rows of V on `stream` (q, mu accumulate) and trsm_update_kernel folds them into the rows below,
// while the factorisation continues on its own streams.  V holds K(X, X*) on entry (assembled on `stream`).
struct SweepPipe {
    hipStream_t stream;                  // in-panel solves + the update of the next panel pair's rows
    hipStream_t bulk;                    // the updates of everything below that
    double *V;
    int64_t ldv, m_pad;
    double *zvec;                        // contiguous copy of z, written panel by panel by the diagonal kernel
    double *q, *mu;                      // zeroed on `stream` by the caller
    bool lower_tri;                      // the right-hand sides are lower triangular (identity: V = L^-1), so rows
                                         // [r0, r0+klen) only reach columns < r0+klen: launch just those strips
    int group;                           // G >= 2: updates in groups of G pairs (K = 256 G on `bulk`), see sweep_pipe_pair
    int lead = 0;                        // pairs that go alone AHEAD of the first group (their bulk update, K = 256, can start
                                         // as soon as they are solved: the bulk stream does not idle until a whole group is)
    int tail_begin;                      // rows from here on (a multiple of 256; n_pad = none) are left to ONE
                                         // left-looking strip launch once the factorisation is complete
    std::vector<hipEvent_t> *events;     // factorisation -> sweep dependencies, grown on demand
    void (*mark)(void *user, hipStream_t st, int begin, double flops);   // optional: around every sweep launch (timers)
    void *user;
};
// info_dev: 1 + kCholFlagSlots ints (status word, then one publication counter per 128-row panel)
constexpr int kCholFlagSlots = 1024;
constexpr int kCholFusedTimeout = -2147483647 - 1;     // status word when a strip of a fused launch gave up waiting
constexpr int kFusedSpinLimit = 1 << 22;               // polls before that give-up (negative: at the first wait)
// The factorisation's launch forms (cbo_init reads them from the environment, DESIGN.md's knob list)
struct CholOptions {
    int panel_form = 4;                  // CBO_HIP_PANEL_FORM: 4 = diagonal block + row panel in one launch; 5 = the same as
                                         // two launches, the block's and an LDS-free one of the strips; 2 = separate launches
    int spin_limit = kFusedSpinLimit;    // CBO_HIP_FUSED_SPIN_LIMIT: polls of a fused launch's strip, of a vector chain
    int bulk_group = 4;                  // CBO_HIP_BULK_GROUP: the most pairs per group of bulk updates (1 = pairs only)
    int group4_rows = 10240;             // CBO_HIP_BULK_GROUP4_ROWS: groups of four while this many rows lie below the group
};
// info_zeroed: the caller's launch_rhs has cleared the first cholesky_info_ints(n_pad) ints of info_dev on the same stream
void launch_cholesky(hipStream_t s, hipStream_t side, std::vector<hipEvent_t> &events, double *A, int64_t lda,
                     int64_t n_pad, double *invDt, int *info_dev, const CholOptions &opt, const SweepPipe *pipe = nullptr,
                     bool info_zeroed = false);
inline int cholesky_info_ints(int64_t n_pad)
{
    const int np = (int)(n_pad / 128);
    return 2 * np <= kCholFlagSlots ? 1 + 2 * np : 1;
}
// pair p of the pipelined sweep: rows [r0, r0 + klen) of the factor are final on stream `chain`
void sweep_pipe_pair(const SweepPipe &pipe, hipStream_t chain, const double *A, int64_t lda, const double *invDt,
                     int64_t n_pad, int p, int r0, int klen);
void sweep_pipe_tail(const SweepPipe &pipe, hipStream_t chain, const double *A, int64_t lda, const double *invDt,
                     int64_t n_pad, int pairs_done);
// alpha = U^-1 z  (z = first rhs column of A).
void launch_backsolve(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *alpha);
// out = L^-1 w for one contiguous n_pad vector (w is destroyed): the forward counterpart, one launch per block
void launch_forward_vec(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *w,
                        double *out);
void launch_gather_column(hipStream_t s, const double *V, int64_t ldv, int64_t n_pad, double *dst);
// one-launch forms (a chain of workgroups, one per 128-row block); false = not applicable (one block, or form 1 =
// CBO_HIP_VEC_SOLVE_FORM's per-block launches), nothing was launched.  `info` is the model's status word: a give-up
// (spin_limit polls) leaves kCholFusedTimeout in it and the caller repeats the solve with the per-block launches
// (launch_backsolve_vec / launch_forward_vec) after resetting it.
bool launch_backsolve_chain(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt,
                            const double *src, int64_t src_stride, double *work, double *out, int *info, int spin_limit,
                            int form);
bool launch_forward_chain(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, const double *w,
                          double *out, int *info, int spin_limit, int form);
void launch_backsolve_vec(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt,
                          const double *src, int64_t src_stride, double *work, double *out);
// Gradients of the posterior mean and variance w.r.t. the prediction inputs (GPy predictive_gradients), batched:
// dmean[c][k] = sum_i alpha_i dk(x_i, x*_c)/dx*_k, dvar[c][k] = -2 sum_i w_ic dk(x_i, x*_c)/dx*_k (RBF part only) for the
// `cols` workspace columns that hold candidates [c_begin, c_begin + cols); W = Ky^-1 K* in reversed row order.
void launch_pred_gradients(hipStream_t s, const PointSet &X, int64_t n_pad, const PointSet &C, int64_t c_begin,
                           int64_t cols, int64_t m, const KernelHyper &h, const double *inv_ls_dev, const double *alpha,
                           const double *W, int64_t ldw, double *dmean, double *dvar);
// the factor for the backward substitution through the forward strip kernel (kernels_kmat.hip), row reversal, dot pair
void launch_reversed_factor(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *T,
                            int64_t ldt, double *invT);
void launch_reverse_rows(hipStream_t s, const double *V, int64_t ldv, int64_t n_pad, int64_t cols, double *W, int64_t ldw);
void launch_dot2(hipStream_t s, const double *a, const double *b, int64_t n, double *out2);
void launch_sum(hipStream_t s, const double *a, int64_t n, double *out);
void launch_expand_interventions(hipStream_t s, const double *observed, int64_t n_obs, int d, const double *values, int n_iv,
                                 const int *iv_index, int64_t m, double *raw);

// V <- L^-1 V on m_pad columns (64-column strips); optional q[c] = sum_i V[i][c]^2, mu[c] = sum_i V[i][c] z[i].
void launch_trsm_strips(hipStream_t s, const double *U, int64_t ldu, const double *invDt, double *V, int64_t ldv,
                        int64_t n, int64_t m_pad, const double *z, double *q, double *mu, bool accumulate = false,
                        bool half_lds = false);
// C[i0_begin:i0_end, 0:m_pad] -= U[k0:k0+klen, i0_begin:i0_end]^T V[k0:k0+klen, 0:m_pad] (C may be V itself: the
// pipelined sweep); upper_only skips the workgroups that lie entirely below the diagonal
void launch_gemm_update(hipStream_t s, const double *U, int64_t ldu, const double *V, int64_t ldv, double *C,
                        int64_t ldc, int k0, int klen, int i0_begin, int i0_end, int64_t m_pad, bool upper_only,
                        const int *skip_if = nullptr);

// One (model, candidate set) pair of a multi-set sweep of small models (kernels_sets.hip, small_sets_kernel): every
// pointer is device memory; filled on the host per call and uploaded as an array.
struct cbo_small_set {
    const double *xs, *sq, *sv, *pm, *y;               // model: SoA points (ld), |x|^2, sqrt(v) or null, m(X) or null, targets
    const double *cxs, *csq, *csv, *cpm, *cpv;         // candidates (scaled SoA, ld = cld), prior closures at them or null
    int64_t ld, cld, m, index_offset;
    int n, d, zero_diag, task;
    double variance, lengthscale, noise_var, diag_add, y_best, ei_jitter, cost;
    int ard, pad_;                                     // inputs pre-scaled per dimension (lengthscale gradient per dimension)
                                                       // pad_: 0, but in small_sets_con_kernel's list of pairs, where descriptor
                                                       // s carries the index of set s's first pair
    // cbo_trial_step: the model's NEW data have not been uploaded -- they sit in pinned (device-mapped) memory as
    // [X (n,d) | y (n) | prior mean (n) | prior variance (n)] and every workgroup of the set prepares the points from there
    // itself (the arithmetic of prep_points_staged_kernel); the set's first workgroup also fills the resident copies
    // (raw, y, pm, pv and xs, sq, sv above).  nullptr: the resident copies are current.
    const double *stage, *stage_ls;                    // stage_ls: per-dimension lengthscales (ARD) or nullptr
    double *raw, *pv;
};
struct cbo_small_result {
    double best_val;
    int64_t best_idx;
    int info;                                          // first non-positive pivot (1-based) or 0
    int seq;                                           // the call's sequence number, stored last: the record is complete
};
size_t small_sets_scratch_doubles(int n_sets, int blocks_per_set);
// one-launch likelihood + gradients of a small model (kernels_chol.hip): terms[0] = variance sum, terms[1 + k] =
// lengthscale sums per dimension, then z^T z, sum log diag(U), alpha^T alpha, tr(Ky^-1)
constexpr int kSmallLmlTerms = 1 + CBO_MAX_DIM + 4;
struct cbo_small_lml_result {
    double terms[kSmallLmlTerms];
    int info, seq;
};
size_t small_lml_scratch_doubles();
void launch_small_lml(hipStream_t s, const cbo_small_set &st, double *scratch, int *info, cbo_small_lml_result *out, int seq);
// n_models models (n <= 256) in one launch: descriptors (pinned, device-mapped), `stride` doubles of scratch per model
// (small_lml_scratch_doubles() when every n <= 128, else mid_lml_scratch_doubles()), info[b] zero on entry (zero
// again afterwards), record out[b] (pinned) per model
size_t mid_lml_scratch_doubles();
void launch_small_lml_batch(hipStream_t s, const cbo_small_set *sets, int n_models, double *scratch, int64_t stride,
                            int *info, cbo_small_lml_result *out, int seq);
// ---- leave-one-out cross-validation (kernels_loo.hip) ---------------------------------------------
// record of one model of small_loo_batch_kernel (pinned host memory, written by the kernel): the three per-point outputs
// of its n <= 128 points, their lpd summed in index order, the first non-positive pivot (1-based) or 0
struct cbo_small_loo_result {
    double sum;
    double mean[128], var[128], lpd[128];
    int info, seq;
};
size_t small_loo_scratch_doubles();                    // per model: factor rows + inverses
// n_models models (n <= 128) in one launch: descriptors (pinned, device-mapped), info[b] zero on entry (zero again afterwards)
void launch_small_loo_batch(hipStream_t s, const cbo_small_set *sets, int n_models, double *scratch, int *info,
                            cbo_small_loo_result *out, int seq);
// V[i][j] = 1 where i == j + shift, else 0, for i < rows, j < cols (cols even, V + i ldv + j 16-byte aligned): columns
// [c0, c0 + cols) of the identity seen from row r0 = c0 - shift on
void launch_loo_identity_chunk(hipStream_t s, double *V, int64_t ldv, int64_t rows, int64_t cols, int64_t shift);
// mean, var, lpd (each may be null) of the points i < n from c = diag(Ky^-1), alpha and y; sum_out[0] = sum of lpd in a
// fixed order through partial (loo_finish_blocks(n) doubles of scratch)
int loo_finish_blocks(int64_t n);
void launch_loo_finish(hipStream_t s, const double *c, const double *alpha, const double *y, int64_t n, double *mean_out,
                       double *var_out, double *lpd_out, double *partial, double *sum_out);
// The one-workgroup sweeps (small_sets_kernel, small_sets_con_kernel, hyper_avg_kernel, hyper_sets_kernel) take two launches from this many
// candidate blocks per model on.  Few blocks (the reference's 100-200 candidates): every workgroup factors its model
// itself, ONE launch, no dependency between workgroups.  Many blocks (16k-candidate grids on 25 coral sets: 6400
// workgroups): factoring the model 256 times over costs more than a second launch -- one workgroup per model factors,
// then the sweep workgroups start from the factor.  profiles/hyper_avg_timing.json has both schedules of hyper_avg_kernel
// at the three shapes of DESIGN.md §4j.
constexpr int kSmallTwoPhaseFromBlocks = 12;
// sets / out may be pinned host memory (device-mapped): the kernel then reads the descriptors and writes the results
// across the host link itself and the call needs no copy operation (the host may poll out[].seq instead of
// synchronising the stream); info and ticket (device, n_sets ints each) must be zero on entry and are zero again afterwards.
// kind (kernels_sets.hip, small_sets_kernel<KIND>): kEiKind = the causal EI, or the point-wise epilogue
// CBO_ACQ_LCB / _PI / _VAR / _MPEI; the descriptors' ei_jitter then carries the kind's parameter, y_best PI's incumbent
// (the plug-in EI forms its own inside the launch)
constexpr int kEiKind = 0;
// Two further kinds, internal (beyond CBO_ACQ_*), read what the descriptor has no room for through `aux`:
//   kMesKind      max-value entropy search's epilogue (mes_of, so cbo_acq_sweep_mes' bits): set s scores against the
//                 per_set[s].count (1..kMesMaxSamples) Gumbel samples data[per_set[s].off ...]; task is 'min';
//   kPredictKind  no acquisition and no arg-max: the predictive mean and variance (noise included) of candidate c of set s
//                 go to mean_out / var_out[per_set[s].off + c] (cbo_gp_mes_gumbel_sets' grids); the record carries the
//                 status word alone.
// per_set and data may be pinned host memory (device-mapped), like the descriptors.
constexpr int kMesKind = 5;
constexpr int kPredictKind = 6;
// ... and one that reads nothing more than the EI does: log Expected Improvement, log_ei_of's epilogue --
// log EI - log cost, task 'max' mirrored; ei_jitter is the jitter, y_best the incumbent.  Internal: the public kind codes
// (CBO_ACQ_*) do not name it, the entry points cbo_acq_sweep_logei / _sweep_sets_logei / _refine_sets_logei do.
constexpr int kLogEiKind = 7;
// ... and two that price every candidate at its own cost: set s reads cost[c] from aux's cost[s], the cost
// vector of its candidate set (cbo_cands_set_cost); the descriptor's cost is 1.  kEiPointKind: acquisition_of at cost 1 over
// cost[c], the IEEE quotient; kLogEiPointKind: log_ei_of with log(cost[c]).  Internal, reached through the *_pointcost entry
// points alone; in the refinement kernel they also select the gradient with the cost's own derivative.
constexpr int kEiPointKind = 8;
constexpr int kLogEiPointKind = 9;
struct cbo_small_aux {
    int64_t off, count;
};
struct SmallAux {
    const cbo_small_aux *per_set = nullptr;
    const double *data = nullptr;
    double *mean_out = nullptr, *var_out = nullptr;
    const double *const *cost = nullptr;               // per set (pinned, device-mapped): its candidates' cost vector
};
// What every launch of these kernels takes from its context beside the descriptors: scratch and partial winners per
// workgroup, one status word, one ticket and one (pinned) record per set, and the call's sequence number, which closes a
// record.  The host wrappers below take it whole and unpack it into the kernels' parameter lists.
struct SmallLaunch {
    double *scratch, *part_val;
    int64_t *part_idx;
    int *info, *ticket;
    cbo_small_result *out;
    int seq;
};
void launch_small_sets(hipStream_t s, int kind, const cbo_small_set *sets, int n_sets, int blocks_per_set, const SmallLaunch &L,
                       const SmallAux &aux = SmallAux());
// ---- gradient refinement of every set's starts in one launch (kernels_sets_refine.hip) ----------------------
// What a set's searches need beside the model's descriptor (pinned, device-mapped: read by the kernel directly): the box,
// the cost c(x) = sum_k (fix[k] + (variable[k] ? |x_k| : 0)), the per-dimension lengthscales of an ARD model (the moving
// point is scaled as prep_points_kernel scales a candidate), the number of starts and where the set's rows begin in the
// call's starts / x_out / grad_out (row_off, in doubles) and in val_out / rounds_out / status_out (out_off).
struct cbo_small_refine {
    double lo[CBO_MAX_DIM], hi[CBO_MAX_DIM], fix[CBO_MAX_DIM], ls[CBO_MAX_DIM];
    int variable[CBO_MAX_DIM];
    int64_t row_off;
    int k, out_off, ard, pad_;
    const struct DoPriorView *prior;   // the do-calculus prior of a causal set on the device, else nullptr
};
int small_refine_starts_per_block(int d);              // 4 floor(16 / (1 + d)): a start fills 1 + d of a wave's 16 columns
// sets / refs / starts and the five outputs may be pinned host memory; scratch: small_sets_scratch_doubles(n_sets,
// blocks_per_set); info: n_sets ints, zero on entry, a set's word non-zero afterwards when its factorisation met a
// non-positive pivot (the kernel then wrote CBO_REFINE_DECLINED for the set's starts and nothing else).  kind: kEiKind or
// CBO_ACQ_*, the descriptors' scalars as for launch_small_sets; descriptors carry no candidates.  max_rounds <= 1000.
// prior: every set of the list carries one (refs[].prior) and its model is causal -- the kernel's causal instantiation;
// false: none does.
void launch_small_sets_refine(hipStream_t s, int kind, bool prior, const cbo_small_set *sets, const cbo_small_refine *refs,
                              const double *starts, int n_sets, int blocks_per_set, double *scratch, int *info, int max_rounds,
                              double *x_out, double *val_out, double *grad_out, int *rounds_out, int *status_out);
// ---- ... of every set's CONSTRAINED acquisition (kernels_sets_refine_con.hip) --------------------------------
// A set is 1 + n_con consecutive descriptors of `pairs`, the objective first (launch_small_sets_con's convention: set s's
// first descriptor rides in pairs[s].pad_; a constraint's value, jitter and sense in y_best, ei_jitter and task; no
// candidates); pair_ls[p] holds descriptor p's per-dimension lengthscales (read when its model is ARD); refs[s] the set's box,
// cost table, starts and offsets (ls, ard and prior are not read).  Every model of a set has the set's d; none is causal.
// slots: the most models a set of the launch has.  scratch: small_refine_con_scratch_doubles(n_sets, blocks_per_set, slots)
// -- per workgroup `slots` factor slots of kSmallScratch doubles, then the rings of its at most 32 starts.  info, the
// outputs and max_rounds as for launch_small_sets_refine.
struct cbo_small_refine_pair {
    double ls[CBO_MAX_DIM];
};
constexpr int kRefineConRing = 64;                     // doubles of one ring (8 curvature pairs of at most CBO_MAX_DIM)
constexpr int kRefineConRings = 32 * 2 * kRefineConRing;   // a workgroup's: 32 starts (d = 1), S and Y each
size_t small_refine_con_scratch_doubles(int n_sets, int blocks_per_set, int slots);
void launch_small_sets_refine_con(hipStream_t s, bool log_form, const cbo_small_set *pairs, const cbo_small_refine_pair *pair_ls,
                                  int n_pairs, const cbo_small_refine *refs, const double *starts, int n_sets,
                                  int blocks_per_set, int slots, double *scratch, int *info, int max_rounds, double *x_out,
                                  double *val_out, double *grad_out, int *rounds_out, int *status_out);
// ---- the device-resident do-calculus prior (kernels_do_prior.hip, do_prior_device.h) ------------------------
constexpr int kDoPriorMaxN = CBO_DO_PRIOR_MAX_N;   // rows of a graph GP a handle takes
constexpr int kDoPriorGroup = 256;                 // lanes that evaluate one point together: a whole workgroup
// What a handle keeps on the device (every pointer device memory owned by the handle).  M is symmetric to the bit, so
// column r of it is read as row r: lanes walk the rows of M side by side.
struct DoPriorView {
    const double *w;                // [n]       sigma^2 alpha_i mean_r b_ri
    const double *M;                // [n][ldm]  sigma^4 (Ky^-1 o b^T b / N_obs)
    const double *xi;               // [n_col][ldx] the intervened columns of X_g, scaled as the kernels scale points
    int64_t ldm, ldx;
    double ls[CBO_MAX_DIM];         // lengthscale of intervened column k (ARD), else 1
    double inv_l2, vmax;            // 1 / l^2 (1 for ARD); sigma^2 + sigma_n^2
    int src[CBO_MAX_DIM];           // the column of `values` that intervened column k takes
    int n, n_col, n_iv, ard;
};
// b[r][i] = exp(-1/2 sum over the n_free columns c = col[k] that are NOT intervened of ((obs[r][c] - X_g[i][c]) / l_c)^2) for
// r < n_obs, i < n, zero elsewhere in [rows_pad][ldb]: k-major, the layout V has.  obs: raw (n_obs, d) on the device; xs:
// the graph GP's scaled SoA points; ls[k]: lengthscale of column col[k] (ARD; the observed value is scaled as a point is).
struct DoPriorRowsArgs {
    const double *obs, *xs; double *b;
    int64_t n_obs, rows_pad, ldb, ldx;
    double ls[CBO_MAX_DIM], inv_l2;
    int col[CBO_MAX_DIM];
    int n, d, n_free, ard;
};
void launch_do_prior_rows(hipStream_t s, const DoPriorRowsArgs &a);
// w[i] = (variance alpha[i]) (sum_r b[r][i] / n_obs), r ascending, i < n
void launch_do_prior_weights(hipStream_t s, const double *b, int64_t ldb, int64_t n_obs, const double *alpha, double variance,
                             int n, double *w);
// Gram products on kernels_joint.hip's tile loop: out[i][j] = sum_{k < n_k} A[k][i] A[k][j] for i, j < n (row-major, ldo) --
// or, with prev given (it may be out), (prev[i][j] (that sum / divisor)) scale, the element-wise product's epilogue.  A is
// k-major [n_k rounded up to 16][lda] with at least round_up(n, 128) readable columns.
struct GramArgs {
    const double *A; int64_t lda; int n_k;
    const double *prev; double *out; int64_t ldo;
    int n;
    double divisor, scale;
};
void launch_gram_tiles(hipStream_t s, GramArgs a);
// (m, v) of m points (values: m x view->n_iv on the device) by do_prior_at, one point per workgroup and turn; scratch:
// do_prior_eval_blocks(m) * kDoPriorMaxN doubles
int do_prior_eval_blocks(int64_t m);
void launch_do_prior_eval(hipStream_t s, const DoPriorView *view, const double *values, int64_t m, double *scratch,
                          double *mean_out, double *var_out);
// ---- every model's HMC chain over its hyper-parameters in one launch (kernels_hmc.hip) -----------------------
// What a model's chain needs beside the model's descriptor (pinned, device-mapped: read by the kernel directly): the start,
// the chain's shape, and where its draws (n_params x num_samples momenta, then num_samples uniforms) and its rows / accept
// flags begin in the call's arrays.  n_params = 1 + n_ls + sample_noise.
struct cbo_small_hmc {
    double theta0[CBO_HMC_MAX_PARAMS];
    double stepsize;
    int64_t draw_off, row_off, acc_off;
    int n_params, n_ls, sample_noise, num_samples, hmc_iters;
    int n_prior;                                   // how many of priors[0..n_params) are not NONE; 0: the stage is skipped
    cbo_hyper_prior priors[CBO_HMC_MAX_PARAMS];    // the model's priors in the row's order (hyper_prior.h)
};
// sets / chains / draws and the four outputs may be pinned host memory; scratch: `stride` >= small_lml_scratch_doubles()
// doubles per model; info: n_models ints, zero on entry and zero again afterwards.  final_out: per model theta
// [CBO_HMC_MAX_PARAMS], lml, dlml / dtheta [CBO_HMC_MAX_PARAMS]; status_out: CBO_HMC_OK or CBO_HMC_NOT_PD per model (a
// chain that met a non-positive pivot wrote rows up to there and no final state).
void launch_hmc_sets(hipStream_t s, const cbo_small_set *sets, const cbo_small_hmc *chains, const double *draws, int n_models,
                     double *scratch, int64_t stride, int *info, double *rows_out, int *accept_out, double *final_out,
                     int *status_out);
// ---- every model's hyper-parameter MLE in one launch (kernels_mle.hip) --------------------------------------
// One RUN of the launch: a (model, start) pair -- the index of the model's descriptor, the start and the search's shape
// (pinned, device-mapped: read by the kernel directly).  n_params = 1 + n_ls + fit_noise.
struct cbo_small_mle {
    double theta0[CBO_HMC_MAX_PARAMS];
    int model, n_params, n_ls, fit_noise, max_rounds;
    int n_prior;                                   // how many of priors[0..n_params) are not NONE; 0: the stage is skipped
    cbo_hyper_prior priors[CBO_HMC_MAX_PARAMS];    // the model's priors in the row's order (hyper_prior.h)
};
// a run's two rings of curvature pairs (mle_search.h): S then Y, 8 pairs x CBO_HMC_MAX_PARAMS doubles each
constexpr int kMleRingDoubles = 2 * 8 * CBO_HMC_MAX_PARAMS;
// One workgroup per run.  sets (n_models descriptors) / runs and the three outputs may be pinned host memory; scratch:
// `stride` >= small_lml_scratch_doubles() doubles per RUN; info: n_runs ints, zero on entry and zero again afterwards; rings
// (device): kMleRingDoubles doubles per run.  final_out: per run theta [CBO_HMC_MAX_PARAMS], lml, dlml / dtheta
// [CBO_HMC_MAX_PARAMS] at the search's end point; status_out: CBO_REFINE_PGTOL .. CBO_REFINE_NAN_START, or CBO_MLE_NOT_PD
// (the start's Ky is not positive definite as assembled: no final state); rounds_out: the rounds taken.
void launch_mle_sets(hipStream_t s, const cbo_small_set *sets, int n_models, const cbo_small_mle *runs, int n_runs,
                     double *scratch, int64_t stride, int *info, double *rings, double *final_out, int *status_out,
                     int *rounds_out);
// ... and for models of 128 < n <= 256 observations (kernels_mle_mid.hip, mle_mid_kernel): the same
// arguments and outputs; scratch: `stride` >= mid_mle_scratch_doubles() doubles per RUN -- the two-block slab of
// mid_lml_scratch_doubles() and behind it the region the run's points are prepared into.
size_t mid_mle_scratch_doubles();
void launch_mle_mid(hipStream_t s, const cbo_small_set *sets, int n_models, const cbo_small_mle *runs, int n_runs,
                    double *scratch, int64_t stride, int *info, double *rings, double *final_out, int *status_out,
                    int *rounds_out);
// ---- the hyper-parameters' log prior of many models in one launch (kernels_prior.hip) -------------------------
// One lane per model: hyper_prior_at over the model's n_params entries at theta.  items (pinned, device-mapped) are read and
// written by the kernel directly; the caller synchronises the stream before it reads lp / dlp.
struct cbo_prior_item {
    cbo_hyper_prior priors[CBO_HMC_MAX_PARAMS];
    double theta[CBO_HMC_MAX_PARAMS];
    double lp, dlp[CBO_HMC_MAX_PARAMS];
    int n_params, done;                            // done: 0 on entry, 1 once lp / dlp are written
};
void launch_log_prior(hipStream_t s, cbo_prior_item *items, int n_models);
// the same launch with the batch epilogue (kernels_sets_batch.hip, small_sets_batch_kernel): batch_size >= 2
// Kriging-believer picks per set.  Sets of at most kSmallBatchMaxCands candidates: the set's V = L^-1 K* stays in global
// scratch (1 MiB per set at the cap) and the call's widest set has at most 16 candidate blocks.  batch_scratch:
// small_sets_batch_doubles(...) doubles (V [128][m_pad], W [batch_size - 1][m_pad], q and mu [m_pad] per set, m_pad =
// 64 blocks_per_set); h_vals / h_idxs (pinned, device-mapped): n_sets x batch_size winners, set-major, complete when
// the set's record is; everything else as launch_small_sets.  log_form: the kernel's LOG instantiation, every
// pick scored by log EI - log cost.
constexpr int kSmallBatchMaxCands = 1024;
struct SmallBatchArgs {
    double *V, *W, *q, *mu;
    double *h_vals; int64_t *h_idxs;
    int64_t m_pad;
    int batch_size, update_incumbent;
};
size_t small_sets_batch_doubles(int n_sets, int blocks_per_set, int batch_size);
void launch_small_sets_batch(hipStream_t s, const cbo_small_set *sets, int n_sets, int blocks_per_set, const SmallLaunch &L,
                             double *batch_scratch, int batch_size, int update_incumbent, double *h_vals, int64_t *h_idxs,
                             bool log_form = false);
// the same launch with the constrained epilogue (kernels_sets_con.hip, small_sets_con_kernel): `pairs` holds
// one descriptor per (model, candidate set) pair, a set's pairs consecutive with the objective first; a constraint's value,
// jitter and sense ride in y_best, ei_jitter and task; pairs[s].pad_ = index of set s's first pair.  max_pairs = the most
// pairs of one set (<= 1 + CBO_MAX_CONSTRAINTS).  scratch, part_val, part_idx: n_sets * blocks_per_set slots; info, ticket,
// out: one per SET, as above.  log_form: the sum of the terms' logarithms less log(cost), the general log
// pass's bits
void launch_small_sets_con(hipStream_t s, const cbo_small_set *pairs, int n_pairs, int n_sets, int max_pairs,
                           int blocks_per_set, const SmallLaunch &L, bool log_form = false);

// ---- hyper-parameter-marginalised EI (kernels_hyper.hip) ----------------------------------------------
// One launch (schedule 1) or two (2; 0 = by the number of candidate blocks) for a model of at most 128 observations: st is
// fill_small_model's descriptor plus the candidates' prior closures, m, index_offset and EI's scalars; craw the set's raw AoS
// coordinates; hyper (pinned, device-mapped) n_samples rows of (variance, lengthscale x n_ls, noise_var); acq_out (device, m)
// or null.  scratch: hyper_avg_scratch_doubles(blocks, n_samples); part_val / part_idx: `blocks` entries; info[0], ticket[0]
// zero on entry (zero again afterwards); the record out[0] (pinned) carries the winner and the status word.
size_t hyper_avg_scratch_doubles(int blocks, int n_samples);
// log_form: the kernels' log instantiation -- log((1 / H) sum_h EI_h) - log cost by the streaming
// log-sum-exp of lse_stream.h over log_ei_of's terms at log cost 0
void launch_hyper_avg(hipStream_t s, const cbo_small_set &st, const double *craw, const double *hyper, int n_samples,
                      int n_ls, double *acq_out, int blocks, int schedule, const SmallLaunch &L, bool log_form = false);
// The multi-set form (hyper_sets_kernel).  One descriptor per set: hyper_avg_kernel's arguments (acq_out
// null) and `first`, the sum of the n_samples of the sets before it -- the scratch slot of the set's sample 0 in the
// two-launch form.  sets may be pinned host memory (read by the kernel directly beyond kSmallByValue sets).
struct HyperArgs {
    cbo_small_set st;                  // fill_small_model's descriptor + the candidates' prior closures, m, index_offset, EI's scalars
    const double *craw;                // the candidates' raw AoS coordinates
    const double *hyper;               // n_samples rows of (variance, lengthscale x n_ls, noise_var): pinned host memory
    int n_samples, n_ls;
    double *acq_out;                   // [m] device, or null
};
struct HyperSet {
    HyperArgs a;
    int first, pad_;
};
// scratch: hyper_sets_scratch_doubles(...); part_val / part_idx: n_sets * blocks_per_set entries; info, ticket (n_sets ints
// each) zero on entry (zero again afterwards); one record out[s] (pinned) per set.  two_phase: a first launch of
// total_samples workgroups factors every sample of every set once, the sweep reads the factors back.
size_t hyper_sets_scratch_doubles(int n_sets, int blocks_per_set, int total_samples, bool two_phase);
void launch_hyper_sets(hipStream_t s, const HyperSet *sets, int n_sets, int blocks_per_set, int total_samples, bool two_phase,
                       const SmallLaunch &L, bool log_form = false);
// the general path: sum[i] = (first ? 0 : sum[i]) + acq[i] for i < m; then acq_out[i] = sum[i] / n_samples (acq_out may be
// null) with arg-max partials per workgroup (n_blocks <= 2048) for launch_argmax_final
void launch_hyper_accumulate(hipStream_t s, double *sum, const double *acq, int64_t m, bool first, int n_blocks);
void launch_hyper_finish(hipStream_t s, const double *sum, int64_t m, int n_samples, double *acq_out, double *part_val,
                         int64_t *part_idx, int64_t index_offset, int n_blocks);
// the log form's general path: (M, S)[i] = lse_start(term[i]) when first, else lse_push(term[i]) into them;
// then acq_out[i] = lse_close(M[i], S[i], n_samples, log(cost)) (acq_out may be null) with the arg-max partials as above
void launch_hyper_lse_accumulate(hipStream_t s, double *M, double *S, const double *term, int64_t m, bool first, int n_blocks);
void launch_hyper_lse_finish(hipStream_t s, const double *M, const double *S, int64_t m, int n_samples, double cost,
                             double *acq_out, double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks);

struct AcqParams {
    double variance, noise_var, y_best, ei_jitter, cost;
    int task, include_noise, want_ei;
    const double *y_best_dev = nullptr;                // when set, acq_kernel reads the incumbent from here (device memory)
};
// var = clip(kss - q) (+ noise), mean = mu + m(X*), acq = +-EI / cost; per-block arg-max partials.
void launch_acq(hipStream_t s, const double *q, const double *mu, const double *pm, const double *pv, int64_t m,
                const AcqParams &p, double *mean_out, double *var_out, double *acq_out, double *part_val,
                int64_t *part_idx, int64_t index_offset, int n_blocks);
void launch_argmax_final(hipStream_t s, const double *part_val, const int64_t *part_idx, int n, double *best_val,
                         int64_t *best_idx, const int *status_src = nullptr, int *status_dst = nullptr);
int acq_blocks_for(int64_t m);
// ---- max-value entropy search (kernels_mes.hip) -----------------------------------------------------------------
// The Gumbel samples travel in the kernel arguments: at most kMesMaxSamples of them.
constexpr int kMesMaxSamples = 64;
struct MesParams {
    double variance, noise_var, cost;
    int k;
    double mins[kMesMaxSamples];
};
// acq_kernel's mean and variance (noise included), then mes = mean over the k samples of emukit's per-sample term, / cost;
// launch grid and arg-max partials as launch_acq (acq_blocks_for)
void launch_mes_acq(hipStream_t s, const double *q, const double *mu, const double *pm, const double *pv, int64_t m,
                    const MesParams &p, double *mean_out, double *var_out, double *acq_out, double *part_val,
                    int64_t *part_idx, int64_t index_offset, int n_blocks);
// The three bisections of emukit's _fit_gumbel (vals 0.25, 0.5, 0.75) on the predictive mean / variance of m grid points,
// one workgroup each: out[0..3) the quantiles, out[3] = left, out[4] = right; status[j] = 0 converged, 1 the bracket does
// not change sign (scipy's ValueError), 2 no convergence within maxiter (scipy's RuntimeError).
// n_sets sets in one launch (a (3, n_sets) grid): set s reads its (mean, var, m) from table[s] (device-visible) and writes
// out[5 s ..], status[3 s ..]; table == nullptr: one set, `one`, which travels in the kernel arguments.
struct GumbelSet {
    const double *mean, *var;
    int64_t m;
};
void launch_gumbel_quantiles(hipStream_t s, const GumbelSet &one, const GumbelSet *table, int n_sets, double *out,
                             int64_t *status);
// ---- constrained acquisition (kernels_con.hip) ------------------------------------------------------------------
// EI times probabilities of feasibility over a cost, from the q, mu of several (model, candidate set) pairs at once.  The
// pointer table travels in the kernel arguments: model 0 is the objective when has_objective, every other one a constraint.
constexpr int kConMaxModels = CBO_MAX_CONSTRAINTS + 1;
struct ConModel {
    const double *q, *mu, *pm, *pv;                    // pm, pv: the set's prior closures, null for a non-causal model
    double *out;                                       // the model's own term per candidate (EI, pof_k) or null
    double variance, noise_var;
    double value, jitter;                              // constraints: bound and jitter
    int sense, pad_;                                   // constraints: CBO_CON_LE / CBO_CON_GE
};
struct ConParams {
    ConModel mdl[kConMaxModels];
    double y_best, ei_jitter, cost;
    int n_models, has_objective, task, pad_;
};
// acq = (((t_0 t_1) t_2) ...) / cost for i < m (acq_out may be null), t_0 = acquisition_of at cost 1 when has_objective,
// every other t_k = ndtr(+-(value - (mean + jitter)) / sqrt(var)) of acq_kernel's mean and variance (noise included);
// launch grid and arg-max partials as launch_acq (acq_blocks_for).
// log_form: acq = (((l_0 + l_1) + l_2) ...) - log(cost), l_0 = log_ei_of at log cost 0.0 (task 'max' the
// mirror), every other l_k = log_ndtr of the same u: finite where the product underflows
void launch_constrained_acq(hipStream_t s, const ConParams &p, int64_t m, double *acq_out, double *part_val,
                            int64_t *part_idx, int64_t index_offset, int n_blocks, bool log_form = false);
// ---- point-wise acquisitions (kernels_pointwise.hip) -------------------------------------------------
// kind CBO_ACQ_LCB / _PI / _VAR: acq_kernel's mean and variance (noise included), then the kind's value / cost.  p.ei_jitter
// carries the kind's parameter (beta; PI's jitter), p.y_best PI's incumbent; p.want_ei is not read, p.y_best_dev by kLogEiKind alone: when set, the
// log EI's incumbent is read from there (cbo_acq_sweep_batch_logei's moved incumbent).
// Launch grid and arg-max partials as launch_acq (acq_blocks_for).
void launch_pointwise_acq(hipStream_t s, int kind, const double *q, const double *mu, const double *pm, const double *pv,
                          int64_t m, const AcqParams &p, double *mean_out, double *var_out, double *acq_out,
                          double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks);
// ---- per-candidate intervention costs (kernels_pointwise.hip) -----------------------------------------
// The reference's cost table of one exploration set, c(x) = sum_k (fix[k] + (variable[k] ? |x_k| : 0)): cbo_refine_set's pair.
struct CostTable {
    double fix[CBO_MAX_DIM];
    int variable[CBO_MAX_DIM];
};
// cost[j] = c(raw row j) for j < m, in the refinement kernel's (and one_row_cost's) operation order
void launch_cands_cost(hipStream_t s, const double *raw, int64_t m, int d, const CostTable &t, double *cost);
// launch_pointwise_acq's pass with the candidates' own costs as a fifth operand stream: acquisition_of at cost 1 over cost[j]
// (the IEEE quotient), or log_ei_of with log(cost[j]) when log_form.  p.cost must be 1.
void launch_pointcost_acq(hipStream_t s, bool log_form, const double *q, const double *mu, const double *pm, const double *pv,
                          const double *cost, int64_t m, const AcqParams &p, double *mean_out, double *var_out,
                          double *acq_out, double *part_val, int64_t *part_idx, int64_t index_offset, int n_blocks);
// out[0] (device) = min (CBO_TASK_MIN) or max of mean[0:n), NaN if any of them is
void launch_plugin_incumbent(hipStream_t s, const double *mean, int64_t n, int task, double *out);
// out[g] = mean of in[g*group .. (g+1)*group)
void launch_group_mean(hipStream_t s, const double *in, int64_t n_groups, int64_t group, double *out);

// out[0] = sum z_i^2, out[1] = sum log U_ii over the n_pad rows (padding contributes 0)
void launch_lml_terms(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *z, double *out2);
// likelihood gradients: out[0] = sum M k, out[1 + k] = sum M k ((x_ik - x_jk)/l_k)^2 over all i, j < n with
// M = alpha alpha^T + negW; partial: lml_grad_tiles(n_pad) * (1 + d) doubles
int lml_grad_tiles(int64_t n_pad);
void launch_lml_grad(hipStream_t s, const PointSet &X, const KernelHyper &h, const double *alpha, const double *negW,
                     int64_t ldw, int64_t n_pad, double *partial, double *out);
void launch_set_identity(hipStream_t s, double *V, int64_t ldv, int64_t n_pad);
void launch_gather_diag(hipStream_t s, const double *A, int64_t lda, int64_t n, double *diag);
void launch_export_lower(hipStream_t s, const double *A, int64_t lda, int64_t n, double *L_rowmajor);
void launch_export_sym(hipStream_t s, const double *A, int64_t lda, int64_t n, double *K_rowmajor);

int run_mfma_selftest(hipStream_t s, double *max_err);

// append-only trial step (kernels_acq.hip): commit column n of the factor (l from column 0 of l_src), the new
// diagonal entry, z_n, the point's coordinates and the diagonal tile's inverse; extend a resident V by row n
void launch_append_commit(hipStream_t s, double *A, int64_t lda, int64_t n, int64_t n_pad, const double *l_src,
                          int64_t ld_src, double d, double zn, double *z, double *lvec, PointSet &X, const PointSet &P,
                          double pm_new, double pv_new, double *y, double y_new, double *invDt);
int append_row_slices(int64_t n);
void launch_append_row(hipStream_t s, double *V, int64_t ldv, int64_t n, const double *lvec, int64_t m_pad,
                       const double *krow, double d, double zn, double *partial, double *q, double *mu);

// ---- block append (kernels_append.hip) ------------------------------------------------------------
constexpr int kAppendLd = 64;                          // leading dimension of B [n_pad][64] and L22 [64][64]
constexpr int kAppendMaxSlices = 8;                    // row slices of the pass over V (partial: slices x kp x m_pad)
// out = L^-1 W for the first kp (a multiple of 16, <= 64) columns of W [n_pad][ldw] (W is destroyed); out: [n_pad][kAppendLd]
void launch_append_forward(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *W,
                           int64_t ldw, int kp, double *out);
struct AppendSchurArgs {
    const double *part; int slices;                    // set by the launcher: append_schur_slices(n) x 65 x 64 doubles
    int k;
    const double *Kbb; int64_t ldk;                    // K(Xb, Xb), X2 explicit, causal term included
    const double *pv, *pm;                             // the new points' prior variance and mean (null: non-causal)
    const double *y_new;
    double variance, sigma;                            // sigma = noise_var + 1e-8
    double *L22, *zb;                                  // [64][64] lower (zero elsewhere), [64]
    int *status;                                       // 0, or the first pivot (1-based) that is not positive and finite
};
int append_schur_slices(int64_t n);
void launch_append_schur(hipStream_t s, const double *B, int64_t n, const double *z, AppendSchurArgs a);
struct AppendCommitArgs {
    double *A; int64_t lda, n, n_pad; int k;
    const double *B, *L22, *zb, *y_new;
    double *z, *y;
    int dims; double *xs; int64_t ldx; double *sq, *sv, *pm, *pv;       // the model's points (sv null: non-causal)
    const double *pxs; int64_t ldp; const double *psq, *psv, *pm_new, *pv_new;   // the block's points as a candidate set
};
void launch_append_block_commit(hipStream_t s, const AppendCommitArgs &a, double *invDt);
struct AppendRowsArgs {
    const double *part; int slices;                    // set by the launcher
    int k; int64_t m_pad;
    const double *Kb; int64_t ldk;                     // K(Xb, X*) [64][ldk]
    const double *L22, *zb;
    double *Vnew; int64_t ldv;                         // row n of the resident V
    double *q, *mu;
};
void append_rows_plan(int64_t rows, int64_t m_pad, int *slices, int *rows_per_slice);
// rows: the rows of V the block was appended to (n before the append); part: slices * kp * m_pad doubles of scratch
void launch_append_rows(hipStream_t s, const double *V, int64_t ldv, const double *B, int64_t rows, int kp, double *part,
                        const AppendRowsArgs &a);

// ---- greedy batch selection (kernels_batch.hip) --------------------------------------------------
// One further pick of cbo_acq_sweep_batch.  Pick t >= 1 reads its pivot -- the winner of pick t - 1 -- from device memory.
constexpr int kBatchMaxSlices = 64;                    // row slices of the pass over V (partial: kBatchMaxSlices x m_pad)
struct BatchState {                                    // the current pick's scalars, device memory
    double d;                                          // sqrt of the believed point's predictive variance + 1e-8
    double x[CBO_MAX_DIM], sq, sv;                     // its scaled coordinates, |x|^2, sqrt(v(x))
    double y_best;                                     // the incumbent (moves with update_incumbent)
    double wp[CBO_MAX_BATCH];                          // W[s][p] of the earlier fantasy rows
    int64_t p;                                         // its local index
};
struct BatchPivotArgs {
    const double *best_val; const int64_t *best_idx;   // device: the previous pick's winner
    int64_t index_offset, m, m_pad, n;
    const double *V; int64_t ldv;
    double *col;                                       // [n] the pivot column, contiguous
    const double *W;                                   // [t - 1][m_pad] earlier fantasy rows
    const double *q, *mu, *pm, *pv;                    // working q; mu and the prior closures (pm, pv null: non-causal)
    const double *xs, *sq, *sv; int64_t ldx; int dims; // the candidates' scaled SoA points
    double variance, noise_var;
    int t, task, update_incumbent;
    BatchState *state;
    double *h_vals; int64_t *h_idxs;                   // pinned host: slot t - 1 takes the previous winner
};
struct BatchFinalArgs {
    const double *partial; int slices;                 // set by the launcher
    int64_t m, m_pad;
    double *W; double *q;                              // row t - 1 of W is written, q updated in place
    const double *xs, *sq, *sv; int64_t ldx;           // sv null: non-causal
    double variance, inv_l2;
    int t;
    const BatchState *state;
};
int batch_slices(int64_t n);
void launch_batch_state_init(hipStream_t s, BatchState *st, double y_best);
void launch_batch_record(hipStream_t s, const double *best_val, const int64_t *best_idx, int slot, double *h_vals,
                         int64_t *h_idxs);
// pivot, pass and final stage of one pick; col: n doubles, partial: batch_slices(n) * m_pad doubles of scratch
void launch_batch_pick(hipStream_t s, const BatchPivotArgs &pa, BatchFinalArgs fa, double *col, double *partial);

// Monte-Carlo target of an additive SEM: mean_out[i] = mean over draws of node `target` under intervention i.
// partial: m * sem_partial_blocks(n_draws) doubles of workspace.
int sem_partial_blocks(int64_t n_draws);
void launch_sem_target(hipStream_t s, const cbo_sem_spec &spec, const double *eps_cm, int64_t n_draws, int target,
                       int64_t m, int n_iv, const int *iv_nodes_host, const int *iv_nodes, const double *iv_values,
                       double *partial, double *mean_out);

}  // namespace cbo

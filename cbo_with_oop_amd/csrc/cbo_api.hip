// C-ABI host side of libcbo_hip.so (declared in include/cbo_hip.h): handle management, the jitchol
// retry ladder, candidate chunking, profiling events.  All arithmetic of the path runs in the HIP
// kernels of kernels_*.hip; there is no CPU fallback here.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <map>
#include <utility>
#include <vector>

#include "cbo_internal.h"
#include "hyper_prior.h"
#include "lml_outputs.h"
#include "schedule_tuner.h"

using namespace cbo;

static thread_local std::string g_err;
static std::atomic<uint64_t> g_fit_stamp{0};

static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
namespace cbo {
int set_error(int code, const std::string &msg) { return fail(code, msg); }
}

// Every context that cbo_init handed out and cbo_shutdown has not seen yet.  A context owns CU-masked streams
// (hipExtStreamCreateWithCUMask); when those are still alive while the HIP runtime runs its own exit handlers,
// tools that hook finalisation (rocprofv3) crash inside __cxa_finalize.  The first cbo_init therefore registers an
// atexit handler -- after the runtime's own, so it runs BEFORE them -- that shuts down whatever the caller left
// open: a C or ctypes consumer that exits without cbo_shutdown is safe too.  cbo_shutdown ignores handles that are
// not (or no longer) registered, which also makes a second call on the same handle harmless.
static std::mutex g_live_mutex;
static std::vector<cbo_ctx *> g_live;
static void shutdown_all_at_exit()
{
    for (;;) {
        cbo_ctx *c = nullptr;
        {
            std::lock_guard<std::mutex> lock(g_live_mutex);
            if (g_live.empty()) break;
            c = g_live.back();
        }
        cbo_shutdown(c);
    }
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(CBO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

constexpr size_t kStageBytes = 64 << 10;

enum Phase { PH_KXX = 0, PH_CHOL, PH_ALPHA, PH_KSTAR, PH_TRSM, PH_ACQ, PH_CONVERT, PH_COUNT };

struct EventPair {
    hipEvent_t a, b;
    int phase;
};

// A grow-only buffer of `cap` elements (device memory, or pinned host memory that the kernels read and write directly),
// resized only by grow() below and freed with its owner.  It converts to its pointer.
template <class T, bool Pinned = false>
struct GrowBuf {
    T *p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) Pinned ? hipHostFree(p) : hipFree(p); p = nullptr; cap = 0; }
};
template <class T>
using PinnedBuf = GrowBuf<T, true>;

struct cbo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;        // look-ahead stream of the Cholesky
    hipStream_t sweep_stream = nullptr;       // the sweep when it is pipelined with the factorisation (lower priority)
    hipStream_t bulk_stream = nullptr;        // its bulk updates (lowest priority)
    std::vector<hipEvent_t> chol_events;
    std::vector<hipEvent_t> pipe_events;      // factorisation -> sweep dependencies
    hipEvent_t ev_join = nullptr, ev_join2 = nullptr, ev_fork = nullptr;
    hipEvent_t region_a = nullptr, region_b = nullptr;
    double pipe_tail_frac = -1.0;    // CBO_HIP_PIPE_TAIL: rows (fraction) left to the closing left-looking launch; < 0 = automatic
    int pipe_group = 0;              // CBO_HIP_PIPE_GROUP: 1 = never grouped, G >= 2 = groups of G pairs, 0 = automatic
    int pipe_lead = -1;              // CBO_HIP_PIPE_LEAD: pairs alone ahead of the first group; < 0 = automatic
    CholOptions chol;                // the factorisation's launch forms
    int vec_solve_form = 2;          // CBO_HIP_VEC_SOLVE_FORM: 1 = the single-vector solves as per-block launches
    int n_cu = 256;
    int n_cu_pipe = 256;             // CUs the pipelined sweep's streams may use (the rest is kept for the factorisation)
    ScheduleTable schedule;          // (padded rows, padded candidates) -> measured schedule of cbo_gp_fit_sweep (schedule_tuner.h)
    int64_t fused_fallbacks = 0;     // factorisations repeated with separate launches after a fused launch gave up
    bool sweep_cache = true;         // CBO_HIP_SWEEP_CACHE=0: never reuse a candidate set's q, mu between sweeps
    bool small_sets = true;          // CBO_HIP_SMALL_SETS=0: cbo_acq_sweep_sets always takes the general path
    int sweep_mode = -1;             // CBO_HIP_SWEEP: 0 = always left-looking, 1 = always right-looking, else automatic
    int overlap_mode = -1;           // CBO_HIP_OVERLAP: 0 = cbo_gp_fit_sweep never overlaps, 1 = always, else automatic
    bool profiling = false;
    std::vector<EventPair> pending;
    EventPair pipe_cur{};                     // the launch pipe_mark is currently bracketing
    std::vector<hipEvent_t> pool;
    cbo_timers timers{};
    // sweep workspaces (grown on demand)
    GrowBuf<double> V;                                // the fp32 sweep's workspace too (as floats)
    GrowBuf<double> W;                                // -Ky^-1 for the likelihood gradients, L^-T V for the prediction's
    GrowBuf<double> gpart;
    GrowBuf<double> mupart;                           // fp32 sweep: per-row-tile partial sums of K*^T alpha
    // multi-set sweep of small models (cbo_acq_sweep_sets): descriptors, per-workgroup scratch, partial and final winners
    PinnedBuf<cbo_small_set> sets_host;                         // read by the kernel directly
    PinnedBuf<cbo_small_result> small_out;                      // written by the kernel directly
    GrowBuf<double> small_scratch;
    GrowBuf<double> small_part_val; GrowBuf<int64_t> small_part_idx;
    GrowBuf<int> small_info;                                    // cap / 2 status words + cap / 2 tickets (zero between calls)
    int small_seq = 0;                                          // sequence number of the last polled launch
    int polled_launches = 0;                                    // launches completed by polling since the last stream sync
    PinnedBuf<cbo_small_lml_result> lml_out;                    // written by small_lml_kernel
    PinnedBuf<cbo_small_lml_result> lml_batch_out;              // written by small_lml_batch_kernel
    PinnedBuf<cbo_small_loo_result> loo_out;                    // written by small_loo_batch_kernel
    int loo_route = 0;               // CBO_HIP_LOO_ROUTE: 1 = trailing-system chunks always, 2 = full-height chunks, else automatic
    // cbo_acq_sweep_hyper, cbo_acq_sweep_sets_hyper: the samples as the kernel reads them (pinned, every set's rows one
    // after the other), the general path's running sum [m_pad]
    PinnedBuf<double> hyper_host;
    PinnedBuf<HyperSet> hyper_sets_host;                        // cbo_acq_sweep_sets_hyper: one descriptor per set
    GrowBuf<double> hyper_sum;
    GrowBuf<double> hyper_lse_s;                                // the log form's S beside hyper_sum as M
    // cbo_acq_sweep_sets_mes, cbo_gp_mes_gumbel_sets: one (offset, count) per set and the sets' Gumbel samples as the kernel
    // reads them (pinned); the grids' mean / var workspace, every set's points one after the other; the bisections' table,
    // quantiles and status words
    PinnedBuf<cbo_small_aux> aux_host;
    PinnedBuf<const double *> cost_ptrs_host;                   // cbo_acq_sweep_sets_pointcost: every small set's cost vector
    PinnedBuf<double> mes_host;
    GrowBuf<double> gumbel_mean, gumbel_var, gumbel_out;
    GrowBuf<int64_t> gumbel_status;
    PinnedBuf<GumbelSet> gumbel_sets_host;
    int hyper_schedule = 0;          // CBO_HIP_HYPER_SCHEDULE: 1 = every workgroup factors every sample, 2 = two launches, else automatic
    GrowBuf<double> q, mu, mean, var, acq;                      // per candidate
    double *part_val = nullptr; int64_t *part_idx = nullptr;
    double *best_val = nullptr; int64_t *best_idx = nullptr;   // device
    double *h_best_val = nullptr; int64_t *h_best_idx = nullptr; // pinned host
    int *h_info = nullptr;
    // host-buffer entry points (cbo_gp_predict, _grouped, _gradients, cbo_acq_sweep_host) reuse ONE grow-only candidate
    // set instead of creating and destroying one per call; gradient / export scratch likewise
    cbo_cands *scratch_k = nullptr;
    GrowBuf<double> grads;
    GrowBuf<double> export_buf;
    GrowBuf<double> cov;                               // output of cbo_gp_predict_cov / cbo_gp_cov_between
    // cbo_gp_posterior_samples: the factor of Sigma in the factorisation's layout, its diagonal-tile inverses and status
    // words, the transposed normals, the samples (which first hold the uploaded normals)
    GrowBuf<double> samp_A, samp_invDt;
    GrowBuf<int> samp_info;
    GrowBuf<double> samp_Z, samp_out;
    GrowBuf<double> ivr_part;                          // cbo_gp_integrated_variance_reduction: [m][tiles] partials
    GrowBuf<double> con_terms;                         // cbo_acq_sweep_constrained: [n_con][m_pad] probabilities of feasibility
    GrowBuf<double> plugin_y;                          // cbo_acq_sweep_kind (MPEI), cbo_gp_plugin_incumbent: the incumbent, one double
    // cbo_acq_sweep_batch: the fantasy rows [batch_size - 1][m_pad], the working copy of q, the pivot column [n_pad], the
    // slice sums of the pass over V [kBatchMaxSlices][m_pad], the pick's scalars, and the winners (pinned: written by kernels)
    GrowBuf<double> batch_W, batch_q, batch_col, batch_part;
    // cbo_acq_sweep_sets_batch: every small set's V, W, q and mu (small_sets_batch_doubles), the winners [n_sets][batch_size]
    GrowBuf<double> sets_batch_scratch;
    PinnedBuf<double> sets_batch_h_vals; PinnedBuf<int64_t> sets_batch_h_idxs;
    // cbo_acq_refine_sets: the sets' search descriptors, starts and results as the kernel reads and writes them (pinned),
    // one status word per set
    PinnedBuf<cbo_small_refine> refine_host;
    PinnedBuf<double> refine_starts, refine_x, refine_grad, refine_val;
    PinnedBuf<int> refine_rounds, refine_status;
    GrowBuf<int> refine_info;
    PinnedBuf<cbo_small_refine_pair> refine_pair_host;  // cbo_acq_refine_sets_constrained: every model's own lengthscales
    // cbo_gp_hmc_sets: the chains' descriptors and draws as the kernel reads them, rows, accept flags, final states and
    // status words as it writes them (all pinned)
    PinnedBuf<cbo_small_hmc> hmc_host;
    PinnedBuf<double> hmc_draws, hmc_rows, hmc_final;
    PinnedBuf<int> hmc_accept, hmc_status;
    // cbo_gp_mle_sets: the runs' descriptors as the kernel reads them, final states, status words and rounds as it writes
    // them (all pinned); the runs' rings of curvature pairs (device)
    PinnedBuf<cbo_small_mle> mle_host;
    PinnedBuf<double> mle_final;
    PinnedBuf<int> mle_status, mle_rounds;
    GrowBuf<double> mle_rings;
    PinnedBuf<cbo_prior_item> prior_host;              // cbo_gp_log_prior_batch: one item per model, read and written by the kernel
    GrowBuf<double> append_part;                       // block append: slice sums of the pass over V [slices][kp][m_pad]
    GrowBuf<BatchState> batch_state;
    PinnedBuf<double> batch_h_vals; PinnedBuf<int64_t> batch_h_idxs;
    // small uploads (cbo_gp_upload_data / cbo_gp_set_data of a few KB, every trial of the reference's loop): one
    // pinned staging buffer the preparation kernel reads directly; `stage_done` guards its reuse
    double *stage = nullptr; hipEvent_t stage_done = nullptr; bool stage_pending = false;
    size_t max_ws_bytes = (size_t)32 << 30;   // V workspace cap: 288 GB of HBM per GPU, one chunk whenever possible
    char name[128] = {0};
};

struct cbo_gp {
    cbo_ctx *ctx = nullptr;
    int64_t n = 0, n_pad = 0, lda = 0;
    int d = 0;
    PointSet X;                      // scaled SoA coordinates
    double *raw = nullptr;           // staging for AoS upload (n*d)
    double *y = nullptr, *ls_dev = nullptr;
    std::vector<double> ls;          // per-dim lengthscales (ard) or single value
    std::vector<double> h_pv;        // host copy of prior variance (diag check of jitchol)
    KernelHyper h{};
    double noise_var = 0.0;
    double *A = nullptr;             // [n_pad][lda] Ky -> U, rhs strip at column n_pad
    double *invDt = nullptr;         // [n_pad/16][16][16]
    double *alpha = nullptr;         // [2*n_pad]
    double *z = nullptr;             // [n_pad] contiguous copy of L^-1 r
    int *info = nullptr;
    bool fitted = false;
    uint64_t fit_stamp = 0;          // unique per successful fit (0 = not fitted); candidates key their cache on it
    bool alpha_ready = false;
    int tries = 0;
    double jitter = 0.0;
    // append-only trial step: the fit this one extends by one observation, and what extending V needs
    uint64_t parent_stamp = 0;
    double append_d = 0.0, append_zn = 0.0;
    double *lvec = nullptr;          // [n_pad] the new column of U, contiguous
    cbo_cands *probe = nullptr;      // the appended point as a one-candidate set (scaled coordinates, prior)
    // cbo_gp_append_block: the last block, allocated on first use.  Two sides: a call builds its block on the side that
    // is not current and makes it current only when it commits, so a declined call leaves the last block's intact.
    int k_last = 1;                  // observations the last successful append added (1: cbo_gp_append)
    int blk_side = 0;                // the side that holds the last committed block
    int64_t blk_rows = 0;            // padded rows the buffers below were allocated for
    double *blk_mem = nullptr;       // everything below, one allocation
    double *blk_B[2] = {nullptr, nullptr};       // [n_pad][64]  B = L^-1 K(X, Xb)
    double *blk_L22[2] = {nullptr, nullptr};     // [64][64]     lower Cholesky factor of the Schur block
    double *blk_zb[2] = {nullptr, nullptr};      // [64]
    double *blk_y[2] = {nullptr, nullptr};       // [64]         the block's targets as uploaded
    double *blk_Kbb[2] = {nullptr, nullptr};     // [64][80]     K(Xb, Xb)
    double *blk_part = nullptr;                  // [64][65][64] slice sums of B^T B and B^T z
    int *blk_status = nullptr;                   // the Schur kernel's status word
    cbo_cands *blk_probe[2] = {nullptr, nullptr};   // the block's points as a candidate set (scaled coordinates, prior)
    // backward substitution through the forward kernel (prediction gradients of whole grids): the reversed factor and
    // its diagonal-tile inverses, built on first use after a fit; 1 / lengthscale per dimension (ARD)
    double *T = nullptr, *invT = nullptr, *inv_ls_dev = nullptr;
    uint64_t t_stamp = 0;
    // CBO_DTYPE_F32: fp32 copies of the factor for the sweep (kernels_f32.hip), refreshed by every successful fit
    int dtype = CBO_DTYPE_F64;
    int64_t n32 = 0, ldu32 = 0;
    float *Uf = nullptr, *invF = nullptr;
    uint64_t f32_stamp = 0;          // fit stamp the copies belong to
    // cbo_gp_set_priors: one descriptor per parameter (variance, lengthscale(s), noise variance), or empty -- no priors.
    // Nothing but cbo_gp_set_priors writes it: data, hyper-parameters and fits leave it alone.
    std::vector<cbo_hyper_prior> priors;
};

struct cbo_cands {
    cbo_ctx *ctx = nullptr;
    int64_t m = 0, m_pad = 0;
    int d = 0;
    int64_t cap_m_pad = 0; int cap_d = 0; bool cap_prior = false;      // what the buffers below can hold (grow-only)
    double *raw = nullptr;           // AoS (m,d) as uploaded
    double *pm = nullptr, *pv = nullptr;
    bool has_prior = false;          // pm / pv carry this set's prior closures (the buffers may outlive that)
    int64_t index_offset = 0;
    // scaled view for the GP it was last prepared for
    PointSet P;
    const cbo_gp *prepared_for = nullptr;
    std::vector<double> prepared_ls;
    // q = sum V^2 and mu = V^T z of the last sweep, valid while the model's fit stamp is the one recorded here:
    // between refits only the incumbent changes, and EI / cost / arg-max are recomputed from these two vectors
    GrowBuf<double> q, mu;
    uint64_t fit_stamp = 0;
    // cbo_cands_keep_solution: V = L^-1 K* stays resident so that an appended observation extends it by one row
    bool keep_v = false;
    double *V = nullptr;
    int64_t v_ld = 0, v_rows_cap = 0, v_rows = 0;
    uint64_t v_stamp = 0;
    double *partial = nullptr;       // [64][m_pad] slice sums of the row update
    // cbo_cands_set_cost: c(x_j) of every raw point under the table it was formed from; has_cost falls
    // wherever the raw points are replaced (cands_describe: only the context's scratch sets are ever refilled)
    GrowBuf<double> cost;
    CostTable cost_table{};
    bool has_cost = false;
};

// b to at least n elements (nothing happens when they fit): an old buffer is freed only after the queued work that may
// read it is done.  A failed allocation leaves b empty and is cleared from the runtime's error state, where it would
// otherwise fail the next call's launch check.  zero: a new buffer is cleared.
template <class T, bool Pinned>
static int grow(cbo_ctx *c, GrowBuf<T, Pinned> &b, size_t n, bool zero = false)
{
    if (n <= b.cap) return CBO_OK;
    if (b.p) HIP_TRY(hipStreamSynchronize(c->stream));
    b.release();
    void *p = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&p, sizeof(T) * n) : hipMalloc(&p, sizeof(T) * n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CBO_ERR_HIP, std::string(Pinned ? "hipHostMalloc" : "hipMalloc") + " of " +
                                     std::to_string(sizeof(T) * n) + " bytes: " + hipGetErrorString(e));
    }
    b.p = static_cast<T *>(p);
    b.cap = n;
    if (zero && Pinned) std::memset(p, 0, sizeof(T) * n);
    if (zero && !Pinned) HIP_TRY(hipMemset(p, 0, sizeof(T) * n));
    return CBO_OK;
}

// ---- profiling helpers ---------------------------------------------------------------------------
static hipEvent_t get_event(cbo_ctx *c)
{
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreateWithFlags(&e, hipEventDisableSystemFence);   // device-scope ordering is all the stream needs
    return e;
}

struct PhaseScope {
    cbo_ctx *c;
    EventPair p{};
    bool on;
    hipStream_t st;
    PhaseScope(cbo_ctx *ctx, int phase, hipStream_t stream = nullptr)
        : c(ctx), on(ctx->profiling), st(stream ? stream : ctx->stream)
    {
        if (on) {
            p.a = get_event(c);
            p.b = get_event(c);
            p.phase = phase;
            hipEventRecord(p.a, st);
        }
    }
    ~PhaseScope()
    {
        if (on) {
            hipEventRecord(p.b, st);
            c->pending.push_back(p);
        }
    }
};

static void resolve_events(cbo_ctx *c)
{
    if (c->pending.empty()) return;
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->sweep_stream);
    hipStreamSynchronize(c->bulk_stream);
    for (auto &p : c->pending) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, p.a, p.b);
        switch (p.phase) {
            case PH_KXX: c->timers.ms_kxx += ms; break;
            case PH_CHOL: c->timers.ms_chol += ms; break;
            case PH_ALPHA: c->timers.ms_alpha += ms; break;
            case PH_KSTAR: c->timers.ms_kstar += ms; break;
            case PH_TRSM: c->timers.ms_trsm += ms; break;
            case PH_ACQ: c->timers.ms_acq += ms; break;
            case PH_CONVERT: c->timers.ms_f32_convert += ms; break;
        }
        c->pool.push_back(p.a);
        c->pool.push_back(p.b);
    }
    c->pending.clear();
}

// ---- context -------------------------------------------------------------------------------------
static void destroy_ctx(cbo_ctx *c);

extern "C" int cbo_abi_version(void) { return CBO_HIP_ABI_VERSION; }
extern "C" const char *cbo_last_error(void) { return g_err.c_str(); }

extern "C" int cbo_device_count(int *count_out)
{
    if (!count_out) return fail(CBO_ERR_INVALID, "count_out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count_out = n;
    return CBO_OK;
}

extern "C" int cbo_init(int device_id, cbo_ctx **out)
{
    if (!out) return fail(CBO_ERR_INVALID, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(CBO_ERR_NO_DEVICE, "no HIP device visible: libcbo_hip has no CPU fallback");
    }
    if (device_id < 0 || device_id >= n) return fail(CBO_ERR_INVALID, "device_id out of range");
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CBO_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName +
                                           ", this library carries gfx950 code objects only");
    cbo_ctx *c = new cbo_ctx();
    c->device = device_id;
    std::snprintf(c->name, sizeof(c->name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    // the factorisation's streams outrank the sweep stream: its kernels are short, few and on the critical path
    int prio_low = 0, prio_high = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_high);
    // The look-ahead stream of the factorisation carries the bulk trailing updates: an ordinary stream one priority below
    // the chain's (keeping CUs away from it, or raising it to the chain's priority, measured neutral to -4 %: NOTES.md).
    if (e == hipSuccess)
        e = hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, (prio_low + prio_high) / 2);
    // The sweep streams leave a few CUs per XCD to the factorisation: its diagonal-block kernel needs a whole
    // CU's LDS and would otherwise wait behind a queue of half-LDS sweep workgroups that keep every CU partly
    // occupied.  CU-mask bit b is CU b/8 of XCD b%8 on this device (scripts/probes/cumask_probe.hip).  Four CUs per XCD
    // measured best of 2-10 (profiles/r04_reserve_scan.txt).
    if (e == hipSuccess) {
        constexpr int reserve = 4;
        const int n_cu = prop.multiProcessorCount;
        std::vector<uint32_t> mask((size_t)(n_cu + 31) / 32, 0u);
        for (int b = 0; b < n_cu; ++b)
            if (b / 8 >= reserve) mask[(size_t)b / 32] |= 1u << (b % 32);
        bool masked = false;
        c->n_cu_pipe = n_cu;
        if (reserve * 8 < n_cu) {
            masked = hipExtStreamCreateWithCUMask(&c->sweep_stream, (uint32_t)mask.size(), mask.data()) == hipSuccess &&
                     hipExtStreamCreateWithCUMask(&c->bulk_stream, (uint32_t)mask.size(), mask.data()) == hipSuccess;
            if (masked) c->n_cu_pipe = n_cu - reserve * 8;
            if (!masked) {                       // no CU masking on this stack: plain lower-priority streams instead
                (void)hipGetLastError();
                if (c->sweep_stream) { hipStreamDestroy(c->sweep_stream); c->sweep_stream = nullptr; }
                if (c->bulk_stream) { hipStreamDestroy(c->bulk_stream); c->bulk_stream = nullptr; }
            }
        }
        if (!masked) {
            e = hipStreamCreateWithPriority(&c->sweep_stream, hipStreamNonBlocking, (prio_low + prio_high) / 2);
            if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->bulk_stream, hipStreamNonBlocking, prio_low);
        }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming | hipEventDisableSystemFence);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming | hipEventDisableSystemFence);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence);
    if (e == hipSuccess) e = hipMalloc(&c->part_val, 2048 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&c->part_idx, 2048 * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc(&c->best_val, sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&c->best_idx, sizeof(int64_t));
    if (e == hipSuccess) e = hipHostMalloc(&c->h_best_val, sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc(&c->h_best_idx, sizeof(int64_t));
    if (e == hipSuccess) e = hipHostMalloc(&c->h_info, sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc(&c->stage, kStageBytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->stage_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        destroy_ctx(c);
        return fail(CBO_ERR_HIP, std::string("cbo_init: ") + hipGetErrorString(e));
    }
    const char *ws = std::getenv("CBO_HIP_WORKSPACE_MB");
    if (ws) c->max_ws_bytes = (size_t)std::atoll(ws) << 20;
    c->n_cu = prop.multiProcessorCount;
    const char *sm = std::getenv("CBO_HIP_SWEEP");
    if (sm) c->sweep_mode = std::atoi(sm);
    const char *lr = std::getenv("CBO_HIP_LOO_ROUTE");
    if (lr) c->loo_route = std::atoi(lr);
    const char *hs = std::getenv("CBO_HIP_HYPER_SCHEDULE");
    if (hs) c->hyper_schedule = std::atoi(hs);
    const char *sc = std::getenv("CBO_HIP_SWEEP_CACHE");
    if (sc && std::atoi(sc) == 0) c->sweep_cache = false;
    const char *ss = std::getenv("CBO_HIP_SMALL_SETS");
    if (ss && std::atoi(ss) == 0) c->small_sets = false;
    const char *om = std::getenv("CBO_HIP_OVERLAP");
    if (om) c->overlap_mode = std::atoi(om);
    const char *tf = std::getenv("CBO_HIP_PIPE_TAIL");
    if (tf) c->pipe_tail_frac = std::atof(tf);
    // (groups beyond 4 pairs -- K = 1024 -- are not covered by the tests: clamped)
    const char *pg = std::getenv("CBO_HIP_PIPE_GROUP");
    if (pg) c->pipe_group = std::min(std::max(std::atoi(pg), 0), 4);
    const char *pl = std::getenv("CBO_HIP_PIPE_LEAD");
    if (pl) c->pipe_lead = std::atoi(pl);
    const char *pf = std::getenv("CBO_HIP_PANEL_FORM");
    if (pf && (std::atoi(pf) == 2 || std::atoi(pf) == 5)) c->chol.panel_form = std::atoi(pf);     // any other value means 4
    const char *sl = std::getenv("CBO_HIP_FUSED_SPIN_LIMIT");
    if (sl) c->chol.spin_limit = std::atoi(sl);
    const char *bg = std::getenv("CBO_HIP_BULK_GROUP");
    if (bg) c->chol.bulk_group = std::atoi(bg);
    const char *g4 = std::getenv("CBO_HIP_BULK_GROUP4_ROWS");
    if (g4) c->chol.group4_rows = std::atoi(g4);
    const char *vf = std::getenv("CBO_HIP_VEC_SOLVE_FORM");
    if (vf) c->vec_solve_form = std::atoi(vf);
    {
        static std::once_flag once;
        std::call_once(once, [] { std::atexit(shutdown_all_at_exit); });
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live.push_back(c);
    }
    *out = c;
    return CBO_OK;
}

namespace cbo {
hipStream_t ctx_stream(cbo_ctx *c) { return c->stream; }
int ctx_device(cbo_ctx *c) { return c->device; }
}

extern "C" void cbo_shutdown(cbo_ctx *c)
{
    if (!c) return;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        auto it = std::find(g_live.begin(), g_live.end(), c);
        if (it == g_live.end()) return;              // already shut down (or never ours): the pointer is not touched
        g_live.erase(it);
    }
    destroy_ctx(c);
}

// (the grow-only buffers go with `delete c`)
static void destroy_ctx(cbo_ctx *c)
{
    hipSetDevice(c->device);
    if (c->scratch_k) { cbo_cands_destroy(c->scratch_k); c->scratch_k = nullptr; }
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto &p : c->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto e : c->pool) hipEventDestroy(e);
    hipFree(c->part_val); hipFree(c->part_idx); hipFree(c->best_val); hipFree(c->best_idx);
    hipHostFree(c->h_best_val); hipHostFree(c->h_best_idx); hipHostFree(c->h_info); hipHostFree(c->stage);
    if (c->stage_done) hipEventDestroy(c->stage_done);
    for (auto e : c->chol_events) hipEventDestroy(e);
    for (auto e : c->pipe_events) hipEventDestroy(e);
    if (c->region_a) hipEventDestroy(c->region_a);
    if (c->region_b) hipEventDestroy(c->region_b);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->ev_join2) hipEventDestroy(c->ev_join2);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->sweep_stream) hipStreamDestroy(c->sweep_stream);
    if (c->bulk_stream) hipStreamDestroy(c->bulk_stream);
    if (c->side_stream) hipStreamDestroy(c->side_stream);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int cbo_synchronize(cbo_ctx *c)
{
    if (!c) return fail(CBO_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());            // every stream of the device, the communicator's included
    return CBO_OK;
}

extern "C" int cbo_set_profiling(cbo_ctx *c, int enabled)
{
    if (!c) return fail(CBO_ERR_INVALID, "ctx is NULL");
    c->profiling = enabled != 0;
    return CBO_OK;
}

extern "C" int cbo_reset_timers(cbo_ctx *c)
{
    if (!c) return fail(CBO_ERR_INVALID, "ctx is NULL");
    resolve_events(c);
    c->timers = cbo_timers{};
    return CBO_OK;
}

extern "C" int cbo_get_timers(cbo_ctx *c, cbo_timers *out)
{
    if (!c || !out) return fail(CBO_ERR_INVALID, "NULL argument");
    resolve_events(c);
    *out = c->timers;
    return CBO_OK;
}

// One event pair on the main stream around a region of calls: device time of the region whatever runs inside
// (several streams join the main stream before every call returns).
extern "C" int cbo_region_begin(cbo_ctx *c)
{
    if (!c) return fail(CBO_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->region_a) {
        HIP_TRY(hipEventCreate(&c->region_a));
        HIP_TRY(hipEventCreate(&c->region_b));
    }
    HIP_TRY(hipEventRecord(c->region_a, c->stream));
    return CBO_OK;
}

extern "C" int cbo_region_end(cbo_ctx *c, double *ms_out)
{
    if (!c || !ms_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (!c->region_a) return fail(CBO_ERR_INVALID, "cbo_region_end without cbo_region_begin");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->region_b, c->stream));
    HIP_TRY(hipEventSynchronize(c->region_b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->region_a, c->region_b));
    *ms_out = ms;
    return CBO_OK;
}

extern "C" int cbo_device_name(cbo_ctx *c, char *buf, int buflen)
{
    if (!c || !buf || buflen <= 0) return fail(CBO_ERR_INVALID, "NULL argument");
    std::snprintf(buf, (size_t)buflen, "%s", c->name);
    return CBO_OK;
}

// ---- GP ------------------------------------------------------------------------------------------
static void free_gp_data(cbo_gp *g)
{
    hipFree(g->X.xs); hipFree(g->X.sq); hipFree(g->X.sv); hipFree(g->X.pm); hipFree(g->X.pv);
    hipFree(g->raw); hipFree(g->y); hipFree(g->A); hipFree(g->invDt); hipFree(g->alpha); hipFree(g->z); hipFree(g->lvec);
    hipFree(g->Uf); hipFree(g->invF); hipFree(g->T); hipFree(g->invT);
    g->Uf = g->invF = nullptr; g->f32_stamp = 0;
    g->T = g->invT = nullptr; g->t_stamp = 0;
    g->X = PointSet{};
    g->raw = g->y = g->A = g->invDt = g->alpha = g->z = g->lvec = nullptr;
    g->parent_stamp = 0;
    g->n = g->n_pad = 0;             // no storage: every entry point that needs data checks g->n
    g->fitted = false;
}

// X (n, d) | y | prior mean | prior variance into the context's pinned staging buffer once the kernel that read it last is
// done, and the model's host copy of the prior variance
static int stage_data(cbo_gp *g, int64_t n, const double *X, const double *y, const double *pm, const double *pv)
{
    cbo_ctx *c = g->ctx;
    if (c->stage_pending) { HIP_TRY(hipEventSynchronize(c->stage_done)); c->stage_pending = false; }
    double *st = c->stage;
    std::memcpy(st, X, sizeof(double) * n * g->d);
    std::memcpy(st + n * g->d, y, sizeof(double) * n);
    g->h_pv.clear();
    if (pv) {
        std::memcpy(st + n * g->d + n, pm, sizeof(double) * n);
        std::memcpy(st + n * g->d + 2 * n, pv, sizeof(double) * n);
        g->h_pv.assign(pv, pv + n);
    }
    return CBO_OK;
}

static int upload_gp_data(cbo_gp *g, int64_t n, const double *X, const double *y, const double *pm, const double *pv)
{
    cbo_ctx *c = g->ctx;
    if (n <= 0 || !X || !y) return fail(CBO_ERR_INVALID, "n must be positive and X, y non-NULL");
    if ((pm == nullptr) != (pv == nullptr))
        return fail(CBO_ERR_INVALID, "prior mean and prior variance must be given together");
    if (n > ((int64_t)1 << 30)) return fail(CBO_ERR_INVALID, "n too large");
    const int64_t n_pad = round_up(n, kPadN);
    if (n_pad != g->n_pad || (pv != nullptr) != (g->X.sv != nullptr)) {
        free_gp_data(g);
        g->lda = n_pad + kRhsCols + kLdExtra;
        HIP_TRY(hipMalloc(&g->X.xs, sizeof(double) * g->d * n_pad));
        HIP_TRY(hipMalloc(&g->X.sq, sizeof(double) * n_pad));
        if (pv) {
            HIP_TRY(hipMalloc(&g->X.sv, sizeof(double) * n_pad));
            HIP_TRY(hipMalloc(&g->X.pm, sizeof(double) * n_pad));
            HIP_TRY(hipMalloc(&g->X.pv, sizeof(double) * n_pad));
        }
        HIP_TRY(hipMalloc(&g->raw, sizeof(double) * n_pad * g->d));
        HIP_TRY(hipMalloc(&g->y, sizeof(double) * n_pad));
        HIP_TRY(hipMalloc(&g->A, sizeof(double) * n_pad * g->lda));
        HIP_TRY(hipMalloc(&g->invDt, sizeof(double) * (n_pad / 16) * 256));
        HIP_TRY(hipMalloc(&g->alpha, sizeof(double) * 2 * n_pad));
        HIP_TRY(hipMalloc(&g->z, sizeof(double) * n_pad));
        HIP_TRY(hipMalloc(&g->lvec, sizeof(double) * n_pad));
        if (g->dtype == CBO_DTYPE_F32) {
            g->n32 = round_up(n_pad, kPadN32);
            g->ldu32 = g->n32 + 32;
            HIP_TRY(hipMalloc(&g->Uf, sizeof(float) * (size_t)g->n32 * (size_t)g->ldu32));
            HIP_TRY(hipMalloc(&g->invF, sizeof(float) * (size_t)(g->n32 / 16) * 256));
        }
        g->n_pad = n_pad;            // only now: a failed allocation above leaves the handle empty (n_pad == 0)
    }
    g->n = n;
    g->X.n = n; g->X.ld = n_pad; g->X.d = g->d;
    g->fitted = false;
    const size_t stage_need = sizeof(double) * (size_t)(n * g->d + n + (pv ? 2 * n : 0));
    if (stage_need <= kStageBytes) {
        // small upload: host arrays -> pinned staging -> ONE kernel that reads the staging buffer itself.  The
        // caller's buffers are free as soon as they are copied here; nothing to wait for on the stream.
        const int rc = stage_data(g, n, X, y, pm, pv);
        if (rc != CBO_OK) return rc;
        launch_prep_points_staged(c->stream, c->stage, n, g->d, g->h.ard ? g->ls_dev : nullptr, pv != nullptr, g->raw, g->y,
                                  g->X.pm, g->X.pv, g->X.xs, n_pad, g->X.sq, g->X.sv);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->stage_done, c->stream));
        c->stage_pending = true;
        return CBO_OK;
    }
    HIP_TRY(hipMemcpyAsync(g->raw, X, sizeof(double) * n * g->d, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(g->y, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    g->h_pv.clear();
    if (pv) {
        HIP_TRY(hipMemcpyAsync(g->X.pm, pm, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(g->X.pv, pv, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        g->h_pv.assign(pv, pv + n);
    }
    launch_prep_points(c->stream, g->raw, n, g->d, g->h.ard ? g->ls_dev : nullptr, pv ? g->X.pv : nullptr, g->X.xs,
                       n_pad, g->X.sq, g->X.sv);
    HIP_TRY(hipGetLastError());
    // host buffers are the caller's: make sure the copies are done before returning
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

extern "C" int cbo_gp_create(cbo_ctx *c, int dtype, int64_t n, int d, const double *X, const double *y,
                             const double *pm, const double *pv, double variance, const double *lengthscale,
                             int ard, double noise_var, int zero_diag, cbo_gp **out)
{
    if (!c || !out || !lengthscale) return fail(CBO_ERR_INVALID, "NULL argument");
    if (dtype != CBO_DTYPE_F64 && dtype != CBO_DTYPE_F32) return fail(CBO_ERR_INVALID, "dtype must be CBO_DTYPE_F64 or CBO_DTYPE_F32");
    if (d < 1 || d > CBO_MAX_DIM) return fail(CBO_ERR_INVALID, "d must be in [1, CBO_MAX_DIM]");
    HIP_TRY(hipSetDevice(c->device));
    cbo_gp *g = new cbo_gp();
    g->ctx = c;
    g->d = d;
    g->dtype = dtype;
    g->noise_var = noise_var;
    g->h.variance = variance;
    g->h.ard = ard ? 1 : 0;
    g->h.zero_diag = zero_diag ? 1 : 0;
    g->h.lengthscale = ard ? 1.0 : lengthscale[0];
    g->ls.assign(lengthscale, lengthscale + (ard ? d : 1));
    if (hipMalloc(&g->info, sizeof(int) * (1 + kCholFlagSlots)) != hipSuccess) { delete g; return fail(CBO_ERR_HIP, "hipMalloc info"); }
    if (ard) {
        if (hipMalloc(&g->ls_dev, sizeof(double) * d) != hipSuccess ||
            hipMemcpy(g->ls_dev, lengthscale, sizeof(double) * d, hipMemcpyHostToDevice) != hipSuccess) {
            cbo_gp_destroy(g);
            return fail(CBO_ERR_HIP, "hipMalloc/hipMemcpy lengthscales");
        }
    }
    const int rc = upload_gp_data(g, n, X, y, pm, pv);
    if (rc != CBO_OK) { cbo_gp_destroy(g); return rc; }
    *out = g;
    return CBO_OK;
}

extern "C" void cbo_gp_destroy(cbo_gp *g)
{
    if (g && g->probe) { cbo_cands_destroy(g->probe); g->probe = nullptr; }
    if (!g) return;
    for (cbo_cands *&p : g->blk_probe)
        if (p) { cbo_cands_destroy(p); p = nullptr; }
    hipSetDevice(g->ctx->device);
    hipStreamSynchronize(g->ctx->stream);
    hipFree(g->blk_mem);
    free_gp_data(g);
    hipFree(g->info);
    hipFree(g->ls_dev); hipFree(g->inv_ls_dev);
    delete g;
}

extern "C" int64_t cbo_gp_n(const cbo_gp *g) { return g ? g->n : -1; }
extern "C" int cbo_gp_dtype(const cbo_gp *g) { return g ? g->dtype : -1; }

extern "C" int cbo_gp_jitter(const cbo_gp *g, int *tries_out, double *jitter_out)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    if (tries_out) *tries_out = g->tries;
    if (jitter_out) *jitter_out = g->jitter;
    return CBO_OK;
}

// the factorisation's launch forms for one attempt: `separate` = the repeat after a fused diagonal + panel launch gave up
// (kCholFusedTimeout), with the separate-launch kernels whatever CBO_HIP_PANEL_FORM says
static CholOptions chol_options(const cbo_ctx *c, bool separate)
{
    CholOptions o = c->chol;
    if (separate) o.panel_form = 2;
    return o;
}

static void enqueue_factor(cbo_gp *g, double jitter, bool separate)
{
    cbo_ctx *c = g->ctx;
    {
        PhaseScope ps(c, PH_KXX);
        launch_kxx(c->stream, g->X, g->h, g->noise_var + kGpyDiagJitter, jitter, g->A, g->lda, g->n_pad);
        launch_rhs(c->stream, g->y, g->X.pm, g->n, g->A, g->lda, g->n_pad, g->info, cholesky_info_ints(g->n_pad));
    }
    {
        PhaseScope ps(c, PH_CHOL);
        launch_cholesky(c->stream, c->side_stream, c->chol_events, g->A, g->lda, g->n_pad, g->invDt, g->info,
                        chol_options(c, separate), nullptr, true);
    }
}

// GPy util.linalg.jitchol after a failed attempt: first `base` (1e-6 mean(diag)), then x10 per retry, at most 5
// retries.  false: the ladder is exhausted (the caller reports CBO_ERR_NOT_PD).
static bool jitter_step(double base, int *tries, double *jitter)
{
    *jitter = *tries == 0 ? base : *jitter * 10.0;
    ++*tries;
    return *tries <= 5 && std::isfinite(*jitter);
}

// the next jitter of the model's own ladder, whose base is 1e-6 mean(diag Ky)
static int next_jitter(cbo_gp *g, int *tries, double *jitter)
{
    double base = 0.0;
    if (*tries == 0) {
        // diag of Ky as assembled (jitter-free): variance + v_i + (noise + 1e-8); the kernel's own
        // diagonal differs from this only when zero_diag is off and |x|^2 rounds differently from
        // x.x, i.e. by O(1e-16) relative -- irrelevant for a 1e-6 * mean(diag) jitter.
        // (summed in extended precision and rounded once: numpy's pairwise diagA.mean() is exact for n equal entries,
        //  a sequential double sum of 16384 of them is 4e-13 off)
        long double sum = 0.0L;
        bool nonpos = false;
        for (int64_t i = 0; i < g->n; ++i) {
            const double dv = g->h.variance + (g->h_pv.empty() ? 0.0 : g->h_pv[i]) + (g->noise_var + kGpyDiagJitter);
            if (!(dv > 0.0)) nonpos = true;
            sum += (long double)dv;
        }
        if (nonpos) return fail(CBO_ERR_NONPOS_DIAG, "not pd: non-positive diagonal elements");
        base = (double)(sum / (long double)g->n) * 1e-6;
    }
    if (!jitter_step(base, tries, jitter)) return fail(CBO_ERR_NOT_PD, "not positive definite, even with jitter.");
    return CBO_OK;
}

// one attempt at a factorisation: enqueue(separate) queues it on c->stream (separate: see chol_options), info is its
// device status word; *pd says whether it went through
template <class Enqueue>
static int attempt_factor(cbo_ctx *c, const int *info, Enqueue enqueue, bool *pd)
{
    for (bool separate = false;;) {
        enqueue(separate);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_info, info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (*c->h_info == kCholFusedTimeout) {
            // a strip of a fused diagonal + panel launch gave up waiting (see potrf_panel_fused_kernel): the same
            // attempt again with the separate-launch kernels -- same bits, no protocol between workgroups
            if (separate)
                return fail(CBO_ERR_HIP, "a fused diagonal + panel launch gave up waiting, and so did the separate-launch repeat");
            separate = true;
            ++c->fused_fallbacks;
            continue;
        }
        *pd = *c->h_info == 0;
        return CBO_OK;
    }
}

// the model is fitted from here on, at `tries` steps of the jitter ladder: a new stamp for every cache keyed on the fit
static void mark_fitted(cbo_gp *g, int tries, double jitter)
{
    g->fitted = true;
    g->fit_stamp = ++g_fit_stamp;
    g->parent_stamp = 0;
    g->alpha_ready = false;
    g->tries = tries;
    g->jitter = jitter;
    if (g->ctx->profiling) g->ctx->timers.n_fit += 1;
}

// the factor in g->A is the model's: what every consumer of a fitted model expects beside it
static int adopt_factor(cbo_gp *g, int tries, double jitter)
{
    cbo_ctx *c = g->ctx;
    // contiguous z = L^-1 (y - m) for the sweep: the posterior mean is (L^-1 k*)^T z, so the backward
    // solve for alpha = L^-T z is not on the sweep's path and is materialised on first use (ensure_alpha)
    HIP_TRY(hipMemcpy2DAsync(g->z, sizeof(double), g->A + g->n_pad, sizeof(double) * g->lda, sizeof(double),
                             (size_t)g->n_pad, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipGetLastError());
    mark_fitted(g, tries, jitter);
    return CBO_OK;
}

extern "C" int cbo_gp_fit(cbo_gp *g, int *tries_out, double *jitter_out)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "gp holds no data (a previous upload failed)");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    g->fitted = false;
    // GPy util.linalg.jitchol: plain attempt, then mean(diag)*1e-6 jitter, x10 per retry, <= 5 retries.
    double jitter = 0.0;
    int tries = 0;
    for (;;) {
        bool pd = false;
        int rc = attempt_factor(c, g->info, [&](bool separate) { enqueue_factor(g, jitter, separate); }, &pd);
        if (rc != CBO_OK) return rc;
        if (pd) break;
        rc = next_jitter(g, &tries, &jitter);
        if (rc != CBO_OK) return rc;
    }
    const int rc = adopt_factor(g, tries, jitter);
    if (rc != CBO_OK) return rc;
    if (tries_out) *tries_out = tries;
    if (jitter_out) *jitter_out = jitter;
    return CBO_OK;
}

// The jitter of level `level` of jitchol's ladder (0: none; k: mean(diag) * 1e-6 * 10^(k-1), by the same repeated
// multiplication as the retries of cbo_gp_fit): CBO_ERR_NONPOS_DIAG / CBO_ERR_NOT_PD as the ladder reports them.
static int ladder_jitter(cbo_gp *g, int level, double *jitter)
{
    *jitter = 0.0;
    int tries = 0;
    while (tries < level) {
        const int rc = next_jitter(g, &tries, jitter);
        if (rc != CBO_OK) return rc;
    }
    return CBO_OK;
}

// ONE level of the ladder, for ranks that walk it side by side (cbo_with_oop_amd/sharding.py, fit_over_ranks: with the
// posterior replicated on G ranks, rank r tries level r while the others try theirs, instead of every rank trying them
// all in turn).  *status: 1 = factored at this level (the model is fitted, tries = level), 0 = not positive definite at
// this level, -1 = the diagonal has non-positive entries (jitchol gives up before its first retry: levels >= 1 only).
// A level beyond jitchol's five retries is CBO_ERR_NOT_PD.
extern "C" int cbo_gp_fit_level(cbo_gp *g, int level, int *status, double *jitter_out)
{
    if (!g || !status) return fail(CBO_ERR_INVALID, "NULL argument");
    if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "gp holds no data (a previous upload failed)");
    if (level < 0) return fail(CBO_ERR_INVALID, "level must be >= 0");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    g->fitted = false;
    double jitter = 0.0;
    int rc = ladder_jitter(g, level, &jitter);
    if (rc == CBO_ERR_NONPOS_DIAG) { *status = -1; return CBO_OK; }
    if (rc != CBO_OK) return rc;
    bool pd = false;
    rc = attempt_factor(c, g->info, [&](bool separate) { enqueue_factor(g, jitter, separate); }, &pd);
    if (rc != CBO_OK) return rc;
    *status = pd ? 1 : 0;
    if (jitter_out) *jitter_out = jitter;
    return pd ? adopt_factor(g, level, jitter) : CBO_OK;
}

// for cbo_comm_share_factor (cbo_comm.hip): where the factor lives, and its adoption by a rank that received it
namespace cbo {
int gp_factor_view(cbo_gp *g, double **A, int64_t *lda, int64_t *n_pad, double **invDt, cbo_ctx **ctx)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "gp holds no data");
    *A = g->A; *lda = g->lda; *n_pad = g->n_pad; *invDt = g->invDt; *ctx = g->ctx;
    return CBO_OK;
}
bool gp_is_fitted_at(const cbo_gp *g, int level) { return g && g->fitted && g->tries == level; }
int gp_adopt_received_factor(cbo_gp *g, int level)
{
    HIP_TRY(hipSetDevice(g->ctx->device));
    double jitter = 0.0;
    const int rc = ladder_jitter(g, level, &jitter);
    if (rc != CBO_OK) return rc;
    return adopt_factor(g, level, jitter);
}
}  // namespace cbo

// GPy's woodbury_vector alpha = Ky^-1 (y - m) = L^-T z (dpotrs): needed by posterior export and by
// prediction gradients, not by predict / the acquisition sweep.
static int ensure_alpha(cbo_gp *g)
{
    if (g->alpha_ready) return CBO_OK;
    cbo_ctx *c = g->ctx;
    bool chained;
    {
        PhaseScope ps(c, PH_ALPHA);
        // one launch (a chain of workgroups); the per-block launches where that form does not apply
        chained = launch_backsolve_chain(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->A + g->n_pad, g->lda,
                                         g->alpha + g->n_pad, g->alpha, g->info, c->chol.spin_limit, c->vec_solve_form);
        if (!chained) launch_backsolve(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->alpha);
    }
    HIP_TRY(hipGetLastError());
    if (chained) {
        // the chain's polls are bounded: a give-up is in the status word, and the solve is repeated the old way
        HIP_TRY(hipMemcpyAsync(c->h_info, g->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (*c->h_info != 0) {
            HIP_TRY(hipMemsetAsync(g->info, 0, sizeof(int), c->stream));
            ++c->fused_fallbacks;
            PhaseScope ps(c, PH_ALPHA);
            launch_backsolve(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->alpha);
            HIP_TRY(hipGetLastError());
        }
    }
    g->alpha_ready = true;
    return CBO_OK;
}

extern "C" int cbo_gp_set_data(cbo_gp *g, int64_t n, const double *X, const double *y, const double *pm,
                               const double *pv)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    HIP_TRY(hipSetDevice(g->ctx->device));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    const int rc = upload_gp_data(g, n, X, y, pm, pv);
    if (rc != CBO_OK) return rc;
    return cbo_gp_fit(g, nullptr, nullptr);
}

extern "C" int cbo_gp_upload_data(cbo_gp *g, int64_t n, const double *X, const double *y, const double *pm,
                                  const double *pv)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    HIP_TRY(hipSetDevice(g->ctx->device));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    return upload_gp_data(g, n, X, y, pm, pv);      // leaves the model unfitted
}

extern "C" int cbo_gp_get_posterior(cbo_gp *g, double *L_out, double *alpha_out)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (L_out) {
        int rc = grow(c, c->export_buf, (size_t)g->n * (size_t)g->n);
        if (rc != CBO_OK) return rc;
        launch_export_lower(c->stream, g->A, g->lda, g->n, c->export_buf);
        HIP_TRY(hipMemcpyAsync(L_out, c->export_buf, sizeof(double) * g->n * g->n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (alpha_out) {
        const int rc = ensure_alpha(g);
        if (rc != CBO_OK) return rc;
        HIP_TRY(hipMemcpyAsync(alpha_out, g->alpha, sizeof(double) * g->n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CBO_OK;
}

extern "C" int cbo_gp_assemble_kxx(cbo_gp *g, double *K_out)
{
    if (!g || !K_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "gp holds no data (a previous upload failed)");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    // scratch: [n_pad x lda] assembly + [n x n] symmetric export, from the context's grow-only export buffer
    const size_t a_elems = (size_t)g->n_pad * (size_t)g->lda;
    int rc = grow(c, c->export_buf, a_elems + (size_t)g->n * (size_t)g->n);
    if (rc != CBO_OK) return rc;
    double *Atmp = c->export_buf, *tmp = c->export_buf + a_elems;
    launch_kxx(c->stream, g->X, g->h, g->noise_var + kGpyDiagJitter, 0.0, Atmp, g->lda, g->n_pad);
    launch_export_sym(c->stream, Atmp, g->lda, g->n, tmp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(K_out, tmp, sizeof(double) * g->n * g->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

// ---- candidates ----------------------------------------------------------------------------------
// buffers for m points of dimension d (with prior closures if `prior`): grow-only, nothing happens when they fit
static int cands_reserve(cbo_cands *k, int64_t m, int d, bool prior)
{
    cbo_ctx *c = k->ctx;
    const int64_t m_pad = round_up(m, kStrip);
    if (m_pad > k->cap_m_pad || d > k->cap_d || (prior && !k->cap_prior)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int64_t cap = m_pad > k->cap_m_pad ? m_pad : k->cap_m_pad;
        const int cd = d > k->cap_d ? d : k->cap_d;
        const bool cp = prior || k->cap_prior;
        hipFree(k->raw); hipFree(k->P.xs); hipFree(k->P.sq); hipFree(k->P.sv); hipFree(k->pm); hipFree(k->pv);
        k->q.release(); k->mu.release(); k->cost.release();
        k->raw = k->P.xs = k->P.sq = k->P.sv = k->pm = k->pv = nullptr;
        k->cap_m_pad = 0; k->cap_d = 0; k->cap_prior = false; k->fit_stamp = 0;
        hipError_t e = hipMalloc(&k->raw, sizeof(double) * cap * cd);
        if (e == hipSuccess) e = hipMalloc(&k->P.xs, sizeof(double) * cd * cap);
        if (e == hipSuccess) e = hipMalloc(&k->P.sq, sizeof(double) * cap);
        if (e == hipSuccess && cp) e = hipMalloc(&k->P.sv, sizeof(double) * cap);
        if (e == hipSuccess && cp) e = hipMalloc(&k->pm, sizeof(double) * cap);
        if (e == hipSuccess && cp) e = hipMalloc(&k->pv, sizeof(double) * cap);
        if (e != hipSuccess) return fail(CBO_ERR_HIP, std::string("candidate buffers: ") + hipGetErrorString(e));
        k->cap_m_pad = cap; k->cap_d = cd; k->cap_prior = cp;
    }
    return CBO_OK;
}

// a candidate set now holds m points of dimension d (its buffers reserved for them): every cache keyed on its old
// contents is dropped
static void cands_describe(cbo_cands *k, int64_t m, int d, bool prior, int64_t index_offset)
{
    k->m = m; k->d = d; k->index_offset = index_offset;
    k->m_pad = round_up(m, kStrip);
    k->P.n = m; k->P.ld = k->m_pad; k->P.d = d;
    k->has_prior = prior;
    k->prepared_for = nullptr; k->prepared_ls.clear();
    k->fit_stamp = 0; k->v_stamp = 0;
    k->has_cost = false;                               // (the raw points are about to change)
}

// the set's cost vector from its raw points and its cost table (queued)
static int cands_form_cost(cbo_cands *k)
{
    cbo_ctx *c = k->ctx;
    const int rc = grow(c, k->cost, (size_t)k->cap_m_pad);
    if (rc != CBO_OK) return rc;
    launch_cands_cost(c->stream, k->raw, k->m, k->d, k->cost_table, k->cost);
    HIP_TRY(hipGetLastError());
    k->has_cost = true;
    return CBO_OK;
}

// (re)fill a candidate set from host arrays
static int cands_fill(cbo_cands *k, int64_t m, int d, const double *Xs, const double *pm, const double *pv,
                      int64_t index_offset)
{
    cbo_ctx *c = k->ctx;
    int rc = cands_reserve(k, m, d, pv != nullptr);
    if (rc != CBO_OK) return rc;
    cands_describe(k, m, d, pv != nullptr, index_offset);
    hipError_t e = hipMemcpyAsync(k->raw, Xs, sizeof(double) * m * d, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && pv) e = hipMemcpyAsync(k->pm, pm, sizeof(double) * m, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && pv) e = hipMemcpyAsync(k->pv, pv, sizeof(double) * m, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // the host buffers are the caller's
    if (e != hipSuccess) return fail(CBO_ERR_HIP, std::string("candidate upload: ") + hipGetErrorString(e));
    return CBO_OK;
}

static int check_cands_args(cbo_ctx *c, int64_t m, int d, const double *Xs, const double *pm, const double *pv)
{
    if (!c || !Xs) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0) return fail(CBO_ERR_INVALID, "m must be positive");
    if (d < 1 || d > CBO_MAX_DIM) return fail(CBO_ERR_INVALID, "d must be in [1, CBO_MAX_DIM]");
    if ((pm == nullptr) != (pv == nullptr))
        return fail(CBO_ERR_INVALID, "prior mean and prior variance must be given together");
    return CBO_OK;
}

extern "C" int cbo_cands_create(cbo_ctx *c, int64_t m, int d, const double *Xs, const double *pm, const double *pv,
                                int64_t index_offset, cbo_cands **out)
{
    if (!out) return fail(CBO_ERR_INVALID, "NULL argument");
    int rc = check_cands_args(c, m, d, Xs, pm, pv);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    cbo_cands *k = new cbo_cands();
    k->ctx = c;
    rc = cands_fill(k, m, d, Xs, pm, pv, index_offset);
    if (rc != CBO_OK) { cbo_cands_destroy(k); return rc; }
    *out = k;
    return CBO_OK;
}

// the context's reusable candidate set for the host-buffer entry points (no allocation once it has grown)
static cbo_cands *scratch_set(cbo_ctx *c)
{
    if (!c->scratch_k) { c->scratch_k = new cbo_cands(); c->scratch_k->ctx = c; }
    return c->scratch_k;
}

static int scratch_cands(cbo_ctx *c, int64_t m, int d, const double *Xs, const double *pm, const double *pv,
                         cbo_cands **out)
{
    int rc = check_cands_args(c, m, d, Xs, pm, pv);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = cands_fill(scratch_set(c), m, d, Xs, pm, pv, 0);
    if (rc != CBO_OK) return rc;
    *out = c->scratch_k;
    return CBO_OK;
}

// The scratch set of m host points for model g: prior closures only when g is causal.  pm == nullptr: the posterior mean
// is not wanted, and the prior variance stands in for the prior mean the set carries beside it (the mean formed from it
// is discarded).
static int scratch_points(cbo_gp *g, int64_t m, const double *Xs, const double *pm, const double *pv, cbo_cands **out)
{
    const bool causal = g->X.sv != nullptr;
    return scratch_cands(g->ctx, m, g->d, Xs, causal ? (pm ? pm : pv) : nullptr, causal ? pv : nullptr, out);
}

// The scratch set [X1 | filler | X2] for model g: X2 starts on column round_up(m1, align), so that one solve gives both
// sets' solutions side by side; the filler repeats X1's first point (its columns are never read).  pv1 / pv2: the prior
// variances of a causal model (no mean is formed).
static int scratch_pair(cbo_gp *g, int64_t m1, const double *X1, const double *pv1, int64_t m2, const double *X2,
                        const double *pv2, int64_t align, cbo_cands **out)
{
    const bool causal = g->X.sv != nullptr;
    const int d = g->d;
    const int64_t off = round_up(m1, align), mt = off + m2;
    std::vector<double> xs((size_t)mt * d), vs(causal ? (size_t)mt : 0);
    std::memcpy(xs.data(), X1, sizeof(double) * (size_t)m1 * d);
    for (int64_t i = m1; i < off; ++i) std::memcpy(&xs[(size_t)i * d], X1, sizeof(double) * d);
    std::memcpy(&xs[(size_t)off * d], X2, sizeof(double) * (size_t)m2 * d);
    if (causal) {
        std::memcpy(vs.data(), pv1, sizeof(double) * (size_t)m1);
        for (int64_t i = m1; i < off; ++i) vs[(size_t)i] = pv1[0];
        std::memcpy(&vs[(size_t)off], pv2, sizeof(double) * (size_t)m2);
    }
    return scratch_points(g, mt, xs.data(), nullptr, vs.data(), out);
}

// the candidates' own copies of q, mu (the sweep cache), allocated on first use for the buffers' capacity
static int cands_cache_vectors(cbo_cands *k)
{
    int rc = grow(k->ctx, k->q, (size_t)k->cap_m_pad);
    if (rc == CBO_OK) rc = grow(k->ctx, k->mu, (size_t)k->cap_m_pad);
    return rc;
}

// ---- per-candidate intervention costs -------------------------------------------------------------------
// cbo_acq_refine_sets' checks of a cost table: finite fixed costs, flags 0 or 1, a fixed-cost sum above 0 -- so c(x) > 0
static int check_cost_table(int d, const double *fix, const int *variable, const std::string &where = "")
{
    double fix_sum = 0.0;
    for (int k = 0; k < d; ++k) {
        if (!std::isfinite(fix[k])) return fail(CBO_ERR_INVALID, "the fixed costs must be finite" + where);
        if (variable[k] != 0 && variable[k] != 1) return fail(CBO_ERR_INVALID, "cost_variable must be 0 or 1" + where);
        fix_sum += fix[k];
    }
    if (!(fix_sum > 0.0)) return fail(CBO_ERR_INVALID, "the fixed costs must sum to a positive cost" + where);
    return CBO_OK;
}

extern "C" int cbo_cands_set_cost(cbo_cands *k, const double *fix, const int *variable)
{
    if (!k || !fix || !variable) return fail(CBO_ERR_INVALID, "NULL argument: cands, fix and variable must be given");
    int rc = check_cost_table(k->d, fix, variable);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipSetDevice(k->ctx->device));
    k->cost_table = CostTable{};
    for (int j = 0; j < k->d; ++j) { k->cost_table.fix[j] = fix[j]; k->cost_table.variable[j] = variable[j]; }
    rc = cands_form_cost(k);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipStreamSynchronize(k->ctx->stream));
    return CBO_OK;
}

extern "C" int cbo_cands_get_cost(const cbo_cands *k, double *out)
{
    if (!k || !out) return fail(CBO_ERR_INVALID, "NULL argument: cands and out must be given");
    if (!k->has_cost) return fail(CBO_ERR_INVALID, "the candidate set has no cost vector (cbo_cands_set_cost)");
    HIP_TRY(hipSetDevice(k->ctx->device));
    HIP_TRY(hipMemcpyAsync(out, k->cost.p, sizeof(double) * k->m, hipMemcpyDeviceToHost, k->ctx->stream));
    HIP_TRY(hipStreamSynchronize(k->ctx->stream));
    return CBO_OK;
}

extern "C" int cbo_cands_clear_cost(cbo_cands *k)
{
    if (!k) return fail(CBO_ERR_INVALID, "NULL argument: cands");
    k->has_cost = false;
    return CBO_OK;
}

extern "C" void cbo_cands_destroy(cbo_cands *k)
{
    if (!k) return;
    hipSetDevice(k->ctx->device);
    hipStreamSynchronize(k->ctx->stream);
    hipFree(k->raw); hipFree(k->pm); hipFree(k->pv); hipFree(k->V); hipFree(k->partial);
    hipFree(k->P.xs); hipFree(k->P.sq); hipFree(k->P.sv);
    delete k;
}

// the per-candidate vectors q, mu and the epilogue's mean, var, acq for m_pad candidates
static int grow_vectors(cbo_ctx *c, int64_t m_pad)
{
    for (GrowBuf<double> *b : {&c->q, &c->mu, &c->mean, &c->var, &c->acq}) {
        const int rc = grow(c, *b, (size_t)m_pad);
        if (rc != CBO_OK) return rc;
    }
    return CBO_OK;
}

static int ensure_workspaces(cbo_ctx *c, int64_t n_pad, int64_t m_pad, int64_t *chunk_cols, int64_t *ldv,
                             size_t elem = sizeof(double))
{
    // V chunk: as many 64-column strips as fit the workspace budget (at least one strip).  elem = 4: the fp32
    // sweep's workspace (n_pad is then its 256-padded row count), 128 B of row padding either way.
    int64_t cols = m_pad;
    const int64_t max_cols = (int64_t)(c->max_ws_bytes / (elem * (size_t)n_pad)) / kStrip * kStrip;
    if (cols > max_cols) cols = max_cols < kStrip ? kStrip : max_cols;
    const int64_t ld = cols + (int64_t)(128 / elem);
    int rc = grow(c, c->V, (elem * (size_t)n_pad * (size_t)ld + sizeof(double) - 1) / sizeof(double));
    if (rc == CBO_OK) rc = grow_vectors(c, m_pad);
    if (rc != CBO_OK) return rc;
    *chunk_cols = cols;
    *ldv = ld;
    return CBO_OK;
}

// Scale / transpose the candidate coordinates for this GP's lengthscales (GPy ARD divides the inputs).
static int prepare_cands(cbo_gp *g, cbo_cands *k)
{
    cbo_ctx *c = g->ctx;
    if (k->prepared_for == g && k->prepared_ls == g->ls) return CBO_OK;
    launch_prep_points(c->stream, k->raw, k->m, k->d, g->h.ard ? g->ls_dev : nullptr, k->has_prior ? k->pv : nullptr,
                       k->P.xs, k->m_pad, k->P.sq, k->has_prior ? k->P.sv : nullptr);
    HIP_TRY(hipGetLastError());
    k->prepared_for = g;
    k->prepared_ls = g->ls;
    return CBO_OK;
}

// timers of the right-looking sweep: one event pair per launch on the stream it goes to
static void pipe_mark(void *user, hipStream_t st, int begin, double flops)
{
    cbo_ctx *c = static_cast<cbo_ctx *>(user);
    if (!c->profiling) return;
    EventPair &cur = c->pipe_cur;
    if (begin) {
        cur.a = get_event(c);
        cur.b = get_event(c);
        cur.phase = PH_TRSM;
        hipEventRecord(cur.a, st);
        c->timers.n_trsm_launches += 1;
        c->timers.trsm_flops += flops;
    } else {
        hipEventRecord(cur.b, st);
        c->pending.push_back(cur);
    }
}

static SweepPipe make_pipe(cbo_gp *g, double *V, int64_t ldv, int64_t cols, double *q, double *mu)
{
    cbo_ctx *c = g->ctx;
    SweepPipe pipe{};
    pipe.stream = c->sweep_stream;
    pipe.bulk = c->bulk_stream;
    pipe.V = V; pipe.ldv = ldv; pipe.m_pad = cols;
    pipe.zvec = g->z; pipe.q = q; pipe.mu = mu;
    pipe.events = &c->pipe_events;
    pipe.mark = pipe_mark; pipe.user = c;
    pipe.tail_begin = (int)g->n_pad;                     // no tail unless the caller sets one
    pipe.group = 0;
    return pipe;
}

// Which schedule for a sweep of `cols` candidate columns against a factor that is already complete?
// The left-looking strip kernel is the more efficient one (no read-modify-write of V, no launch chain) but it
// has one workgroup per 64 columns: its time is whole rounds of n_cu strips.  The right-looking schedule
// (strip kernel on a panel pair, then trsm_update_kernel over strips x row chunks, pair after pair) fills the
// device whatever the column count and costs about a sixth more per column.  Same bits either way.
static bool prefer_right_looking(const cbo_ctx *c, int64_t n_pad, int64_t cols)
{
    if (c->sweep_mode == 0) return false;
    if (c->sweep_mode == 1) return true;
    if (n_pad < 1024) return false;
    const int64_t strips = cols / kStrip;
    const int64_t rounds = (strips + c->n_cu - 1) / c->n_cu;
    return rounds * c->n_cu * 5 >= strips * 6;
}

// ---- the schedule of cbo_gp_fit_sweep is measured on the calls the caller makes: schedule_tuner.h ----------------------

static int enqueue_right_looking(cbo_gp *g, double *V, int64_t ldv, int64_t cols, double *q, double *mu,
                                 bool lower_tri = false)
{
    cbo_ctx *c = g->ctx;
    SweepPipe pipe = make_pipe(g, V, ldv, cols, q, mu);
    pipe.lower_tri = lower_tri;
    HIP_TRY(hipMemsetAsync(q, 0, sizeof(double) * cols, c->stream));
    HIP_TRY(hipMemsetAsync(mu, 0, sizeof(double) * cols, c->stream));
    int p = 0;
    for (int r0 = 0; r0 < (int)g->n_pad; r0 += 256, ++p)
        sweep_pipe_pair(pipe, c->stream, g->A, g->lda, g->invDt, g->n_pad, p, r0,
                        (r0 + 256 <= (int)g->n_pad) ? 256 : 128);
    HIP_TRY(hipEventRecord(c->ev_join, c->sweep_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    HIP_TRY(hipEventRecord(c->ev_join2, c->bulk_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join2, 0));
    return CBO_OK;
}

// The candidates' own V buffer (cbo_cands_keep_solution), sized for the model's padded row count.
static int own_solution_buffer(cbo_gp *g, cbo_cands *k, double **V, int64_t *ldv)
{
    cbo_ctx *c = g->ctx;
    if (!k->V || k->v_rows_cap != g->n_pad || k->v_ld != k->m_pad + kLdExtra) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        hipFree(k->V); hipFree(k->partial);
        k->V = nullptr; k->partial = nullptr; k->v_stamp = 0;
        k->v_ld = k->m_pad + kLdExtra;
        HIP_TRY(hipMalloc(&k->V, sizeof(double) * (size_t)g->n_pad * (size_t)k->v_ld));
        HIP_TRY(hipMalloc(&k->partial, sizeof(double) * 64 * (size_t)k->m_pad));
        k->v_rows_cap = g->n_pad;
    }
    *V = k->V;
    *ldv = k->v_ld;
    return CBO_OK;
}

// fp32 sweep (CBO_DTYPE_F32 models): K* in fp64 arithmetic rounded to fp32, substitution on the f32 MFMA, q and mu
// accumulated in fp64.  Left-looking strip kernel only; the fp32 copies of the factor follow the fit lazily.
static int enqueue_posterior_f32(cbo_gp *g, cbo_cands *k)
{
    cbo_ctx *c = g->ctx;
    int64_t chunk = 0, ldv = 0;
    int rc = ensure_workspaces(c, g->n32, k->m_pad, &chunk, &ldv, sizeof(float));
    if (rc != CBO_OK) return rc;
    rc = ensure_alpha(g);                     // the mean is K*^T alpha in fp64 (GPy's formula), see kernels_f32.hip
    if (rc != CBO_OK) return rc;
    rc = grow(c, c->mupart, (size_t)(g->n32 / 64) * (size_t)chunk);
    if (rc != CBO_OK) return rc;
    if (g->f32_stamp != g->fit_stamp) {
        PhaseScope ps(c, PH_CONVERT);
        launch_factor_to_f32(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->Uf, g->ldu32, g->invF, g->n32);
        g->f32_stamp = g->fit_stamp;
    }
    float *Vf = reinterpret_cast<float *>(c->V.p);
    k->v_stamp = 0;
    for (int64_t c0 = 0; c0 < k->m_pad; c0 += chunk) {
        const int64_t cols = (k->m_pad - c0 < chunk) ? (k->m_pad - c0) : chunk;
        {
            PhaseScope ps(c, PH_KSTAR);
            launch_kstar_f32(c->stream, g->X, k->P, c0, cols, g->h, Vf, ldv, g->n32, g->alpha, c->mupart, c->mu + c0);
        }
        {
            PhaseScope ps(c, PH_TRSM);
            launch_trsm_strips_f32(c->stream, g->Uf, g->ldu32, g->invF, Vf, ldv, g->n32, cols, c->q + c0);
        }
        if (c->profiling) {
            c->timers.n_trsm_launches += 1;
            c->timers.trsm_flops += (double)g->n32 * (double)g->n32 * (double)cols;
        }
    }
    HIP_TRY(hipGetLastError());
    return CBO_OK;
}

// V[:, 0:cols) = L^-1 K(X, X*) for the candidates [c_begin, c_begin + cols) of k (cols a multiple of kStrip) on the fp64
// factor, with q, mu of those columns: the K* kernel, then the substitution in the schedule prefer_right_looking picks
static int solve_columns(cbo_gp *g, const cbo_cands *k, int64_t c_begin, int64_t cols, double *V, int64_t ldv, double *q,
                         double *mu)
{
    cbo_ctx *c = g->ctx;
    {
        PhaseScope ps(c, PH_KSTAR);
        launch_kstar(c->stream, g->X, k->P, c_begin, cols, g->h, V, ldv, g->n_pad);
    }
    if (prefer_right_looking(c, g->n_pad, cols)) return enqueue_right_looking(g, V, ldv, cols, q, mu);
    {
        PhaseScope ps(c, PH_TRSM);
        launch_trsm_strips(c->stream, g->A, g->lda, g->invDt, V, ldv, g->n_pad, cols, g->z, q, mu);
    }
    if (c->profiling) {
        c->timers.n_trsm_launches += 1;
        c->timers.trsm_flops += (double)g->n_pad * (double)g->n_pad * (double)cols;
    }
    return CBO_OK;
}

// q = colsum((L^-1 K*)^2), mu = (L^-1 K*)^T z for all candidates, chunk by chunk.
static int enqueue_posterior(cbo_gp *g, cbo_cands *k, bool want_f64_solution = false)
{
    cbo_ctx *c = g->ctx;
    int rc = prepare_cands(g, k);
    if (rc != CBO_OK) return rc;
    // (prediction gradients read V = L^-1 K* back from the fp64 workspace: they stay on the fp64 factor)
    if (g->dtype == CBO_DTYPE_F32 && !want_f64_solution) return enqueue_posterior_f32(g, k);
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, g->n_pad, k->m_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    double *Vws = c->V;
    k->v_stamp = 0;
    if (k->keep_v && chunk >= k->m_pad) {                    // one chunk: the solution can stay with the candidates
        rc = own_solution_buffer(g, k, &Vws, &ldv);
        if (rc != CBO_OK) return rc;
    }
    for (int64_t c0 = 0; c0 < k->m_pad; c0 += chunk) {
        const int64_t cols = (k->m_pad - c0 < chunk) ? (k->m_pad - c0) : chunk;
        rc = solve_columns(g, k, c0, cols, Vws, ldv, c->q + c0, c->mu + c0);
        if (rc != CBO_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    if (Vws != c->V) { k->v_stamp = g->fit_stamp; k->v_rows = g->n; }
    return CBO_OK;
}

static int check_sweep_args(const cbo_gp *g, const cbo_cands *k, int task)
{
    if (!g || !k) return fail(CBO_ERR_INVALID, "NULL argument");
    if (g->ctx != k->ctx) return fail(CBO_ERR_INVALID, "gp and candidates live on different contexts");
    if (g->d != k->d) return fail(CBO_ERR_INVALID, "gp and candidates have different dimensions");
    if ((g->X.sv != nullptr) && !k->has_prior)
        return fail(CBO_ERR_INVALID, "causal gp needs candidate prior mean/variance");
    if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    return CBO_OK;
}

// EI / cost and arg-max from q, mu (already on the device), results to the host
// The epilogue of a sweep from q = sum V^2 and mu = V^T z: variance, mean, EI / cost, arg-max, and the copies to the host.
// enqueue_finish only queues (cbo_gp_fit_sweep queues it behind the closing launch, ahead of its one synchronisation:
// the factorisation's status and the winner come back together); complete_finish reads the winner after the stream has
// been synchronised.
// the per-candidate vectors of the epilogue to the caller's host buffers (queued; the caller synchronises)
static int copy_posterior_out(cbo_ctx *c, const cbo_cands *k, double *acq_out, double *mean_out, double *var_out)
{
    if (acq_out) HIP_TRY(hipMemcpyAsync(acq_out, c->acq, sizeof(double) * k->m, hipMemcpyDeviceToHost, c->stream));
    if (mean_out) HIP_TRY(hipMemcpyAsync(mean_out, c->mean, sizeof(double) * k->m, hipMemcpyDeviceToHost, c->stream));
    if (var_out) HIP_TRY(hipMemcpyAsync(var_out, c->var, sizeof(double) * k->m, hipMemcpyDeviceToHost, c->stream));
    return CBO_OK;
}

// mes: max-value entropy search's epilogue (mes_acq_kernel) in the place of EI's; y_best, task and ei_jitter are then unused
// kind: CBO_ACQ_LCB / _PI / _VAR / kLogEiKind: pointwise_acq_kernel in the place of EI's, ei_jitter being the kind's parameter;
// kEiPointKind / kLogEiPointKind: pointcost_acq_kernel over the set's cost vector (the caller has checked it has one); 0 and
// CBO_ACQ_MPEI: EI -- with y_best_dev, its incumbent is read from there (device memory) and y_best is unused
static int enqueue_finish(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost, double *acq_out,
                          double *mean_out, double *var_out, const double *q_src, const double *mu_src,
                          bool with_status = false, bool copy_out = true, const MesParams *mes = nullptr, int kind = 0,
                          const double *y_best_dev = nullptr)
{
    cbo_ctx *c = g->ctx;
    const bool causal = g->X.sv != nullptr;
    AcqParams p;
    p.variance = g->h.variance; p.noise_var = g->noise_var; p.y_best = y_best; p.ei_jitter = ei_jitter; p.cost = cost;
    p.task = task; p.include_noise = 1; p.want_ei = 1;
    p.y_best_dev = y_best_dev;
    const int nb = acq_blocks_for(k->m);
    {
        PhaseScope ps(c, PH_ACQ);
        if (mes)
            launch_mes_acq(c->stream, q_src, mu_src, causal ? k->pm : nullptr, causal ? k->pv : nullptr, k->m, *mes,
                           mean_out ? c->mean : nullptr, var_out ? c->var : nullptr, acq_out ? c->acq : nullptr,
                           c->part_val, c->part_idx, k->index_offset, nb);
        else if (kind == kEiPointKind || kind == kLogEiPointKind)   // (cost is 1: every candidate is priced at k->cost)
            launch_pointcost_acq(c->stream, kind == kLogEiPointKind, q_src, mu_src, causal ? k->pm : nullptr,
                                 causal ? k->pv : nullptr, k->cost, k->m, p, mean_out ? c->mean : nullptr,
                                 var_out ? c->var : nullptr, acq_out ? c->acq : nullptr, c->part_val, c->part_idx,
                                 k->index_offset, nb);
        else if (kind == CBO_ACQ_LCB || kind == CBO_ACQ_PI || kind == CBO_ACQ_VAR || kind == kLogEiKind)
            launch_pointwise_acq(c->stream, kind, q_src, mu_src, causal ? k->pm : nullptr, causal ? k->pv : nullptr, k->m, p,
                                 mean_out ? c->mean : nullptr, var_out ? c->var : nullptr, acq_out ? c->acq : nullptr,
                                 c->part_val, c->part_idx, k->index_offset, nb);
        else
            launch_acq(c->stream, q_src, mu_src, causal ? k->pm : nullptr, causal ? k->pv : nullptr, k->m, p,
                       mean_out ? c->mean : nullptr, var_out ? c->var : nullptr, acq_out ? c->acq : nullptr, c->part_val,
                       c->part_idx, k->index_offset, nb);
        // the winner (and, behind a factorisation, its status word) goes straight to pinned host memory
        launch_argmax_final(c->stream, c->part_val, c->part_idx, nb, c->h_best_val, c->h_best_idx,
                            with_status ? g->info : nullptr, with_status ? c->h_info : nullptr);
    }
    HIP_TRY(hipGetLastError());
    if (copy_out) return copy_posterior_out(c, k, acq_out, mean_out, var_out);
    return CBO_OK;
}

static void complete_finish(cbo_ctx *c, double *best_val, int64_t *best_idx)
{
    if (best_val) *best_val = *c->h_best_val;
    if (best_idx) *best_idx = *c->h_best_idx;
    if (c->profiling) c->timers.n_sweep += 1;
}

// Where the epilogue reads a pair's q, mu.  They are kept with the candidates (two small device copies) so that the next
// sweep of an unchanged model skips the substitution altogether; `own`: they must END in the candidates' own buffers, also
// with the sweep cache off (an epilogue over several pairs: the context's vectors hold one pair's at a time) -- the
// buffers are then storage only, the stamp that would let a later sweep reuse them stays unset.
static int settle_vectors(cbo_gp *g, cbo_cands *k, bool own, const double **q_src, const double **mu_src)
{
    cbo_ctx *c = g->ctx;
    const bool cached = k->fit_stamp != 0 && k->fit_stamp == g->fit_stamp;
    if (!cached && (c->sweep_cache || own)) {
        const int rc = cands_cache_vectors(k);
        if (rc != CBO_OK) return rc;
        HIP_TRY(hipMemcpyAsync(k->q, c->q, sizeof(double) * k->m_pad, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(k->mu, c->mu, sizeof(double) * k->m_pad, hipMemcpyDeviceToDevice, c->stream));
        if (c->sweep_cache) k->fit_stamp = g->fit_stamp;
    }
    *q_src = (cached || own) ? k->q : c->q;
    *mu_src = (cached || own) ? k->mu : c->mu;
    return CBO_OK;
}

static int finish_sweep(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                        double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx,
                        const MesParams *mes = nullptr, int kind = 0, const double *y_best_dev = nullptr)
{
    cbo_ctx *c = g->ctx;
    const double *q_src = nullptr, *mu_src = nullptr;
    int rc = settle_vectors(g, k, false, &q_src, &mu_src);
    if (rc != CBO_OK) return rc;
    rc = enqueue_finish(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, q_src, mu_src, false, true, mes,
                        kind, y_best_dev);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    complete_finish(c, best_val, best_idx);
    return CBO_OK;
}

// V[n-1, :] for a model that was extended by cbo_gp_append: k(x_new, X*) by the K* kernel with the appended point as
// its only row, then the row update; q, mu (the candidates' cached copies) move along and take the new fit stamp.
static int extend_solution_by_one_row(cbo_gp *g, cbo_cands *k)
{
    cbo_ctx *c = g->ctx;
    int rc = prepare_cands(g, k);
    if (rc != CBO_OK) return rc;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, g->n_pad, k->m_pad, &chunk, &ldv);      // c->V: scratch for the 64-row K* slab
    if (rc != CBO_OK) return rc;
    if (chunk < k->m_pad) return CBO_OK;                               // cannot happen for a resident V; fall through
    const int64_t row = g->n - 1;
    PointSet one = g->probe->P;                                        // the appended point, scaled as the model's
    one.n = 1;
    launch_kstar(c->stream, one, k->P, 0, k->m_pad, g->h, c->V, ldv, 64);
    launch_append_row(c->stream, k->V, k->v_ld, row, g->lvec, k->m_pad, c->V, g->append_d, g->append_zn, k->partial,
                      k->q, k->mu);
    HIP_TRY(hipGetLastError());
    k->v_rows = g->n;
    k->v_stamp = g->fit_stamp;
    k->fit_stamp = g->fit_stamp;
    return CBO_OK;
}

extern "C" int cbo_cands_keep_solution(cbo_cands *k, int on)
{
    if (!k) return fail(CBO_ERR_INVALID, "cands is NULL");
    k->keep_v = on != 0;
    if (!k->keep_v) {
        hipSetDevice(k->ctx->device);
        hipStreamSynchronize(k->ctx->stream);
        hipFree(k->V); hipFree(k->partial);
        k->V = nullptr; k->partial = nullptr; k->v_stamp = 0; k->v_rows_cap = 0;
    }
    return CBO_OK;
}

// One more observation for a fitted model (the step src/Monitor.py:148-160 + src/CBO.py:224-235 take every trial):
// the factor, z and the resident data grow by one row instead of being rebuilt.  *appended_out = 0 (and nothing
// changed) when the shortcut does not apply -- the current factor carries jitter, the padded size is exhausted, or
// the new pivot is not positive -- and the caller refits with cbo_gp_set_data.
extern "C" int cbo_gp_append(cbo_gp *g, const double *x_new, double y_new, double prior_mean_new, double prior_var_new,
                             int *appended_out)
{
    if (!g || !x_new || !appended_out) return fail(CBO_ERR_INVALID, "NULL argument");
    *appended_out = 0;
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    if (g->tries != 0 || g->n >= g->n_pad) return CBO_OK;
    if (g->dtype != CBO_DTYPE_F64) return CBO_OK;       // the resident V of the row update is an fp64 object
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool causal = g->X.sv != nullptr;
    // the new point as a one-candidate set (kept with the model: no allocation after the first append)
    if (g->probe) {
        cbo_cands *p = g->probe;
        HIP_TRY(hipMemcpyAsync(p->raw, x_new, sizeof(double) * g->d, hipMemcpyHostToDevice, c->stream));
        if (causal) {
            HIP_TRY(hipMemcpyAsync(p->pm, &prior_mean_new, sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(p->pv, &prior_var_new, sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));          // x_new and the two scalars are the caller's / this frame's
        p->prepared_for = nullptr;
        p->fit_stamp = 0;
    } else {
        int rc = cbo_cands_create(c, 1, g->d, x_new, causal ? &prior_mean_new : nullptr, causal ? &prior_var_new : nullptr,
                                  0, &g->probe);
        if (rc != CBO_OK) return rc;
    }
    // k(X, x_new) by the K* kernel (64 padded columns, column 0 is the point), then l = L^-1 k by the
    // single-right-hand-side forward solve; l^T l and l^T z on the host (two n-vectors come back)
    int rc = prepare_cands(g, g->probe);
    if (rc != CBO_OK) return rc;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, g->n_pad, g->probe->m_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    launch_kstar(c->stream, g->X, g->probe->P, 0, g->probe->m_pad, g->h, c->V, ldv, g->n_pad);
    launch_gather_column(c->stream, c->V, ldv, g->n_pad, g->alpha + g->n_pad);      // work vector (alpha's scratch half)
    const bool chained = launch_forward_chain(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->alpha + g->n_pad, g->lvec,
                                              g->info, c->chol.spin_limit, c->vec_solve_form);
    if (!chained) launch_forward_vec(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->alpha + g->n_pad, g->lvec);
    HIP_TRY(hipGetLastError());
    // l^T z and l^T l by one device reduction (16 bytes come back)
    launch_dot2(c->stream, g->lvec, g->z, g->n, c->part_val);
    HIP_TRY(hipGetLastError());
    double hd[2];
    HIP_TRY(hipMemcpyAsync(hd, c->part_val, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
    if (chained) HIP_TRY(hipMemcpyAsync(c->h_info, g->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (chained && *c->h_info != 0) {                       // the chain gave up (bounded polls): the per-block launches
        HIP_TRY(hipMemsetAsync(g->info, 0, sizeof(int), c->stream));
        ++c->fused_fallbacks;
        launch_forward_vec(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->alpha + g->n_pad, g->lvec);
        launch_dot2(c->stream, g->lvec, g->z, g->n, c->part_val);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hd, c->part_val, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const double h2[2] = {hd[1], hd[0]};                    // {l^T l, l^T z}
    g->alpha_ready = false;                                 // its scratch half was used
    const double kappa = g->h.variance + (causal ? prior_var_new : 0.0) + (g->noise_var + kGpyDiagJitter);
    const double d2 = kappa - h2[0];
    if (!(d2 > 0.0) || !std::isfinite(d2)) return CBO_OK;  // jitchol's business: full refit
    const double d = std::sqrt(d2);
    const double zn = ((y_new - (causal ? prior_mean_new : 0.0)) - h2[1]) / d;
    HIP_TRY(hipMemcpyAsync(g->raw + g->n * g->d, x_new, sizeof(double) * g->d, hipMemcpyHostToDevice, c->stream));
    launch_append_commit(c->stream, g->A, g->lda, g->n, g->n_pad, g->lvec, 1, d, zn, g->z, g->lvec, g->X, g->probe->P,
                         prior_mean_new, prior_var_new, g->y, y_new, g->invDt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (causal) g->h_pv.push_back(prior_var_new);
    g->n += 1;
    g->X.n = g->n;
    g->append_d = d;
    g->append_zn = zn;
    g->k_last = 1;
    g->parent_stamp = g->fit_stamp;
    g->fit_stamp = ++g_fit_stamp;
    g->alpha_ready = false;
    *appended_out = 1;
    return CBO_OK;
}

// ---- block append (kernels_append.hip) --------------------------------------------------------------------
// the model's block buffers for its padded size (one allocation; a model whose padded size changed was refitted since)
static int ensure_block_buffers(cbo_gp *g)
{
    cbo_ctx *c = g->ctx;
    if (g->blk_mem && g->blk_rows == g->n_pad) return CBO_OK;
    if (g->blk_mem) HIP_TRY(hipStreamSynchronize(c->stream));
    hipFree(g->blk_mem);
    g->blk_mem = nullptr; g->blk_rows = 0;
    const size_t per_side = (size_t)g->n_pad * kAppendLd + (size_t)kAppendLd * kAppendLd + 2 * (size_t)kAppendLd +
                            (size_t)kAppendLd * (kAppendLd + kLdExtra);
    const size_t part = (size_t)64 * (kAppendLd + 1) * kAppendLd;
    const size_t total = 2 * per_side + part + 2;                     // the last two doubles hold the status word
    const hipError_t e = hipMalloc(&g->blk_mem, sizeof(double) * total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g->blk_mem = nullptr;
        return fail(CBO_ERR_HIP, std::string("block append buffers: ") + hipGetErrorString(e));
    }
    HIP_TRY(hipMemsetAsync(g->blk_mem, 0, sizeof(double) * total, c->stream));
    double *p = g->blk_mem;
    for (int s = 0; s < 2; ++s) {
        g->blk_B[s] = p; p += (size_t)g->n_pad * kAppendLd;
        g->blk_L22[s] = p; p += (size_t)kAppendLd * kAppendLd;
        g->blk_zb[s] = p; p += kAppendLd;
        g->blk_y[s] = p; p += kAppendLd;
        g->blk_Kbb[s] = p; p += (size_t)kAppendLd * (kAppendLd + kLdExtra);
    }
    g->blk_part = p; p += part;
    g->blk_status = reinterpret_cast<int *>(p);
    g->blk_rows = g->n_pad;
    return CBO_OK;
}

extern "C" int cbo_gp_append_block(cbo_gp *g, int k, const double *X_new, const double *y_new,
                                   const double *prior_mean_new, const double *prior_var_new, int *appended_out)
{
    if (!g || !X_new || !y_new || !appended_out) return fail(CBO_ERR_INVALID, "NULL argument");
    *appended_out = 0;
    if (k < 1 || k > CBO_MAX_APPEND)
        return fail(CBO_ERR_INVALID, "k must be in 1.." + std::to_string(CBO_MAX_APPEND));
    const bool causal = g->X.sv != nullptr;
    if (causal && (!prior_mean_new || !prior_var_new))
        return fail(CBO_ERR_INVALID, "a causal model needs the prior mean and the prior variance of the new points");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    if (k == 1)
        return cbo_gp_append(g, X_new, y_new[0], causal ? prior_mean_new[0] : 0.0, causal ? prior_var_new[0] : 0.0,
                             appended_out);
    if (g->tries != 0 || g->n + k > g->n_pad) return CBO_OK;
    if (g->dtype != CBO_DTYPE_F64) return CBO_OK;
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_block_buffers(g);
    if (rc != CBO_OK) return rc;
    const int side = 1 - g->blk_side;
    // the new points as a candidate set (kept with the model: no allocation after the first block on each side); the
    // caller's arrays are read by the copies queued here, which are complete at the call's first synchronisation
    if (!g->blk_probe[side]) { g->blk_probe[side] = new cbo_cands(); g->blk_probe[side]->ctx = c; }
    cbo_cands *p = g->blk_probe[side];
    rc = cands_reserve(p, CBO_MAX_APPEND, g->d, causal);
    if (rc != CBO_OK) return rc;
    cands_describe(p, k, g->d, causal, 0);
    HIP_TRY(hipMemcpyAsync(p->raw, X_new, sizeof(double) * k * g->d, hipMemcpyHostToDevice, c->stream));
    if (causal) {
        HIP_TRY(hipMemcpyAsync(p->pm, prior_mean_new, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(p->pv, prior_var_new, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(g->blk_y[side], y_new, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
    rc = prepare_cands(g, p);
    if (rc != CBO_OK) return rc;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, g->n_pad, p->m_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    const int kp = (int)round_up(k, 16);
    const int64_t ldk = kAppendLd + kLdExtra;
    // K(X, Xb) and K(Xb, Xb) by the K* kernel, B by the k-column forward solve, then the Schur block
    launch_kstar(c->stream, g->X, p->P, 0, p->m_pad, g->h, c->V, ldv, g->n_pad);
    PointSet pb = p->P;
    pb.n = k;
    launch_kstar(c->stream, pb, p->P, 0, p->m_pad, g->h, g->blk_Kbb[side], ldk, 64);
    launch_append_forward(c->stream, g->A, g->lda, g->n_pad, g->invDt, c->V, ldv, kp, g->blk_B[side]);
    AppendSchurArgs sa{};
    sa.part = g->blk_part; sa.k = k;
    sa.Kbb = g->blk_Kbb[side]; sa.ldk = ldk;
    sa.pv = causal ? p->pv : nullptr; sa.pm = causal ? p->pm : nullptr;
    sa.y_new = g->blk_y[side];
    sa.variance = g->h.variance; sa.sigma = g->noise_var + kGpyDiagJitter;
    sa.L22 = g->blk_L22[side]; sa.zb = g->blk_zb[side]; sa.status = g->blk_status;
    launch_append_schur(c->stream, g->blk_B[side], g->n, g->z, sa);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_info, g->blk_status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (*c->h_info != 0) return CBO_OK;                     // jitchol's business: full refit
    HIP_TRY(hipMemcpyAsync(g->raw + g->n * g->d, p->raw, sizeof(double) * k * g->d, hipMemcpyDeviceToDevice, c->stream));
    AppendCommitArgs ca{};
    ca.A = g->A; ca.lda = g->lda; ca.n = g->n; ca.n_pad = g->n_pad; ca.k = k;
    ca.B = g->blk_B[side]; ca.L22 = g->blk_L22[side]; ca.zb = g->blk_zb[side]; ca.y_new = g->blk_y[side];
    ca.z = g->z; ca.y = g->y;
    ca.dims = g->X.d; ca.xs = g->X.xs; ca.ldx = g->X.ld; ca.sq = g->X.sq; ca.sv = g->X.sv; ca.pm = g->X.pm; ca.pv = g->X.pv;
    ca.pxs = p->P.xs; ca.ldp = p->P.ld; ca.psq = p->P.sq; ca.psv = p->P.sv; ca.pm_new = p->pm; ca.pv_new = p->pv;
    launch_append_block_commit(c->stream, ca, g->invDt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (causal) g->h_pv.insert(g->h_pv.end(), prior_var_new, prior_var_new + k);
    g->n += k;
    g->X.n = g->n;
    g->k_last = k;
    g->blk_side = side;
    g->parent_stamp = g->fit_stamp;
    g->fit_stamp = ++g_fit_stamp;
    g->alpha_ready = false;
    *appended_out = 1;
    return CBO_OK;
}

// V[n-k : n, :] for a model that was extended by cbo_gp_append_block: K(Xb, X*) by the K* kernel with the block's points
// as its rows, then one pass over V for all k rows; q, mu (the candidates' cached copies) move along and take the new
// fit stamp.
static int extend_solution_by_block(cbo_gp *g, cbo_cands *k)
{
    cbo_ctx *c = g->ctx;
    int rc = prepare_cands(g, k);
    if (rc != CBO_OK) return rc;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, g->n_pad, k->m_pad, &chunk, &ldv);      // c->V: scratch for the 64-row K* slab
    if (rc != CBO_OK) return rc;
    if (chunk < k->m_pad) return CBO_OK;                               // cannot happen for a resident V; fall through
    const int kb = g->k_last, kp = (int)round_up(kb, 16), side = g->blk_side;
    const int64_t n0 = g->n - kb;
    int slices = 1, rps = 64;
    append_rows_plan(n0, k->m_pad, &slices, &rps);
    rc = grow(c, c->append_part, (size_t)slices * (size_t)kp * (size_t)k->m_pad);
    if (rc != CBO_OK) return rc;
    PointSet pb = g->blk_probe[side]->P;                               // the block's points, scaled as the model's
    pb.n = kb;
    launch_kstar(c->stream, pb, k->P, 0, k->m_pad, g->h, c->V, ldv, 64);
    AppendRowsArgs ra{};
    ra.k = kb; ra.m_pad = k->m_pad;
    ra.Kb = c->V; ra.ldk = ldv;
    ra.L22 = g->blk_L22[side]; ra.zb = g->blk_zb[side];
    ra.Vnew = k->V + n0 * k->v_ld; ra.ldv = k->v_ld;
    ra.q = k->q; ra.mu = k->mu;
    launch_append_rows(c->stream, k->V, k->v_ld, g->blk_B[side], n0, kp, c->append_part, ra);
    HIP_TRY(hipGetLastError());
    k->v_rows = g->n;
    k->v_stamp = g->fit_stamp;
    k->fit_stamp = g->fit_stamp;
    return CBO_OK;
}

// q, mu of the candidates for the fitted model: the cached copies, one appended row, or the substitution (which leaves
// them in the context's vectors for settle_vectors)
static int enqueue_vectors(cbo_gp *g, cbo_cands *k, bool *substituted = nullptr)
{
    int rc = CBO_OK;
    cbo_ctx *c = g->ctx;
    if (k->keep_v && k->V && k->v_stamp != 0 && k->v_stamp == g->parent_stamp && k->v_rows == g->n - g->k_last &&
        k->v_rows_cap == g->n_pad && k->fit_stamp == k->v_stamp && k->q) {
        // the model is the one this V belongs to plus the last appended block: its new rows instead of the substitution
        // (one observation, cbo_gp_append: the one-row kernels)
        rc = g->k_last == 1 ? extend_solution_by_one_row(g, k) : extend_solution_by_block(g, k);
        if (rc != CBO_OK) return rc;
    }
    if (!(c->sweep_cache && k->fit_stamp != 0 && k->fit_stamp == g->fit_stamp)) {
        k->fit_stamp = 0;
        if (substituted) *substituted = true;
        return enqueue_posterior(g, k);
    }
    return grow_vectors(c, k->m_pad);                    // mean / var / acq scratch of the epilogue
}

// then the epilogue: EI / cost, max-value entropy search / cost when mes is given, or a point-wise kind's (enqueue_finish)
static int sweep_impl(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost, double *acq_out,
                      double *mean_out, double *var_out, double *best_val, int64_t *best_idx, const MesParams *mes,
                      int kind = 0, const double *y_best_dev = nullptr)
{
    HIP_TRY(hipSetDevice(g->ctx->device));
    const int rc = enqueue_vectors(g, k);
    if (rc != CBO_OK) return rc;
    return finish_sweep(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_val, best_idx, mes, kind,
                        y_best_dev);
}

extern "C" int cbo_acq_sweep(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                             double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx)
{
    int rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    return sweep_impl(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_val, best_idx, nullptr);
}

// ---- greedy batch selection (kernels_batch.hip) ---------------------------------------------------------
// emukit GreedyBatchPointCalculator over a candidate set without touching the model: pick 0 is the plain sweep; every
// further pick is one pass over the resident V = L^-1 K* whose pivot the device reads from the previous pick's winner,
// then the EI / arg-max epilogue on the working copy of q.  Everything is queued; the call synchronises once.
// log_form (cbo_acq_sweep_batch_logei): the same sequence, every pick scored by the log-EI candidate pass
// (pointwise_acq_kernel<kLogEiKind>; under update_incumbent its variant that reads the moved incumbent from the device) --
// the scalars are checked first, as the log-EI calls check them (check_kind_args), then the handles.
static int check_kind_args(int n_sets, int kind, const double *y_best, int *task, double *param, const double *costs,
                           bool logei);
static int sweep_batch_impl(bool log_form, cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                            int batch_size, int update_incumbent, double *best_vals, int64_t *best_idxs, double *acq_out,
                            double *mean_out, double *var_out)
{
    int rc = log_form ? check_kind_args(1, kLogEiKind, &y_best, &task, &ei_jitter, &cost, true) : CBO_OK;
    if (rc != CBO_OK) return rc;
    if (log_form && (batch_size < 1 || batch_size > CBO_MAX_BATCH))
        return fail(CBO_ERR_INVALID, "batch_size must be in 1.." + std::to_string(CBO_MAX_BATCH));
    if (log_form && update_incumbent != 0 && update_incumbent != 1)
        return fail(CBO_ERR_INVALID, "update_incumbent must be 0 or 1");
    rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    const int kind = log_form ? kLogEiKind : 0;
    if (batch_size < 1 || batch_size > CBO_MAX_BATCH)
        return fail(CBO_ERR_INVALID, "batch_size must be in 1.." + std::to_string(CBO_MAX_BATCH));
    if (batch_size > k->m) return fail(CBO_ERR_INVALID, "batch_size exceeds the number of candidates");
    if (!best_vals || !best_idxs) return fail(CBO_ERR_INVALID, "NULL argument");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    if (update_incumbent != 0 && update_incumbent != 1) return fail(CBO_ERR_INVALID, "update_incumbent must be 0 or 1");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool f32 = g->dtype == CBO_DTYPE_F32;
    if (batch_size == 1 && !f32)
        return sweep_impl(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_vals, best_idxs, nullptr, kind);
    int64_t chunk = 0, ld_ws = 0;
    rc = ensure_workspaces(c, g->n_pad, k->m_pad, &chunk, &ld_ws);
    if (rc != CBO_OK) return rc;
    if (batch_size > 1 && chunk < k->m_pad)
        return fail(CBO_ERR_UNSUPPORTED, std::string(log_form ? "cbo_acq_sweep_batch_logei" : "cbo_acq_sweep_batch") +
                                             " needs L^-1 K* of all " + std::to_string(k->m_pad) +
                                             " padded candidates resident at once; the workspace holds " +
                                             std::to_string(chunk) + " columns: raise CBO_HIP_WORKSPACE_MB");
    // q, mu of pick 0 as cbo_acq_sweep reaches them; an fp32 model answers from its fp64 factor and leaves the
    // candidates' cache (which holds the fp32 sweep's vectors) alone
    const double *q_src = nullptr, *mu_src = nullptr;
    bool substituted = false;
    if (f32) {
        rc = enqueue_posterior(g, k, true);
        substituted = true;
        q_src = c->q; mu_src = c->mu;
    } else {
        rc = enqueue_vectors(g, k, &substituted);
        if (rc == CBO_OK) rc = settle_vectors(g, k, false, &q_src, &mu_src);
    }
    if (rc != CBO_OK) return rc;
    auto kept = [&] {
        return k->keep_v && k->V && k->v_stamp != 0 && k->v_stamp == g->fit_stamp && k->v_rows == g->n &&
               k->v_rows_cap == g->n_pad;
    };
    const double *V = nullptr;
    int64_t ldv = 0;
    if (batch_size > 1) {
        if (!kept() && !substituted) {           // q, mu came from the cache (q_src is the candidates' copy): V alone
            rc = enqueue_posterior(g, k);
            if (rc != CBO_OK) return rc;
        }
        if (kept()) { V = k->V; ldv = k->v_ld; }
        else { V = c->V; ldv = ld_ws; }
    }
    const int64_t m_pad = k->m_pad;
    rc = grow(c, c->batch_state, 1);
    if (rc == CBO_OK) rc = grow(c, c->batch_h_vals, CBO_MAX_BATCH);
    if (rc == CBO_OK) rc = grow(c, c->batch_h_idxs, CBO_MAX_BATCH);
    if (rc == CBO_OK && batch_size > 1) rc = grow(c, c->batch_W, (size_t)(batch_size - 1) * (size_t)m_pad);
    if (rc == CBO_OK && batch_size > 1) rc = grow(c, c->batch_q, (size_t)m_pad);
    if (rc == CBO_OK && batch_size > 1) rc = grow(c, c->batch_col, (size_t)g->n_pad);
    if (rc == CBO_OK && batch_size > 1) rc = grow(c, c->batch_part, (size_t)batch_slices(g->n) * (size_t)m_pad);
    if (rc != CBO_OK) return rc;
    const bool causal = g->X.sv != nullptr;
    const double *pm = causal ? k->pm : nullptr, *pv = causal ? k->pv : nullptr;
    AcqParams p;
    p.variance = g->h.variance; p.noise_var = g->noise_var; p.y_best = y_best; p.ei_jitter = ei_jitter; p.cost = cost;
    p.task = task; p.include_noise = 1; p.want_ei = 1;
    const int nb = acq_blocks_for(k->m);
    {
        PhaseScope ps(c, PH_ACQ);
        launch_batch_state_init(c->stream, c->batch_state, y_best);
        const double *q_cur = q_src;
        for (int t = 0; t < batch_size; ++t) {
            const bool last = t == batch_size - 1;
            if (t == 1)
                HIP_TRY(hipMemcpyAsync(c->batch_q, q_src, sizeof(double) * m_pad, hipMemcpyDeviceToDevice, c->stream));
            if (t >= 1) {
                BatchPivotArgs pa{};
                pa.best_val = c->best_val; pa.best_idx = c->best_idx;
                pa.index_offset = k->index_offset; pa.m = k->m; pa.m_pad = m_pad; pa.n = g->n;
                pa.V = V; pa.ldv = ldv; pa.col = c->batch_col; pa.W = c->batch_W;
                pa.q = c->batch_q; pa.mu = mu_src; pa.pm = pm; pa.pv = pv;
                pa.xs = k->P.xs; pa.sq = k->P.sq; pa.sv = causal ? k->P.sv : nullptr; pa.ldx = k->P.ld; pa.dims = k->d;
                pa.variance = g->h.variance; pa.noise_var = g->noise_var;
                pa.t = t; pa.task = task; pa.update_incumbent = update_incumbent;
                pa.state = c->batch_state; pa.h_vals = c->batch_h_vals; pa.h_idxs = c->batch_h_idxs;
                BatchFinalArgs fa{};
                fa.m = k->m; fa.m_pad = m_pad; fa.W = c->batch_W; fa.q = c->batch_q;
                fa.xs = k->P.xs; fa.sq = k->P.sq; fa.sv = pa.sv; fa.ldx = k->P.ld;
                fa.variance = g->h.variance; fa.inv_l2 = 1.0 / (g->h.lengthscale * g->h.lengthscale);
                fa.t = t; fa.state = c->batch_state;
                launch_batch_pick(c->stream, pa, fa, c->batch_col, c->batch_part);
                q_cur = c->batch_q;
                if (update_incumbent) p.y_best_dev = &c->batch_state.p->y_best;
            }
            double *mean_dst = (last && mean_out) ? c->mean.p : nullptr, *var_dst = (last && var_out) ? c->var.p : nullptr;
            double *acq_dst = (last && acq_out) ? c->acq.p : nullptr;
            if (log_form)
                launch_pointwise_acq(c->stream, kLogEiKind, q_cur, mu_src, pm, pv, k->m, p, mean_dst, var_dst, acq_dst,
                                     c->part_val, c->part_idx, k->index_offset, nb);
            else
                launch_acq(c->stream, q_cur, mu_src, pm, pv, k->m, p, mean_dst, var_dst, acq_dst, c->part_val, c->part_idx,
                           k->index_offset, nb);
            launch_argmax_final(c->stream, c->part_val, c->part_idx, nb, c->best_val, c->best_idx);
        }
        launch_batch_record(c->stream, c->best_val, c->best_idx, batch_size - 1, c->batch_h_vals, c->batch_h_idxs);
    }
    HIP_TRY(hipGetLastError());
    rc = copy_posterior_out(c, k, acq_out, mean_out, var_out);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int t = 0; t < batch_size; ++t) {
        best_vals[t] = c->batch_h_vals.p[t];
        best_idxs[t] = c->batch_h_idxs.p[t];
    }
    if (c->profiling) c->timers.n_sweep += 1;
    return CBO_OK;
}

extern "C" int cbo_acq_sweep_batch(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                                   int batch_size, int update_incumbent, double *best_vals, int64_t *best_idxs,
                                   double *acq_out, double *mean_out, double *var_out)
{
    return sweep_batch_impl(false, g, k, y_best, task, ei_jitter, cost, batch_size, update_incumbent, best_vals, best_idxs,
                            acq_out, mean_out, var_out);
}

// The Kriging believer on the log Expected Improvement: cbo_acq_sweep_batch's picks scored by log EI - log
// cost, finite and ordered where every pick's EI is an exact 0.  batch_size == 1 on an fp64 model is cbo_acq_sweep_logei.
extern "C" int cbo_acq_sweep_batch_logei(cbo_gp *g, cbo_cands *k, double y_best, int task, double jitter, double cost,
                                         int batch_size, int update_incumbent, double *best_vals, int64_t *best_idxs,
                                         double *acq_out, double *mean_out, double *var_out)
{
    return sweep_batch_impl(true, g, k, y_best, task, jitter, cost, batch_size, update_incumbent, best_vals, best_idxs, acq_out,
                            mean_out, var_out);
}

// ---- max-value entropy search (kernels_mes.hip) ------------------------------------------------------------------------
// emukit MaxValueEntropySearch.evaluate over a candidate set: the EI sweep's path up to q, mu (cached re-sweep, appended
// row, fp32 strip), then mes_acq_kernel in the place of acq_kernel
extern "C" int cbo_acq_sweep_mes(cbo_gp *g, cbo_cands *k, int n_samples, const double *mins, double cost, double *acq_out,
                                 double *mean_out, double *var_out, double *best_val, int64_t *best_idx)
{
    int rc = check_sweep_args(g, k, CBO_TASK_MIN);
    if (rc != CBO_OK) return rc;
    if (n_samples <= 0 || n_samples > kMesMaxSamples)
        return fail(CBO_ERR_INVALID, "the number of Gumbel samples must be in 1.." + std::to_string(kMesMaxSamples));
    if (!mins) return fail(CBO_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n_samples; ++i)
        if (!std::isfinite(mins[i])) return fail(CBO_ERR_INVALID, "the Gumbel samples must be finite");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    MesParams p{};
    p.variance = g->h.variance; p.noise_var = g->noise_var; p.cost = cost; p.k = n_samples;
    for (int i = 0; i < n_samples; ++i) p.mins[i] = mins[i];
    return sweep_impl(g, k, 0.0, CBO_TASK_MIN, 0.0, cost, acq_out, mean_out, var_out, best_val, best_idx, &p);
}

// ---- constrained acquisition (kernels_con.hip) -------------------------------------------------------------------------
// EI times the constraints' probabilities of feasibility over a cost, one pass with the arg-max.  Every (model, set) pair is
// brought up to date by the sweep's own steps (enqueue_vectors, settle_vectors), one after the other on the stream, its
// vectors ending in the set's own buffers; then the one epilogue reads them all.
// log_form (cbo_acq_sweep_constrained_log): the same steps, the epilogue's log instantiation; ei_out and
// pof_out then carry log EI and the log probabilities.
static int sweep_constrained_impl(bool log_form, cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter,
                                  double cost, int n_con, cbo_gp *const *con_gps, cbo_cands *const *con_cands,
                                  const double *con_value, const double *con_jitter, const int *con_sense, double *acq_out,
                                  double *ei_out, double *pof_out, double *best_val, int64_t *best_idx)
{
    if (n_con < 0 || n_con > CBO_MAX_CONSTRAINTS)
        return fail(CBO_ERR_INVALID, "the number of constraints must be in 0.." + std::to_string(CBO_MAX_CONSTRAINTS));
    if ((g == nullptr) != (k == nullptr)) return fail(CBO_ERR_INVALID, "gp and candidates must be given (or left out) together");
    const bool objective = g != nullptr;
    if (!objective && n_con < 1) return fail(CBO_ERR_INVALID, "no objective and no constraint");
    if (!objective && ei_out) return fail(CBO_ERR_INVALID, "ei_out without an objective");
    if (n_con > 0 && (!con_gps || !con_cands || !con_value || !con_jitter || !con_sense))
        return fail(CBO_ERR_INVALID, "NULL argument");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    if (log_form && objective && !std::isfinite(ei_jitter)) return fail(CBO_ERR_INVALID, "jitter must be finite");
    if (log_form && objective && !std::isfinite(y_best)) return fail(CBO_ERR_INVALID, "y_best must be finite");
    cbo_gp *gps[kConMaxModels];
    cbo_cands *sets[kConMaxModels];
    int nm = 0;
    if (objective) { gps[nm] = g; sets[nm] = k; ++nm; }
    for (int i = 0; i < n_con; ++i, ++nm) {
        gps[nm] = con_gps[i];
        sets[nm] = con_cands[i];
        if (!std::isfinite(con_value[i]) || !std::isfinite(con_jitter[i]))
            return fail(CBO_ERR_INVALID, "the constraints' values and jitters must be finite");
        if (con_sense[i] != CBO_CON_LE && con_sense[i] != CBO_CON_GE)
            return fail(CBO_ERR_INVALID, "a constraint's sense must be CBO_CON_LE or CBO_CON_GE");
    }
    for (int i = 0; i < nm; ++i) {
        const int rc = check_sweep_args(gps[i], sets[i], (objective && i == 0) ? task : CBO_TASK_MIN);
        if (rc != CBO_OK) return rc;
        if (gps[i]->ctx != gps[0]->ctx) return fail(CBO_ERR_INVALID, "the pairs live on different contexts");
        if (sets[i]->m != sets[0]->m) return fail(CBO_ERR_INVALID, "the candidate sets differ in size");
        for (int j = 0; j < i; ++j)
            if (sets[j] == sets[i] && gps[j] != gps[i])
                return fail(CBO_ERR_INVALID, "one candidate set with two models: its q, mu are one model's");
    }
    for (int i = 0; i < nm; ++i)
        if (!gps[i]->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t m = sets[0]->m;
    ConParams p{};
    p.y_best = y_best; p.ei_jitter = ei_jitter; p.cost = cost;
    p.n_models = nm; p.has_objective = objective ? 1 : 0; p.task = objective ? task : CBO_TASK_MIN;
    for (int i = 0; i < nm; ++i) {
        bool seen = false;                                   // (the same pair twice: its vectors are settled already)
        for (int j = 0; j < i; ++j) seen = seen || sets[j] == sets[i];
        const double *q_src = sets[i]->q, *mu_src = sets[i]->mu;
        if (!seen) {
            int rc = enqueue_vectors(gps[i], sets[i]);
            if (rc == CBO_OK) rc = settle_vectors(gps[i], sets[i], true, &q_src, &mu_src);
            if (rc != CBO_OK) return rc;
        }
        const bool causal = gps[i]->X.sv != nullptr;
        ConModel &md = p.mdl[i];
        md.q = q_src; md.mu = mu_src;
        md.pm = causal ? sets[i]->pm : nullptr; md.pv = causal ? sets[i]->pv : nullptr;
        md.variance = gps[i]->h.variance; md.noise_var = gps[i]->noise_var;
        const int ci = i - (objective ? 1 : 0);
        if (ci >= 0) { md.value = con_value[ci]; md.jitter = con_jitter[ci]; md.sense = con_sense[ci]; }
    }
    // per-candidate outputs: acq and the objective's EI in the epilogue's vectors, the constraints' terms in one of their own
    int rc = grow_vectors(c, sets[0]->m_pad);
    const int64_t ldt = sets[0]->m_pad;                      // (rows of whole strips: every row starts 16-byte aligned)
    if (rc == CBO_OK && pof_out) rc = grow(c, c->con_terms, (size_t)n_con * (size_t)ldt);
    if (rc != CBO_OK) return rc;
    if (ei_out) p.mdl[0].out = c->mean;
    if (pof_out)
        for (int i = 0; i < n_con; ++i) p.mdl[i + (objective ? 1 : 0)].out = c->con_terms + (int64_t)i * ldt;
    const int nb = acq_blocks_for(m);
    {
        PhaseScope ps(c, PH_ACQ);
        launch_constrained_acq(c->stream, p, m, acq_out ? c->acq.p : nullptr, c->part_val, c->part_idx, sets[0]->index_offset,
                               nb, log_form);
        launch_argmax_final(c->stream, c->part_val, c->part_idx, nb, c->h_best_val, c->h_best_idx);
    }
    HIP_TRY(hipGetLastError());
    rc = copy_posterior_out(c, sets[0], acq_out, ei_out, nullptr);
    if (rc != CBO_OK) return rc;
    for (int i = 0; pof_out && i < n_con; ++i)
        HIP_TRY(hipMemcpyAsync(pof_out + (int64_t)i * m, c->con_terms + (int64_t)i * ldt, sizeof(double) * (size_t)m,
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    complete_finish(c, best_val, best_idx);
    return CBO_OK;
}

extern "C" int cbo_acq_sweep_constrained(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                                         int n_con, cbo_gp *const *con_gps, cbo_cands *const *con_cands,
                                         const double *con_value, const double *con_jitter, const int *con_sense,
                                         double *acq_out, double *ei_out, double *pof_out, double *best_val,
                                         int64_t *best_idx)
{
    return sweep_constrained_impl(false, g, k, y_best, task, ei_jitter, cost, n_con, con_gps, con_cands, con_value, con_jitter,
                                  con_sense, acq_out, ei_out, pof_out, best_val, best_idx);
}

// log EI plus the constraints' log probabilities of feasibility less log cost: finite and ordered where
// the product above is an exact 0.  With no constraint cbo_acq_sweep_logei's bits.
extern "C" int cbo_acq_sweep_constrained_log(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                                             int n_con, cbo_gp *const *con_gps, cbo_cands *const *con_cands,
                                             const double *con_value, const double *con_jitter, const int *con_sense,
                                             double *acq_out, double *logei_out, double *logpof_out, double *best_val,
                                             int64_t *best_idx)
{
    return sweep_constrained_impl(true, g, k, y_best, task, ei_jitter, cost, n_con, con_gps, con_cands, con_value, con_jitter,
                                  con_sense, acq_out, logei_out, logpof_out, best_val, best_idx);
}

// Refit and sweep in one call, the two overlapped: what CBO.intervene() does for the set it has just
// intervened on (set_data -> refit, then find_next_y_point -> acquisition over the candidates,
// /root/reference/src/Monitor.py:160, src/CBO.py:250-257).  The factorisation is a chain of short kernels
// that leaves most CUs idle; the sweep's rows become solvable panel by panel as the chain advances, so it
// runs right-looking on a second stream underneath (SweepPipe).  Same results as cbo_gp_fit followed by
// cbo_acq_sweep (the per-element operation order is the same; only q and mu are summed panel-wise).
extern "C" int cbo_gp_fit_sweep(cbo_gp *g, cbo_cands *k, double y_best, int task, double ei_jitter, double cost,
                                double *acq_out, double *mean_out, double *var_out, double *best_val,
                                int64_t *best_idx, int *tries_out, double *jitter_out)
{
    int rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "gp holds no data (a previous upload failed)");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (g->dtype == CBO_DTYPE_F32) {
        // the fp32 sweep needs the finished fp64 factor (down-converted once): the plain sequence
        rc = cbo_gp_fit(g, tries_out, jitter_out);
        if (rc != CBO_OK) return rc;
        return cbo_acq_sweep(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_val, best_idx);
    }
    rc = prepare_cands(g, k);
    if (rc != CBO_OK) return rc;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, g->n_pad, k->m_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    if (chunk < k->m_pad) {
        // the candidates do not fit one V workspace: no overlap, the plain sequence
        rc = cbo_gp_fit(g, tries_out, jitter_out);
        if (rc != CBO_OK) return rc;
        return cbo_acq_sweep(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_val, best_idx);
    }
    // The schedule: forced by the environment (CBO_HIP_OVERLAP / CBO_HIP_PIPE_TAIL / CBO_HIP_PIPE_GROUP: diagnostics and
    // scripts/schedule_scan.py), or the one this context has measured for the shape (schedule_choose above).  A model of
    // one panel pair or less has nothing to pipeline.
    using clk = std::chrono::steady_clock;
    const clk::time_point t_call = clk::now();
    auto us_since = [](clk::time_point a) { return std::chrono::duration<double, std::micro>(clk::now() - a).count(); };
    const int nb = (int)(g->n_pad / 128);
    const int all_pairs = (nb + 1) / 2;
    const bool forced = c->overlap_mode == 0 || c->overlap_mode == 1 || c->pipe_tail_frac >= 0.0 || c->pipe_group != 0 ||
                        all_pairs < 2;
    ScheduleEntry *entry = nullptr;
    ScheduleChoice choice;
    if (forced) {
        choice.group = c->pipe_group >= 2 ? c->pipe_group : (c->pipe_group == 0 && k->m_pad / kStrip >= c->n_cu_pipe) ? 2 : 0;
        if (c->overlap_mode == 0 || (all_pairs < 2 && c->overlap_mode != 1)) choice.pairs = kSequence;
        else if (c->pipe_tail_frac >= 0.0) {
            int tail_blocks = (int)(c->pipe_tail_frac * nb + 0.5);
            tail_blocks += (nb - tail_blocks) & 1;
            choice.pairs = (nb - (tail_blocks > nb ? nb : tail_blocks)) / 2;
        } else choice.pairs = all_pairs >= 4 ? all_pairs / 4 : 1;    // (only overlap / grouping forced: a quarter of the rows)
    } else {
        entry = &schedule_entry(c->schedule, c->n_cu_pipe, g->n_pad, k->m_pad / kStrip, k->m_pad);
        choice = schedule_choose(*entry, !c->profiling, c->n_cu, c->n_cu_pipe);
        entry->ran_pairs = choice.pairs;
        entry->ran_group = choice.pairs > 0 ? choice.group : 0;
    }
    if (choice.pairs == kSequence) {
        int tries = 0;
        double jitter = 0.0;
        const clk::time_point t_fit = clk::now();
        rc = cbo_gp_fit(g, &tries, &jitter);
        if (tries_out) *tries_out = tries;
        if (jitter_out) *jitter_out = jitter;
        if (rc != CBO_OK) return rc;
        const double fact_us = us_since(t_fit);
        const clk::time_point t_sweep = clk::now();
        rc = cbo_acq_sweep(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_val, best_idx);
        if (rc == CBO_OK && entry)
            schedule_report(c->n_cu, c->n_cu_pipe, *entry, choice, tries, us_since(t_call) * 1e-3, fact_us, us_since(t_sweep));
        return rc;
    }
    g->fitted = false;
    double *Vws = c->V;
    k->v_stamp = 0;
    if (k->keep_v) {
        rc = own_solution_buffer(g, k, &Vws, &ldv);
        if (rc != CBO_OK) return rc;
    }
    // q = sum V^2 and mu = V^T z go straight to the candidates' own copies when those are kept (the next sweep of the
    // unchanged model starts from them): no device copies between the closing launch and the acquisition kernel
    double *qbuf = c->q, *mubuf = c->mu;
    if (c->sweep_cache) {
        rc = cands_cache_vectors(k);
        if (rc != CBO_OK) return rc;
        qbuf = k->q;
        mubuf = k->mu;
        k->fit_stamp = 0;                                  // not valid until this call has succeeded
    }
    const bool speculate = qbuf == k->q;
    SweepPipe pipe = make_pipe(g, Vws, ldv, k->m_pad, qbuf, mubuf);
    pipe.group = choice.group;
    // pairs that do not fill a group go alone ahead of the first one (CBO_HIP_PIPE_LEAD forces the count where the schedule is
    // forced; there the default stays 0: whole groups from the first pair, what the forced schedules of rounds 3-5 meant)
    int pairs = choice.pairs;
    pipe.lead = 0;
    if (pipe.group >= 2 && pairs >= 1 && pairs * 256 < (int)g->n_pad)
        pipe.lead = forced ? (c->pipe_lead > 0 ? c->pipe_lead : 0) : (c->pipe_lead >= 0 ? c->pipe_lead : pairs % pipe.group);
    pipe.tail_begin = pairs * 256;
    if (pipe.tail_begin > (int)g->n_pad) pipe.tail_begin = (int)g->n_pad;
    double jitter = 0.0;
    int tries = 0;
    bool separate = false;                                 // the attempts after a fused launch gave up (chol_options)
    for (;;) {
        // fork: the sweep stream starts after what is queued on the main stream (candidate preparation)
        HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->sweep_stream, c->ev_fork, 0));
        // K(X,X) first: it heads the factorisation's chain, K(X,X*) is not needed before the first pair is solved.  (Until
        // round 5 the host queued K(X,X*) and two hipMemsetAsync ahead of it -- a kernel trace showed K(X,X) starting 69 us
        // after K(X,X*), most of it the host's time in those calls; q and mu are now cleared by one small launch.)
        {
            PhaseScope ps(c, PH_KXX);
            launch_kxx(c->stream, g->X, g->h, g->noise_var + kGpyDiagJitter, jitter, g->A, g->lda, g->n_pad);
            launch_rhs(c->stream, g->y, g->X.pm, g->n, g->A, g->lda, g->n_pad, g->info, cholesky_info_ints(g->n_pad));
        }
        {
            PhaseScope ps(c, PH_KSTAR, c->sweep_stream);
            launch_kstar(c->sweep_stream, g->X, k->P, 0, k->m_pad, g->h, Vws, ldv, g->n_pad);
        }
        launch_zero_pair(c->sweep_stream, qbuf, mubuf, k->m_pad);
        {
            PhaseScope ps(c, PH_CHOL);
            launch_cholesky(c->stream, c->side_stream, c->chol_events, g->A, g->lda, g->n_pad, g->invDt, g->info,
                            chol_options(c, separate), &pipe, true);
        }
        // join: everything the sweep streams were given is done before the main stream goes on (the last
        // pair has no rows below it, so the bulk stream's last launch precedes the sweep stream's in-panel solve
        // of that pair only through the events: wait for both)
        HIP_TRY(hipEventRecord(c->ev_join, c->sweep_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
        HIP_TRY(hipEventRecord(c->ev_join2, c->bulk_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join2, 0));
        HIP_TRY(hipGetLastError());
        // the epilogue's KERNELS ride behind the closing launch on the assumption that the factorisation succeeded (they
        // read q, mu where the sweep left them, and write device scratch and the pinned winner record only); the caller's
        // acq / mean / var buffers are written after the status word is known to be good (below): on an error return --
        // CBO_ERR_NOT_PD after the ladder is exhausted -- they are left untouched, as the two-call sequence leaves them
        if (speculate) {
            rc = enqueue_finish(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, qbuf, mubuf, true, false);
            if (rc != CBO_OK) return rc;
        } else {
            HIP_TRY(hipMemcpyAsync(c->h_info, g->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (*c->h_info == 0) break;
        if (*c->h_info == kCholFusedTimeout) {                 // as in cbo_gp_fit: the attempt again, separate launches
            if (separate)
                return fail(CBO_ERR_HIP, "a fused diagonal + panel launch gave up waiting, and so did the separate-launch repeat");
            separate = true;
            ++c->fused_fallbacks;
            continue;
        }
        rc = next_jitter(g, &tries, &jitter);
        if (rc != CBO_OK) return rc;
    }
    mark_fitted(g, tries, jitter);
    if (tries_out) *tries_out = tries;
    if (jitter_out) *jitter_out = jitter;
    if (Vws != c->V) { k->v_stamp = g->fit_stamp; k->v_rows = g->n; }
    if (qbuf == k->q) k->fit_stamp = g->fit_stamp;         // the candidates' q, mu are this fit's
    if (speculate) {
        if (acq_out || mean_out || var_out) {
            rc = copy_posterior_out(c, k, acq_out, mean_out, var_out);
            if (rc != CBO_OK) return rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        complete_finish(c, best_val, best_idx);
        if (entry) schedule_report(c->n_cu, c->n_cu_pipe, *entry, choice, separate ? -1 : tries, us_since(t_call) * 1e-3, 0.0, 0.0);
        return CBO_OK;
    }
    rc = finish_sweep(g, k, y_best, task, ei_jitter, cost, acq_out, mean_out, var_out, best_val, best_idx);
    if (rc == CBO_OK && entry)
        schedule_report(c->n_cu, c->n_cu_pipe, *entry, choice, separate ? -1 : tries, us_since(t_call) * 1e-3, 0.0, 0.0);
    return rc;
}

// ---- every exploration set of a trial in one call ------------------------------------------------------------------
// CBO.compute_best_acquisition_values (/root/reference/src/CBO.py:237-260) loops find_next_y_point over the S
// exploration sets.  Sets whose model has at most 128 observations -- every model the reference itself builds
// (10 + <= 40 points, src/ArgumentParser.py:18,25) -- are swept by ONE launch that factors and sweeps inside LDS
// (kernels_sets.hip, small_sets_kernel): no per-set launch chain, no per-set synchronisation, one copy back.  Such a
// model need not be fitted: the launch works from its resident data (cbo_gp_upload_data is enough) and leaves its
// fitted state alone.  A set whose factorisation meets a non-positive pivot there (jitchol's business), a larger
// model, or an fp32 model takes the general path: cbo_gp_fit_sweep when the model is not fitted, cbo_acq_sweep
// otherwise.
// How long the host polls the pinned result record of a one-launch job before it lets the runtime wait on the stream.
// Measured (round 3, CBO_HIP_TRACE_SLOW=1): a blocking hipStreamSynchronize behind such a launch returns after the
// kernel's ~40 us -- except about once in 600-1000 calls, when it returns after 62.75 ms +- 0.03 (a timed wait inside
// the runtime running out: the completion wake-up was missed, the kernel had long finished).  Round 2 polled for
// 32768 reads, which is ~10 us, not the 0.3 ms it was meant to be, so nearly every call ended in that blocking wait.
// The poll is now bounded by the clock: the record of a small job arrives within it and the host never sleeps on the
// stream; only jobs that really take longer fall through to hipStreamSynchronize.
constexpr double kPollBudgetUs = 2000.0;
// A launch whose result was polled is still "in flight" for the runtime: every so many of them the (idle) stream is
// synchronised so that their completion records are reaped; their signals have completed, the call does not sleep.
constexpr int kPolledLaunchesPerSync = 256;
template <class Pred>
static bool poll_until(Pred done, double budget_us)
{
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    for (;;) {
        for (int spin = 0; spin < 256; ++spin)
            if (done()) return true;
        if (std::chrono::duration<double, std::micro>(clk::now() - t0).count() > budget_us) return done();
    }
}

// One launch whose results come back in n pinned records out[0..n), each closed by the call's sequence number, which
// launch(seq) receives when it queues the launch (it returns CBO_OK or an error).  The records are polled
// (kPollBudgetUs); the stream is synchronised when the poll gave up, when profiling, or when the periodic reap is due.
// A record that has not arrived then is the error `missing`; the caller reads the records after this call's fence.
// CBO_HIP_TRACE_SLOW=1: a call that takes more than a millisecond says on stderr where the time went (a value above 1 is
// the threshold in microseconds instead).
// the sequence number of the context's next one-workgroup launch (never 0: the records are zero between calls)
static int next_small_seq(cbo_ctx *c)
{
    if (++c->small_seq == 0) c->small_seq = 1;
    return c->small_seq;
}

template <class Rec, class Launch>
static int polled_launch(cbo_ctx *c, const char *name, const Rec *out, int n, const char *missing, Launch launch)
{
    const int seq = next_small_seq(c);
    static const bool trace_slow = std::getenv("CBO_HIP_TRACE_SLOW") != nullptr;
    static const double trace_over_us = trace_slow && std::atof(std::getenv("CBO_HIP_TRACE_SLOW")) > 1.0
                                            ? std::atof(std::getenv("CBO_HIP_TRACE_SLOW")) : 1000.0;
    using clk = std::chrono::steady_clock;
    const clk::time_point t_begin = trace_slow ? clk::now() : clk::time_point();
    const int rc = launch(seq);
    if (rc != CBO_OK) return rc;
    const clk::time_point t_launched = trace_slow ? clk::now() : clk::time_point();
    const bool all = poll_until([&] {
        for (int j = 0; j < n; ++j)
            if (*reinterpret_cast<const volatile int *>(&out[j].seq) != seq) return false;
        return true;
    }, kPollBudgetUs);
    const clk::time_point t_polled = trace_slow ? clk::now() : clk::time_point();
    const bool reap = ++c->polled_launches >= kPolledLaunchesPerSync;
    if (reap) c->polled_launches = 0;
    if (!all || c->profiling || reap) HIP_TRY(hipStreamSynchronize(c->stream));
    if (trace_slow) {
        const clk::time_point t_end = clk::now();
        auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        if (us(t_begin, t_end) > trace_over_us)
            std::fprintf(stderr, "[cbo] slow %s call #%d: launch %.1f us, poll %.1f us (%s), synchronise %.1f us (%s)\n",
                         name, seq, us(t_begin, t_launched), us(t_launched, t_polled), all ? "records arrived" : "gave up",
                         us(t_polled, t_end), !all ? "after the poll gave up" : reap ? "periodic reap" : "none");
    }
    for (int j = 0; j < n; ++j)
        if (out[j].seq != seq) return fail(CBO_ERR_HIP, missing);
    std::atomic_thread_fence(std::memory_order_acquire);
    return CBO_OK;
}

// the model half of a one-workgroup kernel's descriptor
static void fill_small_model(cbo_small_set &st, const cbo_gp *g)
{
    const bool causal = g->X.sv != nullptr;
    st.xs = g->X.xs; st.sq = g->X.sq; st.sv = g->X.sv; st.pm = causal ? g->X.pm : nullptr; st.y = g->y;
    st.ld = g->X.ld;
    st.n = (int)g->n; st.d = g->d; st.zero_diag = g->h.zero_diag; st.ard = g->h.ard; st.pad_ = 0;
    st.variance = g->h.variance; st.lengthscale = g->h.lengthscale; st.noise_var = g->noise_var;
    st.diag_add = g->noise_var + kGpyDiagJitter;
    st.stage = nullptr; st.stage_ls = nullptr; st.raw = g->raw; st.pv = g->X.pv;
}

// the candidate half: set k as prepare_cands has scaled it for model g, the prior closures for a causal model
static void fill_small_cands(cbo_small_set &st, const cbo_gp *g, const cbo_cands *k)
{
    const bool causal = g->X.sv != nullptr;
    st.cxs = k->P.xs; st.csq = k->P.sq; st.csv = causal ? k->P.sv : nullptr;
    st.cpm = causal ? k->pm : nullptr; st.cpv = causal ? k->pv : nullptr;
    st.cld = k->P.ld; st.m = k->m; st.index_offset = k->index_offset;
}

// a model the one-workgroup sweeps take: fp64, at most 128 observations (CBO_HIP_SMALL_SETS=0: none)
static bool small_sweep_model(const cbo_gp *g) { return g->dtype == CBO_DTYPE_F64 && g->n_pad == kPadN && g->ctx->small_sets; }

// descriptors, result records, status words and tickets for n_sets sets (at least 32), scratch and partial winners for
// `blocks` workgroups per set
static int ensure_small_buffers(cbo_ctx *c, int n_sets, int blocks)
{
    const size_t cap = n_sets < 32 ? 32 : (size_t)n_sets;
    const size_t scratch = small_sets_scratch_doubles(n_sets, blocks), parts = (size_t)n_sets * (size_t)blocks;
    int rc = grow(c, c->sets_host, cap);
    if (rc == CBO_OK) rc = grow(c, c->small_out, cap, true);
    if (rc == CBO_OK) rc = grow(c, c->small_info, 2 * cap, true);
    if (rc == CBO_OK) rc = grow(c, c->small_scratch, scratch);
    if (rc == CBO_OK) rc = grow(c, c->small_part_val, parts);
    if (rc == CBO_OK) rc = grow(c, c->small_part_idx, parts);
    return rc;
}

// ---- the routing policy of the one-workgroup kernels, written once ---------------------------------------
// (1) the handles of a multi-set call: every (gp, cands) passes check_sweep_args, lives on first's context and -- unless the
// caller is about to give it data (cbo_trial_step's refit_set) -- holds data.  `what`: "sets" or "models", for the message.
static int check_set_handle(const cbo_gp *g, const cbo_cands *k, int task, const cbo_gp *first, const char *what = "sets",
                            bool needs_data = true)
{
    const int rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    if (g->ctx != first->ctx) return fail(CBO_ERR_INVALID, std::string("all ") + what + " must live on one context");
    if (needs_data && (g->n <= 0 || g->n_pad <= 0)) return fail(CBO_ERR_INVALID, "a gp holds no data");
    return CBO_OK;
}
static int check_set_handles(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int task)
{
    for (int i = 0; i < n_sets; ++i) {
        const int rc = check_set_handle(gps[i], cands[i], task, gps[0]);
        if (rc != CBO_OK) return rc;
    }
    return CBO_OK;
}
// ... and of a call that takes models alone (the likelihood and leave-one-out batches)
static int check_model_handles(int n_models, cbo_gp *const *gps)
{
    for (int i = 0; i < n_models; ++i) {
        if (!gps[i]) return fail(CBO_ERR_INVALID, "NULL gp");
        if (gps[i]->ctx != gps[0]->ctx) return fail(CBO_ERR_INVALID, "all models must live on one context");
    }
    return CBO_OK;
}

// (2) which items the one launch takes -- those `eligible` accepts, in index order -- and how many workgroups the widest of
// them needs.  A grid dimension holds 65535 workgroups: a wider item sends the WHOLE call to the general path (a call that
// wants only that item sent there says so in `eligible`).
constexpr int64_t kMaxGridBlocks = 65535;
static int64_t cand_blocks(const cbo_cands *k) { return (k->m + 63) / 64; }     // 64 candidates per workgroup
template <class Eligible, class Blocks>
static int partition_small(int n_items, Eligible eligible, Blocks blocks_of, std::vector<int> &small)
{
    int64_t widest = 1;
    for (int i = 0; i < n_items; ++i) {
        if (!eligible(i)) continue;
        small.push_back(i);
        const int64_t b = blocks_of(i);
        if (b > widest) widest = b;
    }
    if (widest > kMaxGridBlocks) small.clear();
    return (int)widest;
}

// (3) the descriptor of one (model, candidate set) pair with the acquisition's scalars.  staged (cbo_trial_step): the
// model's new data sit in the context's staging buffer and the launch prepares and stores them.
static int fill_small_set(cbo_small_set &st, cbo_gp *g, cbo_cands *k, int task, double y_best, double ei_jitter, double cost,
                          bool staged = false)
{
    const int rc = prepare_cands(g, k);
    if (rc != CBO_OK) return rc;
    fill_small_model(st, g);
    if (staged) {
        st.stage = g->ctx->stage;
        st.stage_ls = g->h.ard ? g->ls_dev : nullptr;
    }
    fill_small_cands(st, g, k);
    st.task = task; st.y_best = y_best; st.ei_jitter = ei_jitter; st.cost = cost;
    return CBO_OK;
}
// ... and of the marginalised EI, whose kernels scale the raw candidates per sample themselves
static void fill_hyper_set(cbo_small_set &st, const cbo_gp *g, const cbo_cands *k, int task, double y_best, double ei_jitter,
                           double cost)
{
    const bool causal = g->X.sv != nullptr;
    fill_small_model(st, g);
    st.cpm = causal ? k->pm : nullptr; st.cpv = causal ? k->pv : nullptr;
    st.m = k->m; st.index_offset = k->index_offset;
    st.task = task; st.y_best = y_best; st.ei_jitter = ei_jitter; st.cost = cost;
}

// (4) the context buffers of one launch (ensure_small_buffers has sized them); the tickets are the upper half of small_info
static SmallLaunch small_launch(cbo_ctx *c, int seq)
{
    return SmallLaunch{c->small_scratch, c->small_part_val, c->small_part_idx, c->small_info,
                       c->small_info + c->small_info.cap / 2, c->small_out, seq};
}

// (5) run and fall back.  When the launch takes any item: prepare() sizes the call's buffers and fills the descriptors of
// small[0..ns), launch(L) queues the kernel on the buffers L, its records -- records.p[0..ns), pinned -- are polled, and
// harvest(j, i) reads record j, which answers item i = small[j].  An item whose record reports a model that is not positive
// definite as assembled (info != 0: jitchol's business) joins the items the launch did not take: general(i), in index
// order -- which is "fit if not fitted, then the single-model call" (ensure_fitted: the jitchol ladder lives in cbo_gp_fit).
static int ensure_fitted(cbo_gp *g) { return g->fitted ? CBO_OK : cbo_gp_fit(g, nullptr, nullptr); }
template <class Records, class Prepare, class Launch, class Harvest, class General>
static int run_small_or_general(cbo_ctx *c, const char *name, const char *missing, int n_items, const std::vector<int> &small,
                                const Records &records, Prepare prepare, Launch launch, Harvest harvest, General general)
{
    HIP_TRY(hipSetDevice(c->device));
    std::vector<char> done((size_t)n_items, 0);
    if (!small.empty()) {
        int rc = prepare();
        if (rc != CBO_OK) return rc;
        const auto *out = records.p;
        rc = polled_launch(c, name, out, (int)small.size(), missing, [&](int seq) -> int {
            launch(small_launch(c, seq));
            HIP_TRY(hipGetLastError());
            return CBO_OK;
        });
        if (rc != CBO_OK) return rc;
        for (size_t j = 0; j < small.size(); ++j) {
            if (out[j].info != 0) continue;
            rc = harvest((int)j, small[j]);
            if (rc != CBO_OK) return rc;
            done[(size_t)small[j]] = 1;
        }
    }
    for (int i = 0; i < n_items; ++i) {
        if (done[(size_t)i]) continue;
        const int rc = general(i);
        if (rc != CBO_OK) return rc;
    }
    return CBO_OK;
}

// staged_set >= 0 (cbo_trial_step): that set's new data sit in the context's staging buffer, its model's host-side state
// is already the new one, and the one-launch path -- which the caller has checked the set takes -- prepares and stores them.
// kind: kEiKind = the causal EI (small_sets_kernel, cbo_gp_fit_sweep / cbo_acq_sweep), else one of CBO_ACQ_* (DESIGN.md §4l:
// small_sets_kernel<kind>, cbo_gp_fit + cbo_acq_sweep_kind), ei_jitter then being the kind's parameter -- the caller has run
// check_kind_args.  kMesKind (small_sets_kernel<kMesKind>, cbo_gp_fit + cbo_acq_sweep_mes): set i scores
// against mins[i][0..n_samples[i]); y_best is not read (it may be NULL), task is 'min' -- cbo_acq_sweep_sets_mes has checked.
static int sweep_sets_impl(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                           double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs, int staged_set,
                           int kind, const int *n_samples = nullptr, const double *const *mins = nullptr);

extern "C" int cbo_acq_sweep_sets(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                                  double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs)
{
    return sweep_sets_impl(n_sets, gps, cands, y_best, task, ei_jitter, costs, best_vals, best_idxs, -1, kEiKind);
}

// cbo_acq_sweep_kind's checks of its scalars for every set of a multi-set call, before anything is touched; what the kind
// does not read is put to cbo_acq_sweep_kind's neutral values (the model variance reads neither task nor parameter)
// logei: the caller is one of the log-EI entry points, whose kind is kLogEiKind (no public kind code names it: every other
// caller keeps refusing it) -- the jitter and the incumbent are checked as the probability of improvement's are
static int check_kind_args(int n_sets, int kind, const double *y_best, int *task, double *param, const double *costs,
                           bool logei = false)
{
    if (!(logei && kind == kLogEiKind) && kind != CBO_ACQ_LCB && kind != CBO_ACQ_PI && kind != CBO_ACQ_VAR && kind != CBO_ACQ_MPEI)
        return fail(CBO_ERR_INVALID, "kind must be CBO_ACQ_LCB, CBO_ACQ_PI, CBO_ACQ_VAR or CBO_ACQ_MPEI");
    if (n_sets <= 0 || !y_best || !costs) return fail(CBO_ERR_INVALID, "bad argument");
    if (kind == CBO_ACQ_VAR) { *task = CBO_TASK_MIN; *param = 0.0; }
    if (*task != CBO_TASK_MIN && *task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    if (!std::isfinite(*param)) return fail(CBO_ERR_INVALID, "param (beta / jitter) must be finite");
    if (kind == CBO_ACQ_LCB && *param < 0.0) return fail(CBO_ERR_INVALID, "beta must not be negative");
    for (int i = 0; i < n_sets; ++i) {
        if ((kind == CBO_ACQ_PI || kind == kLogEiKind) && !std::isfinite(y_best[i]))
            return fail(CBO_ERR_INVALID, "y_best must be finite");
        if (!(costs[i] > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    }
    return CBO_OK;
}

// the scalar checks of the *_pointcost entry points: cbo_acq_sweep_logei's, and the set's cost vector
static int check_pointcost_args(int n_sets, int log_form, const double *y_best, int *task, double *jitter)
{
    if (log_form != 0 && log_form != 1) return fail(CBO_ERR_INVALID, "log_form must be 0 or 1");
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!y_best) return fail(CBO_ERR_INVALID, "NULL argument: y_best");
    const std::vector<double> ones((size_t)n_sets, 1.0);
    return check_kind_args(n_sets, kLogEiKind, y_best, task, jitter, ones.data(), true);
}
static int check_has_cost(const cbo_cands *k, const std::string &where = "")
{
    if (!k->has_cost) return fail(CBO_ERR_INVALID, "the candidate set has no cost vector (cbo_cands_set_cost)" + where);
    return CBO_OK;
}

extern "C" int cbo_acq_sweep_sets_kind(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int kind,
                                       const double *y_best, int task, double param, const double *costs,
                                       double *best_vals, int64_t *best_idxs)
{
    const int rc = check_kind_args(n_sets, kind, y_best, &task, &param, costs);
    if (rc != CBO_OK) return rc;
    return sweep_sets_impl(n_sets, gps, cands, y_best, task, param, costs, best_vals, best_idxs, -1, kind);
}

// cbo_acq_sweep_sets_kind for the log Expected Improvement: the same checks, the same routing, the epilogue
// log_ei_of -- per set cbo_acq_sweep_logei's bits on a fitted twin
extern "C" int cbo_acq_sweep_sets_logei(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                                        double jitter, const double *costs, double *best_vals, int64_t *best_idxs)
{
    const int rc = check_kind_args(n_sets, kLogEiKind, y_best, &task, &jitter, costs, true);
    if (rc != CBO_OK) return rc;
    return sweep_sets_impl(n_sets, gps, cands, y_best, task, jitter, costs, best_vals, best_idxs, -1, kLogEiKind);
}

// cbo_acq_sweep_sets with every candidate priced at its own cost: the same routing, the epilogues of
// kEiPointKind / kLogEiPointKind -- per set cbo_acq_sweep_pointcost's bits on a fitted twin
extern "C" int cbo_acq_sweep_sets_pointcost(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int log_form,
                                            const double *y_best, int task, double jitter, double *best_vals,
                                            int64_t *best_idxs)
{
    int rc = check_pointcost_args(n_sets, log_form, y_best, &task, &jitter);
    if (rc != CBO_OK) return rc;
    if (!gps || !cands || !best_vals || !best_idxs) return fail(CBO_ERR_INVALID, "bad argument");
    rc = check_set_handles(n_sets, gps, cands, task);
    if (rc != CBO_OK) return rc;
    for (int i = 0; i < n_sets; ++i) {
        rc = check_has_cost(cands[i], " (set " + std::to_string(i) + ")");
        if (rc != CBO_OK) return rc;
    }
    const std::vector<double> ones((size_t)n_sets, 1.0);
    return sweep_sets_impl(n_sets, gps, cands, y_best, task, jitter, ones.data(), best_vals, best_idxs, -1,
                           log_form ? kLogEiPointKind : kEiPointKind);
}

// cbo_acq_sweep_sets for max-value entropy search: cbo_acq_sweep_mes' checks of its scalars for every set,
// before anything is touched, then sweep_sets_impl's routing
extern "C" int cbo_acq_sweep_sets_mes(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const int *n_samples,
                                      const double *const *mins, const double *costs, double *best_vals, int64_t *best_idxs)
{
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!n_samples || !mins || !costs || !best_vals || !best_idxs)
        return fail(CBO_ERR_INVALID, "NULL argument: n_samples, mins, costs, best_vals and best_idxs must be given");
    for (int i = 0; i < n_sets; ++i) {
        const std::string where = " (set " + std::to_string(i) + ")";
        if (n_samples[i] <= 0 || n_samples[i] > kMesMaxSamples)
            return fail(CBO_ERR_INVALID, "the number of Gumbel samples must be in 1.." + std::to_string(kMesMaxSamples) + where);
        if (!mins[i]) return fail(CBO_ERR_INVALID, "NULL argument: mins" + where);
        for (int k = 0; k < n_samples[i]; ++k)
            if (!std::isfinite(mins[i][k])) return fail(CBO_ERR_INVALID, "the Gumbel samples must be finite" + where);
        if (!(costs[i] > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive" + where);
    }
    return sweep_sets_impl(n_sets, gps, cands, nullptr, CBO_TASK_MIN, 0.0, costs, best_vals, best_idxs, -1, kMesKind,
                           n_samples, mins);
}

// the record of a one-launch sweep is the set's winner
static int harvest_winner(const cbo_ctx *c, int j, int i, double *best_vals, int64_t *best_idxs)
{
    best_vals[i] = c->small_out[j].best_val;
    best_idxs[i] = c->small_out[j].best_idx;
    return CBO_OK;
}

static int sweep_sets_impl(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                           double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs, int staged_set,
                           int kind, const int *n_samples, const double *const *mins)
{
    if (n_sets <= 0 || !gps || !cands || (!y_best && kind != kMesKind) || !costs || !best_vals || !best_idxs)
        return fail(CBO_ERR_INVALID, "bad argument");
    int rc = check_set_handles(n_sets, gps, cands, task);
    if (rc != CBO_OK) return rc;
    cbo_ctx *c = gps[0]->ctx;
    std::vector<int> small;
    const int blocks = partition_small(n_sets, [&](int i) { return small_sweep_model(gps[i]); },
                                       [&](int i) { return cand_blocks(cands[i]); }, small);
    const int ns = (int)small.size();
    SmallAux aux;
    auto prepare = [&]() -> int {
        int rc = ensure_small_buffers(c, ns, blocks);
        if (rc == CBO_OK && kind == kMesKind) {
            // the small sets' samples, one set after the other, and where each set's begin
            size_t total = 0;
            for (int j = 0; j < ns; ++j) total += (size_t)n_samples[small[(size_t)j]];
            rc = grow(c, c->aux_host, ns < 32 ? (size_t)32 : (size_t)ns);
            if (rc == CBO_OK) rc = grow(c, c->mes_host, total);
            if (rc != CBO_OK) return rc;
            size_t at = 0;
            for (int j = 0; j < ns; ++j) {
                const size_t k = (size_t)n_samples[small[(size_t)j]];
                std::memcpy(c->mes_host.p + at, mins[small[(size_t)j]], sizeof(double) * k);
                c->aux_host[j] = cbo_small_aux{(int64_t)at, (int64_t)k};
                at += k;
            }
            aux.per_set = c->aux_host;
            aux.data = c->mes_host;
        }
        if (rc == CBO_OK && (kind == kEiPointKind || kind == kLogEiPointKind)) {
            rc = grow(c, c->cost_ptrs_host, ns < 32 ? (size_t)32 : (size_t)ns);
            if (rc != CBO_OK) return rc;
            for (int j = 0; j < ns; ++j) c->cost_ptrs_host[j] = cands[small[(size_t)j]]->cost.p;
            aux.cost = c->cost_ptrs_host;
        }
        for (int j = 0; rc == CBO_OK && j < ns; ++j) {
            const int i = small[(size_t)j];
            // (only the EI, its logarithm and the probability of improvement read the caller's incumbent)
            const double incumbent = (kind == kEiKind || kind == CBO_ACQ_PI || kind == kLogEiKind || kind == kEiPointKind ||
                                      kind == kLogEiPointKind) ? y_best[i] : 0.0;
            rc = fill_small_set(c->sets_host[j], gps[i], cands[i], task, incumbent, ei_jitter, costs[i], i == staged_set);
        }
        return rc;
    };
    auto general = [&](int i) -> int {
        if (kind == kEiKind && !gps[i]->fitted)
            return cbo_gp_fit_sweep(gps[i], cands[i], y_best[i], task, ei_jitter, costs[i], nullptr, nullptr, nullptr,
                                    &best_vals[i], &best_idxs[i], nullptr, nullptr);
        const int rc = ensure_fitted(gps[i]);
        if (rc != CBO_OK) return rc;
        if (kind == kMesKind)
            return cbo_acq_sweep_mes(gps[i], cands[i], n_samples[i], mins[i], costs[i], nullptr, nullptr, nullptr, &best_vals[i],
                                     &best_idxs[i]);
        if (kind == kEiPointKind || kind == kLogEiPointKind)
            return cbo_acq_sweep_pointcost(gps[i], cands[i], kind == kLogEiPointKind, y_best[i], task, ei_jitter, nullptr,
                                           nullptr, nullptr, &best_vals[i], &best_idxs[i]);
        if (kind == kLogEiKind)
            return cbo_acq_sweep_logei(gps[i], cands[i], y_best[i], task, ei_jitter, costs[i], nullptr, nullptr, nullptr,
                                       &best_vals[i], &best_idxs[i]);
        if (kind != kEiKind)
            return cbo_acq_sweep_kind(gps[i], cands[i], kind, y_best[i], task, ei_jitter, costs[i], nullptr, nullptr, nullptr,
                                      &best_vals[i], &best_idxs[i]);
        return cbo_acq_sweep(gps[i], cands[i], y_best[i], task, ei_jitter, costs[i], nullptr, nullptr, nullptr, &best_vals[i],
                             &best_idxs[i]);
    };
    return run_small_or_general(
        c, kind == kEiKind ? "cbo_acq_sweep_sets" : kind == kMesKind ? "cbo_acq_sweep_sets_mes"
           : kind == kLogEiKind ? "cbo_acq_sweep_sets_logei"
           : (kind == kEiPointKind || kind == kLogEiPointKind) ? "cbo_acq_sweep_sets_pointcost" : "cbo_acq_sweep_sets_kind",
        "multi-set sweep: no result record", n_sets, small, c->small_out, prepare,
        [&](const SmallLaunch &L) { launch_small_sets(c->stream, kind, c->sets_host, ns, blocks, L, aux); },
        [&](int j, int i) { return harvest_winner(c, j, i, best_vals, best_idxs); }, general);
}

// ---- greedy batch selection for every set of a trial (kernels_sets_batch.hip) ---------------------------------
// batch_size Kriging-believer picks per set, set-major in best_vals / best_idxs: per set cbo_acq_sweep_batch's bits on a
// fitted twin.  sweep_sets_impl's routing plus one cap: an fp64 model of at most 128 observations whose set has at most
// kSmallBatchMaxCands candidates takes ONE small_sets_batch_kernel launch (no fit, no model or candidate state touched);
// every other set -- and a set whose status word reports a non-positive pivot -- takes cbo_gp_fit when it is not fitted,
// then cbo_acq_sweep_batch.  batch_size == 1 is cbo_acq_sweep_sets.
// the winners array and the sets' V / W / q / mu scratch of one call
static int ensure_small_batch_buffers(cbo_ctx *c, int n_sets, int blocks, int batch_size)
{
    const size_t winners = (size_t)(n_sets < 32 ? 32 : n_sets) * (size_t)batch_size;
    int rc = grow(c, c->sets_batch_scratch, small_sets_batch_doubles(n_sets, blocks, batch_size));
    if (rc == CBO_OK) rc = grow(c, c->sets_batch_h_vals, winners, true);
    if (rc == CBO_OK) rc = grow(c, c->sets_batch_h_idxs, winners, true);
    return rc;
}

// log_form (cbo_acq_sweep_sets_batch_logei): small_sets_batch_kernel's LOG instantiation, the general path
// cbo_acq_sweep_batch_logei, a batch of one cbo_acq_sweep_sets_logei; ei_jitter is the log EI's jitter and must be finite.
static int sweep_sets_batch_impl(bool log_form, int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best,
                                 int task, double ei_jitter, const double *costs, int batch_size, int update_incumbent,
                                 double *best_vals, int64_t *best_idxs)
{
    // what needs no handle first
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!y_best || !costs || !best_vals || !best_idxs)
        return fail(CBO_ERR_INVALID, "NULL argument: y_best, costs, best_vals and best_idxs must be given");
    if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    if (batch_size < 1 || batch_size > CBO_MAX_BATCH)
        return fail(CBO_ERR_INVALID, "batch_size must be in 1.." + std::to_string(CBO_MAX_BATCH));
    if (update_incumbent != 0 && update_incumbent != 1) return fail(CBO_ERR_INVALID, "update_incumbent must be 0 or 1");
    if (log_form && !std::isfinite(ei_jitter)) return fail(CBO_ERR_INVALID, "jitter must be finite");
    for (int i = 0; i < n_sets; ++i) {
        if (!(costs[i] > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive (set " + std::to_string(i) + ")");
        if (!std::isfinite(y_best[i])) return fail(CBO_ERR_INVALID, "y_best must be finite (set " + std::to_string(i) + ")");
    }
    if (!gps || !cands) return fail(CBO_ERR_INVALID, "NULL argument: gps and cands must be given");
    for (int i = 0; i < n_sets; ++i) {
        const int rc = check_set_handle(gps[i], cands[i], task, gps[0]);
        if (rc != CBO_OK) return rc;
        if (batch_size > cands[i]->m)
            return fail(CBO_ERR_INVALID, "batch_size exceeds the number of candidates (set " + std::to_string(i) + ")");
    }
    if (batch_size == 1)
        return sweep_sets_impl(n_sets, gps, cands, y_best, task, ei_jitter, costs, best_vals, best_idxs, -1,
                               log_form ? kLogEiKind : kEiKind);
    cbo_ctx *c = gps[0]->ctx;
    const size_t B = (size_t)batch_size;
    std::vector<int> small;
    const int blocks = partition_small(
        n_sets, [&](int i) { return small_sweep_model(gps[i]) && cands[i]->m <= kSmallBatchMaxCands; },
        [&](int i) { return cand_blocks(cands[i]); }, small);
    const int ns = (int)small.size();
    auto prepare = [&]() -> int {
        int rc = ensure_small_buffers(c, ns, blocks);
        if (rc == CBO_OK) rc = ensure_small_batch_buffers(c, ns, blocks, batch_size);
        for (int j = 0; rc == CBO_OK && j < ns; ++j) {
            const int i = small[(size_t)j];
            rc = fill_small_set(c->sets_host[j], gps[i], cands[i], task, y_best[i], ei_jitter, costs[i]);
        }
        return rc;
    };
    return run_small_or_general(
        c, log_form ? "cbo_acq_sweep_sets_batch_logei" : "cbo_acq_sweep_sets_batch", "multi-set batch sweep: no result record",
        n_sets, small, c->small_out, prepare,
        [&](const SmallLaunch &L) {
            launch_small_sets_batch(c->stream, c->sets_host, ns, blocks, L, c->sets_batch_scratch, batch_size, update_incumbent,
                                    c->sets_batch_h_vals, c->sets_batch_h_idxs, log_form);
        },
        [&](int j, int i) {                                      // the set's winners, complete when its record is
            std::memcpy(best_vals + (size_t)i * B, c->sets_batch_h_vals.p + (size_t)j * B, sizeof(double) * B);
            std::memcpy(best_idxs + (size_t)i * B, c->sets_batch_h_idxs.p + (size_t)j * B, sizeof(int64_t) * B);
            return CBO_OK;
        },
        [&](int i) -> int {
            const int rc = ensure_fitted(gps[i]);
            if (rc != CBO_OK) return rc;
            return sweep_batch_impl(log_form, gps[i], cands[i], y_best[i], task, ei_jitter, costs[i], batch_size,
                                    update_incumbent, best_vals + (size_t)i * B, best_idxs + (size_t)i * B, nullptr, nullptr,
                                    nullptr);
        });
}

extern "C" int cbo_acq_sweep_sets_batch(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best, int task,
                                        double ei_jitter, const double *costs, int batch_size, int update_incumbent,
                                        double *best_vals, int64_t *best_idxs)
{
    return sweep_sets_batch_impl(false, n_sets, gps, cands, y_best, task, ei_jitter, costs, batch_size, update_incumbent,
                                 best_vals, best_idxs);
}

// cbo_acq_sweep_sets_batch on the log Expected Improvement: per set cbo_acq_sweep_batch_logei's bits on a
// fitted twin, in the one launch
extern "C" int cbo_acq_sweep_sets_batch_logei(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best,
                                              int task, double jitter, const double *costs, int batch_size,
                                              int update_incumbent, double *best_vals, int64_t *best_idxs)
{
    return sweep_sets_batch_impl(true, n_sets, gps, cands, y_best, task, jitter, costs, batch_size, update_incumbent, best_vals,
                                 best_idxs);
}

// a device-resident do-calculus prior (cbo_do_prior_create, below)
struct cbo_do_prior {
    cbo_ctx *ctx = nullptr;
    DoPriorView h{};                 // the view as the host filled it
    double *mem = nullptr;           // w | M | xi, one allocation
    DoPriorView *view = nullptr;     // the same view on the device
};

// the rows of one set of a refinement launch from the context's pinned buffers to the caller's arrays: a set one of whose
// starts the kernel left declined (a non-positive pivot) is declined whole, its status entries alone written
static void harvest_refined(const cbo_ctx *c, const cbo_small_refine &rf, int d, double *x_out, double *val_out,
                            double *grad_out, int *rounds_out, int *status_out)
{
    bool declined = false;
    for (int s = 0; s < rf.k; ++s) declined = declined || c->refine_status[rf.out_off + s] == CBO_REFINE_DECLINED;
    for (int s = 0; s < rf.k; ++s) {
        status_out[rf.out_off + s] = declined ? CBO_REFINE_DECLINED : c->refine_status[rf.out_off + s];
        if (declined) continue;
        rounds_out[rf.out_off + s] = c->refine_rounds[rf.out_off + s];
        val_out[rf.out_off + s] = c->refine_val[rf.out_off + s];
        std::memcpy(x_out + rf.row_off + (int64_t)s * d, c->refine_x.p + rf.row_off + (int64_t)s * d, sizeof(double) * (size_t)d);
        std::memcpy(grad_out + rf.row_off + (int64_t)s * d, c->refine_grad.p + rf.row_off + (int64_t)s * d, sizeof(double) * (size_t)d);
    }
}

// one set's handle, box, cost table and starts as every refinement entry point checks them, before anything is touched
static int check_refine_set(cbo_gp *const *gps, const cbo_refine_set *sets, int i)
{
    const std::string where = " (set " + std::to_string(i) + ")";
    const cbo_refine_set &rs = sets[i];
    if (!gps[i]) return fail(CBO_ERR_INVALID, "NULL gp" + where);
    if (gps[i]->ctx != gps[0]->ctx) return fail(CBO_ERR_INVALID, "all sets must live on one context");
    if (gps[i]->n <= 0 || gps[i]->n_pad <= 0) return fail(CBO_ERR_INVALID, "a gp holds no data" + where);
    if (rs.k < 1 || rs.k > CBO_REFINE_MAX_STARTS)
        return fail(CBO_ERR_INVALID, "the number of starts must be in 1.." + std::to_string(CBO_REFINE_MAX_STARTS) + where);
    if (!rs.starts || !rs.lo || !rs.hi || !rs.cost_fix || !rs.cost_variable)
        return fail(CBO_ERR_INVALID, "NULL argument: starts, lo, hi, cost_fix and cost_variable must be given" + where);
    const int d = gps[i]->d;
    double fix_sum = 0.0;
    for (int k = 0; k < d; ++k) {
        if (!std::isfinite(rs.lo[k]) || !std::isfinite(rs.hi[k])) return fail(CBO_ERR_INVALID, "the bounds must be finite" + where);
        if (rs.lo[k] > rs.hi[k]) return fail(CBO_ERR_INVALID, "a lower bound exceeds its upper bound" + where);
        if (!std::isfinite(rs.cost_fix[k])) return fail(CBO_ERR_INVALID, "the fixed costs must be finite" + where);
        if (rs.cost_variable[k] != 0 && rs.cost_variable[k] != 1)
            return fail(CBO_ERR_INVALID, "cost_variable must be 0 or 1" + where);
        fix_sum += rs.cost_fix[k];
    }
    if (!(fix_sum > 0.0)) return fail(CBO_ERR_INVALID, "the fixed costs must sum to a positive cost" + where);
    for (int64_t e = 0; e < (int64_t)rs.k * d; ++e)
        if (!std::isfinite(rs.starts[e])) return fail(CBO_ERR_INVALID, "the starts must be finite" + where);
    return CBO_OK;
}

// ---- gradient refinement of every set's starts (kernels_sets_refine.hip) -----------------------------------
// One launch for every set the kernel takes (small_sweep_model, no prior); the others are declined here, their status
// entries alone written.  The models are only read.  Of the routing policy this call shares the partition alone: it has no
// general path (a set the launch declines is declined), and its outputs come back behind a memset of the status words and a
// stream synchronisation, not through polled records.
// priors: NULL, or per set NULL or the do-calculus prior of the set's causal model -- such a set joins the
// kernel's causal instantiation: the sets without a prior come first in the descriptor arrays and go to one launch, the
// sets with one to a second launch on the same stream.
static int refine_sets_impl(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, const cbo_do_prior *const *priors,
                            int kind, const double *y_best, int task, double param, int max_rounds, double *x_out,
                            double *val_out, double *grad_out, int *rounds_out, int *status_out, bool logei = false,
                            bool pointcost = false)
{
    // pointcost (kind is kEiKind or kLogEiKind): the kernel's instantiation with the cost's own derivative
    const int launch_kind = pointcost ? (kind == kLogEiKind ? kLogEiPointKind : kEiPointKind) : kind;
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!gps || !sets || !y_best || !x_out || !val_out || !grad_out || !rounds_out || !status_out)
        return fail(CBO_ERR_INVALID, "NULL argument");
    if (max_rounds < 0 || max_rounds > CBO_REFINE_ROUNDS_LIMIT)
        return fail(CBO_ERR_INVALID, "max_rounds must be in 0.." + std::to_string(CBO_REFINE_ROUNDS_LIMIT));
    if (kind != kEiKind) {
        std::vector<double> ones((size_t)n_sets, 1.0);
        const int rc = check_kind_args(n_sets, kind, y_best, &task, &param, ones.data(), logei);
        if (rc != CBO_OK) return rc;
    } else {
        if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
        if (!std::isfinite(param)) return fail(CBO_ERR_INVALID, "the jitter must be finite");
    }
    for (int i = 0; i < n_sets; ++i) {
        const std::string where = " (set " + std::to_string(i) + ")";
        const int rc = check_refine_set(gps, sets, i);
        if (rc != CBO_OK) return rc;
        const int d = gps[i]->d;
        if (kind == kEiKind && !std::isfinite(y_best[i])) return fail(CBO_ERR_INVALID, "y_best must be finite" + where);
        if (priors && priors[i]) {
            if (priors[i]->ctx != gps[0]->ctx) return fail(CBO_ERR_INVALID, "a prior lives on another context" + where);
            if (gps[i]->X.sv == nullptr)
                return fail(CBO_ERR_INVALID, "a do-calculus prior was given for a model without a prior of its own" + where);
            if (priors[i]->h.n_iv != d)
                return fail(CBO_ERR_INVALID, "the prior's n_iv (" + std::to_string(priors[i]->h.n_iv) +
                                                 ") differs from the model's d (" + std::to_string(d) + ")" + where);
        }
    }
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    auto prior_of = [&](int i) -> const cbo_do_prior * { return priors ? priors[i] : nullptr; };
    // where each set's rows begin in the caller's arrays; which sets the launch takes
    std::vector<int64_t> row_off((size_t)n_sets);
    std::vector<int> out_off((size_t)n_sets), small;
    int64_t rows = 0;
    int outs = 0;
    for (int i = 0; i < n_sets; ++i) {
        row_off[(size_t)i] = rows;
        out_off[(size_t)i] = outs;
        rows += (int64_t)sets[i].k * gps[i]->d;
        outs += sets[i].k;
    }
    const int blocks = partition_small(n_sets, [&](int i) {
                                           return small_sweep_model(gps[i]) && (gps[i]->X.sv == nullptr || prior_of(i) != nullptr);
                                       },
                                       [&](int i) {
                                           const int per = small_refine_starts_per_block(gps[i]->d);
                                           return (int64_t)((sets[i].k + per - 1) / per);
                                       }, small);
    const int ns = (int)small.size();
    for (int i = 0, j = 0; i < n_sets; ++i) {
        if (j < ns && small[(size_t)j] == i) ++j;
        else std::fill_n(status_out + out_off[(size_t)i], sets[i].k, (int)CBO_REFINE_DECLINED);
    }
    if (small.empty()) return CBO_OK;
    int rc = ensure_small_buffers(c, ns, blocks);
    const size_t cap = ns < 32 ? (size_t)32 : (size_t)ns;
    if (rc == CBO_OK) rc = grow(c, c->refine_host, cap);
    if (rc == CBO_OK) rc = grow(c, c->refine_info, cap);
    if (rc == CBO_OK) rc = grow(c, c->refine_starts, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->refine_x, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->refine_grad, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->refine_val, (size_t)outs);
    if (rc == CBO_OK) rc = grow(c, c->refine_rounds, (size_t)outs);
    if (rc == CBO_OK) rc = grow(c, c->refine_status, (size_t)outs);
    if (rc != CBO_OK) return rc;
    // the launch's order: the sets without a prior, then the sets with one (each group in the caller's order)
    std::stable_partition(small.begin(), small.end(), [&](int i) { return prior_of(i) == nullptr; });
    int n_plain = 0;
    while (n_plain < ns && prior_of(small[(size_t)n_plain]) == nullptr) ++n_plain;
    for (int j = 0; j < ns; ++j) {
        const int i = small[(size_t)j];
        const cbo_gp *g = gps[i];
        cbo_small_set &st = c->sets_host[j];
        fill_small_model(st, g);
        st.cxs = st.csq = st.csv = st.cpm = st.cpv = nullptr;
        st.cld = 0; st.m = 0; st.index_offset = 0;
        st.task = task; st.y_best = (kind == kEiKind || kind == CBO_ACQ_PI || kind == kLogEiKind) ? y_best[i] : 0.0;
        st.ei_jitter = param;
        st.cost = 1.0;                                         // (the kernel prices every point itself)
        cbo_small_refine &rf = c->refine_host[j];
        std::memset(&rf, 0, sizeof(rf));
        for (int k = 0; k < g->d; ++k) {
            rf.lo[k] = sets[i].lo[k]; rf.hi[k] = sets[i].hi[k];
            rf.fix[k] = sets[i].cost_fix[k]; rf.variable[k] = sets[i].cost_variable[k];
            rf.ls[k] = g->h.ard ? g->ls[(size_t)k] : 1.0;
        }
        rf.row_off = row_off[(size_t)i]; rf.out_off = out_off[(size_t)i];
        rf.k = sets[i].k; rf.ard = g->h.ard;
        rf.prior = prior_of(i) ? prior_of(i)->view : nullptr;
        std::memcpy(c->refine_starts.p + rf.row_off, sets[i].starts, sizeof(double) * (size_t)rf.k * (size_t)g->d);
        for (int s = 0; s < rf.k; ++s) c->refine_status[rf.out_off + s] = CBO_REFINE_DECLINED;
    }
    HIP_TRY(hipMemsetAsync(c->refine_info, 0, sizeof(int) * (size_t)ns, c->stream));
    if (n_plain > 0)
        launch_small_sets_refine(c->stream, launch_kind, false, c->sets_host, c->refine_host, c->refine_starts, n_plain, blocks,
                                 c->small_scratch, c->refine_info, max_rounds, c->refine_x, c->refine_val, c->refine_grad,
                                 c->refine_rounds, c->refine_status);
    if (ns > n_plain)
        launch_small_sets_refine(c->stream, kind, true, c->sets_host.p + n_plain, c->refine_host.p + n_plain, c->refine_starts,
                                 ns - n_plain, blocks, c->small_scratch.p + small_sets_scratch_doubles(n_plain, blocks),
                                 c->refine_info.p + n_plain, max_rounds, c->refine_x, c->refine_val, c->refine_grad,
                                 c->refine_rounds, c->refine_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < ns; ++j)
        harvest_refined(c, c->refine_host[j], gps[small[(size_t)j]]->d, x_out, val_out, grad_out, rounds_out, status_out);
    return CBO_OK;
}

extern "C" int cbo_acq_refine_sets(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, int kind, const double *y_best,
                                   int task, double param, int max_rounds, double *x_out, double *val_out, double *grad_out,
                                   int *rounds_out, int *status_out)
{
    return refine_sets_impl(n_sets, gps, sets, nullptr, kind, y_best, task, param, max_rounds, x_out, val_out, grad_out,
                            rounds_out, status_out);
}

// ... for the log Expected Improvement: value log EI(x) - log c(x), gradient d log EI (the cost's gradient is
// the reference's zero).  A causal set is declined: the causal instantiation of this kind is not built.
extern "C" int cbo_acq_refine_sets_logei(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, const double *y_best,
                                         int task, double jitter, int max_rounds, double *x_out, double *val_out,
                                         double *grad_out, int *rounds_out, int *status_out)
{
    // (the scalars first, as the sweeps of this kind check them: before a handle is looked at)
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!y_best) return fail(CBO_ERR_INVALID, "NULL argument: y_best");
    const std::vector<double> ones((size_t)n_sets, 1.0);
    const int rc = check_kind_args(n_sets, kLogEiKind, y_best, &task, &jitter, ones.data(), true);
    if (rc != CBO_OK) return rc;
    return refine_sets_impl(n_sets, gps, sets, nullptr, kLogEiKind, y_best, task, jitter, max_rounds, x_out, val_out, grad_out,
                            rounds_out, status_out, true);
}

// ... with the gradient of EI / c or log EI - log c itself: the same values, d c / d x_k = variable_k sign(x_k)
// in the quotient rule.  Causal sets are declined (priors are not taken), as are larger and fp32 models.
extern "C" int cbo_acq_refine_sets_pointcost(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, int log_form,
                                             const double *y_best, int task, double jitter, int max_rounds, double *x_out,
                                             double *val_out, double *grad_out, int *rounds_out, int *status_out)
{
    const int rc = check_pointcost_args(n_sets, log_form, y_best, &task, &jitter);
    if (rc != CBO_OK) return rc;
    return refine_sets_impl(n_sets, gps, sets, nullptr, log_form ? kLogEiKind : kEiKind, y_best, task, jitter, max_rounds, x_out,
                            val_out, grad_out, rounds_out, status_out, log_form != 0, true);
}

extern "C" int cbo_acq_refine_sets_prior(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets,
                                         const cbo_do_prior *const *priors, int kind, const double *y_best, int task,
                                         double param, int max_rounds, double *x_out, double *val_out, double *grad_out,
                                         int *rounds_out, int *status_out)
{
    return refine_sets_impl(n_sets, gps, sets, priors, kind, y_best, task, param, max_rounds, x_out, val_out, grad_out,
                            rounds_out, status_out);
}

// ---- gradient refinement of every set's CONSTRAINED acquisition (kernels_sets_refine_con.hip) ---------------
// The sets without constraints take cbo_acq_refine_sets' / _logei's own route (refine_sets_impl on the sub-list: their
// bits); the sets with constraints go to one launch of small_sets_refine_con_kernel on the same stream -- those all of
// whose 1 + n_con[i] models are fp64, non-causal and of at most 128 observations; the others are declined, as is a set one
// of whose models meets a non-positive pivot in the launch.  No general path inside the call; the models are only read.
extern "C" int cbo_acq_refine_sets_constrained(int n_sets, cbo_gp *const *gps, const cbo_refine_set *sets, int log_form,
                                               const double *y_best, int task, double ei_jitter, const int *n_con,
                                               cbo_gp *const *con_gps, const double *con_value, const double *con_jitter,
                                               const int *con_sense, int max_rounds, double *x_out, double *val_out,
                                               double *grad_out, int *rounds_out, int *status_out)
{
    // what needs no handle first
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (log_form != 0 && log_form != 1) return fail(CBO_ERR_INVALID, "log_form must be 0 or 1");
    if (!gps || !sets || !y_best || !n_con || !x_out || !val_out || !grad_out || !rounds_out || !status_out)
        return fail(CBO_ERR_INVALID, "NULL argument");
    if (max_rounds < 0 || max_rounds > CBO_REFINE_ROUNDS_LIMIT)
        return fail(CBO_ERR_INVALID, "max_rounds must be in 0.." + std::to_string(CBO_REFINE_ROUNDS_LIMIT));
    if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    if (!std::isfinite(ei_jitter)) return fail(CBO_ERR_INVALID, "the jitter must be finite");
    std::vector<int64_t> first((size_t)n_sets + 1, 0);       // set i's constraints: [first[i], first[i + 1])
    for (int i = 0; i < n_sets; ++i) {
        if (!std::isfinite(y_best[i])) return fail(CBO_ERR_INVALID, "y_best must be finite (set " + std::to_string(i) + ")");
        if (n_con[i] < 0 || n_con[i] > CBO_MAX_CONSTRAINTS)
            return fail(CBO_ERR_INVALID, "n_con of set " + std::to_string(i) + " must be in 0.." +
                                             std::to_string(CBO_MAX_CONSTRAINTS));
        first[(size_t)i + 1] = first[(size_t)i] + n_con[i];
    }
    const int64_t total_con = first[(size_t)n_sets];
    if (total_con > 0) {
        if (!con_gps) return fail(CBO_ERR_INVALID, "con_gps is NULL with constraints");
        if (!con_value) return fail(CBO_ERR_INVALID, "con_value is NULL with constraints");
        if (!con_jitter) return fail(CBO_ERR_INVALID, "con_jitter is NULL with constraints");
        if (!con_sense) return fail(CBO_ERR_INVALID, "con_sense is NULL with constraints");
        for (int64_t j = 0; j < total_con; ++j) {
            if (!std::isfinite(con_value[j])) return fail(CBO_ERR_INVALID, "con_value must be finite");
            if (!std::isfinite(con_jitter[j])) return fail(CBO_ERR_INVALID, "con_jitter must be finite");
            if (con_sense[j] != CBO_CON_LE && con_sense[j] != CBO_CON_GE)
                return fail(CBO_ERR_INVALID, "con_sense must be CBO_CON_LE or CBO_CON_GE");
        }
    }
    // the handles
    for (int i = 0; i < n_sets; ++i) {
        const int rc = check_refine_set(gps, sets, i);
        if (rc != CBO_OK) return rc;
        const std::string where = " (set " + std::to_string(i) + ")";
        for (int64_t j = first[(size_t)i]; j < first[(size_t)i + 1]; ++j) {
            const cbo_gp *g = con_gps[j];
            if (!g) return fail(CBO_ERR_INVALID, "NULL constraint gp" + where);
            if (g->ctx != gps[0]->ctx) return fail(CBO_ERR_INVALID, "a constraint model lives on another context" + where);
            if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "a constraint gp holds no data" + where);
            if (g->d != gps[i]->d)
                return fail(CBO_ERR_INVALID, "a constraint model's d (" + std::to_string(g->d) + ") differs from the set's (" +
                                                 std::to_string(gps[i]->d) + ")" + where);
        }
    }
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int64_t> row_off((size_t)n_sets);
    std::vector<int> out_off((size_t)n_sets);
    int64_t rows = 0;
    int outs = 0;
    for (int i = 0; i < n_sets; ++i) {
        row_off[(size_t)i] = rows;
        out_off[(size_t)i] = outs;
        rows += (int64_t)sets[i].k * gps[i]->d;
        outs += sets[i].k;
    }

    // ---- the sets without constraints: the existing launch on their sub-list, its outputs put where the caller's rows are
    std::vector<int> plain;
    for (int i = 0; i < n_sets; ++i)
        if (n_con[i] == 0) plain.push_back(i);
    if (!plain.empty()) {
        const size_t np = plain.size();
        std::vector<cbo_gp *> pg(np);
        std::vector<cbo_refine_set> ps(np);
        std::vector<double> py(np);
        int64_t prows = 0;
        int pouts = 0;
        for (size_t a = 0; a < np; ++a) {
            const int i = plain[a];
            pg[a] = gps[i]; ps[a] = sets[i]; py[a] = y_best[i];
            prows += (int64_t)sets[i].k * gps[i]->d;
            pouts += sets[i].k;
        }
        std::vector<double> px((size_t)prows), pgr((size_t)prows), pv((size_t)pouts);
        std::vector<int> pr((size_t)pouts), pst((size_t)pouts);
        const int rc = refine_sets_impl((int)np, pg.data(), ps.data(), nullptr, log_form ? kLogEiKind : kEiKind, py.data(), task,
                                        ei_jitter, max_rounds, px.data(), pv.data(), pgr.data(), pr.data(), pst.data(),
                                        log_form != 0);
        if (rc != CBO_OK) return rc;
        int64_t r0 = 0;
        int o0 = 0;
        for (size_t a = 0; a < np; ++a) {
            const int i = plain[a], k = sets[i].k, d = gps[i]->d;
            std::copy_n(pst.data() + o0, k, status_out + out_off[(size_t)i]);
            if (pst[(size_t)o0] != CBO_REFINE_DECLINED) {        // (a declined set's other entries are not written)
                std::copy_n(px.data() + r0, (size_t)k * d, x_out + row_off[(size_t)i]);
                std::copy_n(pgr.data() + r0, (size_t)k * d, grad_out + row_off[(size_t)i]);
                std::copy_n(pv.data() + o0, k, val_out + out_off[(size_t)i]);
                std::copy_n(pr.data() + o0, k, rounds_out + out_off[(size_t)i]);
            }
            r0 += (int64_t)k * d;
            o0 += k;
        }
    }

    // ---- the sets with constraints: which of them the launch takes, and the widest of those
    std::vector<int> small;
    const int blocks = partition_small(n_sets, [&](int i) {
        if (n_con[i] == 0) return false;
        bool ok = small_sweep_model(gps[i]) && gps[i]->X.sv == nullptr;
        for (int64_t j = first[(size_t)i]; ok && j < first[(size_t)i + 1]; ++j)
            ok = small_sweep_model(con_gps[j]) && con_gps[j]->X.sv == nullptr;
        return ok;
    }, [&](int i) {
        const int per = small_refine_starts_per_block(gps[i]->d);
        return (int64_t)((sets[i].k + per - 1) / per);
    }, small);
    const int ns = (int)small.size();
    for (int i = 0, j = 0; i < n_sets; ++i) {
        if (j < ns && small[(size_t)j] == i) ++j;
        else if (n_con[i] > 0) std::fill_n(status_out + out_off[(size_t)i], sets[i].k, (int)CBO_REFINE_DECLINED);
    }
    if (small.empty()) return CBO_OK;
    int n_pairs = 0, slots = 1;
    for (int i : small) {
        n_pairs += 1 + n_con[i];
        if (1 + n_con[i] > slots) slots = 1 + n_con[i];
    }
    // descriptors for every pair, a search record and a status word per set, scratch per workgroup, the pinned rows
    int rc = ensure_small_buffers(c, n_pairs, 1);
    const size_t cap = ns < 32 ? (size_t)32 : (size_t)ns;
    if (rc == CBO_OK) rc = grow(c, c->small_scratch, small_refine_con_scratch_doubles(ns, blocks, slots));
    if (rc == CBO_OK) rc = grow(c, c->refine_pair_host, n_pairs < 32 ? (size_t)32 : (size_t)n_pairs);
    if (rc == CBO_OK) rc = grow(c, c->refine_host, cap);
    if (rc == CBO_OK) rc = grow(c, c->refine_info, cap);
    if (rc == CBO_OK) rc = grow(c, c->refine_starts, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->refine_x, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->refine_grad, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->refine_val, (size_t)outs);
    if (rc == CBO_OK) rc = grow(c, c->refine_rounds, (size_t)outs);
    if (rc == CBO_OK) rc = grow(c, c->refine_status, (size_t)outs);
    if (rc != CBO_OK) return rc;
    int p = 0;
    std::vector<int> first_pair((size_t)ns, 0);
    for (int j = 0; j < ns; ++j) {
        const int i = small[(size_t)j];
        first_pair[(size_t)j] = p;
        for (int a = 0; a <= n_con[i]; ++a, ++p) {
            const int64_t cj = first[(size_t)i] + a - 1;
            const cbo_gp *g = a == 0 ? gps[i] : con_gps[cj];
            cbo_small_set &st = c->sets_host[p];
            fill_small_model(st, g);
            st.cxs = st.csq = st.csv = st.cpm = st.cpv = nullptr;
            st.cld = 0; st.m = 0; st.index_offset = 0;
            // (a constraint's sense, value and jitter ride in task, y_best and ei_jitter)
            st.task = a == 0 ? task : con_sense[cj];
            st.y_best = a == 0 ? y_best[i] : con_value[cj];
            st.ei_jitter = a == 0 ? ei_jitter : con_jitter[cj];
            st.cost = 1.0;                                     // (the kernel prices every point itself)
            for (int k = 0; k < CBO_MAX_DIM; ++k) c->refine_pair_host[p].ls[k] = (k < g->d && g->h.ard) ? g->ls[(size_t)k] : 1.0;
        }
        cbo_small_refine &rf = c->refine_host[j];
        std::memset(&rf, 0, sizeof(rf));
        const int d = gps[i]->d;
        for (int k = 0; k < d; ++k) {
            rf.lo[k] = sets[i].lo[k]; rf.hi[k] = sets[i].hi[k];
            rf.fix[k] = sets[i].cost_fix[k]; rf.variable[k] = sets[i].cost_variable[k];
            rf.ls[k] = 1.0;                                    // (every model's own are in refine_pair_host)
        }
        rf.row_off = row_off[(size_t)i]; rf.out_off = out_off[(size_t)i];
        rf.k = sets[i].k;
        std::memcpy(c->refine_starts.p + rf.row_off, sets[i].starts, sizeof(double) * (size_t)rf.k * (size_t)d);
        for (int s = 0; s < rf.k; ++s) c->refine_status[rf.out_off + s] = CBO_REFINE_DECLINED;
    }
    for (int j = 0; j < ns; ++j) c->sets_host[j].pad_ = first_pair[(size_t)j];      // the table: set j's first pair
    HIP_TRY(hipMemsetAsync(c->refine_info, 0, sizeof(int) * (size_t)ns, c->stream));
    launch_small_sets_refine_con(c->stream, log_form != 0, c->sets_host, c->refine_pair_host, n_pairs, c->refine_host,
                                 c->refine_starts, ns, blocks, slots, c->small_scratch, c->refine_info, max_rounds, c->refine_x,
                                 c->refine_val, c->refine_grad, c->refine_rounds, c->refine_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < ns; ++j)
        harvest_refined(c, c->refine_host[j], gps[small[(size_t)j]]->d, x_out, val_out, grad_out, rounds_out, status_out);
    return CBO_OK;
}

// ---- constrained acquisition for every set of a trial (kernels_sets_con.hip) ------------------------------
// cbo_acq_sweep_sets' routing applied to every model of a set: a set all of whose 1 + n_con[i] models are fp64 with at most
// 128 observations is factored AND swept, model after model, by the workgroups of one launch; every other set -- and a set one
// of whose models met a non-positive pivot there -- takes cbo_gp_fit on its unfitted models and cbo_acq_sweep_constrained.
// log_form (cbo_acq_sweep_sets_constrained_log): the same routing with the log epilogues on both paths.
static int sweep_sets_constrained_impl(bool log_form, int n_sets, cbo_gp *const *gps, cbo_cands *const *cands,
                                       const double *y_best, int task, double ei_jitter, const double *costs, const int *n_con,
                                       cbo_gp *const *con_gps, cbo_cands *const *con_cands, const double *con_value,
                                       const double *con_jitter, const int *con_sense, double *best_vals, int64_t *best_idxs)
{
    // what needs no handle first
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!y_best || !costs || !n_con || !best_vals || !best_idxs)
        return fail(CBO_ERR_INVALID, "NULL argument: y_best, costs, n_con, best_vals and best_idxs must be given");
    if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    if (log_form && !std::isfinite(ei_jitter)) return fail(CBO_ERR_INVALID, "jitter must be finite");
    int64_t total_con = 0;
    for (int i = 0; i < n_sets; ++i) {
        if (log_form && !std::isfinite(y_best[i])) return fail(CBO_ERR_INVALID, "y_best must be finite");
        if (!(costs[i] > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive (set " + std::to_string(i) + ")");
        if (n_con[i] < 0 || n_con[i] > CBO_MAX_CONSTRAINTS)
            return fail(CBO_ERR_INVALID, "n_con of set " + std::to_string(i) + " must be in 0.." +
                                             std::to_string(CBO_MAX_CONSTRAINTS));
        total_con += n_con[i];
    }
    if (total_con > 0) {
        if (!con_value) return fail(CBO_ERR_INVALID, "con_value is NULL with constraints");
        if (!con_jitter) return fail(CBO_ERR_INVALID, "con_jitter is NULL with constraints");
        if (!con_sense) return fail(CBO_ERR_INVALID, "con_sense is NULL with constraints");
        for (int64_t j = 0; j < total_con; ++j) {
            if (!std::isfinite(con_value[j])) return fail(CBO_ERR_INVALID, "con_value must be finite");
            if (!std::isfinite(con_jitter[j])) return fail(CBO_ERR_INVALID, "con_jitter must be finite");
            if (con_sense[j] != CBO_CON_LE && con_sense[j] != CBO_CON_GE)
                return fail(CBO_ERR_INVALID, "con_sense must be CBO_CON_LE or CBO_CON_GE");
        }
    }
    // the handles
    if (!gps || !cands) return fail(CBO_ERR_INVALID, "NULL argument: gps and cands must be given");
    if (total_con > 0 && (!con_gps || !con_cands))
        return fail(CBO_ERR_INVALID, "con_gps / con_cands is NULL with constraints");
    std::vector<int64_t> first((size_t)n_sets + 1, 0);       // set i's constraints: [first[i], first[i + 1])
    for (int i = 0; i < n_sets; ++i) first[(size_t)i + 1] = first[(size_t)i] + n_con[i];
    for (int i = 0; i < n_sets; ++i) {
        cbo_gp *sg[kConMaxModels];
        cbo_cands *sk[kConMaxModels];
        int nm = 0;
        sg[nm] = gps[i]; sk[nm] = cands[i]; ++nm;
        for (int64_t j = first[(size_t)i]; j < first[(size_t)i + 1]; ++j, ++nm) { sg[nm] = con_gps[j]; sk[nm] = con_cands[j]; }
        for (int a = 0; a < nm; ++a) {
            const int rc = check_set_handle(sg[a], sk[a], task, gps[0], "models");
            if (rc != CBO_OK) return rc;
            if (sk[a]->m != sk[0]->m) return fail(CBO_ERR_INVALID, "the candidate sets of a set differ in size");
            for (int b = 0; b < a; ++b)
                if (sk[b] == sk[a] && sg[b] != sg[a])
                    return fail(CBO_ERR_INVALID, "one candidate set with two models: its scaled points are one model's");
        }
    }
    cbo_ctx *c = gps[0]->ctx;
    std::vector<int> small;
    const int blocks = partition_small(n_sets, [&](int i) {          // every model of the set
        bool ok = small_sweep_model(gps[i]);
        for (int64_t j = first[(size_t)i]; ok && j < first[(size_t)i + 1]; ++j) ok = small_sweep_model(con_gps[j]);
        return ok;
    }, [&](int i) { return cand_blocks(cands[i]); }, small);
    const int ns = (int)small.size();
    int n_pairs = 0, max_pairs = 1;
    for (int i : small) {
        n_pairs += 1 + n_con[i];
        if (1 + n_con[i] > max_pairs) max_pairs = 1 + n_con[i];
    }
    auto prepare = [&]() -> int {
        // descriptors for every pair; status words, tickets, records, scratch and partial winners per set
        int rc = ensure_small_buffers(c, n_pairs, 1);
        if (rc == CBO_OK) rc = ensure_small_buffers(c, ns, blocks);
        if (rc != CBO_OK) return rc;
        int p = 0;
        std::vector<int> first_pair((size_t)ns, 0);
        for (int j = 0; j < ns; ++j) {
            const int i = small[(size_t)j];
            first_pair[(size_t)j] = p;
            for (int a = 0; a <= n_con[i]; ++a, ++p) {
                const int64_t cj = first[(size_t)i] + a - 1;
                cbo_small_set &st = c->sets_host[p];
                // (a constraint's sense, value and jitter ride in task, y_best and ei_jitter)
                rc = a == 0 ? fill_small_set(st, gps[i], cands[i], task, y_best[i], ei_jitter, costs[i])
                            : fill_small_set(st, con_gps[cj], con_cands[cj], con_sense[cj], con_value[cj], con_jitter[cj],
                                             costs[i]);
                if (rc != CBO_OK) return rc;
                st.index_offset = cands[i]->index_offset;       // (the set's: the objective's candidates name the winner)
            }
        }
        for (int j = 0; j < ns; ++j) c->sets_host[j].pad_ = first_pair[(size_t)j];      // the table: set j's first pair
        return CBO_OK;
    };
    return run_small_or_general(
        c, log_form ? "cbo_acq_sweep_sets_constrained_log" : "cbo_acq_sweep_sets_constrained",
        "multi-set sweep: no result record", n_sets, small, c->small_out, prepare,
        [&](const SmallLaunch &L) {
            launch_small_sets_con(c->stream, c->sets_host, n_pairs, ns, max_pairs, blocks, L, log_form);
        },
        [&](int j, int i) { return harvest_winner(c, j, i, best_vals, best_idxs); },
        [&](int i) -> int {
            const int64_t f = first[(size_t)i];
            int rc = ensure_fitted(gps[i]);
            for (int64_t j = f; rc == CBO_OK && j < first[(size_t)i + 1]; ++j) rc = ensure_fitted(con_gps[j]);
            if (rc != CBO_OK) return rc;
            return sweep_constrained_impl(log_form, gps[i], cands[i], y_best[i], task, ei_jitter, costs[i], n_con[i],
                                          n_con[i] ? con_gps + f : nullptr, n_con[i] ? con_cands + f : nullptr,
                                          n_con[i] ? con_value + f : nullptr, n_con[i] ? con_jitter + f : nullptr,
                                          n_con[i] ? con_sense + f : nullptr, nullptr, nullptr, nullptr, &best_vals[i],
                                          &best_idxs[i]);
        });
}

extern "C" int cbo_acq_sweep_sets_constrained(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const double *y_best,
                                              int task, double ei_jitter, const double *costs, const int *n_con,
                                              cbo_gp *const *con_gps, cbo_cands *const *con_cands, const double *con_value,
                                              const double *con_jitter, const int *con_sense, double *best_vals,
                                              int64_t *best_idxs)
{
    return sweep_sets_constrained_impl(false, n_sets, gps, cands, y_best, task, ei_jitter, costs, n_con, con_gps, con_cands,
                                       con_value, con_jitter, con_sense, best_vals, best_idxs);
}

// The log form for every set of a trial: per set cbo_acq_sweep_constrained_log's bits on fitted twins.
extern "C" int cbo_acq_sweep_sets_constrained_log(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands,
                                                  const double *y_best, int task, double ei_jitter, const double *costs,
                                                  const int *n_con, cbo_gp *const *con_gps, cbo_cands *const *con_cands,
                                                  const double *con_value, const double *con_jitter, const int *con_sense,
                                                  double *best_vals, int64_t *best_idxs)
{
    return sweep_sets_constrained_impl(true, n_sets, gps, cands, y_best, task, ei_jitter, costs, n_con, con_gps, con_cands,
                                       con_value, con_jitter, con_sense, best_vals, best_idxs);
}

// ---- the causal EI marginalised over hyper-parameter samples (kernels_hyper.hip) -------------------------
// The general path of cbo_acq_sweep_hyper: per sample the model's own set_hyper + fit + sweep, the acquisition kept on the
// device and added into the running sum; then the division with the arg-max; then the model back as it was.
// log_form: per sample cbo_acq_sweep_logei's steps at cost 1 in the place of cbo_acq_sweep's, the term pushed
// into the streaming log-sum-exp's (M, S) = (hyper_sum, hyper_lse_s); the close subtracts log H and the log cost.
static int hyper_general_path(cbo_gp *g, cbo_cands *k, int n_samples, int n_ls, const double *hyper, double y_best, int task,
                              double ei_jitter, double cost, double *acq_out, double *best_val, int64_t *best_idx,
                              bool log_form = false)
{
    cbo_ctx *c = g->ctx;
    const double variance0 = g->h.variance, noise0 = g->noise_var;
    const std::vector<double> ls0 = g->ls;
    const bool was_fitted = g->fitted;
    const int nb = acq_blocks_for(k->m);
    int rc = grow(c, c->hyper_sum, (size_t)k->m_pad);
    if (rc == CBO_OK && log_form) rc = grow(c, c->hyper_lse_s, (size_t)k->m_pad);
    for (int h = 0; h < n_samples && rc == CBO_OK; ++h) {
        const double *row = hyper + (size_t)h * (size_t)(n_ls + 2);
        rc = cbo_gp_set_hyper(g, row[0], row + 1, row[1 + n_ls]);
        if (rc == CBO_OK) rc = cbo_gp_fit(g, nullptr, nullptr);
        if (rc == CBO_OK) rc = enqueue_vectors(g, k);
        const double *q_src = nullptr, *mu_src = nullptr;
        if (rc == CBO_OK) rc = settle_vectors(g, k, false, &q_src, &mu_src);
        // (acq_out only says that the per-candidate values are wanted: they stay in the context's vector)
        if (rc == CBO_OK) rc = enqueue_finish(g, k, y_best, task, ei_jitter, log_form ? 1.0 : cost, c->acq, nullptr, nullptr,
                                              q_src, mu_src, false, false, nullptr, log_form ? kLogEiKind : 0);
        if (rc != CBO_OK) break;
        if (log_form) launch_hyper_lse_accumulate(c->stream, c->hyper_sum, c->hyper_lse_s, c->acq, k->m, h == 0, nb);
        else launch_hyper_accumulate(c->stream, c->hyper_sum, c->acq, k->m, h == 0, nb);
        if (hipGetLastError() != hipSuccess) rc = fail(CBO_ERR_HIP, "hyper_accumulate_kernel launch");
    }
    if (rc == CBO_OK) {
        if (log_form)
            launch_hyper_lse_finish(c->stream, c->hyper_sum, c->hyper_lse_s, k->m, n_samples, cost,
                                    acq_out ? c->acq.p : nullptr, c->part_val, c->part_idx, k->index_offset, nb);
        else
            launch_hyper_finish(c->stream, c->hyper_sum, k->m, n_samples, acq_out ? c->acq.p : nullptr, c->part_val,
                                c->part_idx, k->index_offset, nb);
        launch_argmax_final(c->stream, c->part_val, c->part_idx, nb, c->h_best_val, c->h_best_idx);
        if (hipGetLastError() != hipSuccess) rc = fail(CBO_ERR_HIP, "hyper_finish_kernel launch");
        if (rc == CBO_OK) rc = copy_posterior_out(c, k, acq_out, nullptr, nullptr);
        if (rc == CBO_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(CBO_ERR_HIP, "hipStreamSynchronize");
        if (rc == CBO_OK) complete_finish(c, best_val, best_idx);
    }
    // the model back as it was, whatever happened (the first error is the one reported)
    const std::string err = g_err;
    int back = cbo_gp_set_hyper(g, variance0, ls0.data(), noise0);
    if (back == CBO_OK && was_fitted) back = cbo_gp_fit(g, nullptr, nullptr);
    if (rc != CBO_OK) { g_err = err; return rc; }
    return back;
}

// cbo_acq_sweep_hyper and, with log_form, cbo_acq_sweep_hyper_log: the same checks, routing and paths, the
// kernels' other instantiation
static int sweep_hyper_impl(const char *name, bool log_form, cbo_gp *g, cbo_cands *k, int n_samples, const double *hyper,
                            double y_best, int task, double ei_jitter, double cost, double *acq_out, double *best_val,
                            int64_t *best_idx)
{
    int rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    if (n_samples < 1 || n_samples > CBO_MAX_HYPER_SAMPLES)
        return fail(CBO_ERR_INVALID, "the number of hyper-parameter samples must be in 1.." + std::to_string(CBO_MAX_HYPER_SAMPLES));
    if (!hyper) return fail(CBO_ERR_INVALID, "hyper is NULL");
    if (!acq_out && (!best_val || !best_idx)) return fail(CBO_ERR_INVALID, "nothing to return: acq_out, best_val / best_idx are NULL");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    if (g->n <= 0 || g->n_pad <= 0) return fail(CBO_ERR_INVALID, "gp holds no data (a previous upload failed)");
    const int n_ls = g->h.ard ? g->d : 1;
    const int row_len = n_ls + 2;
    for (int h = 0; h < n_samples; ++h) {
        const double *row = hyper + (size_t)h * (size_t)row_len;
        for (int j = 0; j <= n_ls; ++j)
            if (!std::isfinite(row[j]) || !(row[j] > 0.0))
                return fail(CBO_ERR_INVALID, "hyper row " + std::to_string(h) + ": variance and lengthscales must be finite and positive");
        if (!std::isfinite(row[1 + n_ls]) || row[1 + n_ls] < 0.0)
            return fail(CBO_ERR_INVALID, "hyper row " + std::to_string(h) + ": noise_var must be finite and non-negative");
    }
    // The one-item case of the routing policy, written out: run_small_or_general's two vectors would be this call's only
    // heap allocations.
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (small_sweep_model(g) && cand_blocks(k) <= kMaxGridBlocks) {
        const int blocks = (int)cand_blocks(k);
        rc = ensure_small_buffers(c, 1, blocks > n_samples ? blocks : n_samples);
        if (rc == CBO_OK) rc = grow(c, c->hyper_host, (size_t)CBO_MAX_HYPER_SAMPLES * (CBO_MAX_DIM + 2));
        if (rc == CBO_OK && acq_out) rc = grow_vectors(c, k->m_pad);
        if (rc != CBO_OK) return rc;
        std::memcpy(c->hyper_host.p, hyper, sizeof(double) * (size_t)n_samples * (size_t)row_len);
        cbo_small_set st{};
        fill_hyper_set(st, g, k, task, y_best, ei_jitter, cost);
        auto launch = [&](int seq) -> int {
            launch_hyper_avg(c->stream, st, k->raw, c->hyper_host, n_samples, n_ls, acq_out ? c->acq.p : nullptr, blocks,
                             c->hyper_schedule, small_launch(c, seq), log_form);
            HIP_TRY(hipGetLastError());
            return CBO_OK;
        };
        rc = polled_launch(c, name, c->small_out.p, 1, "marginalised sweep: no result record", launch);
        if (rc != CBO_OK) return rc;
        if (c->small_out[0].info == 0) {
            if (acq_out) {
                HIP_TRY(hipMemcpyAsync(acq_out, c->acq, sizeof(double) * k->m, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
            }
            if (best_val) *best_val = c->small_out[0].best_val;
            if (best_idx) *best_idx = c->small_out[0].best_idx;
            return CBO_OK;
        }
        // a sample that is not positive definite as assembled: the jitchol ladder of the general path
    }
    return hyper_general_path(g, k, n_samples, n_ls, hyper, y_best, task, ei_jitter, cost, acq_out, best_val, best_idx,
                              log_form);
}

extern "C" int cbo_acq_sweep_hyper(cbo_gp *g, cbo_cands *k, int n_samples, const double *hyper, double y_best, int task,
                                   double ei_jitter, double cost, double *acq_out, double *best_val, int64_t *best_idx)
{
    return sweep_hyper_impl("cbo_acq_sweep_hyper", false, g, k, n_samples, hyper, y_best, task, ei_jitter, cost, acq_out,
                            best_val, best_idx);
}

// The log of the marginalised EI: log((1 / H) sum_h EI_h) - log cost, the log-sum-exp of cbo_acq_sweep_logei's
// terms at cost 1.  cbo_acq_sweep_logei's scalar refusals first (a non-finite jitter or y_best), then cbo_acq_sweep_hyper's.
extern "C" int cbo_acq_sweep_hyper_log(cbo_gp *g, cbo_cands *k, int n_samples, const double *hyper, double y_best, int task,
                                       double jitter, double cost, double *acq_out, double *best_val, int64_t *best_idx)
{
    if (!std::isfinite(jitter)) return fail(CBO_ERR_INVALID, "jitter must be finite");
    if (!std::isfinite(y_best)) return fail(CBO_ERR_INVALID, "y_best must be finite");
    return sweep_hyper_impl("cbo_acq_sweep_hyper_log", true, g, k, n_samples, hyper, y_best, task, jitter, cost, acq_out,
                            best_val, best_idx);
}

// ---- the marginalised EI for every set of a trial (hyper_sets_kernel) ------------------------------------
// sweep_sets_impl's routing with cbo_acq_sweep_hyper's two paths: the fp64 models of at most 128 observations are factored
// and swept, sample after sample, by the workgroups of one launch (two from kSmallTwoPhaseFromBlocks blocks per set on, when
// the slots fit); every other set -- and a set whose record reports a non-positive pivot at any sample -- takes
// hyper_general_path, which restores its model.
static int sweep_sets_hyper_impl(const char *name, bool log_form, int n_sets, cbo_gp *const *gps, cbo_cands *const *cands,
                                 const int *n_samples, const double *const *hyper, const double *y_best, int task,
                                 double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs)
{
    // what needs no handle first
    if (n_sets <= 0) return fail(CBO_ERR_INVALID, "n_sets must be positive");
    if (!n_samples || !hyper || !y_best || !costs || !best_vals || !best_idxs)
        return fail(CBO_ERR_INVALID, "NULL argument: n_samples, hyper, y_best, costs, best_vals and best_idxs must be given");
    if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    for (int i = 0; i < n_sets; ++i) {
        if (n_samples[i] < 1 || n_samples[i] > CBO_MAX_HYPER_SAMPLES)
            return fail(CBO_ERR_INVALID, "set " + std::to_string(i) + ": the number of hyper-parameter samples must be in 1.." +
                                             std::to_string(CBO_MAX_HYPER_SAMPLES));
        if (!hyper[i]) return fail(CBO_ERR_INVALID, "hyper of set " + std::to_string(i) + " is NULL");
        if (!(costs[i] > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive (set " + std::to_string(i) + ")");
        if (log_form && !std::isfinite(y_best[i]))
            return fail(CBO_ERR_INVALID, "y_best must be finite (set " + std::to_string(i) + ")");
    }
    if (log_form && !std::isfinite(ei_jitter)) return fail(CBO_ERR_INVALID, "jitter must be finite");
    // the handles, then the rows (whose length is the model's)
    if (!gps || !cands) return fail(CBO_ERR_INVALID, "NULL argument: gps and cands must be given");
    int rc = check_set_handles(n_sets, gps, cands, task);
    if (rc != CBO_OK) return rc;
    std::vector<int> n_ls((size_t)n_sets);
    for (int i = 0; i < n_sets; ++i) {
        const int L = n_ls[(size_t)i] = gps[i]->h.ard ? gps[i]->d : 1;
        for (int h = 0; h < n_samples[i]; ++h) {
            const double *row = hyper[i] + (size_t)h * (size_t)(L + 2);
            const std::string where = "set " + std::to_string(i) + ", hyper row " + std::to_string(h);
            for (int j = 0; j <= L; ++j)
                if (!std::isfinite(row[j]) || !(row[j] > 0.0))
                    return fail(CBO_ERR_INVALID, where + ": variance and lengthscales must be finite and positive");
            if (!std::isfinite(row[1 + L]) || row[1 + L] < 0.0)
                return fail(CBO_ERR_INVALID, where + ": noise_var must be finite and non-negative");
        }
    }
    cbo_ctx *c = gps[0]->ctx;
    std::vector<int> small;
    const int blocks = partition_small(n_sets, [&](int i) { return small_sweep_model(gps[i]); },
                                       [&](int i) { return cand_blocks(cands[i]); }, small);
    const int ns = (int)small.size();
    size_t total = 0, doubles = 0;                              // samples and doubles of the small sets' rows
    for (int i : small) {
        total += (size_t)n_samples[i];
        doubles += (size_t)n_samples[i] * (size_t)(n_ls[(size_t)i] + 2);
    }
    // two launches from kSmallTwoPhaseFromBlocks blocks per set on (CBO_HIP_HYPER_SCHEDULE=1 / =2: never / always) -- but
    // only when one scratch slot per sample of the call fits the workspace limit; else every workgroup factors for itself
    bool two_phase = c->hyper_schedule == 2 || (c->hyper_schedule != 1 && blocks >= kSmallTwoPhaseFromBlocks);
    if (two_phase && sizeof(double) * hyper_sets_scratch_doubles(ns, blocks, (int)total, true) > c->max_ws_bytes)
        two_phase = false;
    auto prepare = [&]() -> int {
        int rc = ensure_small_buffers(c, ns, 1);                // records, status words, tickets
        if (rc == CBO_OK) rc = grow(c, c->hyper_sets_host, ns < 32 ? (size_t)32 : (size_t)ns);
        if (rc == CBO_OK) rc = grow(c, c->hyper_host, doubles);
        if (rc == CBO_OK) rc = grow(c, c->small_scratch, hyper_sets_scratch_doubles(ns, blocks, (int)total, two_phase));
        if (rc == CBO_OK) rc = grow(c, c->small_part_val, (size_t)ns * (size_t)blocks);
        if (rc == CBO_OK) rc = grow(c, c->small_part_idx, (size_t)ns * (size_t)blocks);
        if (rc != CBO_OK) return rc;
        size_t at = 0;
        int first = 0;
        for (int j = 0; j < ns; ++j) {
            const int i = small[(size_t)j];
            const size_t len = (size_t)n_samples[i] * (size_t)(n_ls[(size_t)i] + 2);
            std::memcpy(c->hyper_host.p + at, hyper[i], sizeof(double) * len);
            HyperSet &hs = c->hyper_sets_host[j];
            hs = HyperSet{};
            fill_hyper_set(hs.a.st, gps[i], cands[i], task, y_best[i], ei_jitter, costs[i]);
            hs.a.craw = cands[i]->raw; hs.a.hyper = c->hyper_host.p + at; hs.a.n_samples = n_samples[i];
            hs.a.n_ls = n_ls[(size_t)i]; hs.a.acq_out = nullptr;
            hs.first = first;
            at += len;
            first += n_samples[i];
        }
        return CBO_OK;
    };
    return run_small_or_general(
        c, name, "marginalised multi-set sweep: no result record", n_sets, small, c->small_out, prepare,
        [&](const SmallLaunch &L) {
            launch_hyper_sets(c->stream, c->hyper_sets_host, ns, blocks, (int)total, two_phase, L, log_form);
        },
        [&](int j, int i) { return harvest_winner(c, j, i, best_vals, best_idxs); },
        // a larger or fp32 model, or a sample that is not positive definite as assembled: the general path, model restored
        [&](int i) {
            return hyper_general_path(gps[i], cands[i], n_samples[i], n_ls[(size_t)i], hyper[i], y_best[i], task, ei_jitter,
                                      costs[i], nullptr, &best_vals[i], &best_idxs[i], log_form);
        });
}

extern "C" int cbo_acq_sweep_sets_hyper(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const int *n_samples,
                                        const double *const *hyper, const double *y_best, int task, double ei_jitter,
                                        const double *costs, double *best_vals, int64_t *best_idxs)
{
    return sweep_sets_hyper_impl("cbo_acq_sweep_sets_hyper", false, n_sets, gps, cands, n_samples, hyper, y_best, task,
                                 ei_jitter, costs, best_vals, best_idxs);
}

// cbo_acq_sweep_sets_hyper for the log form: per set cbo_acq_sweep_hyper_log's bits
extern "C" int cbo_acq_sweep_sets_hyper_log(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, const int *n_samples,
                                            const double *const *hyper, const double *y_best, int task, double jitter,
                                            const double *costs, double *best_vals, int64_t *best_idxs)
{
    return sweep_sets_hyper_impl("cbo_acq_sweep_sets_hyper_log", true, n_sets, gps, cands, n_samples, hyper, y_best, task,
                                 jitter, costs, best_vals, best_idxs);
}

// The general path's reduction over terms the caller hands in: row h of `terms` goes through
// hyper_lse_accumulate_kernel in order, hyper_lse_finish_kernel closes with n_rows and the cost -- the kernels, and so the bits,
// of cbo_acq_sweep_hyper_log's general path, and by lse_stream.h of its one-launch path.
extern "C" int cbo_lse_rows(cbo_ctx *c, int n_rows, int64_t m, const double *terms, double cost, double *out)
{
    if (!c || !terms || !out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (n_rows < 1 || n_rows > CBO_MAX_HYPER_SAMPLES)
        return fail(CBO_ERR_INVALID, "n_rows must be in 1.." + std::to_string(CBO_MAX_HYPER_SAMPLES));
    if (m < 1) return fail(CBO_ERR_INVALID, "m must be positive");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    HIP_TRY(hipSetDevice(c->device));
    const int nb = acq_blocks_for(m);
    int rc = grow(c, c->hyper_sum, (size_t)m);
    if (rc == CBO_OK) rc = grow(c, c->hyper_lse_s, (size_t)m);
    if (rc == CBO_OK) rc = grow(c, c->acq, (size_t)m);
    if (rc != CBO_OK) return rc;
    for (int h = 0; h < n_rows; ++h) {
        // (pageable memory: the copy has read row h when it returns; the stream orders it behind the previous row's kernel)
        HIP_TRY(hipMemcpyAsync(c->acq, terms + (size_t)h * (size_t)m, sizeof(double) * (size_t)m, hipMemcpyHostToDevice,
                               c->stream));
        launch_hyper_lse_accumulate(c->stream, c->hyper_sum, c->hyper_lse_s, c->acq, m, h == 0, nb);
        HIP_TRY(hipGetLastError());
    }
    launch_hyper_lse_finish(c->stream, c->hyper_sum, c->hyper_lse_s, m, n_rows, cost, c->acq, c->part_val, c->part_idx, 0, nb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->acq, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

// One reference-scale trial in ONE call (src/CBO.py:143-173, CBO.intervene): the model of the set that was intervened on
// last receives its new data (src/CBO.py:224-235 rebuilds it; src/Monitor.py:160), every exploration set is swept
// (src/CBO.py:237-260) and the set to intervene on next is picked (src/CBO.py:269-277) -- cbo_gp_upload_data +
// cbo_acq_sweep_sets + cbo_argmax_sets without the three trips through the caller's language, which at the reference's
// model sizes (one 29 us launch for all sets) cost as much as the device work.
static int trial_step_impl(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int refit_set, int64_t n,
                           const double *X, const double *y, const double *pm, const double *pv, const double *y_best,
                           int task, double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs,
                           int *chosen_out, int kind);

extern "C" int cbo_trial_step(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int refit_set, int64_t n,
                              const double *X, const double *y, const double *pm, const double *pv, const double *y_best,
                              int task, double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs,
                              int *chosen_out)
{
    return trial_step_impl(n_sets, gps, cands, refit_set, n, X, y, pm, pv, y_best, task, ei_jitter, costs, best_vals,
                           best_idxs, chosen_out, kEiKind);
}

// cbo_trial_step with a point-wise epilogue: everything the sweep would refuse is refused before the
// model's host-side state moves to the new data
extern "C" int cbo_trial_step_kind(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int refit_set, int64_t n,
                                   const double *X, const double *y, const double *pm, const double *pv, int kind,
                                   const double *y_best, int task, double param, const double *costs, double *best_vals,
                                   int64_t *best_idxs, int *chosen_out)
{
    const int rc = check_kind_args(n_sets, kind, y_best, &task, &param, costs);
    if (rc != CBO_OK) return rc;
    if (!gps || !cands || !best_vals || !best_idxs || !chosen_out) return fail(CBO_ERR_INVALID, "bad argument");
    return trial_step_impl(n_sets, gps, cands, refit_set, n, X, y, pm, pv, y_best, task, param, costs, best_vals, best_idxs,
                           chosen_out, kind);
}

static int trial_step_impl(int n_sets, cbo_gp *const *gps, cbo_cands *const *cands, int refit_set, int64_t n,
                           const double *X, const double *y, const double *pm, const double *pv, const double *y_best,
                           int task, double ei_jitter, const double *costs, double *best_vals, int64_t *best_idxs,
                           int *chosen_out, int kind)
{
    if (n_sets <= 0 || !gps || !chosen_out) return fail(CBO_ERR_INVALID, "bad argument");
    if (refit_set >= n_sets) return fail(CBO_ERR_INVALID, "refit_set out of range");
    int staged = -1;
    if (refit_set >= 0) {
        cbo_gp *g = gps[refit_set];
        if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
        if (!cands || !y_best || !costs || !best_vals || !best_idxs) return fail(CBO_ERR_INVALID, "bad argument");
        cbo_ctx *c = g->ctx;
        // The upload folded into the sweep's one launch: when the set takes the one-launch path (as every model the
        // reference builds does) its new data go to the staging buffer and the launch's workgroups prepare the points
        // from there themselves -- no preparation launch, no stream synchronisation (15 of a trial's 57 us).  The same
        // conditions as sweep_sets_impl's, plus: the padded size and the prior-ness do not change, the data fit the buffer.
        bool fuse = c->small_sets && g->dtype == CBO_DTYPE_F64 && g->n_pad == kPadN && n > 0 && n <= kPadN && X && y &&
                    ((pm == nullptr) == (pv == nullptr)) && ((pv != nullptr) == (g->X.sv != nullptr)) &&
                    sizeof(double) * (size_t)(n * g->d + n + (pv ? 2 * n : 0)) <= kStageBytes;
        // (everything the sweep would refuse is refused BEFORE the model's host-side state moves to the new data)
        for (int i = 0; i < n_sets; ++i) {
            const int rc = check_set_handle(gps[i], cands[i], task, g, "sets", i != refit_set);   // (its data are on their way)
            if (rc != CBO_OK) return rc;
            if (gps[i]->dtype == CBO_DTYPE_F64 && gps[i]->n_pad == kPadN && cand_blocks(cands[i]) > kMaxGridBlocks) fuse = false;
            // the same model in two sets: the other copy's workgroups would read the resident arrays while the staged set's
            // first workgroup rewrites them in the same launch -- the plain upload first, then the sweep
            if (i != refit_set && gps[i] == g) fuse = false;
        }
        if (fuse) {
            HIP_TRY(hipSetDevice(c->device));
            const int rc = stage_data(g, n, X, y, pm, pv);
            if (rc != CBO_OK) return rc;
            g->n = n;
            g->X.n = n;
            g->fitted = false;
            staged = refit_set;
        } else {
            const int rc = cbo_gp_upload_data(g, n, X, y, pm, pv);      // unfitted: the sweep below refits it
            if (rc != CBO_OK) return rc;
        }
    }
    int rc = sweep_sets_impl(n_sets, gps, cands, y_best, task, ei_jitter, costs, best_vals, best_idxs, staged, kind);
    if (rc != CBO_OK && staged >= 0) {
        // The launch that was to carry the new data into the resident arrays failed (or was never queued): the host-side
        // state already describes the new data, the device arrays may hold either.  Finish the upload from the staging
        // buffer by the plain path -- it is the caller's data either way -- so that model and arrays agree again; if even
        // that fails the model is marked as holding nothing (n = 0: every later call refuses it until new data arrive).
        cbo_gp *g = gps[staged];
        const int up = cbo_gp_upload_data(g, n, X, y, pm, pv);
        if (up != CBO_OK) {
            g->n = 0;
            g->X.n = 0;
            g->fitted = false;
        }
        return rc;
    }
    if (rc != CBO_OK) return rc;
    return cbo_argmax_sets(best_vals, n_sets, chosen_out);
}

// What the context has measured and chosen for cbo_gp_fit_sweep, one line per shape, as text (scripts/schedule_scan.py,
// profiles/r04_schedule_crossover.txt).  Returns the number of shapes still exploring (0 = every schedule is settled), or a
// CBO_ERR_* code (they are negative); `buf` may be NULL (only the count is wanted).
extern "C" int cbo_schedule_report(cbo_ctx *c, char *buf, int64_t cap)
{
    if (!c) return fail(CBO_ERR_INVALID, "ctx is NULL");      // (CBO_ERR_* codes are negative as they are)
    static const char *names[] = {"cold", "sequence", "base", "neighbours", "climb", "grouping", "settled", "renewing the first split"};
    std::string out;
    int exploring = 0;
    char line[512];
    for (const auto &kv : c->schedule) {
        const ScheduleEntry &e = kv.second;
        if (e.state != ScheduleEntry::SETTLED) ++exploring;
        const int nb = (int)(kv.first.first / 128);
        const double rounds = std::ceil((double)e.strips / c->n_cu);
        std::snprintf(line, sizeof(line), "rows %lld candidates %lld: %s after %d calls; pairs %d of %d (%s), updates %s; "
                      "last call ran pairs %d group %d; "
                      "measured alone: factorisation %.0f us = %.1f us/panel, sweep %.0f us = %.2f us/stage and round;",
                      (long long)kv.first.first, (long long)kv.first.second, names[(int)e.state], e.calls, e.cur, e.all_pairs,
                      e.cur < 0 ? "the plain sequence" : e.cur == 0 ? "overlapped, nothing pipelined" :
                      e.cur == e.all_pairs ? "everything pipelined" : "then one left-looking launch",
                      e.group >= 2 ? "in groups of two pairs" : "pair by pair", e.ran_pairs, e.ran_group, e.fact_alone_us,
                      nb ? e.fact_alone_us / nb : 0.0,
                      e.sweep_alone_us, nb ? e.sweep_alone_us / (rounds * 2.0 * nb * (nb + 1)) : 0.0);
        out += line;
        for (const auto &sv : e.samples) {
            std::snprintf(line, sizeof(line), " g%d/p%d:%.3fms x%d", sv.first.first, sv.first.second, sv.second.ms(), sv.second.count);
            out += line;
        }
        out += "\n";
    }
    if (buf && cap > 0) {
        const size_t n = out.size() < (size_t)cap - 1 ? out.size() : (size_t)cap - 1;
        std::memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return exploring;
}

extern "C" int cbo_acq_sweep_host(cbo_gp *g, int64_t m, const double *Xs, const double *pm, const double *pv,
                                  double y_best, int task, double ei_jitter, double cost, double *acq_out,
                                  double *best_val, int64_t *best_idx)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    cbo_cands *k = nullptr;
    int rc = scratch_cands(g->ctx, m, g->d, Xs, pm, pv, &k);
    if (rc != CBO_OK) return rc;
    return cbo_acq_sweep(g, k, y_best, task, ei_jitter, cost, acq_out, nullptr, nullptr, best_val, best_idx);
}

// the posterior mean / variance of the first m points of k from q, mu into the context's mean / var vectors (device):
// acq_kernel without EI
static int enqueue_mean_var(cbo_gp *g, const cbo_cands *k, int64_t m, int include_noise)
{
    cbo_ctx *c = g->ctx;
    const bool causal = g->X.sv != nullptr;
    AcqParams p;
    p.variance = g->h.variance; p.noise_var = g->noise_var; p.y_best = 0.0; p.ei_jitter = 0.0; p.cost = 1.0;
    p.task = CBO_TASK_MIN; p.include_noise = include_noise ? 1 : 0; p.want_ei = 0;
    {
        PhaseScope ps(c, PH_ACQ);
        launch_acq(c->stream, c->q, c->mu, causal ? k->pm : nullptr, causal ? k->pv : nullptr, m, p, c->mean, c->var,
                   nullptr, c->part_val, c->part_idx, 0, acq_blocks_for(m));
    }
    HIP_TRY(hipGetLastError());
    return CBO_OK;
}

// posterior mean / variance of a prepared candidate set into the context's mean / var vectors
// (f64_solution: an fp32 model solves on its fp64 factor too, leaving V = L^-1 K* in the fp64 workspace)
static int posterior_of_set(cbo_gp *g, cbo_cands *k, int include_noise, bool f64_solution = false)
{
    const int rc = enqueue_posterior(g, k, f64_solution);
    if (rc != CBO_OK) return rc;
    return enqueue_mean_var(g, k, k->m, include_noise);
}

// the same for m host points, uploaded to the scratch set
static int posterior_of_host_points(cbo_gp *g, int64_t m, const double *Xs, const double *pm, const double *pv,
                                    int include_noise, cbo_cands **k_out, bool f64_solution = false)
{
    if (g->X.sv != nullptr && (!pm || !pv)) return fail(CBO_ERR_INVALID, "causal gp needs candidate prior mean/variance");
    int rc = scratch_points(g, m, Xs, pm, pv, k_out);
    if (rc != CBO_OK) return rc;
    return posterior_of_set(g, *k_out, include_noise, f64_solution);
}

// group means of the context's mean / var vectors (n_groups groups of `group` consecutive points) into the (now free)
// q / mu vectors, and to the caller
static int group_means_out(cbo_ctx *c, int64_t n_groups, int64_t group, double *mean_out, double *var_out)
{
    launch_group_mean(c->stream, c->mean, n_groups, group, c->q);
    launch_group_mean(c->stream, c->var, n_groups, group, c->mu);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mean_out, c->q, sizeof(double) * n_groups, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(var_out, c->mu, sizeof(double) * n_groups, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

extern "C" int cbo_gp_predict(cbo_gp *g, int64_t m, const double *Xs, const double *pm, const double *pv,
                              int include_noise, double *mean_out, double *var_out)
{
    if (!g || !mean_out || !var_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    cbo_cands *k = nullptr;
    int rc = posterior_of_host_points(g, m, Xs, pm, pv, include_noise, &k);
    if (rc != CBO_OK) return rc;
    rc = copy_posterior_out(c, k, nullptr, mean_out, var_out);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->profiling) c->timers.n_sweep += 1;
    return CBO_OK;
}

// ---- point-wise acquisitions (kernels_pointwise.hip) -------------------------------------------------------
// The plug-in incumbent of emukit's MeanPluginExpectedImprovement, min (max) over model.predict(model.X)[0], into the
// context's device double: the model's own points become the scratch set (device copies of what was uploaded: the raw
// coordinates and the prior closures) and are predicted as cbo_gp_predict predicts host points -- the same preparation,
// substitution and epilogue, so the same bits -- then one reduction.  Queued; the caller synchronises.
static int enqueue_plugin_incumbent(cbo_gp *g, int task)
{
    cbo_ctx *c = g->ctx;
    const bool causal = g->X.sv != nullptr;
    cbo_cands *k = scratch_set(c);
    int rc = cands_reserve(k, g->n, g->d, causal);
    if (rc != CBO_OK) return rc;
    cands_describe(k, g->n, g->d, causal, 0);
    HIP_TRY(hipMemcpyAsync(k->raw, g->raw, sizeof(double) * g->n * g->d, hipMemcpyDeviceToDevice, c->stream));
    if (causal) {
        HIP_TRY(hipMemcpyAsync(k->pm, g->X.pm, sizeof(double) * g->n, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(k->pv, g->X.pv, sizeof(double) * g->n, hipMemcpyDeviceToDevice, c->stream));
    }
    rc = posterior_of_set(g, k, 1);
    if (rc == CBO_OK) rc = grow(c, c->plugin_y, 1);
    if (rc != CBO_OK) return rc;
    launch_plugin_incumbent(c->stream, c->mean, g->n, task, c->plugin_y);
    HIP_TRY(hipGetLastError());
    return CBO_OK;
}

extern "C" int cbo_gp_plugin_incumbent(cbo_gp *g, int task, double *incumbent_out)
{
    if (!g || !incumbent_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (task != CBO_TASK_MIN && task != CBO_TASK_MAX) return fail(CBO_ERR_INVALID, "task must be 0 (min) or 1 (max)");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = enqueue_plugin_incumbent(g, task);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipMemcpyAsync(incumbent_out, c->plugin_y, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

// emukit NegativeLowerConfidenceBound, ProbabilityOfImprovement, ModelVariance and MeanPluginExpectedImprovement over a
// cost: the EI sweep's path up to q, mu (sweep_impl), then the kind's epilogue.  The plug-in EI's incumbent is formed first
// (its prediction uses the context's vectors, which the sweep's substitution then overwrites) and stays on the device.
extern "C" int cbo_acq_sweep_kind(cbo_gp *g, cbo_cands *k, int kind, double y_best, int task, double param, double cost,
                                  double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx)
{
    if (kind != CBO_ACQ_LCB && kind != CBO_ACQ_PI && kind != CBO_ACQ_VAR && kind != CBO_ACQ_MPEI)
        return fail(CBO_ERR_INVALID, "kind must be CBO_ACQ_LCB, CBO_ACQ_PI, CBO_ACQ_VAR or CBO_ACQ_MPEI");
    if (kind == CBO_ACQ_VAR) { y_best = 0.0; task = CBO_TASK_MIN; param = 0.0; }       // not read
    if (kind == CBO_ACQ_MPEI) y_best = 0.0;                                             // not read
    int rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    if (!std::isfinite(param)) return fail(CBO_ERR_INVALID, "param (beta / jitter) must be finite");
    if (kind == CBO_ACQ_LCB && param < 0.0) return fail(CBO_ERR_INVALID, "beta must not be negative");
    if (kind == CBO_ACQ_PI && !std::isfinite(y_best)) return fail(CBO_ERR_INVALID, "y_best must be finite");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    const double *y_best_dev = nullptr;
    if (kind == CBO_ACQ_MPEI) {
        HIP_TRY(hipSetDevice(g->ctx->device));
        rc = enqueue_plugin_incumbent(g, task);
        if (rc != CBO_OK) return rc;
        y_best_dev = g->ctx->plugin_y;
    }
    return sweep_impl(g, k, y_best, task, param, cost, acq_out, mean_out, var_out, best_val, best_idx, nullptr, kind,
                      y_best_dev);
}

// The log Expected Improvement over a cost: cbo_acq_sweep_kind's path with log_ei_of's epilogue --
// acq = log EI - log cost, finite and strictly ordered where the EI itself underflows to 0; mean and var are
// cbo_acq_sweep_kind's bits.  The scalars are checked first (check_kind_args, as the multi-set call checks them), then the handles.
extern "C" int cbo_acq_sweep_logei(cbo_gp *g, cbo_cands *k, double y_best, int task, double jitter, double cost,
                                   double *acq_out, double *mean_out, double *var_out, double *best_val, int64_t *best_idx)
{
    int rc = check_kind_args(1, kLogEiKind, &y_best, &task, &jitter, &cost, true);
    if (rc != CBO_OK) return rc;
    rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    return sweep_impl(g, k, y_best, task, jitter, cost, acq_out, mean_out, var_out, best_val, best_idx, nullptr, kLogEiKind);
}

// The Expected Improvement, or its logarithm, of every candidate over the candidate's OWN cost: cost[j] of
// cbo_cands_set_cost.  cbo_acq_sweep_logei's scalar checks first, then the handles, then the cost vector.
extern "C" int cbo_acq_sweep_pointcost(cbo_gp *g, cbo_cands *k, int log_form, double y_best, int task, double jitter,
                                       double *acq_out, double *mean_out, double *var_out, double *best_val,
                                       int64_t *best_idx)
{
    int rc = check_pointcost_args(1, log_form, &y_best, &task, &jitter);
    if (rc != CBO_OK) return rc;
    rc = check_sweep_args(g, k, task);
    if (rc != CBO_OK) return rc;
    rc = check_has_cost(k);
    if (rc != CBO_OK) return rc;
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    return sweep_impl(g, k, y_best, task, jitter, 1.0, acq_out, mean_out, var_out, best_val, best_idx, nullptr,
                      log_form ? kLogEiPointKind : kEiPointKind);
}

// What gumbel_quantiles_kernel left for one set: the single call's message for the first quantile that failed ("" = none),
// and _fit_gumbel's parameters from the three quantiles -- shared by cbo_gp_mes_gumbel and cbo_gp_mes_gumbel_sets.
static std::string gumbel_failure(const double *out5, const int64_t *status3)
{
    for (int j = 0; j < 3; ++j) {
        char msg[160];
        if (status3[j] == 1) {
            std::snprintf(msg, sizeof msg, "Gumbel fit: f(a) and f(b) must have different signs (quantile %.2f on "
                          "[%.17g, %.17g])", 0.25 * (j + 1), out5[3], out5[4]);
            return msg;
        }
        if (status3[j] != 0) {
            std::snprintf(msg, sizeof msg, "Gumbel fit: bisection of quantile %.2f failed to converge after 10000 "
                          "iterations", 0.25 * (j + 1));
            return msg;
        }
    }
    return std::string();
}
static void gumbel_parameters(const double *out5, double *quantiles3, double *a_out, double *b_out)
{
    for (int j = 0; j < 3; ++j) quantiles3[j] = out5[j];
    // _fit_gumbel: b = (q25 - q75) / (log(log(4/3)) - log(log(4))), a = q50 - b log(log(2))
    const double b = (out5[0] - out5[2]) / (std::log(std::log(4.0 / 3.0)) - std::log(std::log(4.0)));
    *b_out = b;
    *a_out = out5[1] - b * std::log(std::log(2.0));
}

// emukit MaxValueEntropySearch.update_parameters' model.predict(grid) and _fit_gumbel: the grid's predictive mean and
// variance (noise included) as cbo_gp_predict leaves them on the device, then the three bisections in one launch on them;
// only the quantiles (and, when asked, the mean and variance) come back
extern "C" int cbo_gp_mes_gumbel(cbo_gp *g, int64_t m, const double *Xg, const double *pm, const double *pv,
                                 double *quantiles3, double *a_out, double *b_out, double *mean_out, double *var_out)
{
    if (!g || !Xg || !quantiles3 || !a_out || !b_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0) return fail(CBO_ERR_INVALID, "m must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    cbo_cands *k = nullptr;
    int rc = posterior_of_host_points(g, m, Xg, pm, pv, 1, &k);
    if (rc != CBO_OK) return rc;
    // part_val / part_idx: free device scratch between sweeps (2048 entries each)
    launch_gumbel_quantiles(c->stream, GumbelSet{c->mean, c->var, m}, nullptr, 1, c->part_val, c->part_idx);
    HIP_TRY(hipGetLastError());
    double out[5];
    int64_t status[3];
    HIP_TRY(hipMemcpyAsync(out, c->part_val, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, c->part_idx, sizeof(status), hipMemcpyDeviceToHost, c->stream));
    rc = copy_posterior_out(c, k, nullptr, mean_out, var_out);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const std::string err = gumbel_failure(out, status);
    if (!err.empty()) return fail(CBO_ERR_INVALID, err);
    gumbel_parameters(out, quantiles3, a_out, b_out);
    if (c->profiling) c->timers.n_sweep += 1;
    return CBO_OK;
}

// cbo_gp_mes_gumbel for every set of a trial: the grids of the fp64 models of at most 128 observations are
// predicted by small_sets_kernel<kPredictKind> -- no fit; one launch, two from kSmallTwoPhaseFromBlocks blocks per set on --
// into one mean / var workspace, every set's points one after the other; every other model is fitted if need be and
// predicted by the general path into the same workspace; then ONE launch of the bisections for all sets and ONE
// synchronisation.  A small model whose record reports a non-positive pivot is fitted and fitted a Gumbel as the single
// call does it, afterwards.
extern "C" int cbo_gp_mes_gumbel_sets(int n_sets, cbo_gp *const *gps, cbo_cands *const *grids, double *quantiles, double *a,
                                      double *b)
{
    if (n_sets <= 0 || n_sets > 65535) return fail(CBO_ERR_INVALID, "n_sets must be in 1..65535");
    if (!gps || !grids || !quantiles || !a || !b) return fail(CBO_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n_sets; ++i) {
        const int rc = check_set_handle(gps[i], grids[i], CBO_TASK_MIN, gps[0]);
        if (rc != CBO_OK) return rc;
        if (grids[i]->m <= 0) return fail(CBO_ERR_INVALID, "the Gumbel grid of set " + std::to_string(i) + " is empty");
    }
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int64_t> off((size_t)n_sets);
    int64_t total = 0;
    for (int i = 0; i < n_sets; ++i) { off[(size_t)i] = total; total += grids[i]->m; }
    if (2 * sizeof(double) * (size_t)total > c->max_ws_bytes)
        return fail(CBO_ERR_UNSUPPORTED, "the Gumbel grids' mean / variance workspace (" + std::to_string(total) +
                                             " points) exceeds the workspace limit: raise CBO_HIP_WORKSPACE_MB");
    int rc = grow(c, c->gumbel_mean, (size_t)total);
    if (rc == CBO_OK) rc = grow(c, c->gumbel_var, (size_t)total);
    if (rc == CBO_OK) rc = grow(c, c->gumbel_out, 5 * (size_t)n_sets);
    if (rc == CBO_OK) rc = grow(c, c->gumbel_status, 3 * (size_t)n_sets);
    if (rc == CBO_OK) rc = grow(c, c->gumbel_sets_host, (size_t)n_sets);
    if (rc != CBO_OK) return rc;
    // Of the routing policy this call shares the partition, the descriptors and the launch buffers.  Its records are not
    // polled: they are read behind the synchronisation of stage (2), so the launch is no polled launch and only takes its
    // sequence number where those take theirs.  (A grid too wide for the launch sends that set alone to the general path.)
    std::vector<int> small;
    const int blocks = partition_small(
        n_sets, [&](int i) { return small_sweep_model(gps[i]) && cand_blocks(grids[i]) <= kMaxGridBlocks; },
        [&](int i) { return cand_blocks(grids[i]); }, small);
    // (1) the predict: the small models' grids in the one-workgroup launch ...
    const int ns = (int)small.size();
    int seq = 0;
    if (ns > 0) {
        rc = ensure_small_buffers(c, ns, blocks);
        if (rc == CBO_OK) rc = grow(c, c->aux_host, ns < 32 ? (size_t)32 : (size_t)ns);
        for (int j = 0; rc == CBO_OK && j < ns; ++j) {
            const int i = small[(size_t)j];
            rc = fill_small_set(c->sets_host[j], gps[i], grids[i], CBO_TASK_MIN, 0.0, 0.0, 1.0);
            c->aux_host[j] = cbo_small_aux{off[(size_t)i], 0};
        }
        if (rc != CBO_OK) return rc;
        SmallAux aux;
        aux.per_set = c->aux_host;
        aux.mean_out = c->gumbel_mean;
        aux.var_out = c->gumbel_var;
        seq = next_small_seq(c);
        launch_small_sets(c->stream, kPredictKind, c->sets_host, ns, blocks, small_launch(c, seq), aux);
        HIP_TRY(hipGetLastError());
    }
    // ... every other model's on the general path, into the same workspace
    std::vector<char> is_small((size_t)n_sets, 0);
    for (int j = 0; j < ns; ++j) is_small[(size_t)small[(size_t)j]] = 1;
    auto general_predict = [&](int i) -> int {
        int r = ensure_fitted(gps[i]);
        if (r == CBO_OK) r = posterior_of_set(gps[i], grids[i], 1);
        if (r != CBO_OK) return r;
        const size_t bytes = sizeof(double) * (size_t)grids[i]->m;
        HIP_TRY(hipMemcpyAsync(c->gumbel_mean + off[(size_t)i], c->mean, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->gumbel_var + off[(size_t)i], c->var, bytes, hipMemcpyDeviceToDevice, c->stream));
        return CBO_OK;
    };
    for (int i = 0; i < n_sets; ++i) {
        if (is_small[(size_t)i]) continue;
        rc = general_predict(i);
        if (rc != CBO_OK) return rc;
    }
    // (2) the bisections of every set, then the call's one synchronisation
    for (int i = 0; i < n_sets; ++i)
        c->gumbel_sets_host[i] = GumbelSet{c->gumbel_mean + off[(size_t)i], c->gumbel_var + off[(size_t)i], grids[i]->m};
    std::vector<double> out(5 * (size_t)n_sets);
    std::vector<int64_t> status(3 * (size_t)n_sets);
    auto bisect = [&](int first, int count) -> int {
        launch_gumbel_quantiles(c->stream, GumbelSet{}, c->gumbel_sets_host + first, count, c->gumbel_out + 5 * first,
                                c->gumbel_status + 3 * first);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out.data() + 5 * first, c->gumbel_out + 5 * first, sizeof(double) * 5 * (size_t)count,
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(status.data() + 3 * first, c->gumbel_status + 3 * first, sizeof(int64_t) * 3 * (size_t)count,
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return CBO_OK;
    };
    rc = bisect(0, n_sets);
    if (rc != CBO_OK) return rc;
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int j = 0; j < ns; ++j) {
        if (c->small_out[j].seq != seq) return fail(CBO_ERR_HIP, "multi-set Gumbel fit: no result record");
        if (c->small_out[j].info == 0) continue;
        // not positive definite as assembled: the general path's jitchol ladder, and this set's bisections again
        const int i = small[(size_t)j];
        rc = general_predict(i);
        if (rc == CBO_OK) rc = bisect(i, 1);
        if (rc != CBO_OK) return rc;
    }
    for (int i = 0; i < n_sets; ++i) {
        const std::string err = gumbel_failure(out.data() + 5 * i, status.data() + 3 * i);
        if (!err.empty()) return fail(CBO_ERR_INVALID, "set " + std::to_string(i) + ": " + err);
    }
    for (int i = 0; i < n_sets; ++i) gumbel_parameters(out.data() + 5 * i, quantiles + 3 * i, a + i, b + i);
    if (c->profiling) c->timers.n_sweep += 1;
    return CBO_OK;
}

// ---- joint posterior covariance (kernels_joint.hip) --------------------------------------------------------------
// Both entry points solve V = L^-1 K* afresh on every call (a model changed by cbo_gp_append, set_data, set_hyper or a
// refit can never meet an old solution) into the context's fp64 workspace, which must hold all m columns at once, then
// run cov_tile_kernel into the context's grow-only output buffer and copy it to the caller in one piece.

// the fp64 solution of a candidate set with m_pad columns stays resident in ONE workspace chunk: its leading dimension
static int resident_solution_ld(cbo_gp *g, int64_t m_pad, int64_t *ldv)
{
    int64_t chunk = 0;
    int rc = ensure_workspaces(g->ctx, g->n_pad, m_pad, &chunk, ldv);
    if (rc != CBO_OK) return rc;
    if (chunk < m_pad) return fail(CBO_ERR_INVALID, "too many points: their solution L^-1 K* does not fit the workspace");
    return CBO_OK;
}

// C = K(X1, X2) - V1^T V2 for the points of k at columns [a_off, a_off + m1) and [b_off, b_off + m2), into c->cov
// (or into C, row-major with leading dimension ldc)
static void enqueue_cov(cbo_gp *g, const cbo_cands *k, int64_t ldv, int64_t a_off, int64_t m1, int64_t b_off, int64_t m2,
                        bool sym, double noise, double *C = nullptr, int64_t ldc = 0)
{
    const bool causal = g->X.sv != nullptr;
    CovArgs a;
    a.V = g->ctx->V; a.ldv = ldv;
    a.a_off = a_off; a.b_off = b_off; a.v_cols = k->m_pad;
    a.n_k = (int)g->n;
    a.xs1 = k->P.xs + a_off; a.sq1 = k->P.sq + a_off; a.sv1 = causal ? k->P.sv + a_off : nullptr;
    a.xs2 = k->P.xs + b_off; a.sq2 = k->P.sq + b_off; a.sv2 = causal ? k->P.sv + b_off : nullptr;
    a.ldx = k->P.ld;
    a.m1 = m1; a.m2 = m2;
    a.C = C ? C : g->ctx->cov; a.ldc = C ? ldc : m2;
    a.variance = g->h.variance; a.inv_l2 = 1.0 / (g->h.lengthscale * g->h.lengthscale); a.noise = noise;
    a.zero_diag = g->h.zero_diag; a.tiles = 0;
    launch_cov_tiles(g->ctx->stream, g->d, sym, a);
}

extern "C" int cbo_gp_predict_cov(cbo_gp *g, int64_t m, const double *Xs, const double *pm, const double *pv,
                                  int include_noise, double *mean_out, double *cov_out)
{
    if (!g || !Xs || !cov_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0) return fail(CBO_ERR_INVALID, "m must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    const bool causal = g->X.sv != nullptr;
    if (causal && (!pv || (mean_out && !pm)))
        return fail(CBO_ERR_INVALID, "causal gp needs the prior variance at the points (and the prior mean for the mean)");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int64_t ldv = 0;
    int rc = resident_solution_ld(g, round_up(m, kStrip), &ldv);
    if (rc != CBO_OK) return rc;
    rc = grow(c, c->cov, (size_t)m * (size_t)m);
    cbo_cands *k = nullptr;
    if (rc == CBO_OK) rc = scratch_points(g, m, Xs, pm, pv, &k);
    if (rc == CBO_OK) rc = posterior_of_set(g, k, 0, true);
    if (rc != CBO_OK) return rc;
    enqueue_cov(g, k, ldv, 0, m, 0, m, true, include_noise ? g->noise_var : 0.0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cov_out, c->cov, sizeof(double) * (size_t)m * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (mean_out) HIP_TRY(hipMemcpyAsync(mean_out, c->mean, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

extern "C" int cbo_gp_cov_between(cbo_gp *g, int64_t m1, const double *X1, const double *pv1, int64_t m2,
                                  const double *X2, const double *pv2, double *cov_out)
{
    if (!g || !X1 || !X2 || !cov_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m1 <= 0 || m2 <= 0) return fail(CBO_ERR_INVALID, "m1 and m2 must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    const bool causal = g->X.sv != nullptr;
    if (causal && (!pv1 || !pv2)) return fail(CBO_ERR_INVALID, "causal gp needs the prior variance at both point sets");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    // one candidate set [X1 | filler | X2] with X2 starting on a strip boundary: one solve gives V1 and V2 side by side
    const int64_t off = round_up(m1, kStrip);
    int64_t ldv = 0;
    int rc = resident_solution_ld(g, round_up(off + m2, kStrip), &ldv);
    if (rc == CBO_OK) rc = grow(c, c->cov, (size_t)m1 * (size_t)m2);
    cbo_cands *k = nullptr;
    if (rc == CBO_OK) rc = scratch_pair(g, m1, X1, pv1, m2, X2, pv2, kStrip, &k);
    if (rc == CBO_OK) rc = enqueue_posterior(g, k, true);
    if (rc != CBO_OK) return rc;
    enqueue_cov(g, k, ldv, 0, m1, off, m2, false, 0.0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cov_out, c->cov, sizeof(double) * (size_t)m1 * (size_t)m2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

// ---- joint posterior samples (kernels_joint.hip) -----------------------------------------------------------------
// V = L^-1 K* is solved as for cbo_gp_predict_cov; cov_tile_kernel then writes Sigma + jitter I straight into a
// factorisation buffer in the model factor's own layout ([m_pad][m_pad + 80], identity padding, zero right-hand-side
// strip), launch_cholesky factors it and samples_tile_kernel forms mean + L Z^T.  A jitter retry re-runs only the cov
// launch from the resident V.  The model's factor, z, alpha and status word are never written.

extern "C" int cbo_gp_posterior_samples(cbo_gp *g, int64_t m, const double *Xs, const double *pm, const double *pv,
                                        int64_t n_samples, const double *normals, double *samples_out, int *tries_out,
                                        double *jitter_out)
{
    if (!g || !Xs || !normals || !samples_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0) return fail(CBO_ERR_INVALID, "m must be positive");
    if (n_samples <= 0) return fail(CBO_ERR_INVALID, "n_samples must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    const bool causal = g->X.sv != nullptr;
    if (causal && (!pv || !pm)) return fail(CBO_ERR_INVALID, "causal gp needs the prior mean and variance at the points");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t s = n_samples;
    const int64_t m_pad = round_up(m, kPadN), lda = m_pad + kRhsCols + kLdExtra;
    const int64_t ldz = round_up(s, kPadN) + kLdExtra;
    int64_t ldv = 0;
    int rc = resident_solution_ld(g, round_up(m, kStrip), &ldv);
    if (rc == CBO_OK) rc = grow(c, c->samp_A, (size_t)m_pad * (size_t)lda);
    if (rc == CBO_OK) rc = grow(c, c->samp_invDt, (size_t)(m_pad / 16) * 256);
    if (rc == CBO_OK) rc = grow(c, c->samp_Z, (size_t)m_pad * (size_t)ldz);
    if (rc == CBO_OK) rc = grow(c, c->samp_out, (size_t)m * (size_t)s);
    if (rc == CBO_OK) rc = grow(c, c->samp_info, 1 + kCholFlagSlots);
    if (rc != CBO_OK) return rc;
    // the ladder's base: 1e-6 mean(Kdiag(X*)), the prior diagonal variance + v(x) (summed in extended precision)
    long double kdiag = 0.0L;
    for (int64_t i = 0; i < m; ++i) kdiag += (long double)(g->h.variance + (causal ? pv[i] : 0.0));
    const double base = (double)(kdiag / (long double)m) * 1e-6;
    // the normals go through the output buffer (the product overwrites them) into Z = normals^T
    HIP_TRY(hipMemcpyAsync(c->samp_out, normals, sizeof(double) * (size_t)m * (size_t)s, hipMemcpyHostToDevice, c->stream));
    launch_normals_transpose(c->stream, c->samp_out, m, s, c->samp_Z, m_pad, ldz);
    cbo_cands *k = nullptr;
    rc = posterior_of_host_points(g, m, Xs, pm, pv, 0, &k, true);
    if (rc != CBO_OK) return rc;
    double jitter = 0.0;
    int tries = 0;
    // the factor of Sigma + jitter I in c->samp_A
    auto enqueue = [&](bool separate) {
        launch_factor_padding(c->stream, c->samp_A, lda, m, m_pad);
        enqueue_cov(g, k, ldv, 0, m, 0, m, true, jitter, c->samp_A, lda);
        launch_cholesky(c->stream, c->side_stream, c->chol_events, c->samp_A, lda, m_pad, c->samp_invDt, c->samp_info,
                        chol_options(c, separate));
    };
    for (;;) {
        bool pd = false;
        rc = attempt_factor(c, c->samp_info, enqueue, &pd);
        if (rc != CBO_OK) return rc;
        if (pd) break;
        if (!jitter_step(base, &tries, &jitter))
            return fail(CBO_ERR_NOT_PD, "posterior covariance not positive definite, even with jitter.");
    }
    SampArgs a;
    a.U = c->samp_A; a.ldu = lda;
    a.Z = c->samp_Z; a.ldz = ldz;
    a.mean = c->mean;
    a.m = m; a.s = s;
    a.F = c->samp_out; a.ldf = s;
    a.tiles_i = a.tiles_j = 0;
    launch_samples_tiles(c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(samples_out, c->samp_out, sizeof(double) * (size_t)m * (size_t)s, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (tries_out) *tries_out = tries;
    if (jitter_out) *jitter_out = jitter;
    return CBO_OK;
}

// ---- integrated variance reduction (kernels_joint.hip ivr_tile_kernel, kernels_acq.hip ivr_finish_kernel) -------------
// One scratch candidate set [Xs | filler | Xint], the integration points from column `off` (a tile boundary).  The
// candidates are solved once into workspace columns [0, round_up(m, kStrip)) and their predictive variance is taken from
// that solution (acq_kernel, include_noise = 1: cbo_gp_predict's bits).  The integration points follow in chunks of
// whole tiles solved into the columns that remain from `off` on; each chunk's tile pass leaves one partial per
// (candidate, global tile column), so the result does not depend on the chunking.  The model's factor, z, alpha and
// status word are only read.

extern "C" int cbo_gp_integrated_variance_reduction(cbo_gp *g, int64_t m, const double *Xs, const double *pv_s, int64_t p,
                                                    const double *Xint, const double *pv_int, double cost, double *ivr_out,
                                                    double *best_val, int64_t *best_idx)
{
    if (!g || !Xs || !Xint || (!ivr_out && !best_val && !best_idx)) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0 || p <= 0) return fail(CBO_ERR_INVALID, "m and p must be positive");
    if (!(cost > 0.0)) return fail(CBO_ERR_INVALID, "cost must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    const bool causal = g->X.sv != nullptr;
    if (causal && (!pv_s || !pv_int))
        return fail(CBO_ERR_INVALID, "causal gp needs the prior variance at the candidates and the integration points");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int d = g->d;
    const int64_t mc = round_up(m, kStrip), off = round_up(m, kJointTile);
    int64_t chunk = 0, ldv = 0;
    int rc = ensure_workspaces(c, g->n_pad, off + round_up(p, kJointTile), &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    if (chunk < off + kJointTile)
        return fail(CBO_ERR_INVALID, "too many candidates: their solution L^-1 K* and one tile of integration points do "
                                     "not fit the workspace");
    const int64_t pc = (chunk - off) / kJointTile * kJointTile;     // integration points per chunk
    const int64_t tiles = (p + kJointTile - 1) / kJointTile;
    rc = grow(c, c->ivr_part, (size_t)m * (size_t)tiles);
    cbo_cands *k = nullptr;
    if (rc == CBO_OK) rc = scratch_pair(g, m, Xs, pv_s, p, Xint, pv_int, kJointTile, &k);
    if (rc == CBO_OK) rc = prepare_cands(g, k);
    if (rc == CBO_OK) rc = solve_columns(g, k, 0, mc, c->V, ldv, c->q, c->mu);
    if (rc == CBO_OK) rc = enqueue_mean_var(g, k, m, 1);
    if (rc != CBO_OK) return rc;
    IvrArgs a;
    a.Vc = c->V; a.Vi = c->V + off; a.ldv = ldv;
    a.c_cols = mc;
    a.n_k = (int)g->n;
    a.xs1 = k->P.xs; a.sq1 = k->P.sq; a.sv1 = causal ? k->P.sv : nullptr;
    a.ldx = k->P.ld;
    a.m = m;
    a.part = c->ivr_part; a.ldp = tiles;
    a.variance = g->h.variance; a.inv_l2 = 1.0 / (g->h.lengthscale * g->h.lengthscale);
    for (int64_t p0 = 0; p0 < p; p0 += pc) {
        const int64_t pw = (p - p0 < pc) ? (p - p0) : pc;
        const int64_t w = round_up(pw, kStrip);                      // solved columns (<= pc: pc is a multiple of 128)
        // (q and mu of the integration points are not used: the candidates' part of both vectors is left alone)
        rc = solve_columns(g, k, off + p0, w, c->V + off, ldv, c->q + off, c->mu + off);
        if (rc != CBO_OK) return rc;
        a.i_cols = w;
        a.xs2 = k->P.xs + off + p0; a.sq2 = k->P.sq + off + p0; a.sv2 = causal ? k->P.sv + off + p0 : nullptr;
        a.p = pw;
        a.tile0 = p0 / kJointTile;
        launch_ivr_tiles(c->stream, d, a);
    }
    const int nb = ivr_finish_blocks_for(m);
    launch_ivr_finish(c->stream, c->ivr_part, tiles, (int)tiles, c->var, m, (double)p, cost, ivr_out ? c->acq : nullptr,
                      c->part_val, c->part_idx, nb);
    launch_argmax_final(c->stream, c->part_val, c->part_idx, nb, c->h_best_val, c->h_best_idx);
    HIP_TRY(hipGetLastError());
    if (ivr_out) HIP_TRY(hipMemcpyAsync(ivr_out, c->acq, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (best_val) *best_val = *c->h_best_val;
    if (best_idx) *best_idx = *c->h_best_idx;
    return CBO_OK;
}

extern "C" int cbo_gp_set_hyper(cbo_gp *g, double variance, const double *lengthscale, double noise_var)
{
    if (!g || !lengthscale) return fail(CBO_ERR_INVALID, "NULL argument");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    g->h.variance = variance;
    g->noise_var = noise_var;
    g->fitted = false;
    g->alpha_ready = false;
    if (g->h.ard) {
        g->ls.assign(lengthscale, lengthscale + g->d);
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(g->ls_dev, lengthscale, sizeof(double) * g->d, hipMemcpyHostToDevice));
        // GPy ARD scales the inputs: re-derive the scaled SoA coordinates and their squared norms
        launch_prep_points(c->stream, g->raw, g->n, g->d, g->ls_dev, g->X.sv ? g->X.pv : nullptr, g->X.xs, g->n_pad,
                           g->X.sq, g->X.sv);
        HIP_TRY(hipGetLastError());
    } else {
        g->ls.assign(lengthscale, lengthscale + 1);
        g->h.lengthscale = lengthscale[0];
    }
    return CBO_OK;
}

extern "C" int cbo_gp_log_marginal(cbo_gp *g, double *lml_out)
{
    if (!g || !lml_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    double h2[2];
    // part_val is a free 2048-double device scratch between sweeps
    launch_lml_terms(c->stream, g->A, g->lda, g->n_pad, g->z, c->part_val);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h2, c->part_val, sizeof(h2), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // GPy: 0.5 * (-n log(2 pi) - W_logdet - sum(alpha * (Y - m))),  W_logdet = 2 sum log L_ii
    *lml_out = 0.5 * (-(double)g->n * 1.8378770664093453 - 2.0 * h2[1] - h2[0]);
    return CBO_OK;
}

// Gradients of the log marginal likelihood with respect to the kernel variance, the lengthscale(s) and the noise
// variance: 1/2 sum_ij (alpha alpha^T - Ky^-1)_ij dKy_ij/dtheta (GPy ExactGaussianInference: dL_dK ->
// kern.update_gradients_full, dL_dthetaL).  Ky^-1 = L^-T L^-1 on the device: L^-1 by the sweep machinery on
// identity right-hand sides (its q output is diag(Ky^-1)), the product by the GEMM form of the update kernel over
// the non-zero lower-triangular part only, the contraction with dK/dtheta by one pass over the upper tiles.
// host arithmetic shared by both forms of the likelihood gradients: hs = variance sum, lengthscale sums per dimension
static void lml_outputs(const cbo_gp *g, const double *grad_sums, double zz, double logdet, double aa, double tr_w,
                        double *lml_out, double *dvariance_out, double *dlengthscale_out, double *dnoise_out)
{
    lml_outputs_of(g->h.variance, g->h.ard != 0, g->h.ard ? g->ls.data() : &g->h.lengthscale, g->d, (long long)g->n, grad_sums, zz,
                   logdet, aa, tr_w, lml_out, dvariance_out, dlengthscale_out, dnoise_out);
}

// the one-launch form of small_lml_gradients applies to this model
static bool small_lml_eligible(const cbo_gp *g)
{
    return g->dtype == CBO_DTYPE_F64 && g->n_pad == kPadN && g->ctx->small_sets && g->n > 0;
}

// the batched launch also takes the next band, 128 < n <= 256, in its two-block form
static bool mid_lml_eligible(const cbo_gp *g)
{
    return g->dtype == CBO_DTYPE_F64 && g->n_pad == 2 * kPadN && g->ctx->small_sets && g->n > kPadN;
}

// Models of at most 128 observations (every model the reference builds): likelihood and gradients in ONE launch, from
// the data and the current hyper-parameters -- no fit beforehand, none left behind.  Returns 1 when done, 0 when the
// general path has to take over (Ky not positive definite as assembled: the jitchol ladder lives there), < 0 on error.
static int small_lml_gradients(cbo_gp *g, double *lml_out, double *dvariance_out, double *dlengthscale_out,
                               double *dnoise_out)
{
    cbo_ctx *c = g->ctx;
    if (!small_lml_eligible(g)) return 0;
    int rc = ensure_small_buffers(c, 1, 2);            // scratch of two workgroup slots >= factor + L^-1
    if (rc != CBO_OK) return rc;
    rc = grow(c, c->lml_out, 1, true);
    if (rc != CBO_OK) return rc;
    cbo_small_set st{};
    fill_small_model(st, g);
    auto launch = [&](int seq) -> int {
        launch_small_lml(c->stream, st, c->small_scratch, c->small_info, c->lml_out, seq);
        return hipGetLastError() != hipSuccess ? fail(CBO_ERR_HIP, "small_lml_kernel launch") : CBO_OK;
    };
    rc = polled_launch(c, "cbo_gp_lml_gradients", c->lml_out.p, 1, "likelihood kernel: no result record", launch);
    if (rc != CBO_OK) return rc;
    if (c->lml_out.p->info != 0) return 0;
    const double *t = c->lml_out.p->terms;
    lml_outputs(g, t, t[1 + CBO_MAX_DIM], t[1 + CBO_MAX_DIM + 1], t[1 + CBO_MAX_DIM + 2], t[1 + CBO_MAX_DIM + 3], lml_out,
                dvariance_out, dlengthscale_out, dnoise_out);
    return 1;
}

static int general_lml_gradients(cbo_gp *g, double *lml_out, double *dvariance_out, double *dlengthscale_out,
                                 double *dnoise_out);

extern "C" int cbo_gp_lml_gradients(cbo_gp *g, double *lml_out, double *dvariance_out, double *dlengthscale_out,
                                    double *dnoise_out)
{
    if (!g || !dvariance_out || !dlengthscale_out || !dnoise_out) return fail(CBO_ERR_INVALID, "NULL argument");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    {
        const int done = small_lml_gradients(g, lml_out, dvariance_out, dlengthscale_out, dnoise_out);
        if (done < 0) return done;
        if (done == 1) return CBO_OK;
    }
    return general_lml_gradients(g, lml_out, dvariance_out, dlengthscale_out, dnoise_out);
}

// Many models, one launch: every model small_lml_gradients would take goes into ONE small_lml_batch_kernel launch (one
// workgroup each, the same device body, so the same bits), and so does every fp64 model of 128 < n <= 256 (the
// kernel's two-block form; no fit either).  The others -- larger models, and those whose Ky is not positive definite as
// assembled -- are answered one by one by general_lml_gradients, as cbo_gp_lml_gradients would.
extern "C" int cbo_gp_lml_gradients_batch(int n_models, cbo_gp *const *gps, double *lml, double *dvar, double *dls,
                                          double *dnoise, int *status)
{
    if (n_models <= 0 || !gps || !lml || !dvar || !dls || !dnoise || !status) return fail(CBO_ERR_INVALID, "bad argument");
    int rc = check_model_handles(n_models, gps);
    if (rc != CBO_OK) return rc;
    cbo_ctx *c = gps[0]->ctx;
    std::vector<int> small;
    bool any_mid = false;
    partition_small(n_models, [&](int i) {
        const bool mid = mid_lml_eligible(gps[i]);
        any_mid = any_mid || mid;
        return small_lml_eligible(gps[i]) || mid;
    }, [](int) { return (int64_t)1; }, small);
    const int ns = (int)small.size();
    // a scratch slot per model: factor + L^-1 (n <= 128), or the two-block slab
    const size_t stride = any_mid ? mid_lml_scratch_doubles() : small_lml_scratch_doubles();
    auto prepare = [&]() -> int {
        const size_t per_block = small_sets_scratch_doubles(1, 1);
        int rc = ensure_small_buffers(c, ns, (int)((stride + per_block - 1) / per_block));
        if (rc != CBO_OK) return rc;
        if ((size_t)ns * stride > c->small_scratch.cap)
            return fail(CBO_ERR_INVALID, "likelihood batch: scratch smaller than expected");
        rc = grow(c, c->lml_batch_out, ns < 32 ? 32 : (size_t)ns, true);
        for (int j = 0; rc == CBO_OK && j < ns; ++j) {
            c->sets_host[j] = cbo_small_set{};
            fill_small_model(c->sets_host[j], gps[small[(size_t)j]]);
        }
        return rc;
    };
    return run_small_or_general(
        c, "cbo_gp_lml_gradients_batch", "likelihood batch kernel: no result record", n_models, small, c->lml_batch_out, prepare,
        [&](const SmallLaunch &L) {
            launch_small_lml_batch(c->stream, c->sets_host, ns, L.scratch, (int64_t)stride, L.info, c->lml_batch_out, L.seq);
        },
        [&](int j, int i) {
            const double *t = c->lml_batch_out[j].terms;
            lml_outputs(gps[i], t, t[1 + CBO_MAX_DIM], t[1 + CBO_MAX_DIM + 1], t[1 + CBO_MAX_DIM + 2], t[1 + CBO_MAX_DIM + 3],
                        &lml[i], &dvar[i], &dls[(size_t)i * CBO_MAX_DIM], &dnoise[i]);
            status[i] = CBO_OK;
            return CBO_OK;
        },
        // an error is the model's status, not the call's -- unless the device is in trouble: no per-model answer means anything
        [&](int i) -> int {
            int rc = CBO_OK;
            if (mid_lml_eligible(gps[i]) && !gps[i]->fitted) rc = cbo_gp_fit(gps[i], nullptr, nullptr);   // (jitchol ladder)
            if (rc == CBO_OK)
                rc = general_lml_gradients(gps[i], &lml[i], &dvar[i], &dls[(size_t)i * CBO_MAX_DIM], &dnoise[i]);
            status[i] = rc;
            return rc == CBO_ERR_HIP ? rc : CBO_OK;
        });
}

// ---- priors on the hyper-parameters (hyper_prior.h, kernels_prior.hip) ---------------------------------------
static int prior_params(const cbo_gp *g) { return 2 + (g->h.ard ? g->d : 1); }

extern "C" int cbo_gp_set_priors(cbo_gp *g, int n_params, const cbo_hyper_prior *priors)
{
    if (!g) return fail(CBO_ERR_INVALID, "NULL argument");
    if (n_params != prior_params(g))
        return fail(CBO_ERR_INVALID, "n_params must be " + std::to_string(prior_params(g)) +
                                         " (variance, the lengthscale(s), the noise variance)");
    bool any = false;
    for (int k = 0; priors && k < n_params; ++k) {
        const cbo_hyper_prior &p = priors[k];
        const std::string where = " (parameter " + std::to_string(k) + ")";
        if (p.kind == CBO_PRIOR_NONE) continue;
        if (p.kind != CBO_PRIOR_GAUSSIAN && p.kind != CBO_PRIOR_LOGGAUSSIAN && p.kind != CBO_PRIOR_GAMMA &&
            p.kind != CBO_PRIOR_INVGAMMA)
            return fail(CBO_ERR_INVALID, "unknown prior kind " + std::to_string(p.kind) + where);
        if (!std::isfinite(p.p0) || !std::isfinite(p.p1)) return fail(CBO_ERR_INVALID, "a prior's parameters must be finite" + where);
        if (!std::isfinite(p.constant)) return fail(CBO_ERR_INVALID, "a prior's constant must be finite" + where);
        const bool normal = p.kind == CBO_PRIOR_GAUSSIAN || p.kind == CBO_PRIOR_LOGGAUSSIAN;
        if (normal && !(p.p1 > 0.0)) return fail(CBO_ERR_INVALID, "sigma must be positive" + where);
        if (!normal && !(p.p0 > 0.0)) return fail(CBO_ERR_INVALID, "a must be positive" + where);
        if (!normal && !(p.p1 > 0.0)) return fail(CBO_ERR_INVALID, "b must be positive" + where);
        any = true;
    }
    g->priors.clear();
    if (any) {
        g->priors.assign(priors, priors + n_params);
        for (cbo_hyper_prior &p : g->priors) {
            p.pad_ = 0;
            if (p.kind == CBO_PRIOR_NONE) p.p0 = p.p1 = p.constant = 0.0;
        }
    }
    return CBO_OK;
}

extern "C" int cbo_gp_get_priors(const cbo_gp *g, int n_params, cbo_hyper_prior *priors_out)
{
    if (!g || !priors_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (n_params != prior_params(g))
        return fail(CBO_ERR_INVALID, "n_params must be " + std::to_string(prior_params(g)) +
                                         " (variance, the lengthscale(s), the noise variance)");
    for (int k = 0; k < n_params; ++k) priors_out[k] = g->priors.empty() ? cbo_hyper_prior{} : g->priors[(size_t)k];
    return CBO_OK;
}

// The first n_params descriptors of a model's priors into a run's descriptor (the rest stay NONE); how many are priors.
static int copy_run_priors(const cbo_gp *g, int n_params, cbo_hyper_prior *out)
{
    if (g->priors.empty()) return 0;
    for (int k = 0; k < n_params; ++k) out[k] = g->priors[(size_t)k];
    return hyper_prior_count(out, n_params);
}

extern "C" int cbo_gp_log_prior_batch(int n_models, cbo_gp *const *gps, const double *const *thetas, double *lp_out,
                                      double *grad_out, int *status)
{
    if (n_models <= 0 || !gps || !lp_out || !grad_out || !status) return fail(CBO_ERR_INVALID, "bad argument");
    int rc = check_model_handles(n_models, gps);
    if (rc != CBO_OK) return rc;
    for (int i = 0; i < n_models; ++i) {
        const double *t = thetas ? thetas[i] : nullptr;
        for (int k = 0; t && k < prior_params(gps[i]); ++k)
            if (!std::isfinite(t[k])) return fail(CBO_ERR_INVALID, "theta must be finite (model " + std::to_string(i) + ")");
    }
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    bool any = false;
    for (int i = 0; i < n_models; ++i) any = any || !gps[i]->priors.empty();
    for (int i = 0; i < n_models; ++i) {
        lp_out[i] = 0.0;
        status[i] = CBO_OK;
        for (int k = 0; k < CBO_HMC_MAX_PARAMS; ++k) grad_out[(size_t)i * CBO_HMC_MAX_PARAMS + (size_t)k] = 0.0;
    }
    if (!any) return CBO_OK;                                    // (nothing to evaluate: 0 and zeros)
    rc = grow(c, c->prior_host, n_models < 32 ? (size_t)32 : (size_t)n_models);
    if (rc != CBO_OK) return rc;
    for (int i = 0; i < n_models; ++i) {
        const cbo_gp *g = gps[i];
        cbo_prior_item &it = c->prior_host[i];
        std::memset(&it, 0, sizeof(it));
        const int P = prior_params(g), n_ls = P - 2;
        it.n_params = g->priors.empty() ? 0 : P;
        copy_run_priors(g, P, it.priors);
        const double *t = thetas ? thetas[i] : nullptr;
        if (t) {
            std::memcpy(it.theta, t, sizeof(double) * (size_t)P);
        } else {
            it.theta[0] = g->h.variance;
            for (int k = 0; k < n_ls; ++k) it.theta[1 + k] = g->ls[(size_t)k];
            it.theta[1 + n_ls] = g->noise_var;
        }
    }
    launch_log_prior(c->stream, c->prior_host, n_models);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < n_models; ++i) {
        const cbo_prior_item &it = c->prior_host[i];
        if (!it.done) return fail(CBO_ERR_HIP, "log prior kernel: no answer for a model it was given");
        lp_out[i] = it.lp;
        std::memcpy(grad_out + (size_t)i * CBO_HMC_MAX_PARAMS, it.dlp, sizeof(double) * CBO_HMC_MAX_PARAMS);
    }
    return CBO_OK;
}

// ---- every model's HMC chain over its hyper-parameters (kernels_hmc.hip) ------------------------------------
// One launch for every model small_lml_gradients would take; the others are declined here, their status alone written.  The
// models are only read.  Of the routing policy (§4r) this call uses partition_small, ensure_small_buffers and
// fill_small_model: like cbo_acq_refine_sets it has no general path inside the call (a chain the launch cannot finish is
// the caller's to repeat), and its outputs come back behind one stream synchronisation, not through polled records.
extern "C" int cbo_gp_hmc_sets(int n_models, cbo_gp *const *gps, const cbo_hmc_chain *chains, int *status_out)
{
    if (n_models <= 0) return fail(CBO_ERR_INVALID, "n_models must be positive");
    if (!gps || !chains || !status_out) return fail(CBO_ERR_INVALID, "NULL argument");
    int rc = check_model_handles(n_models, gps);
    if (rc != CBO_OK) return rc;
    for (int i = 0; i < n_models; ++i) {
        const std::string where = " (model " + std::to_string(i) + ")";
        const cbo_hmc_chain &ch = chains[i];
        const cbo_gp *g = gps[i];
        if (!ch.theta0 || !ch.momenta || !ch.uniforms || !ch.rows_out || !ch.accept_out || !ch.final_theta || !ch.final_lml ||
            !ch.final_grad)
            return fail(CBO_ERR_INVALID, "NULL argument: theta0, the draws and the outputs must be given" + where);
        if (ch.num_samples < 1 || ch.num_samples > CBO_HMC_MAX_SAMPLES)
            return fail(CBO_ERR_INVALID, "num_samples must be in 1.." + std::to_string(CBO_HMC_MAX_SAMPLES) + where);
        if (ch.hmc_iters < 0) return fail(CBO_ERR_INVALID, "hmc_iters must not be negative" + where);
        if ((int64_t)ch.num_samples * ch.hmc_iters > CBO_HMC_MAX_EVALS)
            return fail(CBO_ERR_INVALID, "num_samples * hmc_iters must not exceed " + std::to_string(CBO_HMC_MAX_EVALS) + where);
        if (!std::isfinite(ch.stepsize) || !(ch.stepsize > 0.0))
            return fail(CBO_ERR_INVALID, "the stepsize must be finite and positive" + where);
        if (ch.sample_noise != 0 && ch.sample_noise != 1) return fail(CBO_ERR_INVALID, "sample_noise must be 0 or 1" + where);
        const int n_ls = g->h.ard ? g->d : 1;
        if (ch.n_params != 1 + n_ls + ch.sample_noise)
            return fail(CBO_ERR_INVALID, "n_params must be " + std::to_string(1 + n_ls + ch.sample_noise) +
                                             " (variance, the lengthscale(s), the noise variance when it is sampled)" + where);
        for (int k = 0; k < ch.n_params; ++k)
            if (!std::isfinite(ch.theta0[k]) || !(ch.theta0[k] > 0.0))
                return fail(CBO_ERR_INVALID, "theta0 must be finite and positive" + where);
        for (int64_t e = 0; e < (int64_t)ch.num_samples * ch.n_params; ++e)
            if (!std::isfinite(ch.momenta[e])) return fail(CBO_ERR_INVALID, "the momenta must be finite" + where);
        for (int e = 0; e < ch.num_samples; ++e)
            if (!std::isfinite(ch.uniforms[e])) return fail(CBO_ERR_INVALID, "the uniforms must be finite" + where);
    }
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int> small;
    partition_small(n_models, [&](int i) { return small_lml_eligible(gps[i]); }, [](int) { return (int64_t)1; }, small);
    const int ns = (int)small.size();
    for (int i = 0, j = 0; i < n_models; ++i) {
        if (j < ns && small[(size_t)j] == i) ++j;
        else status_out[i] = CBO_HMC_DECLINED;
    }
    if (small.empty()) return CBO_OK;
    // where each chain's draws, rows and flags begin in the call's arrays
    int64_t draws = 0, rows = 0, flags = 0;
    for (int j = 0; j < ns; ++j) {
        const cbo_hmc_chain &ch = chains[small[(size_t)j]];
        draws += (int64_t)ch.num_samples * (ch.n_params + 1);
        rows += (int64_t)ch.num_samples * ch.n_params;
        flags += ch.num_samples;
    }
    // a scratch slot per model: factor + L^-1
    const size_t stride = small_lml_scratch_doubles(), per_block = small_sets_scratch_doubles(1, 1);
    const size_t cap = ns < 32 ? (size_t)32 : (size_t)ns;
    constexpr int kFinal = 2 * CBO_HMC_MAX_PARAMS + 1;
    rc = ensure_small_buffers(c, ns, (int)((stride + per_block - 1) / per_block));
    if (rc == CBO_OK && (size_t)ns * stride > c->small_scratch.cap)
        rc = fail(CBO_ERR_INVALID, "HMC chains: scratch smaller than expected");
    if (rc == CBO_OK) rc = grow(c, c->hmc_host, cap);
    if (rc == CBO_OK) rc = grow(c, c->hmc_draws, (size_t)draws);
    if (rc == CBO_OK) rc = grow(c, c->hmc_rows, (size_t)rows);
    if (rc == CBO_OK) rc = grow(c, c->hmc_accept, (size_t)flags);
    if (rc == CBO_OK) rc = grow(c, c->hmc_final, cap * (size_t)kFinal);
    if (rc == CBO_OK) rc = grow(c, c->hmc_status, cap);
    if (rc != CBO_OK) return rc;
    draws = rows = flags = 0;
    for (int j = 0; j < ns; ++j) {
        const int i = small[(size_t)j];
        const cbo_hmc_chain &ch = chains[i];
        c->sets_host[j] = cbo_small_set{};
        fill_small_model(c->sets_host[j], gps[i]);
        cbo_small_hmc &hm = c->hmc_host[j];
        std::memset(&hm, 0, sizeof(hm));
        std::memcpy(hm.theta0, ch.theta0, sizeof(double) * (size_t)ch.n_params);
        hm.stepsize = ch.stepsize;
        hm.draw_off = draws; hm.row_off = rows; hm.acc_off = flags;
        hm.n_params = ch.n_params; hm.n_ls = gps[i]->h.ard ? gps[i]->d : 1; hm.sample_noise = ch.sample_noise;
        hm.num_samples = ch.num_samples; hm.hmc_iters = ch.hmc_iters;
        hm.n_prior = copy_run_priors(gps[i], ch.n_params, hm.priors);
        const size_t np = (size_t)ch.num_samples * (size_t)ch.n_params;
        std::memcpy(c->hmc_draws.p + draws, ch.momenta, sizeof(double) * np);
        std::memcpy(c->hmc_draws.p + draws + np, ch.uniforms, sizeof(double) * (size_t)ch.num_samples);
        c->hmc_status[j] = CBO_HMC_DECLINED;                   // (a launch that never ran answers nothing)
        draws += (int64_t)np + ch.num_samples; rows += (int64_t)np; flags += ch.num_samples;
    }
    launch_hmc_sets(c->stream, c->sets_host, c->hmc_host, c->hmc_draws, ns, c->small_scratch, (int64_t)stride, c->small_info,
                    c->hmc_rows, c->hmc_accept, c->hmc_final, c->hmc_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int j = 0; j < ns; ++j) {
        const int i = small[(size_t)j];
        const cbo_hmc_chain &ch = chains[i];
        const cbo_small_hmc &hm = c->hmc_host[j];
        if (c->hmc_status[j] == CBO_HMC_DECLINED) return fail(CBO_ERR_HIP, "HMC kernel: no status for a model it was given");
        status_out[i] = c->hmc_status[j];
        if (status_out[i] != CBO_HMC_OK) continue;
        const size_t np = (size_t)ch.num_samples * (size_t)ch.n_params;
        std::memcpy(ch.rows_out, c->hmc_rows.p + hm.row_off, sizeof(double) * np);
        std::memcpy(ch.accept_out, c->hmc_accept.p + hm.acc_off, sizeof(int) * (size_t)ch.num_samples);
        const double *fin = c->hmc_final.p + (size_t)j * kFinal;
        std::memcpy(ch.final_theta, fin, sizeof(double) * (size_t)ch.n_params);
        *ch.final_lml = fin[CBO_HMC_MAX_PARAMS];
        std::memcpy(ch.final_grad, fin + CBO_HMC_MAX_PARAMS + 1, sizeof(double) * (size_t)ch.n_params);
    }
    return CBO_OK;
}

// ---- every model's hyper-parameter MLE (kernels_mle.hip; kernels_mle_mid.hip, §4z) ---------------------------
// cbo_gp_hmc_sets' skeleton with one workgroup, scratch slot and info word per RUN (a (model, start) pair) instead of per
// model: the models small_lml_gradients would take go into one mle_sets_kernel launch; with max_rows = 256 those the batched
// likelihood takes in its two-block form go into one mle_mid_kernel launch on the same stream, behind one synchronisation for
// both; the others are declined here, their status alone written.  The small runs come first in every per-run buffer, the
// mid runs behind them.  The models are only read; the call returns every run and chooses none.
constexpr int kMaxMidRuns = 256;       // one workgroup per CU and about 256 MB of slabs
extern "C" int cbo_gp_mle_sets_rows(int n_models, cbo_gp *const *gps, const cbo_mle_run *runs, int max_rows,
                                    int *model_status_out)
{
    if (n_models <= 0) return fail(CBO_ERR_INVALID, "n_models must be positive");
    if (!gps || !runs || !model_status_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (max_rows != kPadN && max_rows != 2 * kPadN) return fail(CBO_ERR_INVALID, "max_rows must be 128 or 256");
    int rc = check_model_handles(n_models, gps);
    if (rc != CBO_OK) return rc;
    for (int i = 0; i < n_models; ++i) {
        const std::string where = " (model " + std::to_string(i) + ")";
        const cbo_mle_run &r = runs[i];
        const cbo_gp *g = gps[i];
        if (!r.theta0 || !r.theta_out || !r.lml_out || !r.grad_out || !r.status_out || !r.rounds_out)
            return fail(CBO_ERR_INVALID, "NULL argument: theta0 and the outputs must be given" + where);
        if (r.n_starts < 1 || r.n_starts > CBO_MLE_MAX_STARTS)
            return fail(CBO_ERR_INVALID, "n_starts must be in 1.." + std::to_string(CBO_MLE_MAX_STARTS) + where);
        if (r.max_rounds < 0 || r.max_rounds > CBO_MLE_MAX_ROUNDS)
            return fail(CBO_ERR_INVALID, "max_rounds must be in 0.." + std::to_string(CBO_MLE_MAX_ROUNDS) + where);
        if (r.fit_noise != 0 && r.fit_noise != 1) return fail(CBO_ERR_INVALID, "fit_noise must be 0 or 1" + where);
        const int n_ls = g->h.ard ? g->d : 1;
        if (r.n_params != 1 + n_ls + r.fit_noise)
            return fail(CBO_ERR_INVALID, "n_params must be " + std::to_string(1 + n_ls + r.fit_noise) +
                                             " (variance, the lengthscale(s), the noise variance when it is fitted)" + where);
        for (int k = 0; k < r.n_starts * r.n_params; ++k)
            if (!std::isfinite(r.theta0[k]) || !(r.theta0[k] > 0.0))
                return fail(CBO_ERR_INVALID, "theta0 must be finite and positive" + where);
    }
    cbo_ctx *c = gps[0]->ctx;
    HIP_TRY(hipSetDevice(c->device));
    // the launch's models in launch order: the small ones, then the mid ones
    std::vector<int> taken, mid;
    partition_small(n_models, [&](int i) { return small_lml_eligible(gps[i]); }, [](int) { return (int64_t)1; }, taken);
    const int ns = (int)taken.size();
    if (max_rows == 2 * kPadN)
        partition_small(n_models, [&](int i) { return mid_lml_eligible(gps[i]); }, [](int) { return (int64_t)1; }, mid);
    const int nm = (int)mid.size();
    int64_t total_small = 0, total_mid = 0;
    for (int j = 0; j < ns; ++j) total_small += runs[taken[(size_t)j]].n_starts;
    for (int j = 0; j < nm; ++j) total_mid += runs[mid[(size_t)j]].n_starts;
    if (total_small > kMaxGridBlocks) return fail(CBO_ERR_INVALID, "more than 65535 runs in one call");
    if (total_mid > kMaxMidRuns)
        return fail(CBO_ERR_INVALID, "more than 256 runs of models of 129..256 observations in one call (one workgroup per "
                                     "compute unit, about 1 MB of scratch each): split the call");
    for (int i = 0; i < n_models; ++i) model_status_out[i] = CBO_MLE_DECLINED;
    taken.insert(taken.end(), mid.begin(), mid.end());
    for (int i : taken) model_status_out[i] = CBO_OK;
    if (taken.empty()) return CBO_OK;
    const int nr_small = (int)total_small, nr_mid = (int)total_mid, nr = nr_small + nr_mid;
    // per run: a scratch slot (factor + L^-1; a mid run's two-block slab with its point region), an info word, a ring slot
    const size_t stride = small_lml_scratch_doubles(), mid_stride = mid_mle_scratch_doubles();
    const size_t per_block = small_sets_scratch_doubles(1, 1);
    const size_t need = (size_t)nr_small * stride + (size_t)nr_mid * mid_stride;
    const size_t cap = nr < 32 ? (size_t)32 : (size_t)nr;
    constexpr int kFinal = 2 * CBO_HMC_MAX_PARAMS + 1;
    rc = ensure_small_buffers(c, nr, (int)((stride + per_block - 1) / per_block));
    if (rc == CBO_OK && nr_mid > 0) rc = grow(c, c->small_scratch, need);
    if (rc == CBO_OK && need > c->small_scratch.cap) rc = fail(CBO_ERR_INVALID, "MLE runs: scratch smaller than expected");
    if (rc == CBO_OK) rc = grow(c, c->mle_host, cap);
    if (rc == CBO_OK) rc = grow(c, c->mle_final, cap * (size_t)kFinal);
    if (rc == CBO_OK) rc = grow(c, c->mle_status, cap);
    if (rc == CBO_OK) rc = grow(c, c->mle_rounds, cap);
    if (rc == CBO_OK) rc = grow(c, c->mle_rings, cap * (size_t)kMleRingDoubles);
    if (rc != CBO_OK) return rc;
    constexpr int kNoStatus = -2;                               // (a launch that never ran answers nothing)
    for (int j = 0, q = 0; j < ns + nm; ++j) {
        const int i = taken[(size_t)j];
        const cbo_mle_run &r = runs[i];
        c->sets_host[j] = cbo_small_set{};
        fill_small_model(c->sets_host[j], gps[i]);
        for (int s = 0; s < r.n_starts; ++s, ++q) {
            cbo_small_mle &rn = c->mle_host[q];
            std::memset(&rn, 0, sizeof(rn));
            std::memcpy(rn.theta0, r.theta0 + (size_t)s * (size_t)r.n_params, sizeof(double) * (size_t)r.n_params);
            rn.model = j < ns ? j : j - ns;                     // (its descriptor's index within its own launch)
            rn.n_params = r.n_params; rn.n_ls = gps[i]->h.ard ? gps[i]->d : 1; rn.fit_noise = r.fit_noise;
            rn.max_rounds = r.max_rounds;
            rn.n_prior = copy_run_priors(gps[i], r.n_params, rn.priors);
            c->mle_status[q] = kNoStatus;
        }
    }
    if (nr_small > 0)
        launch_mle_sets(c->stream, c->sets_host, ns, c->mle_host, nr_small, c->small_scratch, (int64_t)stride, c->small_info,
                        c->mle_rings, c->mle_final, c->mle_status, c->mle_rounds);
    if (nr_mid > 0)
        launch_mle_mid(c->stream, c->sets_host.p + ns, nm, c->mle_host.p + nr_small, nr_mid,
                       c->small_scratch.p + (size_t)nr_small * stride, (int64_t)mid_stride, c->small_info.p + nr_small,
                       c->mle_rings.p + (size_t)nr_small * kMleRingDoubles, c->mle_final.p + (size_t)nr_small * kFinal,
                       c->mle_status.p + nr_small, c->mle_rounds.p + nr_small);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int j = 0, q = 0; j < ns + nm; ++j) {
        const cbo_mle_run &r = runs[taken[(size_t)j]];
        const size_t P = (size_t)r.n_params;
        for (int s = 0; s < r.n_starts; ++s, ++q) {
            if (c->mle_status[q] == kNoStatus) return fail(CBO_ERR_HIP, "MLE kernel: no status for a run it was given");
            r.status_out[s] = c->mle_status[q];
            r.rounds_out[s] = c->mle_rounds[q];
            if (r.status_out[s] == CBO_MLE_NOT_PD) continue;
            const double *fin = c->mle_final.p + (size_t)q * kFinal;
            std::memcpy(r.theta_out + (size_t)s * P, fin, sizeof(double) * P);
            r.lml_out[s] = fin[CBO_HMC_MAX_PARAMS];
            std::memcpy(r.grad_out + (size_t)s * P, fin + CBO_HMC_MAX_PARAMS + 1, sizeof(double) * P);
        }
    }
    return CBO_OK;
}

extern "C" int cbo_gp_mle_sets(int n_models, cbo_gp *const *gps, const cbo_mle_run *runs, int *model_status_out)
{
    return cbo_gp_mle_sets_rows(n_models, gps, runs, kPadN, model_status_out);
}

static int general_lml_gradients(cbo_gp *g, double *lml_out, double *dvariance_out, double *dlengthscale_out,
                                 double *dnoise_out)
{
    cbo_ctx *c = g->ctx;
    if (!g->fitted) {                      // (a small model that was not positive definite as assembled lands here)
        if (g->n_pad != kPadN) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
        const int frc = cbo_gp_fit(g, nullptr, nullptr);
        if (frc != CBO_OK) return frc;
    }
    int rc = ensure_alpha(g);
    if (rc != CBO_OK) return rc;
    const int64_t n_pad = g->n_pad;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, n_pad, n_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    if (chunk < n_pad) return fail(CBO_ERR_UNSUPPORTED, "likelihood gradients need an n_pad x n_pad workspace (raise CBO_HIP_WORKSPACE_MB)");
    const int64_t ldw = n_pad + kLdExtra;
    const size_t w_bytes = sizeof(double) * (size_t)n_pad * (size_t)ldw;
    rc = grow(c, c->W, (size_t)n_pad * (size_t)ldw);
    if (rc == CBO_OK) rc = grow(c, c->gpart, (size_t)lml_grad_tiles(n_pad) * (size_t)(1 + g->d));
    if (rc != CBO_OK) return rc;
    // V = L^-1 (identity right-hand sides), q_j = (Ky^-1)_jj
    launch_set_identity(c->stream, c->V, ldv, n_pad);
    if (prefer_right_looking(c, n_pad, n_pad)) {
        rc = enqueue_right_looking(g, c->V, ldv, n_pad, c->q, c->mu, true);
        if (rc != CBO_OK) return rc;
    } else {
        launch_trsm_strips(c->stream, g->A, g->lda, g->invDt, c->V, ldv, n_pad, n_pad, g->z, c->q, c->mu);
    }
    // -Ky^-1 = -(L^-1)^T L^-1: rows [k0, k0+256) of L^-1 only reach columns < k0+256, so pair p touches the
    // leading (k0+256)^2 block; upper part only
    HIP_TRY(hipMemsetAsync(c->W, 0, w_bytes, c->stream));
    for (int k0 = 0; k0 < (int)n_pad; k0 += 256) {
        const int klen = (k0 + 256 <= (int)n_pad) ? 256 : 128;
        launch_gemm_update(c->stream, c->V, ldv, c->V, ldv, c->W, ldw, k0, klen, 0, k0 + klen, k0 + klen, true);
    }
    launch_lml_grad(c->stream, g->X, g->h, g->alpha, c->W, ldw, n_pad, c->gpart, c->part_val);
    launch_lml_terms(c->stream, g->A, g->lda, n_pad, g->z, c->part_val + 16);
    HIP_TRY(hipGetLastError());
    // tr(Ky^-1) = sum q and alpha^T alpha by device reductions: part_val[20..23]
    launch_dot2(c->stream, g->alpha, g->alpha, g->n, c->part_val + 20);
    launch_sum(c->stream, c->q, g->n, c->part_val + 22);
    HIP_TRY(hipGetLastError());
    double hs[24];
    HIP_TRY(hipMemcpyAsync(hs, c->part_val, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    lml_outputs(g, hs, hs[16], hs[17], hs[20], hs[22], lml_out, dvariance_out, dlengthscale_out, dnoise_out);
    return CBO_OK;
}

// ---- leave-one-out cross-validation (kernels_loo.hip) ---------------------------------------------------
// The general path: c = diag(Ky^-1) is the vector of squared column norms of L^-1, which the substitution kernels return
// as q when their right-hand sides are the identity.  The identity goes through in column chunks that fit the workspace.
// Chunk [c0, c0 + w) is zero above row c0, and so is its solution: the kernels get the trailing system only -- factor,
// diagonal inverses, z and V offset to (r0, r0), r0 = c0 rounded down to the pair kernel's 256-row block, height n_pad -
// r0.  Every kernel address is "base + offset" with offsets that are multiples of 128 doubles, so the offset bases keep
// the 16-byte alignment the LDS-DMA loads need.  A model whose whole identity fits the workspace and
// that prefer_right_looking would sweep right-looking takes the schedule of the likelihood gradients instead (lower-
// triangular right-hand sides: the zero part is skipped there too, and the device is filled whatever the column count).
// Outputs are host pointers; each may be null.
static int general_loo(cbo_gp *g, double *mean_out, double *var_out, double *lpd_out, double *sum_out)
{
    cbo_ctx *c = g->ctx;
    int rc = ensure_alpha(g);
    if (rc != CBO_OK) return rc;
    const int64_t n_pad = g->n_pad;
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, n_pad, n_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    const int nb = loo_finish_blocks(g->n);
    rc = grow(c, c->gpart, (size_t)nb + 1);
    if (rc != CBO_OK) return rc;
    if (c->loo_route != 1 && c->loo_route != 2 && chunk >= n_pad && prefer_right_looking(c, n_pad, n_pad)) {
        launch_set_identity(c->stream, c->V, ldv, n_pad);
        rc = enqueue_right_looking(g, c->V, ldv, n_pad, c->q, c->mu, true);
        if (rc != CBO_OK) return rc;
    } else {
        for (int64_t c0 = 0; c0 < n_pad; c0 += chunk) {
            const int64_t cols = (n_pad - c0 < chunk) ? (n_pad - c0) : chunk;
            const int64_t r0 = c->loo_route == 2 ? 0 : c0 / 256 * 256;
            const int64_t rows = n_pad - r0;
            PhaseScope ps(c, PH_TRSM);
            launch_loo_identity_chunk(c->stream, c->V, ldv, rows, cols, c0 - r0);
            launch_trsm_strips(c->stream, g->A + r0 * g->lda + r0, g->lda, g->invDt + (r0 / 16) * 256, c->V, ldv, rows,
                               cols, g->z + r0, c->q + c0, c->mu + c0);
            if (c->profiling) {
                c->timers.n_trsm_launches += 1;
                c->timers.trsm_flops += (double)rows * (double)rows * (double)cols;
            }
        }
    }
    double *partial = c->gpart, *sum_dev = c->gpart + nb;
    launch_loo_finish(c->stream, c->q, g->alpha, g->y, g->n, mean_out ? c->mean.p : nullptr, var_out ? c->var.p : nullptr,
                      lpd_out ? c->acq.p : nullptr, partial, sum_dev);
    HIP_TRY(hipGetLastError());
    const size_t bytes = sizeof(double) * (size_t)g->n;
    if (mean_out) HIP_TRY(hipMemcpyAsync(mean_out, c->mean, bytes, hipMemcpyDeviceToHost, c->stream));
    if (var_out) HIP_TRY(hipMemcpyAsync(var_out, c->var, bytes, hipMemcpyDeviceToHost, c->stream));
    if (lpd_out) HIP_TRY(hipMemcpyAsync(lpd_out, c->acq, bytes, hipMemcpyDeviceToHost, c->stream));
    if (sum_out) HIP_TRY(hipMemcpyAsync(sum_out, sum_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

extern "C" int cbo_gp_loo(cbo_gp *g, double *mean_out, double *var_out, double *lpd_out, double *sum_lpd_out)
{
    if (!g) return fail(CBO_ERR_INVALID, "gp is NULL");
    if (!mean_out && !var_out && !lpd_out && !sum_lpd_out) return fail(CBO_ERR_INVALID, "cbo_gp_loo: every output is NULL");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    HIP_TRY(hipSetDevice(g->ctx->device));
    return general_loo(g, mean_out, var_out, lpd_out, sum_lpd_out);
}

// Many models, one launch: every fp64 model of at most 128 observations goes into ONE small_loo_batch_kernel launch (one
// workgroup each, from the data and the current hyper-parameters: no fit, nothing of the model touched).  The others --
// larger models, and small ones whose Ky is not positive definite as assembled (fitted here with the jitchol ladder) --
// are answered one by one by general_loo, as cbo_gp_loo would.
extern "C" int cbo_gp_loo_batch(int n_models, cbo_gp *const *gps, double *sum_lpd, double *lpd_cat, int *status)
{
    if (n_models <= 0 || !gps || !sum_lpd || !status) return fail(CBO_ERR_INVALID, "bad argument");
    int rc = check_model_handles(n_models, gps);
    if (rc != CBO_OK) return rc;
    cbo_ctx *c = gps[0]->ctx;
    std::vector<int> small;
    std::vector<int64_t> offset((size_t)n_models);
    int64_t total = 0;
    for (int i = 0; i < n_models; ++i) {
        offset[(size_t)i] = total;
        total += gps[i]->n;
    }
    partition_small(n_models, [&](int i) { return small_lml_eligible(gps[i]); }, [](int) { return (int64_t)1; }, small);
    const int ns = (int)small.size();
    auto prepare = [&]() -> int {
        int rc = ensure_small_buffers(c, ns, 1);
        if (rc != CBO_OK) return rc;
        if ((size_t)ns * small_loo_scratch_doubles() > c->small_scratch.cap)
            return fail(CBO_ERR_INVALID, "leave-one-out batch: scratch smaller than expected");
        rc = grow(c, c->loo_out, ns < 32 ? 32 : (size_t)ns, true);
        for (int j = 0; rc == CBO_OK && j < ns; ++j) {
            c->sets_host[j] = cbo_small_set{};
            fill_small_model(c->sets_host[j], gps[small[(size_t)j]]);
        }
        return rc;
    };
    return run_small_or_general(
        c, "cbo_gp_loo_batch", "leave-one-out batch kernel: no result record", n_models, small, c->loo_out, prepare,
        [&](const SmallLaunch &L) { launch_small_loo_batch(c->stream, c->sets_host, ns, L.scratch, L.info, c->loo_out, L.seq); },
        [&](int j, int i) {
            sum_lpd[i] = c->loo_out[j].sum;
            if (lpd_cat) std::memcpy(lpd_cat + offset[(size_t)i], c->loo_out[j].lpd, sizeof(double) * (size_t)gps[i]->n);
            status[i] = CBO_OK;
            return CBO_OK;
        },
        // an error is the model's status, not the call's -- unless the device is in trouble: no per-model answer means anything
        [&](int i) -> int {
            cbo_gp *g = gps[i];
            int rc = CBO_OK;
            if (!g->fitted && g->n_pad == kPadN) rc = cbo_gp_fit(g, nullptr, nullptr);   // (jitchol ladder)
            if (rc == CBO_OK && !g->fitted) rc = fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
            if (rc == CBO_OK) rc = general_loo(g, nullptr, nullptr, lpd_cat ? lpd_cat + offset[(size_t)i] : nullptr, &sum_lpd[i]);
            status[i] = rc;
            return rc == CBO_ERR_HIP ? rc : CBO_OK;
        });
}

// the reversed factor of the backward substitution (kernels_kmat.hip), once per fit
static int ensure_reversed_factor(cbo_gp *g)
{
    cbo_ctx *c = g->ctx;
    if (!g->T) {
        HIP_TRY(hipMalloc(&g->T, sizeof(double) * (size_t)g->n_pad * (size_t)g->lda));
        HIP_TRY(hipMalloc(&g->invT, sizeof(double) * (size_t)(g->n_pad / 16) * 256));
        g->t_stamp = 0;
    }
    if (g->t_stamp != g->fit_stamp) {
        launch_reversed_factor(c->stream, g->A, g->lda, g->n_pad, g->invDt, g->T, g->lda, g->invT);
        HIP_TRY(hipGetLastError());
        g->t_stamp = g->fit_stamp;
    }
    return CBO_OK;
}

// Gradients of the posterior at a batch of points, any size: per workspace chunk, V = L^-1 K* by the forward sweep,
// W = L^-T V by the SAME strip kernel on the reversed system (the factor read backwards is lower triangular again),
// then one pass that forms both gradients from alpha and W.  Nothing is allocated once the workspaces have grown.
extern "C" int cbo_gp_predict_gradients(cbo_gp *g, int64_t m, const double *Xs, const double *pv_s, double *dmean_out,
                                        double *dvar_out)
{
    if (!g || !Xs || !dmean_out || !dvar_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0) return fail(CBO_ERR_INVALID, "m must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool causal = g->X.sv != nullptr;
    if (causal && !pv_s) return fail(CBO_ERR_INVALID, "causal gp needs the prior variance at the prediction points");
    // (the prior mean does not enter the gradients: GPy ignores the mean function there)
    cbo_cands *k = nullptr;
    int rc = scratch_points(g, m, Xs, nullptr, pv_s, &k);
    if (rc != CBO_OK) return rc;
    rc = prepare_cands(g, k);
    if (rc == CBO_OK) rc = ensure_alpha(g);
    if (rc == CBO_OK) rc = ensure_reversed_factor(g);
    if (rc != CBO_OK) return rc;
    // two workspaces of the same shape: V (forward) and W (backward); halve the budget so that both fit it
    int64_t chunk = 0, ldv = 0;
    const size_t saved_cap = c->max_ws_bytes;
    c->max_ws_bytes = saved_cap / 2;
    rc = ensure_workspaces(c, g->n_pad, k->m_pad, &chunk, &ldv);
    c->max_ws_bytes = saved_cap;
    if (rc != CBO_OK) return rc;
    rc = grow(c, c->W, (size_t)g->n_pad * (size_t)ldv);
    if (rc == CBO_OK) rc = grow(c, c->grads, 2 * (size_t)k->m_pad * (size_t)g->d);
    if (rc != CBO_OK) return rc;
    if (g->h.ard && !g->inv_ls_dev) HIP_TRY(hipMalloc(&g->inv_ls_dev, sizeof(double) * CBO_MAX_DIM));
    if (g->h.ard) {
        double il[CBO_MAX_DIM] = {0};
        for (int i = 0; i < g->d; ++i) il[i] = 1.0 / g->ls[(size_t)i];
        HIP_TRY(hipMemcpyAsync(g->inv_ls_dev, il, sizeof(double) * g->d, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));               // `il` lives in this frame
    }
    double *dmean = c->grads, *dvar = c->grads + (size_t)k->m_pad * g->d;
    for (int64_t c0 = 0; c0 < k->m_pad; c0 += chunk) {
        const int64_t cols = (k->m_pad - c0 < chunk) ? (k->m_pad - c0) : chunk;
        launch_kstar(c->stream, g->X, k->P, c0, cols, g->h, c->V, ldv, g->n_pad);
        launch_trsm_strips(c->stream, g->A, g->lda, g->invDt, c->V, ldv, g->n_pad, cols, nullptr, nullptr, nullptr);
        launch_reverse_rows(c->stream, c->V, ldv, g->n_pad, cols, c->W, ldv);
        launch_trsm_strips(c->stream, g->T, g->lda, g->invT, c->W, ldv, g->n_pad, cols, nullptr, nullptr, nullptr);
        launch_pred_gradients(c->stream, g->X, g->n_pad, k->P, c0, cols, m, g->h, g->inv_ls_dev, g->alpha, c->W, ldv,
                              dmean, dvar);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dmean_out, dmean, sizeof(double) * m * g->d, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dvar_out, dvar, sizeof(double) * m * g->d, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

extern "C" int cbo_gp_predict_grouped(cbo_gp *g, int64_t m_groups, int64_t group, const double *Xs, const double *pm,
                                      const double *pv, int include_noise, double *mean_out, double *var_out)
{
    if (!g || !mean_out || !var_out || !Xs) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m_groups <= 0 || group <= 0) return fail(CBO_ERR_INVALID, "m_groups and group must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    cbo_ctx *c = g->ctx;
    const int64_t m = m_groups * group;
    cbo_cands *k = nullptr;
    int rc = posterior_of_host_points(g, m, Xs, pm, pv, include_noise, &k);
    if (rc != CBO_OK) return rc;
    return group_means_out(c, m_groups, group, mean_out, var_out);
}

// Do-calculus prior of a batch of candidate interventions, inputs built on the device (SURVEY.md §8 f1;
// src/DoCalculus.py:34-89): for candidate c the graph-level GP is evaluated at the n_obs observed input rows with the
// intervened columns overwritten by values[c], and mean / variance are averaged over those rows.  Only `observed`
// (n_obs x d) and `values` (m x n_iv) are uploaded; the m * n_obs prediction points exist on the device only.
extern "C" int cbo_gp_predict_do(cbo_gp *g, int64_t m, int64_t n_obs, const double *observed, int n_iv,
                                 const double *values, const int *iv_index, int include_noise, double *mean_out,
                                 double *var_out)
{
    if (!g || !observed || !values || !iv_index || !mean_out || !var_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0 || n_obs <= 0 || n_iv <= 0) return fail(CBO_ERR_INVALID, "m, n_obs and n_iv must be positive");
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    if (g->X.sv != nullptr) return fail(CBO_ERR_INVALID, "the do-calculus inputs go to a graph-level (non-causal) gp");
    for (int j = 0; j < g->d; ++j)
        if (iv_index[j] >= n_iv) return fail(CBO_ERR_INVALID, "iv_index refers to a column values does not have");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t total = m * n_obs;
    cbo_cands *k = scratch_set(c);
    int rc = cands_reserve(k, total, g->d, false);
    if (rc != CBO_OK) return rc;
    // staging for observed | values | iv_index: the export scratch (device), filled by three small copies
    const size_t need = (size_t)(n_obs * g->d) + (size_t)(m * n_iv) + CBO_MAX_DIM;
    rc = grow(c, c->export_buf, need);
    if (rc != CBO_OK) return rc;
    double *d_obs = c->export_buf, *d_val = d_obs + n_obs * g->d;
    int *d_idx = reinterpret_cast<int *>(d_val + m * n_iv);
    HIP_TRY(hipMemcpyAsync(d_obs, observed, sizeof(double) * n_obs * g->d, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_val, values, sizeof(double) * m * n_iv, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_idx, iv_index, sizeof(int) * g->d, hipMemcpyHostToDevice, c->stream));
    cands_describe(k, total, g->d, false, 0);
    launch_expand_interventions(c->stream, d_obs, n_obs, g->d, d_val, n_iv, d_idx, m, k->raw);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));               // the host buffers are the caller's
    rc = posterior_of_set(g, k, include_noise);
    if (rc != CBO_OK) return rc;
    return group_means_out(c, m, n_obs, mean_out, var_out);
}

// ---- the device-resident do-calculus prior (kernels_do_prior.hip) ----------------------------------------
// Preparation, once per handle: W = L^-1 from the identity right-hand sides through the strip kernel (as cbo_gp_loo has it)
// in the V workspace, b in the W workspace (k-major, V's leading dimension), Ky^-1 = W^T W and b^T b on the joint
// posterior's tile loop with the element-wise product as the second product's epilogue, w from b's column means and alpha.
extern "C" int cbo_do_prior_create(cbo_gp *g, int64_t n_obs, const double *observed, int n_iv, const int *iv_index,
                                   cbo_do_prior **out)
{
    if (!g || !observed || !iv_index || !out) return fail(CBO_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_obs <= 0) return fail(CBO_ERR_INVALID, "n_obs must be positive");
    if (n_iv <= 0 || n_iv > CBO_MAX_DIM) return fail(CBO_ERR_INVALID, "n_iv must be in 1.." + std::to_string(CBO_MAX_DIM));
    if (!g->fitted) return fail(CBO_ERR_NOT_FITTED, "gp is not fitted");
    int n_col = 0;
    for (int j = 0; j < g->d; ++j) {
        if (iv_index[j] >= n_iv) return fail(CBO_ERR_INVALID, "intervened_index refers to a column values does not have");
        n_col += iv_index[j] >= 0 ? 1 : 0;
    }
    if (n_col == 0) return fail(CBO_ERR_INVALID, "no column is intervened");
    if (g->dtype != CBO_DTYPE_F64) return fail(CBO_ERR_UNSUPPORTED, "do-calculus prior: an fp32 graph gp is not supported");
    if (g->X.sv != nullptr)
        return fail(CBO_ERR_UNSUPPORTED, "do-calculus prior: a causal graph gp (it has a prior of its own) is not supported");
    if (g->n > kDoPriorMaxN)
        return fail(CBO_ERR_UNSUPPORTED, "do-calculus prior: the graph gp has " + std::to_string(g->n) + " rows, more than CBO_DO_PRIOR_MAX_N = " +
                                             std::to_string(kDoPriorMaxN));
    if (g->tries != 0 || g->jitter != 0.0)
        return fail(CBO_ERR_UNSUPPORTED, "do-calculus prior: the graph gp needed jitchol's jitter");
    const double sn = g->noise_var + kGpyDiagJitter;
    if (!(sn / ((double)g->n * g->h.variance + sn) >= 0x1p-26))
        return fail(CBO_ERR_UNSUPPORTED, "do-calculus prior: the clip rule -- sn / (n_g sigma^2 + sn) is below 2^-26 (noise too "
                                         "small for the factored variance to stay clear of GPy's clip)");
    cbo_ctx *c = g->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_alpha(g);
    if (rc != CBO_OK) return rc;
    const int64_t n_pad = g->n_pad, rows_pad = round_up(n_obs, 16);
    int64_t chunk = 0, ldv = 0;
    rc = ensure_workspaces(c, n_pad, n_pad, &chunk, &ldv);
    if (rc != CBO_OK) return rc;
    if (chunk < n_pad) return fail(CBO_ERR_UNSUPPORTED, "do-calculus prior: the workspace (CBO_HIP_WORKSPACE_MB) does not hold L^-1");
    rc = grow(c, c->W, (size_t)rows_pad * (size_t)ldv);
    if (rc == CBO_OK) rc = grow(c, c->export_buf, (size_t)(n_obs * g->d));
    if (rc != CBO_OK) return rc;

    cbo_do_prior *p = new cbo_do_prior();
    p->ctx = c;
    const size_t doubles = (size_t)n_pad + (size_t)n_pad * (size_t)n_pad + (size_t)n_col * (size_t)n_pad;
    auto bail = [&](int code) {
        if (p->mem) (void)hipFree(p->mem);
        if (p->view) (void)hipFree(p->view);
        delete p;
        return code;
    };
#define PRIOR_TRY(expr)                                                                                     \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            (void)hipGetLastError();                                                                        \
            return bail(fail(CBO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)));              \
        }                                                                                                   \
    } while (0)
    PRIOR_TRY(hipMalloc(&p->mem, sizeof(double) * doubles));
    PRIOR_TRY(hipMalloc(&p->view, sizeof(DoPriorView)));
    double *w = p->mem, *M = w + n_pad, *xi = M + (size_t)n_pad * (size_t)n_pad;
    DoPriorView &h = p->h;
    h.w = w; h.M = M; h.xi = xi; h.ldm = n_pad; h.ldx = n_pad;
    h.inv_l2 = 1.0 / (g->h.lengthscale * g->h.lengthscale);
    h.vmax = g->h.variance + g->noise_var;
    h.n = (int)g->n; h.n_col = n_col; h.n_iv = n_iv; h.ard = g->h.ard;
    DoPriorRowsArgs ra{};
    ra.obs = c->export_buf; ra.xs = g->X.xs; ra.b = c->W;
    ra.n_obs = n_obs; ra.rows_pad = rows_pad; ra.ldb = ldv; ra.ldx = g->X.ld;
    ra.inv_l2 = h.inv_l2; ra.n = (int)g->n; ra.d = g->d; ra.ard = g->h.ard;
    for (int k = 0; k < CBO_MAX_DIM; ++k) { h.ls[k] = 1.0; h.src[k] = 0; ra.ls[k] = 1.0; ra.col[k] = 0; }
    for (int j = 0, ki = 0, kf = 0; j < g->d; ++j) {
        const double l = g->h.ard ? g->ls[(size_t)j] : 1.0;
        if (iv_index[j] >= 0) {
            h.ls[ki] = l; h.src[ki] = iv_index[j];
            PRIOR_TRY(hipMemcpyAsync(xi + (size_t)ki * (size_t)n_pad, g->X.xs + (int64_t)j * g->X.ld, sizeof(double) * (size_t)g->n,
                                     hipMemcpyDeviceToDevice, c->stream));
            ++ki;
        } else {
            ra.ls[kf] = l; ra.col[kf] = j;
            ++kf;
        }
        ra.n_free = kf;
    }
    PRIOR_TRY(hipMemcpyAsync(c->export_buf, observed, sizeof(double) * (size_t)(n_obs * g->d), hipMemcpyHostToDevice, c->stream));
    PRIOR_TRY(hipMemcpyAsync(p->view, &h, sizeof(DoPriorView), hipMemcpyHostToDevice, c->stream));
    // W = L^-1: the identity through the strip kernel
    launch_loo_identity_chunk(c->stream, c->V, ldv, n_pad, n_pad, 0);
    launch_trsm_strips(c->stream, g->A, g->lda, g->invDt, c->V, ldv, n_pad, n_pad, nullptr, nullptr, nullptr);
    launch_do_prior_rows(c->stream, ra);
    launch_do_prior_weights(c->stream, c->W, ldv, n_obs, g->alpha, g->h.variance, (int)g->n, w);
    GramArgs ga{};
    ga.A = c->V; ga.lda = ldv; ga.n_k = (int)n_pad; ga.prev = nullptr; ga.out = M; ga.ldo = n_pad; ga.n = (int)g->n;
    ga.divisor = 1.0; ga.scale = 1.0;
    launch_gram_tiles(c->stream, ga);
    ga.A = c->W; ga.n_k = (int)rows_pad; ga.prev = M; ga.divisor = (double)n_obs;
    ga.scale = (g->h.variance * g->h.variance);
    launch_gram_tiles(c->stream, ga);
    PRIOR_TRY(hipGetLastError());
    PRIOR_TRY(hipStreamSynchronize(c->stream));                // (`observed` and the view are the caller's / this frame's)
#undef PRIOR_TRY
    *out = p;
    return CBO_OK;
}

extern "C" void cbo_do_prior_destroy(cbo_do_prior *p)
{
    if (!p) return;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    hipFree(p->mem);
    hipFree(p->view);
    delete p;
}

extern "C" int cbo_do_prior_eval(const cbo_do_prior *p, int64_t m, const double *values, double *mean_out, double *var_out)
{
    if (!p || !values || !mean_out || !var_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (m <= 0) return fail(CBO_ERR_INVALID, "m must be positive");
    cbo_ctx *c = p->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int n_iv = p->h.n_iv;
    const size_t scratch = (size_t)do_prior_eval_blocks(m) * (size_t)kDoPriorMaxN;
    int rc = grow(c, c->export_buf, (size_t)m * (size_t)n_iv + 2 * (size_t)m + scratch);
    if (rc != CBO_OK) return rc;
    double *d_val = c->export_buf, *d_mean = d_val + (size_t)m * (size_t)n_iv, *d_var = d_mean + m, *d_scr = d_var + m;
    HIP_TRY(hipMemcpyAsync(d_val, values, sizeof(double) * (size_t)m * (size_t)n_iv, hipMemcpyHostToDevice, c->stream));
    launch_do_prior_eval(c->stream, p->view, d_val, m, d_scr, d_mean, d_var);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mean_out, d_mean, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(var_out, d_var, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

// ---- tiny host-side reductions -------------------------------------------------------------------
static bool host_better(double va, int64_t ia, double vb, int64_t ib)
{
    const bool na = std::isnan(va), nb = std::isnan(vb);
    if (na != nb) return na;
    if (na || va == vb) return ia < ib;
    return va > vb;
}

extern "C" int cbo_argmax_sets(const double *ys, int s, int *idx_out)
{
    if (!ys || !idx_out || s <= 0) return fail(CBO_ERR_INVALID, "bad argument");
    // np.where(ys == np.max(ys))[0][0]  (src/CBO.py:275): np.max propagates NaN, and NaN == NaN is
    // false, so the reference raises IndexError there; we report the first NaN instead.
    int best = 0;
    for (int i = 1; i < s; ++i)
        if (host_better(ys[i], i, ys[best], best)) best = i;
    *idx_out = best;
    return CBO_OK;
}

extern "C" int cbo_argmax_pairs(const double *vals, const int64_t *idxs, int n, double *best_val, int64_t *best_idx)
{
    if (!vals || !idxs || n <= 0 || !best_val || !best_idx) return fail(CBO_ERR_INVALID, "bad argument");
    int b = 0;
    for (int i = 1; i < n; ++i)
        if (host_better(vals[i], idxs[i], vals[b], idxs[b])) b = i;
    *best_val = vals[b];
    *best_idx = idxs[b];
    return CBO_OK;
}

// ---- Monte-Carlo interventional target (f4) ----------------------------------------------------------
struct cbo_sem {
    cbo_ctx *ctx = nullptr;
    cbo_sem_spec spec{};
    int64_t n_draws = 0;
    int n_eps = 0;
    double *eps_cm = nullptr;        // n_eps x n_draws (column of the caller's matrix = contiguous run here)
    // per-call workspaces, grown on demand
    double *values = nullptr, *partial = nullptr, *mean = nullptr;
    int *iv_nodes = nullptr;
    int64_t cap_m = 0;
    int cap_iv = 0;
};

static int check_sem_spec(const cbo_sem_spec *sp, int n_eps)
{
    if (sp->n_nodes < 1 || sp->n_nodes > CBO_SEM_MAX_NODES) return fail(CBO_ERR_INVALID, "sem: n_nodes out of range");
    if (sp->term_begin[0] != 0) return fail(CBO_ERR_INVALID, "sem: term_begin[0] must be 0");
    for (int k = 0; k < sp->n_nodes; ++k) {
        if (sp->term_begin[k + 1] < sp->term_begin[k] || sp->term_begin[k + 1] > CBO_SEM_MAX_TERMS)
            return fail(CBO_ERR_INVALID, "sem: term_begin must be non-decreasing and <= CBO_SEM_MAX_TERMS");
        if (sp->eps_index[k] < -1 || sp->eps_index[k] >= n_eps)
            return fail(CBO_ERR_INVALID, "sem: eps_index out of range");
        for (int t = sp->term_begin[k]; t < sp->term_begin[k + 1]; ++t) {
            if (sp->term_parent[t] < 0 || sp->term_parent[t] >= k)
                return fail(CBO_ERR_INVALID, "sem: a term must read an earlier node (evaluation order)");
            if (sp->term_fn[t] < CBO_FN_ID || sp->term_fn[t] > CBO_FN_SIN)
                return fail(CBO_ERR_INVALID, "sem: unknown term function");
        }
    }
    return CBO_OK;
}

extern "C" int cbo_sem_create(cbo_ctx *c, const cbo_sem_spec *spec, int64_t n_samples, int n_eps, const double *eps,
                              cbo_sem **out)
{
    if (!c || !spec || !eps || !out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (n_samples <= 0 || n_eps < 1 || n_eps > CBO_SEM_MAX_NODES)
        return fail(CBO_ERR_INVALID, "sem: n_samples must be positive and n_eps in [1, CBO_SEM_MAX_NODES]");
    int rc = check_sem_spec(spec, n_eps);
    if (rc != CBO_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    cbo_sem *m = new cbo_sem();
    m->ctx = c; m->spec = *spec; m->n_draws = n_samples; m->n_eps = n_eps;
    std::vector<double> cm((size_t)n_samples * n_eps);
    for (int64_t s = 0; s < n_samples; ++s)
        for (int k = 0; k < n_eps; ++k) cm[(size_t)k * n_samples + s] = eps[s * n_eps + k];
    hipError_t e = hipMalloc(&m->eps_cm, sizeof(double) * cm.size());
    if (e == hipSuccess) e = hipMemcpy(m->eps_cm, cm.data(), sizeof(double) * cm.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        cbo_sem_destroy(m);
        return fail(CBO_ERR_HIP, std::string("cbo_sem_create: ") + hipGetErrorString(e));
    }
    *out = m;
    return CBO_OK;
}

extern "C" void cbo_sem_destroy(cbo_sem *m)
{
    if (!m) return;
    hipSetDevice(m->ctx->device);
    hipStreamSynchronize(m->ctx->stream);
    hipFree(m->eps_cm); hipFree(m->values); hipFree(m->partial); hipFree(m->mean); hipFree(m->iv_nodes);
    delete m;
}

extern "C" int cbo_sem_target(cbo_sem *m, int target, int64_t n_iv_sets, int n_iv, const int *iv_nodes,
                              const double *values, double *mean_out)
{
    if (!m || !mean_out) return fail(CBO_ERR_INVALID, "NULL argument");
    if (n_iv_sets <= 0) return fail(CBO_ERR_INVALID, "sem: m must be positive");
    if (target < 0 || target >= m->spec.n_nodes) return fail(CBO_ERR_INVALID, "sem: target node out of range");
    if (n_iv < 0 || n_iv > CBO_SEM_MAX_NODES) return fail(CBO_ERR_INVALID, "sem: n_iv out of range");
    if (n_iv > 0 && (!iv_nodes || !values)) return fail(CBO_ERR_INVALID, "sem: intervention nodes/values missing");
    for (int j = 0; j < n_iv; ++j)
        if (iv_nodes[j] < 0 || iv_nodes[j] >= m->spec.n_nodes)
            return fail(CBO_ERR_INVALID, "sem: intervened node out of range");
    cbo_ctx *c = m->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int nb = sem_partial_blocks(m->n_draws);
    const int iv_cols = n_iv > 0 ? n_iv : 1;
    if (n_iv_sets > m->cap_m || iv_cols > m->cap_iv) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        hipFree(m->values); hipFree(m->partial); hipFree(m->mean); hipFree(m->iv_nodes);
        m->values = m->partial = m->mean = nullptr; m->iv_nodes = nullptr; m->cap_m = 0; m->cap_iv = 0;
        const int64_t cap = n_iv_sets > m->cap_m ? n_iv_sets : m->cap_m;
        HIP_TRY(hipMalloc(&m->values, sizeof(double) * cap * CBO_SEM_MAX_NODES));
        HIP_TRY(hipMalloc(&m->partial, sizeof(double) * cap * nb));
        HIP_TRY(hipMalloc(&m->mean, sizeof(double) * cap));
        HIP_TRY(hipMalloc(&m->iv_nodes, sizeof(int) * CBO_SEM_MAX_NODES));
        m->cap_m = cap; m->cap_iv = CBO_SEM_MAX_NODES;
    }
    if (n_iv > 0) {
        HIP_TRY(hipMemcpyAsync(m->values, values, sizeof(double) * n_iv_sets * n_iv, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(m->iv_nodes, iv_nodes, sizeof(int) * n_iv, hipMemcpyHostToDevice, c->stream));
    }
    launch_sem_target(c->stream, m->spec, m->eps_cm, m->n_draws, target, n_iv_sets, n_iv, iv_nodes, m->iv_nodes, m->values,
                      m->partial, m->mean);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mean_out, m->mean, sizeof(double) * n_iv_sets, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CBO_OK;
}

extern "C" int cbo_selftest_mfma(cbo_ctx *c, double *max_abs_err_out)
{
    if (!c) return fail(CBO_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    double err = -1.0;
    if (run_mfma_selftest(c->stream, &err) != 0) return fail(CBO_ERR_HIP, "mfma selftest launch failed");
    if (max_abs_err_out) *max_abs_err_out = err;
    if (err != 0.0) return fail(CBO_ERR_HIP, "fp64 MFMA lane map differs from what the kernels assume");
    double err32 = -1.0;
    if (run_mfma_f32_selftest(c->stream, &err32) != 0) return fail(CBO_ERR_HIP, "f32 mfma selftest launch failed");
    if (max_abs_err_out) *max_abs_err_out = err32 > err ? err32 : err;
    if (err32 != 0.0) return fail(CBO_ERR_HIP, "fp32 MFMA lane map differs from what the kernels assume");
    return CBO_OK;
}

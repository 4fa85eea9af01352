// Block append (cbo_gp_append_block): k <= 64 observations join a fitted model in one device step.
//
// Appending k rows and columns to Ky leaves the first n rows of its factor and of V = L^-1 K* unchanged, exactly as for
// one row (kernels_acq.hip, "append-only trial step").  With L the current factor, z = L^-1 (y - m), Xb the new points:
//     B   = L^-1 K(X, Xb)                      (n x k)     append_forward_step_kernel, one launch per 128-row block
//     S   = K(Xb, Xb) + sigma I - B^T B        (k x k)     append_schur_partial_kernel + append_schur_final_kernel
//     L22 = chol(S),  zb = L22^-1 ((yb - m(Xb)) - B^T z)   (the same workgroup; status word = first bad pivot, 1-based)
//     U[0:n, n:n+k] = B, U[n:n+k, n:n+k] = L22^T, z[n:n+k] = zb, invDt columns     append_block_commit_kernel + _inverse_
// and for a candidate set whose V is resident
//     C = K(Xb, X*) - B^T V[0:n, :],  W = L22^-1 C,  V[n:n+k, :] = W,  q += sum_r W_r^2,  mu += sum_r W_r zb_r
//                                                          append_rows_pass_kernel (fp64 MFMA) + append_rows_final_kernel
// Lane maps of v_mfma_f64_16x16x4_f64 as run_mfma_selftest pins them: a = A[i = lane & 15][k = lane >> 4],
// b = B[k = lane >> 4][j = lane & 15], acc[r] = C[i = (lane >> 4) + 4 r][j = lane & 15].
// Every sum has a fixed order (slices in slice order, waves in wave order, rows in row order); no atomics.
#include "cbo_device.h"

namespace cbo {

#define APPEND_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

static_assert(kAppendLd == CBO_MAX_APPEND, "B, L22 and the probe set are laid out for the largest block");

// ---- B = L^-1 K(X, Xb): forward_step_kernel (kernels_chol.hip) for kp = 16 RT right-hand sides ---------------------------
// One launch per 128-row block blk.  Every workgroup solves the 128 x 128 diagonal system for all kp columns in LDS
// (16-row sub-blocks: multiply by the transposed stored inv(U_ss), fold into the rows below; the sub-block's panel of U is
// prefetched one step ahead), workgroup 0 stores the block's rows of B, and workgroup g folds them into the 128 rows of
// block blk + 1 + g of the work array on the MFMA:  W[c][r] -= sum_k U[b0 + k][c] l[k][r]  (A operand: rows of U, contiguous
// in c; B operand: the solved rows from LDS).  W: [n_pad][ldw] holding K(X, Xb) on entry; out: [n_pad][kAppendLd].
template <int RT>
__global__ __launch_bounds__(256) void append_forward_step_kernel(const double *__restrict__ A, int64_t lda,
                                                                  const double *__restrict__ invDt, int blk, int nb,
                                                                  double *W, int64_t ldw, double *__restrict__ out)
{
    constexpr int KP = 16 * RT;
    extern __shared__ __align__(16) unsigned char append_smem[];
    double *rs = reinterpret_cast<double *>(append_smem);          // [128][KP] right-hand sides, solved in place
    double *pan = rs + 128 * KP;                                   // [16][128] U[o .. o+16][.] of the current sub-block
    double *Ys = pan + 16 * 128;                                   // [8][256] the block's diagonal-tile inverses
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blk * 128;
    for (int idx = tid; idx < 128 * KP; idx += 256) rs[idx] = W[(b0 + idx / KP) * ldw + idx % KP];
    for (int idx = tid; idx < 8 * 256; idx += 256) Ys[idx] = invDt[(b0 / 16) * 256 + idx];
    // the A operands of the update below (this wave's 32 columns of the block's 128 rows of U) do not depend on the
    // solve: they are requested here and arrive while it runs
    const int g = blockIdx.x, bb = blk + 1 + g;
    const int lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
    const int64_t c0 = (int64_t)bb * 128 + 32 * wave;               // this wave's 32 rows of the block below
    double ua[32][2];
    if (bb < nb) {
        const double *ga = A + (b0 + kq) * lda + c0 + lc;
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) {
            ua[ks][0] = ga[(int64_t)(4 * ks) * lda];
            ua[ks][1] = ga[(int64_t)(4 * ks) * lda + 16];
        }
    }
    double pre[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int idx = tid + 256 * t, k = idx >> 7, c = idx & 127;
        pre[t] = (c >= 16) ? A[(b0 + k) * lda + b0 + c] : 0.0;
    }
    __syncthreads();
    for (int s = 0; s < 8; ++s) {
        const int o = 16 * s;
#pragma unroll
        for (int t = 0; t < 8; ++t) pan[tid + 256 * t] = pre[t];
        if (s < 7) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int idx = tid + 256 * t, k = idx >> 7, c = idx & 127;
                pre[t] = (c >= o + 32) ? A[(b0 + o + 16 + k) * lda + b0 + c] : 0.0;
            }
        }
        // l_s = inv(U_ss)^T r_s for every column: Y[k][i] = inv(U_ss)[k][i], zero for k > i
        double ls[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int idx = tid + 256 * t, i = idx / KP, r = idx % KP;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) acc = fma(Ys[s * 256 + k * 16 + i], rs[(o + k) * KP + r], acc);
            ls[t] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int idx = tid + 256 * t;
            rs[(o + idx / KP) * KP + idx % KP] = ls[t];
        }
        __syncthreads();
        // rows below inside the block: rs[c][r] -= sum_k U[b0 + o + k][b0 + c] l[o + k][r], c >= o + 16
        if (256 % KP == 0) {
            // a thread keeps its column r over the rows c: the 16 solved entries of that column stay in registers
            const int r = tid % KP;
            double lr[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) lr[k] = rs[(o + k) * KP + r];
            for (int c = o + 16 + tid / KP; c < 128; c += 256 / KP) {
                double acc = rs[c * KP + r];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc = fma(-pan[k * 128 + c], lr[k], acc);
                rs[c * KP + r] = acc;
            }
        } else {
            for (int idx = tid; idx < (112 - o) * KP; idx += 256) {
                const int c = o + 16 + idx / KP, r = idx % KP;
                double acc = rs[c * KP + r];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc = fma(-pan[k * 128 + c], rs[(o + k) * KP + r], acc);
                rs[c * KP + r] = acc;
            }
        }
        __syncthreads();
    }
    if (g == 0)
        for (int idx = tid; idx < 128 * KP; idx += 256) out[(b0 + idx / KP) * kAppendLd + idx % KP] = rs[idx];
    if (bb >= nb) return;                                           // the last block has nothing below it (uniform)
    d4 acc[2][RT];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const double a0 = ua[ks][0], a1 = ua[ks][1];
        double bf[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) bf[rt] = rs[(4 * ks + kq) * KP + 16 * rt + lc];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            acc[0][rt] = APPEND_MFMA(a0, bf[rt], acc[0][rt]);
            acc[1][rt] = APPEND_MFMA(a1, bf[rt], acc[1][rt]);
        }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double *w = &W[(c0 + 16 * ct + kq + 4 * r) * ldw + 16 * rt + lc];
                *w -= acc[ct][rt][r];
            }
}

template <int RT>
static void launch_forward_rt(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *W,
                              int64_t ldw, double *out)
{
    constexpr int bytes = (int)sizeof(double) * (128 * 16 * RT + 16 * 128 + 8 * 256);
    // > 64 KiB of dynamic LDS at RT = 4 needs the opt-in on the current device (per call: several devices in one process)
    hipFuncSetAttribute(reinterpret_cast<const void *>(append_forward_step_kernel<RT>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const int nb = (int)(n_pad / 128);
    for (int blk = 0; blk < nb; ++blk) {
        const int below = nb - 1 - blk;
        hipLaunchKernelGGL(append_forward_step_kernel<RT>, dim3(below > 0 ? below : 1), dim3(256), bytes, s, A, lda, invDt,
                           blk, nb, W, ldw, out);
    }
}

void launch_append_forward(hipStream_t s, const double *A, int64_t lda, int64_t n_pad, const double *invDt, double *W,
                           int64_t ldw, int kp, double *out)
{
    switch (kp / 16) {
        case 1: launch_forward_rt<1>(s, A, lda, n_pad, invDt, W, ldw, out); break;
        case 2: launch_forward_rt<2>(s, A, lda, n_pad, invDt, W, ldw, out); break;
        case 3: launch_forward_rt<3>(s, A, lda, n_pad, invDt, W, ldw, out); break;
        default: launch_forward_rt<4>(s, A, lda, n_pad, invDt, W, ldw, out); break;
    }
}

// ---- the Schur block -----------------------------------------------------------------------------------------------------
// part[slice][r][s] = sum over the slice's rows i of B[i][r] B[i][s] (r, s < 64), part[slice][64][r] = sum B[i][r] z[i]:
// thread (tr, tc) keeps the 4 x 4 block (4 tr .., 4 tc ..); rows go through LDS 32 at a time.
__global__ __launch_bounds__(256) void append_schur_partial_kernel(const double *__restrict__ B, int64_t n,
                                                                   int rows_per_slice, const double *__restrict__ z,
                                                                   double *__restrict__ part)
{
    __shared__ double bs[32][kAppendLd];
    __shared__ double zs[32];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int64_t i0 = (int64_t)blockIdx.x * rows_per_slice;
    const int64_t i1 = (i0 + rows_per_slice < n) ? i0 + rows_per_slice : n;
    double g[4][4], t = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) g[a][b] = 0.0;
    for (int64_t base = i0; base < i1; base += 32) {
        __syncthreads();
        for (int idx = tid; idx < 32 * kAppendLd; idx += 256) {
            const int64_t i = base + idx / kAppendLd;
            bs[idx / kAppendLd][idx % kAppendLd] = (i < i1) ? B[i * kAppendLd + idx % kAppendLd] : 0.0;
        }
        if (tid < 32) zs[tid] = (base + tid < i1) ? z[base + tid] : 0.0;
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < 32; ++i) {
            double br[4], bc[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { br[a] = bs[i][4 * tr + a]; bc[a] = bs[i][4 * tc + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) g[a][b] = fma(br[a], bc[b], g[a][b]);
            if (tid < kAppendLd) t = fma(bs[i][tid], zs[i], t);
        }
    }
    double *p = part + (int64_t)blockIdx.x * (kAppendLd + 1) * kAppendLd;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) p[(4 * tr + a) * kAppendLd + 4 * tc + b] = g[a][b];
    if (tid < kAppendLd) p[kAppendLd * kAppendLd + tid] = t;
}

// One workgroup: S from the slice sums (slice order) and K(Xb, Xb), its Cholesky factor in LDS, zb, the status word.
__global__ __launch_bounds__(256) void append_schur_final_kernel(AppendSchurArgs a)
{
    __shared__ double S[kAppendLd + 1][kAppendLd + 1];              // row k carries the right-hand side of zb
    const int tid = threadIdx.x, k = a.k;
    for (int idx = tid; idx < kAppendLd * kAppendLd; idx += 256) {
        const int r = idx / kAppendLd, s = idx % kAppendLd;
        double v = 0.0;
        if (r < k && s <= r) {
            double gsum = 0.0;
#pragma unroll 8
            for (int sl = 0; sl < a.slices; ++sl) gsum += a.part[(int64_t)sl * (kAppendLd + 1) * kAppendLd + idx];
            const double prior = (r == s) ? (a.variance + (a.pv ? a.pv[r] : 0.0)) + a.sigma : a.Kbb[(int64_t)r * a.ldk + s];
            v = prior - gsum;
        }
        S[r][s] = v;
    }
    __syncthreads();                                                // row k of S is written below: k may be 64
    if (tid < kAppendLd) {
        double t = 0.0;
        if (tid < k) {
#pragma unroll 8
            for (int sl = 0; sl < a.slices; ++sl)
                t += a.part[(int64_t)sl * (kAppendLd + 1) * kAppendLd + kAppendLd * kAppendLd + tid];
            t = (a.y_new[tid] - (a.pm ? a.pm[tid] : 0.0)) - t;
        }
        S[k][tid] = t;
    }
    __syncthreads();
    // Right-looking Cholesky of the lower triangle, column by column; the right-hand side rides along as row k, so that
    // it leaves as zb = L22^-1 rhs.  Every thread reads the pivot itself: the decision is uniform without a flag.
    int bad = 0;
    for (int j = 0; j < k; ++j) {
        const double p = S[j][j];
        if (!(p > 0.0) || !isfinite(p)) { bad = j + 1; break; }
        const double d = sqrt(p);
        __syncthreads();                                            // every thread has read the pivot
        if (tid == j) S[j][j] = d;
        if (tid > j && tid <= k) S[tid][j] = S[tid][j] / d;
        __syncthreads();
        for (int idx = tid; idx < (kAppendLd + 1) * kAppendLd; idx += 256) {
            const int r = idx >> 6, s = idx & 63;
            if (r > j && r <= k && s > j && s <= r && s < k) S[r][s] = fma(-S[r][j], S[s][j], S[r][s]);
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) *a.status = bad;
        return;
    }
    for (int idx = tid; idx < kAppendLd * kAppendLd; idx += 256) {
        const int r = idx / kAppendLd, s = idx % kAppendLd;
        a.L22[idx] = (r < k && s <= r) ? S[r][s] : 0.0;
    }
    if (tid < kAppendLd) a.zb[tid] = (tid < k) ? S[k][tid] : 0.0;
    if (tid == 0) *a.status = 0;
}

int append_schur_slices(int64_t n) { const int64_t s = (n + 127) / 128; return (int)(s < 1 ? 1 : (s > 64 ? 64 : s)); }

void launch_append_schur(hipStream_t s, const double *B, int64_t n, const double *z, AppendSchurArgs a)
{
    const int slices = append_schur_slices(n);
    const int rows_per_slice = (int)(((n + slices - 1) / slices + 31) / 32 * 32);
    hipLaunchKernelGGL(append_schur_partial_kernel, dim3(slices), dim3(256), 0, s, B, n, rows_per_slice, z,
                       const_cast<double *>(a.part));
    a.slices = slices;
    hipLaunchKernelGGL(append_schur_final_kernel, dim3(1), dim3(256), 0, s, a);
}

// ---- commit ----------------------------------------------------------------------------------------------------------------
// One thread per row: rows i < n take their k entries of the new columns of U; row n + r takes row r of L22^T, z, y and the
// point's data (append_commit_kernel's stores for every one of the k points).
__global__ void append_block_commit_kernel(AppendCommitArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = a.n;
    const int k = a.k;
    if (i < n) {
        for (int r = 0; r < k; ++r) a.A[i * a.lda + n + r] = a.B[i * kAppendLd + r];
    } else if (i < n + k) {
        const int r = (int)(i - n);
        for (int s = r; s < k; ++s) a.A[i * a.lda + n + s] = a.L22[s * kAppendLd + r];      // U[n + r][n + s] = L22[s][r]
        const double zr = a.zb[r];
        a.A[i * a.lda + a.n_pad] = zr;                              // the rhs column carries z
        a.z[i] = zr;
        a.y[i] = a.y_new[r];
        for (int c = 0; c < a.dims; ++c) a.xs[(int64_t)c * a.ldx + i] = a.pxs[(int64_t)c * a.ldp + r];
        a.sq[i] = a.psq[r];
        if (a.sv) { a.sv[i] = a.psv[r]; a.pm[i] = a.pm_new[r]; a.pv[i] = a.pv_new[r]; }
    }
}

// append_tile_inverse_kernel for every 16 x 16 diagonal tile the block touches (one workgroup each): the columns of the
// inverse that belong to rows n .. n + k - 1.  Columns of older rows keep their bits and the columns right of the block
// stay identity padding, for the reason given there: column b of the inverse of an upper-triangular matrix depends on its
// leading (b + 1) x (b + 1) block only.
__global__ void append_block_inverse_kernel(const double *__restrict__ A, int64_t lda, int64_t n, int k,
                                            double *__restrict__ invDt)
{
    __shared__ double T[16][17];
    const int64_t tile = n / 16 + blockIdx.x;
    const int t = threadIdx.x;
    const int a = t >> 4, b = t & 15;
    T[a][b] = (b >= a) ? A[(tile * 16 + a) * lda + tile * 16 + b] : 0.0;
    __syncthreads();
    const int64_t row = tile * 16 + t;
    if (t < 16 && row >= n && row < n + k) {                        // column t of the inverse by back substitution
        double x[16];
        for (int r = 0; r < 16; ++r) x[r] = 0.0;
        x[t] = 1.0 / T[t][t];
        for (int r = t - 1; r >= 0; --r) {
            double s = 0.0;
            for (int c = r + 1; c <= t; ++c) s = fma(T[r][c], x[c], s);
            x[r] = -s / T[r][r];
        }
        for (int r = 0; r < 16; ++r) invDt[tile * 256 + r * 16 + t] = x[r];
    }
}

void launch_append_block_commit(hipStream_t s, const AppendCommitArgs &a, double *invDt)
{
    hipLaunchKernelGGL(append_block_commit_kernel, dim3((unsigned)((a.n + a.k + 255) / 256)), dim3(256), 0, s, a);
    const int tiles = (int)((a.n + a.k - 1) / 16 - a.n / 16 + 1);
    hipLaunchKernelGGL(append_block_inverse_kernel, dim3(tiles), dim3(256), 0, s, a.A, a.lda, a.n, a.k, invDt);
}

// ---- the k new rows of a resident V ------------------------------------------------------------------------------------------
// part[slice][r][j] = sum over the slice's rows i of B[i][r] V[i][j] for a strip of 64 candidate columns: V is read once
// for all kp rows.  The four waves split every 64-row stage by rows (wave w: rows 16 w .. 16 w + 15, four MFMA k-steps) and
// keep all kp x 64 outputs each; B^T goes through LDS (one coalesced load of the stage's 64 x kp block), V straight from
// HBM into the B operand, 16 bytes per lane: lane (kq, lc) reads columns 32 h + 2 lc + e of row kq, so operand (h, e)
// holds column 32 h + 2 lc + e at j = lc.  The next stage's V is in flight while this one computes.  The waves' sums are
// added in wave order through LDS.
template <int RT>
__global__ __launch_bounds__(256) void append_rows_pass_kernel(const double *__restrict__ V, int64_t ldv,
                                                               const double *__restrict__ B, int64_t rows,
                                                               int rows_per_slice, int64_t m_pad, double *__restrict__ part)
{
    constexpr int KP = 16 * RT;
    __shared__ __align__(16) double bs[64 * KP];                   // the stage of B, then the waves' reduction [KP][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t i1 = (i0 + rows_per_slice < rows) ? i0 + rows_per_slice : rows;      // multiples of 64
    d4 acc[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[rt][f] = d4{0.0, 0.0, 0.0, 0.0};
    const double *gv = V + (16 * wave + kq) * ldv + j0 + 2 * lc;
    d2 cur[4][2], nxt[4][2];
    if (i0 < i1) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) cur[ks][h] = *reinterpret_cast<const d2 *>(gv + (i0 + 4 * ks) * ldv + 32 * h);
    }
    for (int64_t base = i0; base < i1; base += 64) {
        __syncthreads();                                            // the previous stage's reads of bs are done
        for (int idx = tid; idx < 64 * KP / 2; idx += 256) {
            const int row = idx / (KP / 2), c2 = idx % (KP / 2);
            *reinterpret_cast<d2 *>(&bs[row * KP + 2 * c2]) =
                *reinterpret_cast<const d2 *>(&B[(base + row) * kAppendLd + 2 * c2]);
        }
        if (base + 64 < i1) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    nxt[ks][h] = *reinterpret_cast<const d2 *>(gv + (base + 64 + 4 * ks) * ldv + 32 * h);
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            double af[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) af[rt] = bs[(16 * wave + 4 * ks + kq) * KP + 16 * rt + lc];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    acc[rt][2 * h] = APPEND_MFMA(af[rt], cur[ks][h][0], acc[rt][2 * h]);
                    acc[rt][2 * h + 1] = APPEND_MFMA(af[rt], cur[ks][h][1], acc[rt][2 * h + 1]);
                }
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) cur[ks][h] = nxt[ks][h];
    }
    // the four waves' sums, in wave order
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int f = 0; f < 4; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double *p = &bs[(16 * rt + kq + 4 * r) * 64 + 32 * (f >> 1) + 2 * lc + (f & 1)];
                        *p = (w == 0) ? acc[rt][f][r] : *p + acc[rt][f][r];
                    }
        }
    }
    __syncthreads();
    double *po = part + ((int64_t)blockIdx.y * KP) * m_pad + j0;
    for (int idx = tid; idx < KP * 64; idx += 256) po[(int64_t)(idx >> 6) * m_pad + (idx & 63)] = bs[idx];
}

// One thread per candidate column: C_r = K(Xb, X*)_rj - sum over the slices (slice order), the k-step forward substitution
// with L22 (LDS), the stores of the k new rows, q and mu in row order.
template <int RT>
__global__ __launch_bounds__(256) void append_rows_final_kernel(AppendRowsArgs a)
{
    constexpr int KP = 16 * RT;
    __shared__ double Ls[KP * KP];
    __shared__ double zs[KP];
    const int k = a.k;
    for (int idx = threadIdx.x; idx < KP * KP; idx += 256) Ls[idx] = a.L22[(idx / KP) * kAppendLd + idx % KP];
    if (threadIdx.x < KP) zs[threadIdx.x] = a.zb[threadIdx.x];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m_pad) return;
    double w[KP];
    double q = a.q[j], mu = a.mu[j];
#pragma unroll
    for (int r = 0; r < KP; ++r) {
        if (r < k) {
            double s = 0.0;
            for (int sl = 0; sl < a.slices; ++sl) s += a.part[((int64_t)sl * KP + r) * a.m_pad + j];
            double c = a.Kb[(int64_t)r * a.ldk + j] - s;
#pragma unroll
            for (int t = 0; t < r; ++t) c = fma(-Ls[r * KP + t], w[t], c);
            const double v = c / Ls[r * KP + r];
            w[r] = v;
            a.Vnew[(int64_t)r * a.ldv + j] = v;
            q = fma(v, v, q);
            mu = fma(v, zs[r], mu);
        } else {
            w[r] = 0.0;
        }
    }
    a.q[j] = q;
    a.mu[j] = mu;
}

void append_rows_plan(int64_t rows, int64_t m_pad, int *slices, int *rows_per_slice)
{
    const int64_t stages = (rows + 63) / 64, strips = m_pad / 64;
    int64_t want = (512 + strips - 1) / strips;
    if (want > kAppendMaxSlices) want = kAppendMaxSlices;
    if (want > stages) want = stages;
    if (want < 1) want = 1;
    const int64_t per = (stages + want - 1) / want;                 // stages per slice
    *rows_per_slice = (int)(per * 64);
    *slices = (int)(stages > 0 ? (stages + per - 1) / per : 1);
}

template <int RT>
static void launch_rows_rt(hipStream_t s, const double *V, int64_t ldv, const double *B, int64_t rows, int64_t m_pad,
                           double *part, AppendRowsArgs a)
{
    int slices = 1, rps = 64;
    append_rows_plan(rows, m_pad, &slices, &rps);
    const int64_t rows64 = (rows + 63) / 64 * 64;
    hipLaunchKernelGGL(append_rows_pass_kernel<RT>, dim3((unsigned)(m_pad / 64), (unsigned)slices), dim3(256), 0, s, V, ldv, B,
                       rows64, rps, m_pad, part);
    a.part = part;
    a.slices = slices;
    hipLaunchKernelGGL(append_rows_final_kernel<RT>, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, a);
}

void launch_append_rows(hipStream_t s, const double *V, int64_t ldv, const double *B, int64_t rows, int kp, double *part,
                        const AppendRowsArgs &a)
{
    switch (kp / 16) {
        case 1: launch_rows_rt<1>(s, V, ldv, B, rows, a.m_pad, part, a); break;
        case 2: launch_rows_rt<2>(s, V, ldv, B, rows, a.m_pad, part, a); break;
        case 3: launch_rows_rt<3>(s, V, ldv, B, rows, a.m_pad, part, a); break;
        default: launch_rows_rt<4>(s, V, ldv, B, rows, a.m_pad, part, a); break;
    }
}

}  // namespace cbo

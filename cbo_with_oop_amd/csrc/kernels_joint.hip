// The joint posterior on fp64 MFMA (v_mfma_f64_16x16x4_f64), gfx950: covariance, samples and integrated variance reduction.
//
//     cov_tile_kernel:     C[i][j] = K(X1_i, X2_j) - sum_k V1[k][i] V2[k][j]
//     samples_tile_kernel: F[i][j] = mu[i] + sum_{k <= i} U[k][i] Z[k][j]
//     gram_tile_kernel:    G[i][j] = sum_k A[k][i] A[k][j]  (the do-calculus prior's two Gram products)
//
// with V = L^-1 K(X, .) (the sweep's solution, resident), U^T U = Sigma + jitter I (U[k][i] = L[i][k]), Z = normals^T.
//
// All three run one main loop (tile_mainloop).  One 128 x 128 output tile per 256-thread workgroup, wave (wr, wc) owning
// the 64 x 64 quarter (wr, wc) as 4 x 4 MFMA blocks.  Both operands are k-major rows, which is exactly what the f64
// MFMA reads: A fragment "A[i = lane&15][k = lane>>4]" = A[k][i], B fragment "B[k = lane>>4][j = lane&15]" = B[k][j].
// Stages of 16 rows x 128 columns of each operand go to LDS by LDS-DMA (one 1 KiB row per instruction, double
// buffered: the DMA of stage s+1 is in flight while stage s computes); 73,728 B per workgroup, two workgroups per CU.
// No atomics: every output element is one fixed-order sum, two calls give the same bits.
//
// cov_tile_kernel: GPy PosteriorExact._raw_predict, full_cov branch (Kxx - tdot(tmp.T)), and
// posterior_covariance_between_points (K12 - tmp1.T tmp2).  The K(X1, X2) tile is formed in the epilogue from the
// scaled SoA points and squared norms of the candidate set, in GPy's operation order (kernel_value<D>, cbo_device.h);
// no m x m prior matrix goes through HBM.
// SYM (cbo_gp_predict_cov): X1 = X2, V1 = V2; only tiles on or above the diagonal are launched and every element with
// i <= j is stored at (i, j) and (j, i) from one value, so the output is symmetric bit for bit.  The diagonal takes the
// model's zero-distance rule (GPy RBF.K(X) with X2 = None; the causal kernel passes X2 explicitly and takes none) and
// the likelihood noise.
//
// samples_tile_kernel: GPy GP.posterior_samples_f draws np.random.multivariate_normal(mean, Sigma, size);
// cbo_gp_posterior_samples factors Sigma (cov_tile_kernel into the factorisation's own layout, launch_cholesky) and
// applies the factor here.  Triangle-aware (TRI): row tile I reduces over k < 128 (I + 1) only (m^2 s flop in all, not
// 2 m^2 s), and no tile reads a U block below the diagonal.  Below its diagonal the buffer still holds Sigma's
// mirrored lower half (cov SYM stores both halves, the factorisation leaves them), so the stages of the diagonal block
// mask k > i explicitly.  Tiles are dispatched heaviest row first.
//
// ivr_tile_kernel (cbo_gp_integrated_variance_reduction): the cross covariance of candidates and integration points,
// squared and reduced along each row of the tile in the epilogue; one partial per row and tile leaves the kernel.
//
// Roofline: fp64 MFMA bound at the sizes they are meant for: n_pad m^2 flop for SYM (the upper half of the product),
// 2 n_pad m1 m2 for the cross covariance and for IVR, m^2 s for the samples; per tile and k row 2 KiB of operands
// (mostly from L2) against 64 MFMAs.
#include "cbo_device.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace cbo {

#define TILE_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int kTile = 128;                        // output tile side
static_assert(kTile == kJointTile, "cbo_internal.h names the tile side for the host code");
constexpr int kTileKB = 16;                       // k rows per LDS stage (4 MFMA k-steps)
constexpr int kTileLd = kTile + 16;               // LDS row stride: rows kq and kq+1 land 32 banks apart (ds_read_b64)
constexpr int kTileStage = 2 * kTileKB * kTileLd; // doubles per stage: the A rows, then the B rows
constexpr int kTileDma = 2 * kTileKB / 4;         // LDS-DMA instructions per wave and stage (4 A rows + 4 B rows)

// out = sum over nst stages of 16 k rows of A[k][i] B[k][j], this wave's 64 x 64 quarter of the tile.  ga / gb point at
// the lane's two columns in row 0 of each operand (leading dimensions lda / ldb); wave w moves rows 4w .. 4w+3 of both
// operands of every stage.  lds holds 2 * kTileStage doubles.  TRI: the last 128 / 16 stages are the diagonal block,
// where A[k][i] with k > i is not the factor.
template <bool TRI>
__device__ __forceinline__ void tile_mainloop(const double *ga, int64_t lda, const double *gb, int64_t ldb, int nst,
                                              d4 (&out)[4][4], double *lds)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    ga += (int64_t)(4 * wave) * lda;
    gb += (int64_t)(4 * wave) * ldb;
    const unsigned lds_byte0 = lds_byte_address(lds);
    auto issue = [&](int s, int buf) __attribute__((always_inline)) {
        const unsigned la = __builtin_amdgcn_readfirstlane(lds_byte0 + 8u * (unsigned)(buf * kTileStage + 4 * wave * kTileLd));
        const unsigned lb = la + 8u * (unsigned)(kTileKB * kTileLd);
        const double *pa = ga + (int64_t)s * kTileKB * lda;
        const double *pb = gb + (int64_t)s * kTileKB * ldb;
#pragma unroll
        for (int r = 0; r < 4; ++r) glds16(pa + r * lda, la + 8u * (unsigned)(r * kTileLd));
#pragma unroll
        for (int r = 0; r < 4; ++r) glds16(pb + r * ldb, lb + 8u * (unsigned)(r * kTileLd));
    };

    // accumulated in a local and copied out at the end: summed through the reference, the TRI skip branch leaves hipcc
    // with two copies of the accumulator, and samples_tile_kernel spills
    d4 acc[4][4];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = d4{0.0, 0.0, 0.0, 0.0};

    const int diag0 = nst - kTile / kTileKB;           // TRI: first stage of the diagonal block
    const int row_last = wr * 64 + 63;                 // TRI: last tile row of this wave
    issue(0, 0);
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        // the other buffer was last read in stage s-1, which every wave has left (barrier at the bottom)
        if (s + 1 < nst) {
            issue(s + 1, buf ^ 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kTileDma) : "memory");    // this wave's DMA of stage s landed
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                                          // ... and every other wave's
        const int kl0 = (s - diag0) * kTileKB;     // TRI: first k of the stage relative to i0 (< 0 off the diagonal)
        if (!TRI || kl0 <= row_last) {                     // (a stage wholly below this wave's rows adds nothing)
            const double *as = lds + buf * kTileStage + kq * kTileLd + wr * 64 + lc;
            const double *bs = as - wr * 64 + wc * 64 + kTileKB * kTileLd;
            const bool diag = TRI && kl0 >= 0;
#pragma unroll
            for (int ks = 0; ks < kTileKB / 4; ++ks) {
                double af[4], bf[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    af[q] = as[4 * ks * kTileLd + 16 * q];
                    bf[q] = bs[4 * ks * kTileLd + 16 * q];
                }
                if (diag) {
                    // U[k][i] with k > i lies below the factor's diagonal: Sigma's mirror, not the factor (k - i of
                    // block 0 against 16 q, the row offset of block q: fewer registers than k against i)
                    const int kmi = kl0 + 4 * ks + kq - wr * 64 - lc;
#pragma unroll
                    for (int q = 0; q < 4; ++q) af[q] = kmi > 16 * q ? 0.0 : af[q];
                }
#pragma unroll
                for (int bi = 0; bi < 4; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = TILE_MFMA(af[bi], bf[bj], acc[bi][bj]);
            }
        }
        __builtin_amdgcn_s_barrier();
    }
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) out[bi][bj] = acc[bi][bj];
}

template <int D, bool SYM>
__global__ __launch_bounds__(256, 2) void cov_tile_kernel(CovArgs a)
{
    int ti = blockIdx.y, tj = blockIdx.x;
    if (SYM) {
        // the nt (nt + 1) / 2 tiles on and above the diagonal, row by row (row ti starts at ti nt - ti (ti - 1) / 2)
        const int nt = a.tiles;
        const int t = blockIdx.x;
        ti = (int)((2.0 * nt + 1.0 - sqrt((2.0 * nt + 1.0) * (2.0 * nt + 1.0) - 8.0 * (double)t)) * 0.5);
        while (ti > 0 && ti * nt - ti * (ti - 1) / 2 > t) --ti;               // guard the rounding of the root
        while ((ti + 1) * nt - (ti + 1) * ti / 2 <= t) ++ti;
        tj = ti + (t - (ti * nt - ti * (ti - 1) / 2));
    }
    __shared__ __align__(16) double lds[2 * kTileStage];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)ti * kTile, j0 = (int64_t)tj * kTile;

    // Columns past the allocation's readable width are clamped onto its last pair: they only feed outputs that are not
    // stored.
    int64_t ca = a.a_off + i0 + 2 * lane, cb = a.b_off + j0 + 2 * lane;
    ca = ca < a.v_cols - 2 ? ca : a.v_cols - 2;
    cb = cb < a.v_cols - 2 ? cb : a.v_cols - 2;
    d4 acc[4][4];
    tile_mainloop<false>(a.V + ca, a.ldv, a.V + cb, a.ldv, a.n_k / kTileKB, acc, lds);

    // epilogue: the tile's points to LDS (the stage buffers are free), then K - acc element by element
    double *px1 = lds, *px2 = lds + D * kTile;
    double *q1 = lds + 2 * D * kTile, *q2 = q1 + kTile, *v1 = q2 + kTile, *v2 = v1 + kTile;
    const bool causal = a.sv1 != nullptr;
    if (tid < kTile) {
        const int64_t gi = i0 + tid;
        const bool in = gi < a.m1;
#pragma unroll
        for (int k = 0; k < D; ++k) px1[k * kTile + tid] = in ? a.xs1[(int64_t)k * a.ldx + gi] : 0.0;
        q1[tid] = in ? a.sq1[gi] : 0.0;
        v1[tid] = (in && causal) ? a.sv1[gi] : 0.0;
    } else {
        const int t = tid - kTile;
        const int64_t gj = j0 + t;
        const bool in = gj < a.m2;
#pragma unroll
        for (int k = 0; k < D; ++k) px2[k * kTile + t] = in ? a.xs2[(int64_t)k * a.ldx + gj] : 0.0;
        q2[t] = in ? a.sq2[gj] : 0.0;
        v2[t] = (in && causal) ? a.sv2[gj] : 0.0;
    }
    __syncthreads();

#pragma unroll
    for (int bj = 0; bj < 4; ++bj) {
        const int lj = wc * 64 + bj * 16 + lc;
        const int64_t gj = j0 + lj;
        double xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = px2[k * kTile + lj];
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = wr * 64 + bi * 16 + kq + 4 * r;
                const int64_t gi = i0 + li;
                if (gi >= a.m1 || gj >= a.m2) continue;
                if (SYM && gi > gj) continue;                   // stored by the element (gj, gi) as its mirror
                double xi[D];
#pragma unroll
                for (int k = 0; k < D; ++k) xi[k] = px1[k * kTile + li];
                double kv = kernel_value<D>(xi, xj, q1[li], q2[lj], a.variance, a.inv_l2, SYM && a.zero_diag && gi == gj);
                if (causal) kv = __dadd_rn(kv, __dmul_rn(v1[li], v2[lj]));
                double c = __dsub_rn(kv, acc[bi][bj][r]);
                if (SYM && gi == gj) c = __dadd_rn(c, a.noise);
                a.C[gi * a.ldc + gj] = c;
                if (SYM && gi != gj) a.C[gj * a.ldc + gi] = c;
            }
    }
}

// ivr_tile_kernel: emukit IntegratedVarianceReduction, mean_j cov(x_i, x_j)^2 / var(x_i) over the integration points,
// without the m x p covariance: the cross element of cov_tile_kernel (same main loop, same epilogue operations), squared
// and summed over the tile's columns j < p.  Each row's 128 squares go in a fixed order: over bj in the lane, a
// butterfly over the 16 lanes of a row (every lane ends with the same value: a + b == b + a), then the wc = 0 half plus
// the wc = 1 half through LDS.  One partial per (candidate, global tile column); no atomics.
template <int D>
__global__ __launch_bounds__(256, 2) void ivr_tile_kernel(IvrArgs a)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    __shared__ __align__(16) double lds[2 * kTileStage];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)ti * kTile, j0 = (int64_t)tj * kTile;

    // columns past what was solved are clamped onto its last pair: they only feed rows >= m and columns >= p
    int64_t ca = i0 + 2 * lane, cb = j0 + 2 * lane;
    ca = ca < a.c_cols - 2 ? ca : a.c_cols - 2;
    cb = cb < a.i_cols - 2 ? cb : a.i_cols - 2;
    d4 acc[4][4];
    tile_mainloop<false>(a.Vc + ca, a.ldv, a.Vi + cb, a.ldv, a.n_k / kTileKB, acc, lds);

    // epilogue: the tile's points to LDS as in cov_tile_kernel, then (K - acc)^2 summed along the rows
    double *px1 = lds, *px2 = lds + D * kTile;
    double *q1 = lds + 2 * D * kTile, *q2 = q1 + kTile, *v1 = q2 + kTile, *v2 = v1 + kTile;
    double *red = v2 + kTile;                            // [2][kTile]: the row sums of the two column halves
    const bool causal = a.sv1 != nullptr;
    if (tid < kTile) {
        const int64_t gi = i0 + tid;
        const bool in = gi < a.m;
#pragma unroll
        for (int k = 0; k < D; ++k) px1[k * kTile + tid] = in ? a.xs1[(int64_t)k * a.ldx + gi] : 0.0;
        q1[tid] = in ? a.sq1[gi] : 0.0;
        v1[tid] = (in && causal) ? a.sv1[gi] : 0.0;
    } else {
        const int t = tid - kTile;
        const int64_t gj = j0 + t;
        const bool in = gj < a.p;
#pragma unroll
        for (int k = 0; k < D; ++k) px2[k * kTile + t] = in ? a.xs2[(int64_t)k * a.ldx + gj] : 0.0;
        q2[t] = in ? a.sq2[gj] : 0.0;
        v2[t] = (in && causal) ? a.sv2[gj] : 0.0;
    }
    __syncthreads();

    // row by row: the four elements of a row in this lane (bj order), the 16 lanes of the row, the half to LDS
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = wr * 64 + bi * 16 + kq + 4 * r;
            double xi[D];
#pragma unroll
            for (int k = 0; k < D; ++k) xi[k] = px1[k * kTile + li];
            double s = 0.0;
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                const int lj = wc * 64 + bj * 16 + lc;
                double xj[D];
#pragma unroll
                for (int k = 0; k < D; ++k) xj[k] = px2[k * kTile + lj];
                double kv = kernel_value<D>(xi, xj, q1[li], q2[lj], a.variance, a.inv_l2, false);
                if (causal) kv = __dadd_rn(kv, __dmul_rn(v1[li], v2[lj]));
                const double c = __dsub_rn(kv, acc[bi][bj][r]);
                // (a select, not a product: a column past p may hold anything, NaN included)
                s = __dadd_rn(s, j0 + lj < a.p ? __dmul_rn(c, c) : 0.0);
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) s = __dadd_rn(s, __shfl_xor(s, off));
            if (lc == 0) red[wc * kTile + li] = s;
        }
    __syncthreads();
    if (tid < kTile) {
        const int64_t gi = i0 + tid;
        if (gi < a.m) a.part[gi * a.ldp + a.tile0 + tj] = __dadd_rn(red[tid], red[kTile + tid]);
    }
}

// gram_tile_kernel (cbo_do_prior_create): G = A^T A of one k-major operand on the same main loop, both for
// Ky^-1 = W^T W (W = L^-1) and for b^T b; with `prev` the epilogue forms the element-wise product of the two,
// (prev[i][j] (G[i][j] / divisor)) scale, in place.  Element (i, j) and element (j, i) are the same products summed in the
// same order: the result is symmetric to the bit.
__global__ __launch_bounds__(256, 2) void gram_tile_kernel(GramArgs a)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    __shared__ __align__(16) double lds[2 * kTileStage];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)ti * kTile, j0 = (int64_t)tj * kTile;

    d4 acc[4][4];
    tile_mainloop<false>(a.A + i0 + 2 * lane, a.lda, a.A + j0 + 2 * lane, a.lda, a.n_k / kTileKB, acc, lds);

#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = i0 + wr * 64 + bi * 16 + kq + 4 * r;
            if (gi >= a.n) continue;
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                const int64_t gj = j0 + wc * 64 + bj * 16 + lc;
                if (gj >= a.n) continue;
                double v = acc[bi][bj][r];
                if (a.prev) v = __dmul_rn(__dmul_rn(a.prev[gi * a.ldo + gj], __ddiv_rn(v, a.divisor)), a.scale);
                a.out[gi * a.ldo + gj] = v;
            }
        }
}

__global__ __launch_bounds__(256, 2) void samples_tile_kernel(SampArgs a)
{
    const int t = blockIdx.x;
    const int ti = a.tiles_i - 1 - t / a.tiles_j, tj = t % a.tiles_j;
    __shared__ __align__(16) double lds[2 * kTileStage];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)ti * kTile, j0 = (int64_t)tj * kTile;

    // U has >= m_pad columns, Z >= s_pad; row tile ti reduces over k < i0 + 128
    d4 acc[4][4];
    tile_mainloop<true>(a.U + i0 + 2 * lane, a.ldu, a.Z + j0 + 2 * lane, a.ldz, (ti + 1) * (kTile / kTileKB), acc, lds);

    // epilogue: the mean on every row; rows >= m and columns >= s are not stored
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = i0 + wr * 64 + bi * 16 + kq + 4 * r;
            if (gi >= a.m) continue;
            const double mu = a.mean[gi];
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                const int64_t gj = j0 + wc * 64 + bj * 16 + lc;
                if (gj < a.s) a.F[gi * a.ldf + gj] = __dadd_rn(mu, acc[bi][bj][r]);
            }
        }
}

// Z[k][j] = normals[j][k] for k < m, j < s; zero elsewhere in [m_pad][ldz] (32 x 32 tiles through LDS)
__global__ __launch_bounds__(256) void normals_transpose_kernel(const double *normals, int64_t m, int64_t s, double *Z,
                                                                int64_t ldz)
{
    __shared__ double tile[32][33];
    const int64_t k0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
#pragma unroll
    for (int r = 0; r < 32; r += 8) {
        const int64_t j = j0 + ty + r, k = k0 + tx;
        tile[ty + r][tx] = (j < s && k < m) ? normals[j * m + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 32; r += 8) {
        const int64_t k = k0 + ty + r, j = j0 + tx;
        if (j < ldz) Z[k * ldz + j] = tile[tx][ty + r];
    }
}

// the factor buffer's padding: identity on rows >= m, zero on columns >= m of rows < m (right-hand-side strip included)
__global__ __launch_bounds__(256) void factor_padding_kernel(double *A, int64_t lda, int64_t m, int64_t m_pad)
{
    const int64_t upper = m * (lda - m);                    // rows < m, columns [m, lda)
    const int64_t total = upper + (m_pad - m) * lda;        // then rows [m, m_pad), every column
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t i, j;
        if (e < upper) {
            i = e / (lda - m);
            j = m + e % (lda - m);
        } else {
            i = m + (e - upper) / lda;
            j = (e - upper) % lda;
        }
        A[i * lda + j] = i == j ? 1.0 : 0.0;
    }
}

template <bool SYM>
static void launch_cov_d(hipStream_t s, int d, const CovArgs &a, dim3 grid)
{
    CBO_FOR_DIM(d, hipLaunchKernelGGL((cov_tile_kernel<D, SYM>), grid, dim3(256), 0, s, a));
}

void launch_cov_tiles(hipStream_t s, int d, bool sym, CovArgs a)
{
    const int64_t t1 = (a.m1 + kTile - 1) / kTile, t2 = (a.m2 + kTile - 1) / kTile;
    a.n_k = (int)round_up(a.n_k, kTileKB);
    if (sym) {
        a.tiles = (int)t1;
        launch_cov_d<true>(s, d, a, dim3((unsigned)(t1 * (t1 + 1) / 2)));
    } else {
        a.tiles = 0;
        launch_cov_d<false>(s, d, a, dim3((unsigned)t2, (unsigned)t1));
    }
}

void launch_ivr_tiles(hipStream_t s, int d, IvrArgs a)
{
    const dim3 grid((unsigned)((a.p + kTile - 1) / kTile), (unsigned)((a.m + kTile - 1) / kTile));
    a.n_k = (int)round_up(a.n_k, kTileKB);
    CBO_FOR_DIM(d, hipLaunchKernelGGL(ivr_tile_kernel<D>, grid, dim3(256), 0, s, a));
}

void launch_gram_tiles(hipStream_t s, GramArgs a)
{
    const unsigned nt = (unsigned)((a.n + kTile - 1) / kTile);
    a.n_k = (int)round_up(a.n_k, kTileKB);
    hipLaunchKernelGGL(gram_tile_kernel, dim3(nt, nt), dim3(256), 0, s, a);
}

void launch_samples_tiles(hipStream_t st, SampArgs a)
{
    a.tiles_i = (int)((a.m + kTile - 1) / kTile);
    a.tiles_j = (int)((a.s + kTile - 1) / kTile);
    hipLaunchKernelGGL(samples_tile_kernel, dim3((unsigned)(a.tiles_i * a.tiles_j)), dim3(256), 0, st, a);
}

void launch_normals_transpose(hipStream_t st, const double *normals, int64_t m, int64_t s, double *Z, int64_t m_pad,
                              int64_t ldz)
{
    hipLaunchKernelGGL(normals_transpose_kernel, dim3((unsigned)((ldz + 31) / 32), (unsigned)(m_pad / 32)), dim3(256), 0,
                       st, normals, m, s, Z, ldz);
}

void launch_factor_padding(hipStream_t st, double *A, int64_t lda, int64_t m, int64_t m_pad)
{
    const int64_t total = m * (lda - m) + (m_pad - m) * lda;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(factor_padding_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, lda, m, m_pad);
}

}  // namespace cbo

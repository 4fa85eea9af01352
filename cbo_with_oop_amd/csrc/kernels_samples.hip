// Joint posterior samples on fp64 MFMA (v_mfma_f64_16x16x4_f64), gfx950:
//
//     F[i][j] = mu[i] + sum_{k <= i} U[k][i] Z[k][j],      U^T U = Sigma + jitter I (U[k][i] = L[i][k]), Z = normals^T
//
// GPy GP.posterior_samples_f draws np.random.multivariate_normal(mean, Sigma, size); cbo_gp_posterior_samples factors
// Sigma (cov_tile_kernel into the factorisation's own layout, launch_cholesky) and applies the factor here.  The operand
// shape is cov_tile_kernel's: U and Z are both read as k-major rows, A fragment "A[i = lane&15][k = lane>>4]" = U[k][i],
// B fragment "B[k = lane>>4][j = lane&15]" = Z[k][j].  One 128 x 128 output tile per 256-thread workgroup, wave (wr, wc)
// owning the 64 x 64 quarter (wr, wc) as 4 x 4 MFMA blocks; stages of 16 rows x 128 columns of each operand go to LDS by
// LDS-DMA, double buffered; 73,728 B per workgroup, two workgroups per CU.
//
// Triangle-aware: row tile I reduces over k < 128 (I + 1) only (m^2 s flop in all, not 2 m^2 s), and no tile reads a U
// block below the diagonal.  Below its diagonal the buffer still holds Sigma's mirrored lower half (cov SYM stores both
// halves, the factorisation leaves them), so the stages of the diagonal block mask k > i explicitly.  Tiles are
// dispatched heaviest row first.  No atomics: every element is one fixed-order sum, two calls give the same bits.
#include "cbo_device.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace cbo {

#define SAMP_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int kSampT = 128;                       // output tile side
constexpr int kSampKB = 16;                       // k rows per LDS stage (4 MFMA k-steps)
constexpr int kSampLd = kSampT + 16;              // LDS row stride (as kernels_cov.hip)
constexpr int kSampStage = 2 * kSampKB * kSampLd; // doubles per stage: the U rows, then the Z rows
constexpr int kSampDma = 2 * kSampKB / 4;         // LDS-DMA instructions per wave and stage

__global__ __launch_bounds__(256, 2) void samples_tile_kernel(SampArgs a)
{
    const int t = blockIdx.x;
    const int ti = a.tiles_i - 1 - t / a.tiles_j, tj = t % a.tiles_j;
    __shared__ __align__(16) double lds[2 * kSampStage];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)ti * kSampT, j0 = (int64_t)tj * kSampT;

    // wave w moves rows 4w .. 4w+3 of both operands of every stage (U has >= m_pad columns, Z >= s_pad)
    const double *ga = a.U + (int64_t)(4 * wave) * a.ldu + i0 + 2 * lane;
    const double *gb = a.Z + (int64_t)(4 * wave) * a.ldz + j0 + 2 * lane;
    const unsigned lds_byte0 = lds_byte_address(lds);
    auto issue = [&](int s, int buf) __attribute__((always_inline)) {
        const unsigned la = __builtin_amdgcn_readfirstlane(lds_byte0 + 8u * (unsigned)(buf * kSampStage + 4 * wave * kSampLd));
        const unsigned lb = la + 8u * (unsigned)(kSampKB * kSampLd);
        const double *pa = ga + (int64_t)s * kSampKB * a.ldu;
        const double *pb = gb + (int64_t)s * kSampKB * a.ldz;
#pragma unroll
        for (int r = 0; r < 4; ++r) glds16(pa + r * a.ldu, la + 8u * (unsigned)(r * kSampLd));
#pragma unroll
        for (int r = 0; r < 4; ++r) glds16(pb + r * a.ldz, lb + 8u * (unsigned)(r * kSampLd));
    };

    d4 acc[4][4];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = d4{0.0, 0.0, 0.0, 0.0};

    const int nst = (ti + 1) * (kSampT / kSampKB);     // k < i0 + 128
    const int diag0 = ti * (kSampT / kSampKB);         // first stage of the diagonal block
    const int row_last = wr * 64 + 63;                 // last tile row of this wave
    issue(0, 0);
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        // the other buffer was last read in stage s-1, which every wave has left (barrier at the bottom)
        if (s + 1 < nst) {
            issue(s + 1, buf ^ 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kSampDma) : "memory");   // this wave's DMA of stage s landed
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                                          // ... and every other wave's
        const int kl0 = (s - diag0) * kSampKB;             // first k of the stage relative to i0 (< 0 off the diagonal)
        if (kl0 <= row_last) {                             // (a stage wholly below this wave's rows adds nothing)
            const double *as = lds + buf * kSampStage + kq * kSampLd + wr * 64 + lc;
            const double *bs = as - wr * 64 + wc * 64 + kSampKB * kSampLd;
            const bool diag = kl0 >= 0;
#pragma unroll
            for (int ks = 0; ks < kSampKB / 4; ++ks) {
                double af[4], bf[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    af[q] = as[4 * ks * kSampLd + 16 * q];
                    bf[q] = bs[4 * ks * kSampLd + 16 * q];
                }
                if (diag) {
                    // U[k][i] with k > i lies below the factor's diagonal: Sigma's mirror, not the factor
                    const int kl = kl0 + 4 * ks + kq;
#pragma unroll
                    for (int q = 0; q < 4; ++q) af[q] = kl > wr * 64 + 16 * q + lc ? 0.0 : af[q];
                }
#pragma unroll
                for (int bi = 0; bi < 4; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = SAMP_MFMA(af[bi], bf[bj], acc[bi][bj]);
            }
        }
        __builtin_amdgcn_s_barrier();
    }

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

void launch_samples_tiles(hipStream_t st, SampArgs a)
{
    a.tiles_i = (int)((a.m + kSampT - 1) / kSampT);
    a.tiles_j = (int)((a.s + kSampT - 1) / kSampT);
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

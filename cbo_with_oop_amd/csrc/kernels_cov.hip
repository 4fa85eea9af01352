// Joint posterior covariance on fp64 MFMA (v_mfma_f64_16x16x4_f64), gfx950:
//
//     C[i][j] = K(X1_i, X2_j) - sum_k V1[k][i] V2[k][j],      V = L^-1 K(X, .) (the sweep's solution, resident)
//
// GPy PosteriorExact._raw_predict, full_cov branch (Kxx - tdot(tmp.T)), and posterior_covariance_between_points
// (K12 - tmp1.T tmp2).  One 128 x 128 output tile per 256-thread workgroup, wave (wr, wc) owning the 64 x 64 quarter
// (wr, wc) as 4 x 4 MFMA blocks.  Both operands are k-major rows of the V workspace, which is exactly what the f64 MFMA
// reads: A fragment "A[i = lane&15][k = lane>>4]" = V1[k][i], B fragment "B[k = lane>>4][j = lane&15]" = V2[k][j].
// Stages of 16 V rows x 128 columns of each operand go to LDS by LDS-DMA (one 1 KiB row per instruction, double
// buffered: the DMA of stage s+1 is in flight while stage s computes); 73,728 B per workgroup, two workgroups per CU.
// The K(X1, X2) tile is formed in the epilogue from the scaled SoA points and squared norms of the candidate set, in
// GPy's operation order (kernel_value<D>, cbo_device.h); no m x m prior matrix goes through HBM.
//
// SYM (cbo_gp_predict_cov): X1 = X2, V1 = V2; only tiles on or above the diagonal are launched and every element with
// i <= j is stored at (i, j) and (j, i) from one value, so the output is symmetric bit for bit.  The diagonal takes the
// model's zero-distance rule (GPy RBF.K(X) with X2 = None; the causal kernel passes X2 explicitly and takes none) and
// the likelihood noise.  No atomics: every output element is one fixed-order sum, two calls give the same bits.
//
// Roofline: fp64 MFMA bound at the sizes it is meant for: n_pad m^2 flop for SYM (the upper half of the product),
// 2 n_pad m1 m2 otherwise; per tile and V row 2 KiB of operands (mostly from L2) against 64 MFMAs.
#include "cbo_device.h"

#pragma clang fp contract(off)

namespace cbo {

#define COV_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int kCovT = 128;                    // output tile side
constexpr int kCovKB = 16;                    // V rows per LDS stage (4 MFMA k-steps)
constexpr int kCovLd = kCovT + 16;            // LDS row stride: rows kq and kq+1 land 32 banks apart (ds_read_b64)
constexpr int kCovStage = 2 * kCovKB * kCovLd;   // doubles per stage: the A rows, then the B rows
constexpr int kCovDma = 2 * kCovKB / 4;          // LDS-DMA instructions per wave and stage (4 A rows + 4 B rows)

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
    __shared__ __align__(16) double lds[2 * kCovStage];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lc = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)ti * kCovT, j0 = (int64_t)tj * kCovT;

    // wave w moves rows 4w .. 4w+3 of both operands of every stage.  Columns past the allocation's readable width are
    // clamped onto its last pair: they only feed outputs that are not stored.
    int64_t ca = a.a_off + i0 + 2 * lane, cb = a.b_off + j0 + 2 * lane;
    ca = ca < a.v_cols - 2 ? ca : a.v_cols - 2;
    cb = cb < a.v_cols - 2 ? cb : a.v_cols - 2;
    const double *ga = a.V + (int64_t)(4 * wave) * a.ldv + ca;
    const double *gb = a.V + (int64_t)(4 * wave) * a.ldv + cb;
    const unsigned lds_byte0 = lds_byte_address(lds);
    auto issue = [&](int s, int buf) __attribute__((always_inline)) {
        const int64_t roff = (int64_t)s * kCovKB * a.ldv;
        const unsigned la = __builtin_amdgcn_readfirstlane(lds_byte0 + 8u * (unsigned)(buf * kCovStage + 4 * wave * kCovLd));
        const unsigned lb = la + 8u * (unsigned)(kCovKB * kCovLd);
#pragma unroll
        for (int r = 0; r < 4; ++r) glds16(ga + roff + r * a.ldv, la + 8u * (unsigned)(r * kCovLd));
#pragma unroll
        for (int r = 0; r < 4; ++r) glds16(gb + roff + r * a.ldv, lb + 8u * (unsigned)(r * kCovLd));
    };

    d4 acc[4][4];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = d4{0.0, 0.0, 0.0, 0.0};

    const int nst = a.n_k / kCovKB;
    issue(0, 0);
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        // the other buffer was last read in stage s-1, which every wave has left (barrier at the bottom)
        if (s + 1 < nst) {
            issue(s + 1, buf ^ 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kCovDma) : "memory");     // this wave's DMA of stage s landed
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                                          // ... and every other wave's
        const double *as = lds + buf * kCovStage + kq * kCovLd + wr * 64 + lc;
        const double *bs = as - wr * 64 + wc * 64 + kCovKB * kCovLd;
#pragma unroll
        for (int ks = 0; ks < kCovKB / 4; ++ks) {
            double af[4], bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = as[4 * ks * kCovLd + 16 * t];
                bf[t] = bs[4 * ks * kCovLd + 16 * t];
            }
#pragma unroll
            for (int bi = 0; bi < 4; ++bi)
#pragma unroll
                for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = COV_MFMA(af[bi], bf[bj], acc[bi][bj]);
        }
        __builtin_amdgcn_s_barrier();
    }

    // epilogue: the tile's points to LDS (the stage buffers are free), then K - acc element by element
    double *px1 = lds, *px2 = lds + D * kCovT;
    double *q1 = lds + 2 * D * kCovT, *q2 = q1 + kCovT, *v1 = q2 + kCovT, *v2 = v1 + kCovT;
    const bool causal = a.sv1 != nullptr;
    if (tid < kCovT) {
        const int64_t gi = i0 + tid;
        const bool in = gi < a.m1;
#pragma unroll
        for (int k = 0; k < D; ++k) px1[k * kCovT + tid] = in ? a.xs1[(int64_t)k * a.ldx + gi] : 0.0;
        q1[tid] = in ? a.sq1[gi] : 0.0;
        v1[tid] = (in && causal) ? a.sv1[gi] : 0.0;
    } else {
        const int t = tid - kCovT;
        const int64_t gj = j0 + t;
        const bool in = gj < a.m2;
#pragma unroll
        for (int k = 0; k < D; ++k) px2[k * kCovT + t] = in ? a.xs2[(int64_t)k * a.ldx + gj] : 0.0;
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
        for (int k = 0; k < D; ++k) xj[k] = px2[k * kCovT + lj];
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
                for (int k = 0; k < D; ++k) xi[k] = px1[k * kCovT + li];
                double kv = kernel_value<D>(xi, xj, q1[li], q2[lj], a.variance, a.inv_l2, SYM && a.zero_diag && gi == gj);
                if (causal) kv = __dadd_rn(kv, __dmul_rn(v1[li], v2[lj]));
                double c = __dsub_rn(kv, acc[bi][bj][r]);
                if (SYM && gi == gj) c = __dadd_rn(c, a.noise);
                a.C[gi * a.ldc + gj] = c;
                if (SYM && gi != gj) a.C[gj * a.ldc + gi] = c;
            }
    }
}

template <bool SYM>
static void launch_cov_d(hipStream_t s, int d, const CovArgs &a, dim3 grid)
{
    switch (d) {
        case 1: hipLaunchKernelGGL((cov_tile_kernel<1, SYM>), grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL((cov_tile_kernel<2, SYM>), grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL((cov_tile_kernel<3, SYM>), grid, dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL((cov_tile_kernel<4, SYM>), grid, dim3(256), 0, s, a); break;
        case 5: hipLaunchKernelGGL((cov_tile_kernel<5, SYM>), grid, dim3(256), 0, s, a); break;
        case 6: hipLaunchKernelGGL((cov_tile_kernel<6, SYM>), grid, dim3(256), 0, s, a); break;
        case 7: hipLaunchKernelGGL((cov_tile_kernel<7, SYM>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((cov_tile_kernel<8, SYM>), grid, dim3(256), 0, s, a); break;
    }
}

void launch_cov_tiles(hipStream_t s, int d, bool sym, CovArgs a)
{
    const int64_t t1 = (a.m1 + kCovT - 1) / kCovT, t2 = (a.m2 + kCovT - 1) / kCovT;
    a.n_k = (int)round_up(a.n_k, kCovKB);
    if (sym) {
        a.tiles = (int)t1;
        launch_cov_d<true>(s, d, a, dim3((unsigned)(t1 * (t1 + 1) / 2)));
    } else {
        a.tiles = 0;
        launch_cov_d<false>(s, d, a, dim3((unsigned)t2, (unsigned)t1));
    }
}

}  // namespace cbo

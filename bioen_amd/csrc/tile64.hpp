// 64 x 64 tile algebra of the dense factorisation and inversion kernels (kernels_forces_newton.hip,
// kernels_forces_laplace.hip): the staged tile product on v_mfma_f64_16x16x4_f64.  Blocks of 256 threads;
// every index is held against m.
#pragma once

#include "device_utils.hpp"

namespace bioen {

constexpr int kT64 = kFNewtonPanel;     // a tile's rows and columns: the factorisation's panel

// The operands pass through LDS in two halves of 32 inner columns, [64][33] each.  A and B operand of the instruction:
// row = lane & 15, k = lane >> 4; result register r of lane 16 q + c: row 4 r + q, column c (the layouts of k_forces_gram).

// 32 inner columns (half = 0, 1) of a 64 x 64 operand tile into dst[row][inner].  ROWS: element (r, k) of the tile is
// X[r0 + r][k0 + k] (a wave-load is two runs of 256 bytes); else it is X[k0 + k][r0 + r], the tile of X^T (one run of 512).
// The 16 loads of a thread travel together (a fixed count, unrolled).
template <bool ROWS>
__device__ __forceinline__ void t64_stage(double (*dst)[33], const double* X, int ld, int m, int r0, int k0, int half) {
#pragma unroll
    for (int it = 0; it < kT64 * 32 / 256; ++it) {
        const int e = threadIdx.x + 256 * it;
        const int r = ROWS ? e >> 5 : e & 63, k = ROWS ? e & 31 : e >> 6;
        const int gr = r0 + r, gk = k0 + 32 * half + k;
        dst[r][k] = (gr < m && gk < m) ? X[ROWS ? (size_t)gr * ld + gk : (size_t)gk * ld + gr] : 0.0;
    }
}

// acc += the 32 inner columns staged: wave w the tile's rows 16 w .. 16 w + 15 against its four column blocks
__device__ __forceinline__ void t64_mfma(d4 acc[4], const double (*as)[33], const double (*bs)[33], int wave, int lq, int lr) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const double av = as[16 * wave + lr][4 * s + lq];
#pragma unroll
        for (int gb = 0; gb < 4; ++gb) acc[gb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bs[16 * gb + lr][4 * s + lq], acc[gb], 0, 0, 0);
    }
}

// acc[r][c] += sum_k a(r, k) b(c, k) over one 64 x 64 x 64 tile product, inner index ascending
template <bool AROWS, bool BROWS>
__device__ __forceinline__ void t64_tile(d4 acc[4], double (*as)[33], double (*bs)[33], const double* A, int lda, int ar0, int ak0,
                                         const double* B, int ldb, int br0, int bk0, int m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int half = 0; half < 2; ++half) {
        __syncthreads();                                     // the product before has read its operands
        t64_stage<AROWS>(as, A, lda, m, ar0, ak0, half);
        t64_stage<BROWS>(bs, B, ldb, m, br0, bk0, half);
        __syncthreads();
        t64_mfma(acc, as, bs, wave, lane >> 4, lane & 15);
    }
}

}  // namespace bioen

// Forces method, M <= 1024: from the resident Cholesky factor H = L L^T (kernels_forces_newton.hip) to the Laplace error
// bars, without leaving the device (gfx950).  With W = L^-1:
//   H^-1 = W^T W,        C H^-1 C = B^T B,  B = W C        (C symmetric)
// Both covariances are X^T X: symmetric and positive semidefinite by construction; a tile and its mirror are stored from
// the same registers, so both are bitwise symmetric.  64 x 64 tiles, T = ceil(m / 64) <= 16:
//   k_flaplace_tinv        one wave per diagonal tile: D_i = L_ii^-1, lane c owns column c, 64 steps of forward substitution
//                          in registers, L_ii read from LDS at wave-uniform addresses; also hands out diag(L)
//   k_flaplace_trtri       one launch per tile distance d = i - j: W_ij = -D_i sum_{k = j}^{i - 1} L_ik W_kj
//   k_flaplace_ata         S = X^T X on the lower tile triangle, mirrored on store; row tiles k >= i for a lower triangular X
//   k_flaplace_trmm        B = W C, tile (i, j) sums over k <= i
//   k_flaplace_to_colquad  H^-1 as k_forces_colquad takes its P_eff (padded to the strip rows, scaled by s_i s_j), and the
//                          diagonals of both covariances
// Every tile product is tile64.hpp's (v_mfma_f64_16x16x4_f64; k_fnewton_syrk runs the same one).  No cooperative
// launch, no grid-wide wait, no atomics: every element has one writer per launch, and every sum runs over the tiles and
// their inner index in ascending order -- its shape is a function of m alone, so the same bits in give the same bits out.
// Every index is held against m: rows and columns m .. of a padded buffer are never read as data (they enter as zeros).
#include "tile64.hpp"

namespace bioen {

// The diagonal tile at k0 = 64 blockIdx.x (nb = min(64, m - k0) rows): lane c owns column c of X = L11^-1, X L11^T = I
// column by column as k_fnewton_trsm solves its rows (the unit matrix's rows for the panel's).  Rows and columns >= nb
// are the identity's.  One reciprocal per pivot.  ldiag <- the diagonal of L.
__global__ __launch_bounds__(64) void k_flaplace_tinv(const double* __restrict__ L, int ldl, int m, double* __restrict__ W, int ldw,
                                                     double* __restrict__ ldiag) {
    __shared__ double dinv[kT64];
    __shared__ double tt[kT64][kT64 + 2];                      // L11 transposed: tt[j][t] = L11[t][j]
    const int k0 = blockIdx.x * kT64;
    const int nb = min(kT64, m - k0);
    const int c = threadIdx.x;
    for (int r = 0; r < kT64; ++r)                            // row r of the tile, one element per lane
        tt[c][r] = (r < nb && c <= r) ? L[(size_t)(k0 + r) * ldl + k0 + c] : (r == c ? 1.0 : 0.0);
    __syncthreads();
    const double dgc = tt[c][c];
    dinv[c] = 1.0 / dgc;
    if (c < nb) ldiag[k0 + c] = dgc;
    __syncthreads();
    double a[kT64];
#pragma unroll
    for (int t = 0; t < kT64; ++t) a[t] = t == c ? 1.0 : 0.0;
    int z = 0;
#pragma unroll
    for (int j = 0; j < kT64; ++j) {
        const double x = a[j] * dinv[j];
        a[j] = x;
        // (as in k_fnewton_trsm: the column's address passes through a register the compiler cannot see through, or it
        // reads all 2016 entries ahead of the first product and spills them)
        asm volatile("" : "+v"(z) : "v"(x));
        const double* const col = &tt[j][0] + z;
#pragma unroll
        for (int t = j + 1; t < kT64; ++t) a[t] = fma(-x, col[t], a[t]);
    }
#pragma unroll
    for (int t = 0; t < kT64; ++t)
        if (t < nb && c < nb) W[(size_t)(k0 + t) * ldw + k0 + c] = a[t];      // a[t] = X[t][c]: zero above the diagonal
}

// The tiles of distance d below the diagonal, block b the tile (i, j) = (b + d, b):  W_ij = -D_i (sum_{k=j}^{i-1} L_ik W_kj),
// D_i = W_ii.  The W_kj are of distances 0 .. d - 1: written by the launches before.  The sum leaves the registers through
// LDS as the second product's B operand, half by half.
__global__ __launch_bounds__(256) void k_flaplace_trtri(const double* __restrict__ L, int ldl, double* W, int ldw, int m, int d) {
    __shared__ double as[kT64][33], bs[kT64][33];
    const int tj = blockIdx.x, ti = tj + d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    d4 acc[4], out[4];
#pragma unroll
    for (int gb = 0; gb < 4; ++gb) acc[gb] = out[gb] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k = tj; k < ti; ++k) t64_tile<true, false>(acc, as, bs, L, ldl, ti * kT64, k * kT64, W, ldw, tj * kT64, k * kT64, m);
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        t64_stage<true>(as, W, ldw, m, ti * kT64, ti * kT64, half);
        if ((wave >> 1) == half) {                           // the sum's rows 32 half .. 32 half + 31 are these two waves'
#pragma unroll
            for (int gb = 0; gb < 4; ++gb)
#pragma unroll
                for (int r = 0; r < 4; ++r) bs[16 * gb + lr][16 * (wave & 1) + 4 * r + lq] = acc[gb][r];
        }
        __syncthreads();
        t64_mfma(out, as, bs, wave, lq, lr);
    }
#pragma unroll
    for (int gb = 0; gb < 4; ++gb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * kT64 + 16 * wave + 4 * r + lq, j = tj * kT64 + 16 * gb + lr;
            if (i < m && j < m) W[(size_t)i * ldw + j] = -out[gb][r];
        }
}

// S = X^T X (m x m, leading dimension lds), block b the tile pair (ti, tj), tj <= ti, over the row tiles k = (lower ? ti :
// 0) .. T - 1 in order: a lower triangular X has nothing above.  Element (i, j), j <= i, and its mirror are stored from
// one register; in a diagonal tile the entries right of the diagonal are the mirrors of those left of it.
__global__ __launch_bounds__(256) void k_flaplace_ata(const double* __restrict__ X, int ldx, double* __restrict__ S, int lds, int m,
                                                     int lower) {
    __shared__ double as[kT64][33], bs[kT64][33];
    int ti, tj;
    tile_pair(blockIdx.x, ti, tj);
    const int nt = (m + kT64 - 1) / kT64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    d4 acc[4];
#pragma unroll
    for (int gb = 0; gb < 4; ++gb) acc[gb] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k = lower ? ti : 0; k < nt; ++k) t64_tile<false, false>(acc, as, bs, X, ldx, ti * kT64, k * kT64, X, ldx, tj * kT64, k * kT64, m);
#pragma unroll
    for (int gb = 0; gb < 4; ++gb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * kT64 + 16 * wave + 4 * r + lq, j = tj * kT64 + 16 * gb + lr;
            if (i < m && j <= i) {
                S[(size_t)i * lds + j] = acc[gb][r];
                if (j < i) S[(size_t)j * lds + i] = acc[gb][r];
            }
        }
}

// B = W Cm (W lower triangular; Cm symmetric, so its column block is read as a row block), tile (i, j) = (blockIdx.y,
// blockIdx.x) over k = 0 .. i
__global__ __launch_bounds__(256) void k_flaplace_trmm(const double* __restrict__ W, int ldw, const double* __restrict__ Cm, int ldc,
                                                      double* __restrict__ B, int ldb, int m) {
    __shared__ double as[kT64][33], bs[kT64][33];
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    d4 acc[4];
#pragma unroll
    for (int gb = 0; gb < 4; ++gb) acc[gb] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k <= ti; ++k) t64_tile<true, true>(acc, as, bs, W, ldw, ti * kT64, k * kT64, Cm, ldc, tj * kT64, k * kT64, m);
#pragma unroll
    for (int gb = 0; gb < 4; ++gb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * kT64 + 16 * wave + 4 * r + lq, j = tj * kT64 + 16 * gb + lr;
            if (i < m && j < m) B[(size_t)i * ldb + j] = acc[gb][r];
        }
}

// P (mps x mps, every element written) <- Hi_ij (s_i s_j) inside m, zero beyond: k_forces_colquad's P_eff (scale == NULL:
// no affine model, the element itself).  dg[0 .. m) <- diag Hi, dg[ldg .. ldg + m) <- diag Ca (Ca may be NULL).
__global__ __launch_bounds__(256) void k_flaplace_to_colquad(const double* __restrict__ Hi, const double* __restrict__ Ca, int ld, int m,
                                                            const double* __restrict__ scale, double* __restrict__ P, int mps,
                                                            double* __restrict__ dg, int ldg) {
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= mps || j >= mps) return;
    double v = 0.0;
    if (i < m && j < m) {
        v = Hi[(size_t)i * ld + j];
        if (i == j) {
            dg[i] = v;
            if (Ca) dg[ldg + i] = Ca[(size_t)i * ld + i];
        }
        if (scale) v *= scale[i] * scale[j];
    }
    P[(size_t)i * mps + j] = v;
}

// ---- host side ------------------------------------------------------------------------------------
// W (ldw x ldw) <- L^-1, Hi (m x m, dense) <- W^T W, ldiag <- diag L.  1 + (T - 1) + 1 launches.  Enqueues only.
void launch_flaplace_inverse(bioen_hip_ctx* c, const double* L, int ldl, double* W, int ldw, double* Hi, double* ldiag) {
    const int m = c->m, nt = (m + kT64 - 1) / kT64;
    hipLaunchKernelGGL(k_flaplace_tinv, dim3(nt), dim3(64), 0, c->stream, L, ldl, m, W, ldw, ldiag);
    for (int d = 1; d < nt; ++d) hipLaunchKernelGGL(k_flaplace_trtri, dim3(nt - d), dim3(256), 0, c->stream, L, ldl, W, ldw, m, d);
    hipLaunchKernelGGL(k_flaplace_ata, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, W, ldw, Hi, m, m, 1);
}

// B (ldb x ldb) <- W Cm, Ca (m x m, dense) <- B^T B; Cm: m x m, dense, symmetric
void launch_flaplace_averages(bioen_hip_ctx* c, const double* W, int ldw, const double* Cm, double* B, int ldb, double* Ca) {
    const int m = c->m, nt = (m + kT64 - 1) / kT64;
    hipLaunchKernelGGL(k_flaplace_trmm, dim3(nt, nt), dim3(256), 0, c->stream, W, ldw, Cm, m, B, ldb, m);
    hipLaunchKernelGGL(k_flaplace_ata, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, B, ldb, Ca, m, m, 0);
}

// P (mps x mps) <- S Hi S padded with zeros; dg <- diag Hi, dg + ldg <- diag Ca (Ca may be NULL)
void launch_flaplace_to_colquad(bioen_hip_ctx* c, const double* Hi, const double* Ca, const double* scale, double* P, int mps, double* dg,
                                int ldg) {
    const int tb = (mps + 15) / 16;
    hipLaunchKernelGGL(k_flaplace_to_colquad, dim3(tb, tb), dim3(256), 0, c->stream, Hi, Ca, c->m, c->m, scale, P, mps, dg, ldg);
}

}  // namespace bioen

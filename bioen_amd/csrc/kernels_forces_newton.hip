// Forces method, M <= 1024: dense FP64 Cholesky factorisation  A + lambda I = L L^T  (lower) and the two triangular solves,
// on the device, for the Newton minimizer (gfx950).  Blocked and right-looking, panels of kFNewtonPanel = 64
// columns, three launches per panel:
//   k_fnewton_potrf   one wave: the 64 x 64 diagonal tile, lane i owns row i in registers, a column travels through LDS
//   k_fnewton_trsm    one wave (of a block's four, which fetch L11 together) per 64 rows below the tile: lane i owns row i of  X L11^T = A21, L11 read from LDS
//   k_fnewton_syrk    the trailing lower triangle  A22 -= L21 L21^T  in 64 x 64 tiles on v_mfma_f64_16x16x4_f64 -- the only
//                     place the M^3 / 3 flops are
// The tile product is tile64.hpp's, shared with the inversion (kernels_forces_laplace.hip).
// No cooperative launch, no grid-wide wait, no atomics: every element has one writer per launch, and every sum runs over
// the panel's columns in index order -- its shape is a function of m alone, so two factorisations of the same bits give
// the same bits.  Only the lower triangle of the source is ever read; rows and columns m .. mp of the padded buffer are
// never read as data (every index is held against m).
//
// A pivot that is <= 0 or not finite ends the factorisation: the diagonal kernel stores index + 1 (LAPACK's info) into a
// device word with an ordinary store and leaves; every later launch of the factorisation reads the word first and leaves.
//
// k_fnewton_solve: one block, L y = b then L^T x = y for k <= 8 right-hand sides; a diagonal tile is solved by one wave
// per right-hand side (lane t owns unknown t, L11 in LDS), the rest are GEMV updates: forward a wave per 32 rows with a
// butterfly sum (coalesced row segments), backward one column per thread.  A right-hand side's arithmetic does not depend on k: a column of a batch is the single solve.
// (One column per thread ends at column 1023: beyond m = 1024 launch_fnewton_solve hands over to k_fnewton_solve_wide,
// kernels_forces_newton_wide.hip.  fnewton_lane and fnewton_solve_tile, which both use: fnewton.hpp.)
#include "fnewton.hpp"

namespace bioen {

// L <- the lower triangle of src (m x m, row-major, leading dimension lds) + lambda I, zeros above the diagonal; dg <-
// the diagonal of src (without lambda); *info <- 0.  Reads nothing above the diagonal.
__global__ __launch_bounds__(256) void k_fnewton_load(const double* __restrict__ src, int lds, int m, int ldl, double lambda,
                                                      double* __restrict__ L, double* __restrict__ dg, int* __restrict__ info) {
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *info = 0;
    if (i >= m || j >= m) return;
    double v = 0.0;
    if (j <= i) {
        v = src[(size_t)i * lds + j];
        if (i == j) {
            dg[i] = v;
            v += lambda;
        }
    }
    L[(size_t)i * ldl + j] = v;
}

// The diagonal tile at k0 (nb = min(64, m - k0) rows): lane i owns row i.  Step j: lane j takes the root of its pivot,
// every lane below divides its entry of column j by it and shows it in LDS, then subtracts its multiple of the column from
// the rest of its row.  Rows >= nb are rows of the identity.  Entries right of a lane's diagonal are never loaded (zero)
// and what the updates leave there is never stored.
__global__ __launch_bounds__(64) void k_fnewton_potrf(double* __restrict__ L, int ldl, int m, int k0, int* __restrict__ info) {
    __shared__ double col[2][kT64];
    if (*info != 0) return;
    const int i = threadIdx.x;
    const int nb = min(kT64, m - k0);
    double a[kT64];
    double* const row = L + (size_t)(k0 + i) * ldl + k0;
#pragma unroll
    for (int t = 0; t < kT64; ++t) a[t] = (i < nb && t <= i) ? row[t] : (t == i ? 1.0 : 0.0);
    int bad = 0;
#pragma unroll
    for (int j = 0; j < kT64; ++j) {
        const double p = fnewton_lane(a[j], j);                // the pivot, as lane j holds it
        if (!(p > 0.0) || !(p <= 1.7976931348623157e308)) {  // <= 0, NaN or infinite (wave-uniform)
            bad = j + 1;
            break;
        }
        const double d = sqrt(p);
        const double l = i == j ? d : a[j] / d;
        a[j] = l;
        col[j & 1][i] = l;
        __syncthreads();
#pragma unroll
        for (int t = j + 1; t < kT64; ++t) a[t] = fma(-l, col[j & 1][t], a[t]);
    }
    if (bad) {
        if (i == 0) *info = k0 + bad;
        return;
    }
    if (i < nb) {
#pragma unroll
        for (int t = 0; t < kT64; ++t)
            if (t <= i) row[t] = a[t];
    }
}

// The panel below the tile: rows k0 + nb + 64 b + i, lane i owns one; X L11^T = A21 column by column, the multiples of a
// found entry taken off the rest of the row at once (independent fmas).  Columns >= nb of L11 are the identity's.
__global__ __launch_bounds__(256) void k_fnewton_trsm(double* __restrict__ L, int ldl, int m, int k0, const int* __restrict__ info) {
    __shared__ double dinv[kT64];
    __shared__ double tt[kT64][kT64 + 2];                      // L11 transposed: a column of L11 is read as one row (every lane the same address)
    if (*info != 0) return;
    const int nb = min(kT64, m - k0);
    // four waves fetch the tile (16 independent loads per thread); the first solves
#pragma unroll
    for (int it = 0; it < kT64 * kT64 / 256; ++it) {
        const int e = threadIdx.x + 256 * it;
        const int r = e / kT64, s = e % kT64;
        tt[s][r] = (r < nb && s <= r) ? L[(size_t)(k0 + r) * ldl + k0 + s] : (r == s ? 1.0 : 0.0);
    }
    __syncthreads();
    if (threadIdx.x < kT64) dinv[threadIdx.x] = 1.0 / tt[threadIdx.x][threadIdx.x];      // one division per column, not one per row and column
    __syncthreads();
    if (threadIdx.x >= kT64) return;
    const int i = threadIdx.x;
    const int r = k0 + nb + blockIdx.x * kT64 + i;
    const bool live = r < m;
    double* const row = L + (size_t)(live ? r : 0) * ldl + k0;
    double a[kT64];
#pragma unroll
    for (int t = 0; t < kT64; ++t) a[t] = (live && t < nb) ? row[t] : 0.0;
    int z = 0;
#pragma unroll
    for (int j = 0; j < kT64; ++j) {
        const double x = a[j] * dinv[j];
        a[j] = x;
        // column j of L11 is read HERE, behind x: its address passes through a register the compiler cannot see through
        // (z stays 0).  Left alone it reads all 2016 entries ahead of the first product and spills them.
        asm volatile("" : "+v"(z) : "v"(x));
        const double* const c = &tt[j][0] + z;
#pragma unroll
        for (int t = j + 1; t < kT64; ++t) a[t] = fma(-x, c[t], a[t]);
    }
#pragma unroll
    for (int t = 0; t < kT64; ++t)
        if (live && t < nb) row[t] = a[t];
}

// A22 -= L21 L21^T on the lower triangle, 64 x 64 tiles (ti >= tj), four waves: one tile product (tile64.hpp) over the
// panel's columns, the inner index 0 .. nb - 1 in order (columns >= nb are zeros).
__global__ __launch_bounds__(256) void k_fnewton_syrk(double* __restrict__ L, int ldl, int m, int k0, const int* __restrict__ info) {
    __shared__ double as[kT64][33], bs[kT64][33];
    if (*info != 0) return;
    const int base = k0 + min(kT64, m - k0);                  // first trailing row
    int ti, tj;
    tile_pair(blockIdx.x, ti, tj);
    const int r0 = base + ti * kT64, c0 = base + tj * kT64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    d4 acc[4];
#pragma unroll
    for (int gb = 0; gb < 4; ++gb) acc[gb] = d4{0.0, 0.0, 0.0, 0.0};
    t64_tile<true, true>(acc, as, bs, L, ldl, r0, k0, L, ldl, c0, k0, m);
#pragma unroll
    for (int gb = 0; gb < 4; ++gb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = r0 + 16 * wave + 4 * r + lq, j = c0 + 16 * gb + lr;
            if (i < m && j <= i) L[(size_t)i * ldl + j] -= acc[gb][r];
        }
}

// X: [k][ldx], right-hand sides in, solutions out.  1024 threads; wave a < k solves the diagonal tiles of right-hand side a.
__global__ __launch_bounds__(1024) void k_fnewton_solve(const double* __restrict__ L, int ldl, int m, int k, double* __restrict__ X,
                                                        int ldx) {
    __shared__ double t11[kT64][kT64 + 1];
    __shared__ double xs[kMaxBatch][kT64];
    __shared__ double dinv[kT64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = (m + kT64 - 1) / kT64;
    // ---- L y = b, panels first to last
    for (int p = 0; p < np; ++p) {
        const int j0 = p * kT64, nb = min(kT64, m - j0);
        __syncthreads();                                     // the updates of the panel before are in X; t11 and xs are free
        fnewton_solve_tile(t11, dinv, L, ldl, j0, nb);
        if (wave < k) {
            double v = lane < nb ? X[(size_t)wave * ldx + j0 + lane] : 0.0;
            for (int j = 0; j < nb; ++j) {
                if (lane == j) v = v * dinv[j];
                const double xj = fnewton_lane(v, j);
                if (lane > j) v = fma(-xj, t11[lane][j], v);
            }
            xs[wave][lane] = v;
            if (lane < nb) X[(size_t)wave * ldx + j0 + lane] = v;
        }
        __syncthreads();
        // The rows below the panel: a wave takes 32 of them at a time, lane t column t of each (one coalesced row segment
        // per load), and adds the 32 x 64 products up by a butterfly that halves the registers at every stage -- 31 exchanges
        // and one across the wave's halves for 32 row sums, lane r (and r + 32) ends with row r's.  The order of a row's sum
        // is fixed and does not depend on k.
        for (int a = 0; a < k; ++a) {
            const double xa = xs[a][lane];                   // (zero beyond nb)
            for (int c0 = j0 + nb + 32 * wave; c0 < m; c0 += 32 * 16) {
                double pr[32];
#pragma unroll
                for (int r = 0; r < 32; ++r)
                    pr[r] = (c0 + r < m && lane < nb) ? L[(size_t)(c0 + r) * ldl + j0 + lane] * xa : 0.0;
#pragma unroll
                for (int st = 0; st < 5; ++st) {
                    const int o = 16 >> st;
                    const bool up = (lane & o) != 0;
#pragma unroll
                    for (int r = 0; r < o; ++r) {
                        const double keep = up ? pr[r + o] : pr[r];
                        const double send = up ? pr[r] : pr[r + o];
                        pr[r] = keep + __shfl_xor(send, o, 64);
                    }
                }
                const double sum = pr[0] + __shfl_xor(pr[0], 32, 64);
                const int i = c0 + (lane & 31);
                if (lane < 32 && i < m) X[(size_t)a * ldx + i] -= sum;
            }
        }
    }
    // ---- L^T x = y, panels last to first
    for (int p = np - 1; p >= 0; --p) {
        const int j0 = p * kT64, nb = min(kT64, m - j0);
        __syncthreads();
        fnewton_solve_tile(t11, dinv, L, ldl, j0, nb);
        if (wave < k) {
            double v = lane < nb ? X[(size_t)wave * ldx + j0 + lane] : 0.0;
            for (int j = nb - 1; j >= 0; --j) {
                if (lane == j) v = v * dinv[j];
                const double xj = fnewton_lane(v, j);
                if (lane < j) v = fma(-xj, t11[j][lane], v);
            }
            xs[wave][lane] = v;
            if (lane < nb) X[(size_t)wave * ldx + j0 + lane] = v;
        }
        __syncthreads();
        const int i = tid;                                   // one column left of the panel per thread
        if (i < j0) {
            double s[kMaxBatch];
#pragma unroll
            for (int a = 0; a < kMaxBatch; ++a) s[a] = 0.0;
#pragma unroll 16
            for (int t = 0; t < kT64; ++t) {
                const double l = t < nb ? L[(size_t)(j0 + t) * ldl + i] : 0.0;
#pragma unroll
                for (int a = 0; a < kMaxBatch; ++a)
                    if (a < k) s[a] = fma(l, xs[a][t], s[a]);
            }
#pragma unroll
            for (int a = 0; a < kMaxBatch; ++a)
                if (a < k) X[(size_t)a * ldx + i] -= s[a];
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------
// L (ldl x ldl, ldl >= m) <- chol(lower(src) + lambda I); dg <- diag(src); *info as LAPACK's.  Enqueues only.
void launch_fnewton_factor(bioen_hip_ctx* c, const double* src, int lds, double lambda, double* L, int ldl, double* dg, int* info) {
    const int m = c->m;
    const int tb = (m + 15) / 16;
    hipLaunchKernelGGL(k_fnewton_load, dim3(tb, tb), dim3(256), 0, c->stream, src, lds, m, ldl, lambda, L, dg, info);
    for (int k0 = 0; k0 < m; k0 += kT64) {
        hipLaunchKernelGGL(k_fnewton_potrf, dim3(1), dim3(64), 0, c->stream, L, ldl, m, k0, info);
        const int below = m - k0 - kT64;
        if (below <= 0) break;
        const int nt = (below + kT64 - 1) / kT64;
        hipLaunchKernelGGL(k_fnewton_trsm, dim3(nt), dim3(256), 0, c->stream, L, ldl, m, k0, info);
        hipLaunchKernelGGL(k_fnewton_syrk, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, L, ldl, m, k0, info);
    }
}

// X [k][ldx] <- (L L^T)^-1 X
void launch_fnewton_solve(bioen_hip_ctx* c, const double* L, int ldl, int k, double* X, int ldx) {
    if (c->m > 1024) return launch_fnewton_solve_wide(c, L, ldl, k, X, ldx);
    hipLaunchKernelGGL(k_fnewton_solve, dim3(1), dim3(1024), 0, c->stream, L, ldl, c->m, k, X, ldx);
}

}  // namespace bioen

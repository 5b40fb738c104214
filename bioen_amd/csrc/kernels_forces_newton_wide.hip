// The solve of kernels_forces_newton.hip beyond 1024 unknowns (gfx950; DESIGN 6n: the log-weights dual Newton over row
// panels).  A translation unit of its own: beside it in one file, k_fnewton_solve does not keep its instructions.
#include "fnewton.hpp"

namespace bioen {

// k_fnewton_solve for m > 1024 (the log-weights dual Newton over row panels): the same solve, sum for sum, with
// the backward sweep's threads taking the columns tid, tid + 1024, ... left of the panel -- there one thread per column
// stops at column 1023.  A kernel of its own, so that k_fnewton_solve keeps its instructions (as a template's instance it
// does not: the compiler allocates its registers differently).  X: [k][ldx], right-hand sides in, solutions out.
__global__ __launch_bounds__(1024) void k_fnewton_solve_wide(const double* __restrict__ L, int ldl, int m, int k,
                                                             double* __restrict__ X, int ldx) {
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
        for (int i = tid; i < j0; i += 1024) {               // the columns left of the panel, 1024 apart per thread
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

void launch_fnewton_solve_wide(bioen_hip_ctx* c, const double* L, int ldl, int k, double* X, int ldx) {
    hipLaunchKernelGGL(k_fnewton_solve_wide, dim3(1), dim3(1024), 0, c->stream, L, ldl, c->m, k, X, ldx);
}

}  // namespace bioen

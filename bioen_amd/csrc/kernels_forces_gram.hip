// Forces method, M <= 1024: the dense Hessian and the covariance of the observables at a kept point in ONE pass over the
// matrix (gfx950).  With Y' = Y - centre, w the point's weights, q_j - qbar what the point keeps (fpoint_q):
//   G'[u]  = sum_j u_j Y'_j Y'_j^T                       u1_j = w_j,   u2_j = w_j (q_j - qbar)
//   C      = G'[u1] - ybar' ybar'^T                      the covariance of the observables under the weights
//   G2     = G'[u2] - g ybar'^T - ybar' g^T              g = sum_j u2_j Y'_j, the point's unscaled gradient
//   H      = theta C + G2 + C C                          (affine model, S = diag(row_scale): C_A = S C S,
//                                                         H_A = S (theta C + G2) S + C_A C_A)
// The two M x M x N products share every operand: the FP64 matrix cores' only compute-bound kernel of this library.
//
// k_forces_gram reads the row-sum order strip copy (strip.hpp) and is fgram.hpp's FP64 pass (fgram_pass) at the forces
// point: a wave owns a 64 x 64 sub-tile of BOTH matrices (2 x 16 accumulators of 4 doubles: 256 registers; one wave per
// SIMD), a block of four waves a 128 x 128 tile; only tile pairs I >= J are computed (in a diagonal tile the wave above the
// diagonal leaves).  The log-weights covariance (k_logw_gram, kernels_logw_newton.hip) is the same pass at its own point.
// A SET is the accumulation chain from zero over the strips g, g + gs, ... of one canonical segment, in strip order; every
// (set, sub-tile) has exactly one writer; k_fgram_sum_sets adds the sets in the fixed order
//   sum over segments (in index order) of [ the segment's groups added in turn ]
// -- no floating-point atomics, and the shape of the sum is a function of (segcols, M) alone.
// k_forces_gram_bf16 is fgram.hpp's split-BF16 pass (fgram16_pass) at the same point: the Hessian for a Newton
// minimizer, only the two M x M x N products in another precision -- the sets on the same layout, the row sums the same
// bits, everything behind the sets shared (launch_fgram_tail).
#include "fgram.hpp"

namespace bioen {

__global__ __launch_bounds__(256, 1) void k_forces_gram(FGramArgs q) { fgram_pass<ForcesGramPoint<4>>(q); }
// (32 f32 accumulators of 4: 128 AGPRs; one wave per SIMD)
__global__ __launch_bounds__(256, 1) void k_forces_gram_bf16(FGramArgs q) { fgram16_pass<ForcesGramPoint<1>>(q); }

// out[e] = sum over segments (in index order) of [ the segment's gs sets added in turn ], e < count: on the sets' own
// layout (coalesced); out is one more set behind the partials
__global__ __launch_bounds__(kBlock) void k_fgram_sum_sets(const double* __restrict__ partial, size_t set_stride, size_t count,
                                                           int nlocal, int gs, double* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += (size_t)gridDim.x * kBlock) {
        double total = 0.0;
        for (int v = 0; v < nlocal; ++v) {
            double s = 0.0;
            for (int g = 0; g < gs; ++g) s += partial[(size_t)(v * gs + g) * set_stride + e];
            total += s;
        }
        out[e] = total;
    }
}

// The rank corrections, theta, the affine model's scales; the lower triangle is computed and mirrored: C and T = theta C
// + G2 (affine: S . S of both) are bitwise symmetric.  16 x 16 threads per block, blocks above the diagonal leave.
__global__ __launch_bounds__(256) void k_fgram_finish(const double* __restrict__ sum, size_t rows_at, int m, double theta,
                                                      const double* __restrict__ ybar, const double* __restrict__ row_scale,
                                                      bool affine, double* __restrict__ cov, double* __restrict__ hess) {
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= m || j > i) return;
    const double yi = ybar[i], yj = ybar[j], gi = sum[rows_at + i], gj = sum[rows_at + j];
    double cv = fma(-yi, yj, fgram_elem(sum, 2, 0, i, j));
    const double g2 = fma(-yi, gj, fma(-gi, yj, fgram_elem(sum, 2, 1, i, j)));
    double tv = fma(theta, cv, g2);
    if (affine) {
        const double sa = row_scale[i], sb = row_scale[j];
        cv = (sa * cv) * sb;
        tv = (sa * tv) * sb;
    }
    cov[(size_t)i * m + j] = cv;
    cov[(size_t)j * m + i] = cv;
    hess[(size_t)i * m + j] = tv;
    hess[(size_t)j * m + i] = tv;
}

// hess += C C on the lower triangle, mirrored; the inner index runs 0 .. m - 1 in one fma chain per element
__global__ __launch_bounds__(256) void k_fgram_square(const double* __restrict__ cov, int m, double* __restrict__ hess) {
    __shared__ double as[16][17], bs[16][17];
    if (blockIdx.x > blockIdx.y) return;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    double s = 0.0;
    for (int k0 = 0; k0 < m; k0 += 16) {
        as[ty][tx] = (i < m && k0 + tx < m) ? cov[(size_t)i * m + k0 + tx] : 0.0;
        bs[ty][tx] = (k0 + ty < m && j < m) ? cov[(size_t)(k0 + ty) * m + j] : 0.0;
        __syncthreads();
        const int kn = min(16, m - k0);
        for (int kk = 0; kk < kn; ++kk) s = fma(as[ty][kk], bs[kk][tx], s);
        __syncthreads();
    }
    if (i < m && j <= i) {
        const double hv = hess[(size_t)i * m + j] + s;
        hess[(size_t)i * m + j] = hv;
        hess[(size_t)j * m + i] = hv;
    }
}

// ---- host side ------------------------------------------------------------------------------------
// The sets of a dense Gram pass with `mats` matrices per sub-tile, `set_extra` doubles behind a set's row sums, and `tail`
// doubles behind C.  gs: enough sets for two blocks per CU (256 CUs) over the canonical segments' tiles -- a function of
// (segcols, M) alone
GramPlan gram_plan(const bioen_hip_ctx* c, int mats, int set_extra, size_t tail) {
    GramPlan p{};
    const int np = panel_count(c);                  // over row panels (the log-weights pass): 16 slices a full panel
    p.nsl = (np - 1) * (kPanelRows / kWaveRows) + (panel_mps(c, np - 1) + kWaveRows - 1) / kWaveRows;
    const int t = (p.nsl + 1) / 2;
    p.ntiles = t * (t + 1) / 2;
    p.nsub = p.nsl * (p.nsl + 1) / 2;
    const int sps = strip_sps(c);
    p.gs = std::max(1, std::min(sps, (512 + c->nseg * p.ntiles - 1) / (c->nseg * p.ntiles)));
    p.nsets = c->vr * p.gs;
    p.rows_at = (size_t)p.nsub * fgram_sub_doubles(mats);
    p.set_stride = p.rows_at + (size_t)p.nsl * kWaveRows + set_extra;
    p.cov_at = (size_t)(p.nsets + 1) * p.set_stride;
    p.tail_at = p.cov_at + (size_t)c->m * c->m;
    p.doubles = p.tail_at + tail;
    return p;
}
GramPlan forces_gram_plan(const bioen_hip_ctx* c) { return gram_plan(c, 2, 0, (size_t)c->m * c->m); }      // behind C: H

// nlocal x gs sets of set_stride doubles in buf -> their sum in the fixed order, one more set behind them (the log-weights
// Gram pass, kernels_logw_newton.hip, ends here too)
void launch_fgram_sum_sets(bioen_hip_ctx* c, double* buf, size_t set_stride, int nlocal, int gs) {
    const int sum_blocks = (int)std::min<size_t>((set_stride + kBlock - 1) / kBlock, 4096);
    hipLaunchKernelGGL(k_fgram_sum_sets, dim3(sum_blocks), dim3(kBlock), 0, c->stream, buf, set_stride, set_stride, nlocal, gs,
                       buf + (size_t)nlocal * gs * set_stride);
}

// the sets in buf -> their sum behind them, C at buf + cov_at, H at buf + tail_at (both passes end here)
void launch_fgram_tail(bioen_hip_ctx* c, const GramPlan& p, double* buf, const double* ybar, double theta) {
    double* sum = buf + (size_t)p.nsets * p.set_stride;
    launch_fgram_sum_sets(c, buf, p.set_stride, c->vr, p.gs);
    const int tb = (c->m + 15) / 16;
    hipLaunchKernelGGL(k_fgram_finish, dim3(tb, tb), dim3(256), 0, c->stream, sum, p.rows_at, c->m, theta, ybar, c->row_scale,
                       c->affine, buf + p.cov_at, buf + p.tail_at);
    hipLaunchKernelGGL(k_fgram_square, dim3(tb, tb), dim3(256), 0, c->stream, buf + p.cov_at, c->m, buf + p.tail_at);
}

// buf: forces_gram_plan's doubles; x, pscal, qv, ybar: the kept point's.  Leaves C at buf + cov_at, H at buf + tail_at.
// bf16: the sets from k_forces_gram_bf16 (C~, H~; buf a buffer of that pass's own), everything behind them unchanged
void launch_forces_gram(bioen_hip_ctx* c, const GramPlan& p, double* buf, const double* x, const double* pscal,
                        const double* qv, const double* ybar, double theta, bool bf16) {
    hipLaunchKernelGGL(bf16 ? k_forces_gram_bf16 : k_forces_gram, dim3(fgram_blocks(p)), dim3(256), 0, c->stream,
                       fgram_args(c, p, buf, x, pscal, qv));
    launch_fgram_tail(c, p, buf, ybar, theta);
}

}  // namespace bioen

// Log-weights method, M <= 1024 (over row panels: M <= 4096): the dual Newton step's kernels (gfx950).  With w = softmax(g) the weights of the
// kept log-weights point, Y' = Y - centre, grad the point's gradient:
//   G'     = sum_j w_j Y'_j Y'_j^T
//   C      = G' - ybar' ybar'^T                          the covariance of the observables under the weights
//   b      = sum_j grad_j Y'_j - ybar' sum_j grad_j      = Yc grad, the right-hand side of (C + theta I) z = -b
//   (affine model, S = diag(row_scale): C_A = S C S, b_A = S b)
// k_logw_gram is fgram.hpp's FP64 pass (fgram_pass: k_forces_gram's, kernels_forces_gram.hip) at the log-weights point, with
// ONE matrix: the same copy -- the row-sum order strip copy the log-weights forward pass reads, in whichever layout it is
// (strip_phys) --, the same decode, centres, fetch, loop, sets and row sums, half the matrix instructions and half the
// accumulators (128 AGPRs + 224 VGPRs, no scratch; one wave per SIMD as there: with two, in 256 registers, the compiler
// spills 23 of them).  A wave owns a 64 x 64 sub-tile; the row sums ride along with u = grad, and so does sum grad.  One
// writer per (set, sub-tile), the sets added by k_fgram_sum_sets in its fixed order, C finished on the lower triangle and
// mirrored: bitwise symmetric.  k_logw_gram_bf16 is fgram.hpp's split-BF16 pass (fgram16_pass: k_forces_gram_bf16's)
// at the same point, for the loop's step: the sets on the same layout, everything behind them shared, -b the same bits.
// Around it the N-vector kernels of the loop, on the k_hessp_* pattern (kernels_hessp.hip): block partials into the X_GRAD
// stage, met in segment order by a one-block kernel.  The entries that launch them serve unsharded contexts only: the
// stage is not exchanged.
#include "fgram.hpp"

namespace bioen {

__global__ __launch_bounds__(256, 1) void k_logw_gram(FGramArgs q) { fgram_pass<LogwGramPoint<4>>(q); }

// 16 f32 accumulators where k_forces_gram_bf16 has 32: 236 VGPRs, no AGPRs, no scratch -- two waves per SIMD (with bounds of
// one wave the compiler takes 172 VGPRs + 64 AGPRs, runs two all the same, and is no faster: DESIGN 6k)
__global__ __launch_bounds__(256, 2) void k_logw_gram_bf16(FGramArgs q) { fgram16_pass<LogwGramPoint<1>>(q); }

// 1024 < M <= 4096: the same two passes with a wave's two slices taken from their row panels' copies
// (FGramPanelArgs); the panels' pointers, strides and chunk offsets are wave-uniform and live in scalar registers
__global__ __launch_bounds__(256, 1) void k_logw_gram_panels(FGramPanelArgs q) { fgram_pass<LogwGramPoint<4>>(q); }
__global__ __launch_bounds__(256, 2) void k_logw_gram_bf16_panels(FGramPanelArgs q) { fgram16_pass<LogwGramPoint<1>>(q); }

// The rank correction and the affine model's scales on the lower triangle, mirrored; the blocks of tile column 0 also leave
// -b for the solve.  16 x 16 threads per block, blocks above the diagonal leave.
__global__ __launch_bounds__(256) void k_lgram_finish(const double* __restrict__ sum, size_t rows_at, size_t sg_at, int m,
                                                      const double* __restrict__ ybar, const double* __restrict__ center,
                                                      const double* __restrict__ row_scale, bool affine,
                                                      double* __restrict__ cov, double* __restrict__ negb) {
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= m || j > i) return;
    const double yi = ybar[i] - center[i], yj = ybar[j] - center[j];
    double cv = fma(-yi, yj, fgram_elem(sum, 1, 0, i, j));
    if (affine) cv = (row_scale[i] * cv) * row_scale[j];
    cov[(size_t)i * m + j] = cv;
    cov[(size_t)j * m + i] = cv;
    if (negb && j == 0) {
        const double b = fma(-yi, sum[sg_at], sum[rows_at + i]);
        negb[i] = -(affine ? row_scale[i] * b : b);
    }
}

// One block: the centred adjoint's operand r_c + row_scale o z (K = 1, in place: the next evaluation writes r_c anew) and
// the strip adjoint's constants S_B0 = sum_i centre_i u_i, S_UY = sum_i ybar_i u_i, as k_hessp_combine leaves them
__global__ __launch_bounds__(kBlock) void k_logwn_operand(int mp, int m, const double* __restrict__ z,
                                                          const double* __restrict__ row_scale,
                                                          const double* __restrict__ center,
                                                          const double* __restrict__ ybar_c, double* __restrict__ r_c,
                                                          double* __restrict__ scal) {
    __shared__ double sh[kWaves];
    double b0 = 0.0, uy = 0.0;
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        const double u = row < m ? fma(row_scale[row], z[row], r_c[row]) : r_c[row];
        r_c[row] = u;
        b0 = fma(center ? center[row] : 0.0, u, b0);
        uy = fma(ybar_c[row], u, uy);
    }
    b0 = block_sum(b0, sh);
    uy = block_sum(uy, sh);
    if (threadIdx.x == 0) {
        scal[S_B0] = b0;
        scal[S_UY] = uy;
    }
}

// block maxima of |grad|, w = e inv and |gamma|, gamma = theta (x - G - P) + a
__global__ __launch_bounds__(kBlock) void k_logwn_stats(const double* __restrict__ x, const double* __restrict__ G,
                                                        const double* __restrict__ e, const double* __restrict__ grad,
                                                        const double* __restrict__ av, const double* __restrict__ pscal,
                                                        double theta, int n, Xch xo) {
    __shared__ double sh[kWaves];
    const SegPos sp = seg_pos(xo.npl, xo.segcols, n);
    const double inv = pscal[S_INV + sp.v], P = pscal[S_P];
    double gm = 0.0, wm = 0.0, cm = 0.0;
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(xo.npl)) {
        const d2 xv = ld_vec(x + j), Gv = ld_vec(G + j), ev = ld_vec(e + j), gv = ld_vec(grad + j), aa = ld_vec(av + j);
        gm = fmax(gm, fabs(gv.x));
        wm = fmax(wm, ev.x * inv);
        cm = fmax(cm, fabs(fma(theta, (xv.x - Gv.x) - P, aa.x)));
        if (j + 1 < sp.jend) {
            gm = fmax(gm, fabs(gv.y));
            wm = fmax(wm, ev.y * inv);
            cm = fmax(cm, fabs(fma(theta, (xv.y - Gv.y) - P, aa.y)));
        }
    }
    gm = block_max(gm, sh);
    wm = block_max(wm, sh);
    cm = block_max(cm, sh);
    if (threadIdx.x == 0) {
        xput<3>(xo, 0, 0, gm);
        xput<3>(xo, 0, 1, wm);
        xput<3>(xo, 0, 2, cm);
    }
}

// one block: the three maxima over the segments' blocks
__global__ __launch_bounds__(kBlock) void k_logwn_stats_finish(Xch xi, double* __restrict__ out) {
    __shared__ double sh[kWaves];
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (int seg = 0; seg < xi.world; ++seg) {
            const double* p = xseg_ptr<3>(xi, seg, 0, q);
            for (int k = threadIdx.x; k < xi.npl; k += kBlock) s = fmax(s, p[k]);
        }
        s = block_max(s, sh);
        if (threadIdx.x == 0) out[LN_GMAX + q] = s;
    }
}

// u = -[(x - G - P) + c / theta]; block partials of grad . u (the padding of grad is zero, that of u is written as zero: the
// trial x + alpha u keeps its padding)
template <bool POLICY>
__global__ __launch_bounds__(kBlock) void k_logwn_step(const double* __restrict__ x, const double* __restrict__ G,
                                                       const double* __restrict__ cadj, const double* __restrict__ grad,
                                                       const double* __restrict__ pscal, double theta, int n,
                                                       double* __restrict__ u, Xch xo) {
    __shared__ double sh[kWaves];
    const SegPos sp = seg_pos(xo.npl, xo.segcols, n);
    const double P = pscal[S_P], it = 1.0 / theta;
    double gu = 0.0;
    const int jseg = sp.j0 + xo.segcols;
    for (int j = seg_first(sp); j < jseg; j += seg_step(xo.npl)) {
        d2 uv = {0.0, 0.0};
        if (j < sp.jend) {
            const d2 xv = ld_vec(x + j), Gv = ld_vec(G + j), cc = ld_vec(cadj + j), gv = ld_vec(grad + j);
            uv.x = -fma(cc.x, it, (xv.x - Gv.x) - P);
            gu = fma(gv.x, uv.x, gu);
            if (j + 1 < sp.jend) {
                uv.y = -fma(cc.y, it, (xv.y - Gv.y) - P);
                gu = fma(gv.y, uv.y, gu);
            }
        }
        st_vec<POLICY>(u + j, uv);
    }
    gu = block_sum(gu, sh);
    if (threadIdx.x == 0) xput<1>(xo, 0, 0, gu);
}

// one block: grad . u, the segments' totals met in segment order
__global__ __launch_bounds__(kBlock) void k_logwn_step_finish(Xch xi, double* __restrict__ out) {
    __shared__ double sh[kShRed];
    const double s = xsum<1>(xi, 0, 0, sh);
    if (threadIdx.x == 0) out[LN_SLOPE] = s;
}

// ---- host side ------------------------------------------------------------------------------------
// gram_plan's sets with one matrix per sub-tile; behind a set's row sums sum grad (8 doubles), behind C the loop's scalars
GramPlan logw_gram_plan(const bioen_hip_ctx* c) { return gram_plan(c, 1, 8, kLogwnScal); }

void launch_logw_gram(bioen_hip_ctx* c, const GramPlan& p, double* buf, const double* e, const double* grad,
                      const double* pscal, const double* ybar, double* negb, bool bf16) {
    if (paneled(c))
        hipLaunchKernelGGL(bf16 ? k_logw_gram_bf16_panels : k_logw_gram_panels, dim3(fgram_blocks(p)), dim3(256), 0, c->stream,
                           fgram_panel_args(c, p, buf, e, pscal, grad));
    else
        hipLaunchKernelGGL(bf16 ? k_logw_gram_bf16 : k_logw_gram, dim3(fgram_blocks(p)), dim3(256), 0, c->stream,
                           fgram_args(c, p, buf, e, pscal, grad));
    launch_fgram_sum_sets(c, buf, p.set_stride, c->vr, p.gs);
    const double* sum = buf + (size_t)p.nsets * p.set_stride;
    const int tb = (c->m + 15) / 16;
    hipLaunchKernelGGL(k_lgram_finish, dim3(tb, tb), dim3(256), 0, c->stream, sum, p.rows_at,
                       p.rows_at + (size_t)p.nsl * kWaveRows, c->m, ybar, c->strip_center, c->row_scale, c->affine,
                       buf + p.cov_at, negb);
}

void launch_logwn_operand(bioen_hip_ctx* c, const double* z, double* scal) {
    hipLaunchKernelGGL(k_logwn_operand, dim3(1), dim3(kBlock), 0, c->stream, c->mp, c->m, z, c->row_scale, c->strip_center,
                       c->ybar_c, c->r_c, scal);
}

void launch_logwn_stats(bioen_hip_ctx* c, const double* x, const double* e, const double* grad, const double* a,
                        const double* pscal, double theta, double* out) {
    const Xch xs = make_xch(c, X_GRAD, 3 * vec_grid(c));
    hipLaunchKernelGGL(k_logwn_stats, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, x, c->fixed, e, grad, a, pscal, theta, c->n, xs);
    hipLaunchKernelGGL(k_logwn_stats_finish, dim3(1), dim3(kBlock), 0, c->stream, xs, out);
}

void launch_logwn_step(bioen_hip_ctx* c, const double* x, const double* cadj, const double* grad, const double* pscal,
                       double theta, double* u, double* out) {
    const Xch xs = make_xch(c, X_GRAD, vec_grid(c));
    if (c->nvec_nt)
        hipLaunchKernelGGL(k_logwn_step<true>, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, x, c->fixed, cadj, grad, pscal,
                           theta, c->n, u, xs);
    else
        hipLaunchKernelGGL(k_logwn_step<false>, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, x, c->fixed, cadj, grad, pscal,
                           theta, c->n, u, xs);
    hipLaunchKernelGGL(k_logwn_step_finish, dim3(1), dim3(kBlock), 0, c->stream, xs, out);
}

}  // namespace bioen

// Log-weights method, M <= 1024: the Laplace error bars at a kept log-weights point (gfx950).  With
// w = softmax(g), a_j = y_j - ybar, C = sum_j w_j a_j a_j^T (k_logw_gram's) and P = (C + theta I)^-1 (the inverse
// kernels_forces_laplace.hip forms from the factor of kernels_forces_newton.hip):
//   cov_averages = I - theta P                                   (= C P)
//   leverage_j   = w_j q_j,  q_j = a_j^T P a_j                   (k_forces_colquad's pass)
//   var(ln w_j)  = (1 - w_j - leverage_j) / (theta w_j),  std_w_j = sqrt(w_j (1 - w_j - leverage_j) / theta)
//   var(obar)    = (Var_w(o) - c^T P c) / theta,  c = sum_j w_j (o_j - obar) a_j      for any per-structure quantity o
// The matrix kernels and the quadratic-form pass are launched as they are; here are the kernels between them, on the
// k_hessp_* / k_logwn_* pattern (kernels_hessp.hip, kernels_logw_newton.hip): an N-vector kernel walks its segment in
// 16-byte pairs, block partials go into the X_GRAD stage and a one-block kernel meets them in segment order -- every sum
// over structures has the shape of the canonical segments, none depends on the grid.  One writer per output, no atomics,
// no scratch.  The entry that launches them serves unsharded contexts only: the stage is not exchanged.
#include "device_utils.hpp"

namespace bioen {

// cov_averages = I - theta P on the lower triangle, mirrored (bitwise symmetric), m x m dense both; the blocks of tile
// column 0 also leave ybar' = ybar - centre, what k_forces_colquad centres its operand on.  16 x 16 threads per block,
// blocks above the diagonal leave.
__global__ __launch_bounds__(256) void k_logwl_matrices(const double* __restrict__ P, int m, double theta,
                                                        const double* __restrict__ ybar, const double* __restrict__ center,
                                                        double* __restrict__ Ca, double* __restrict__ ybp) {
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= m || j > i) return;
    const double v = fma(-theta, P[(size_t)i * m + j], i == j ? 1.0 : 0.0);
    Ca[(size_t)i * m + j] = v;
    Ca[(size_t)j * m + i] = v;
    if (j == 0) ybp[i] = ybar[i] - center[i];
}

// Per structure, from e (w_j = e_j S_INV[segment], as LogwGramPoint forms it) and q (the quadratic forms): the outputs
// that are asked for (a NULL pointer: not written).  1 - w - w q is formed as it stands, never as 1 / w - 1 - q.  Past
// column n nothing is written but the zero that completes the last pair.
template <bool POLICY>
__global__ __launch_bounds__(kBlock) void k_logwl_finish(const double* __restrict__ e, const double* __restrict__ q,
                                                         const double* __restrict__ pscal, double theta, int n, SegMap sm,
                                                         double* __restrict__ w, double* __restrict__ lev,
                                                         double* __restrict__ vlw, double* __restrict__ sdw) {
    const SegPos sp = seg_pos(sm.npl, sm.segcols, n);
    const double inv = pscal[S_INV + sp.v];
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(sm.npl)) {
        const d2 ee = ld_vec(e + j), qq = ld_vec(q + j);
        const bool two = j + 1 < sp.jend;
        d2 wv, lv, vv, sv;
        wv.x = ee.x * inv;
        lv.x = wv.x * qq.x;
        const double rx = (1.0 - wv.x) - lv.x;
        vv.x = rx / (theta * wv.x);
        sv.x = sqrt(fmax(wv.x * rx, 0.0) / theta);
        wv.y = two ? ee.y * inv : 0.0;
        lv.y = two ? wv.y * qq.y : 0.0;
        const double ry = (1.0 - wv.y) - lv.y;
        vv.y = two ? ry / (theta * wv.y) : 0.0;
        sv.y = two ? sqrt(fmax(wv.y * ry, 0.0) / theta) : 0.0;
        if (w) st_vec<POLICY>(w + j, wv);
        if (lev) st_vec<POLICY>(lev + j, lv);
        if (vlw) st_vec<POLICY>(vlw + j, vv);
        if (sdw) st_vec<POLICY>(sdw + j, sv);
    }
}

// Held-out observable a = blockIdx.y: block partials of sum_j e_j (o_j - obar)^2, obar where k_hessp_tangent has left it
// (S_SPARE0); the padding of e is zero
__global__ __launch_bounds__(kBlock) void k_logwl_obs_var(HesspArgs h, int n, Xch xo) {
    __shared__ double sh[kWaves];
    const int a = blockIdx.y;
    const double* __restrict__ o = h.v[a];
    const double* __restrict__ e = h.e;
    const double obar = h.scal[a][S_SPARE0];
    const SegPos sp = seg_pos(xo.npl, xo.segcols, n);
    double s = 0.0;
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(xo.npl)) {
        const d2 oo = ld_vec(o + j), ee = ld_vec(e + j);
        const double dx = oo.x - obar, dy = oo.y - obar;
        s = fma(ee.x * dx, dx, s);
        if (j + 1 < sp.jend) s = fma(ee.y * dy, dy, s);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) xput<1>(xo, a, 0, s);
}

// One block per observable: c = Y' t from the segments' shares of the forward pass, met with the point's factors in
// segment order as k_hessp_combine meets them (affine model: S c, as b_A = S b) -> the solve's right-hand side X[a] and a
// copy of it in keep[a] (rows m .. mp: zero); Var_w(o) = sum_v fac_v (sum_j e_j (o_j - obar)^2)_v and obar -> sc[2 a],
// sc[2 a + 1]
__global__ __launch_bounds__(kBlock) void k_logwl_obs_rhs(Xch xi, Xch xv, int mp, int m, int K, HesspArgs h,
                                                          const double* __restrict__ row_scale, double* __restrict__ X,
                                                          double* __restrict__ keep, double* __restrict__ sc) {
    __shared__ double fac[kShRed], tot[kShRed];
    const int a = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    for (int r = threadIdx.x; r < xi.world; r += kBlock) fac[r] = h.fac[r];
    for (int seg = wave; seg < xv.world; seg += kWaves) {
        const double t = wave_seg_total(xseg_ptr<1>(xv, seg, a, 0), xv.npl);
        if ((threadIdx.x & 63) == 0) tot[seg] = t;
    }
    __syncthreads();
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        double s = 0.0;
        for (int r = 0; r < xi.world; ++r) s = fma(fac[r], xi.base[(size_t)r * xi.payload + (size_t)row * K + a], s);
        const double cv = row < m ? s * row_scale[row] : 0.0;
        X[(size_t)a * mp + row] = cv;
        keep[(size_t)a * mp + row] = cv;
    }
    if (threadIdx.x == 0) {
        double var = 0.0;
        for (int seg = 0; seg < xv.world; ++seg) var = fma(fac[seg], tot[seg], var);
        sc[2 * a] = var;
        sc[2 * a + 1] = h.scal[a][S_SPARE0];
    }
}

// One block per observable, after the solve x = P c: out[a] = obar, out[kMaxBatch + a] = (Var_w(o) - c . x) / theta
__global__ __launch_bounds__(kBlock) void k_logwl_obs_finish(int mp, int m, double theta, const double* __restrict__ X,
                                                             const double* __restrict__ keep, const double* __restrict__ sc,
                                                             double* __restrict__ out) {
    __shared__ double sh[kWaves];
    const int a = blockIdx.y;
    double s = 0.0;
    for (int row = threadIdx.x; row < m; row += kBlock) s = fma(keep[(size_t)a * mp + row], X[(size_t)a * mp + row], s);
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        out[a] = sc[2 * a + 1];
        out[kMaxBatch + a] = (sc[2 * a] - s) / theta;
    }
}

// ---- host side ------------------------------------------------------------------------------------
void launch_logwl_matrices(bioen_hip_ctx* c, const double* P, double theta, const double* ybar, double* Ca, double* ybp) {
    const int tb = (c->m + 15) / 16;
    hipLaunchKernelGGL(k_logwl_matrices, dim3(tb, tb), dim3(256), 0, c->stream, P, c->m, theta, ybar, c->strip_center, Ca, ybp);
}

void launch_logwl_finish(bioen_hip_ctx* c, const double* e, const double* q, const double* pscal, double theta, double* w,
                         double* lev, double* vlw, double* sdw) {
    if (c->nvec_nt)
        hipLaunchKernelGGL(k_logwl_finish<true>, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, e, q, pscal, theta, c->n,
                           seg_map(c), w, lev, vlw, sdw);
    else
        hipLaunchKernelGGL(k_logwl_finish<false>, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, e, q, pscal, theta, c->n,
                           seg_map(c), w, lev, vlw, sdw);
}

// the partials go into the X_GRAD stage, behind k_hessp_tangent's reading of k_hessp_dots' there
void launch_logwl_obs_var(bioen_hip_ctx* c, const HesspArgs& h) {
    hipLaunchKernelGGL(k_logwl_obs_var, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, c->stream, h, c->n,
                       make_xch(c, X_GRAD, h.n * vec_grid(c)));
}

void launch_logwl_obs_rhs(bioen_hip_ctx* c, const HesspArgs& h, double* X, double* keep, double* sc) {
    hipLaunchKernelGGL(k_logwl_obs_rhs, dim3(1, h.n), dim3(kBlock), 0, c->stream, make_xch(c, X_YBAR, ybar_payload(c, h.n, false)),
                       make_xch(c, X_GRAD, h.n * vec_grid(c)), c->mp, c->m, h.n, h, c->row_scale, X, keep, sc);
}

void launch_logwl_obs_finish(bioen_hip_ctx* c, int k, double theta, const double* X, const double* keep, const double* sc,
                             double* out) {
    hipLaunchKernelGGL(k_logwl_obs_finish, dim3(1, k), dim3(kBlock), 0, c->stream, c->mp, c->m, theta, X, keep, sc, out);
}

}  // namespace bioen

// Hessian-vector products of the log-weights objective (gfx950): the N-vector kernels and the M-vector combine around
// the two matrix passes an evaluation already has.  With w = softmax(g), vbar = sum_j w_j v_j:
//   dw_k   = w_k (v_k - vbar)
//   dr     = yTilde dw                                         (forward pass)
//   c_k    = sum_i dr_i (yTilde_ik - ybar_i)                   (centred adjoint pass, ybar of the POINT)
//   (Hv)_k = (v_k - vbar) grad_k + w_k [ theta (v_k - vbar) + c_k - v . grad ]
// Conventions of kernels_logw.hip: blockIdx.y = position a of the direction in the call's batch, the segment walk of
// SegPos, block partials into an exchange stage, POLICY = the cache policy of the streams.  Every direction performs the
// arithmetic it would perform alone: K directions in one call give the bits of K calls.
#include "device_utils.hpp"

namespace bioen {

// After the K = 1 evaluation that sets the point (one block): every segment's softmax factor e^{m_v - M} / S from the
// tails of the X_YBAR stage, formed as k_rows_combine forms S_INV, and the raw averages out of ybar_c.
__global__ __launch_bounds__(kBlock) void k_hessp_keep(Xch xi, int mp, const double* __restrict__ ybar_c,
                                                       double* __restrict__ fac, double* __restrict__ ybar) {
    const size_t tail_at = (size_t)mp;                  // K = 1, a = 0
    double gmax = -DBL_MAX;
    for (int r = 0; r < xi.world; ++r) gmax = fmax(gmax, xi.base[(size_t)r * xi.payload + tail_at + 2]);
    double S = 0.0;
    for (int r = 0; r < xi.world; ++r) {
        const double* tail = xi.base + (size_t)r * xi.payload + tail_at;
        S = fma(exp(tail[2] - gmax), tail[0], S);
    }
    const double invS = 1.0 / S;
    for (int r = threadIdx.x; r < xi.world; r += kBlock)
        fac[r] = exp(xi.base[(size_t)r * xi.payload + tail_at + 2] - gmax) * invS;
    for (int row = threadIdx.x; row < mp; row += kBlock) ybar[row] = ybar_c[row];
}

// block partials of sum_j e_j v_j and sum_j grad_j v_j (the padding of e, grad and v is zero)
template <bool POLICY>
__global__ __launch_bounds__(kBlock) void k_hessp_dots(HesspArgs h, int n, Xch xo) {
    __shared__ double sh[kWaves];
    const int a = blockIdx.y;
    const double* __restrict__ v = h.v[a];
    const double* __restrict__ e = h.e;
    const double* __restrict__ g = h.grad;
    double ev = 0.0, gv = 0.0;
    const SegPos sp = seg_pos(xo.npl, xo.segcols, n);
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(xo.npl)) {
        const d2 vv = ld_vec(v + j);
        const d2 ee = ld_vec(e + j);
        const d2 gg = ld_vec(g + j);
        ev = fma(ee.x, vv.x, ev);
        gv = fma(gg.x, vv.x, gv);
        ev = fma(ee.y, vv.y, ev);
        gv = fma(gg.y, vv.y, gv);
    }
    ev = block_sum(ev, sh);
    gv = block_sum(gv, sh);
    if (threadIdx.x == 0) {
        xput<2>(xo, a, 0, ev);
        xput<2>(xo, a, 1, gv);
    }
}

// Every block finishes the two sums in its prologue -- the segments' totals (wave_seg_total) met in segment order from
// +0.0, e . v with the segment's factor: vbar = sum_v fac_v (e . v)_v --, then t = e (v - vbar).  The 1 / sum e of the
// weights stays deferred to the M sums (k_hessp_combine), as in the evaluation; the padding of t is zero.
template <bool POLICY>
__global__ __launch_bounds__(kBlock) void k_hessp_tangent(HesspArgs h, int n, Xch xi) {
    __shared__ double sh[2 * kShRed];
    const int a = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    for (int task = wave; task < 2 * xi.world; task += kWaves) {
        const int q = task / xi.world, seg = task - q * xi.world;
        const double tot = wave_seg_total(xseg_ptr<2>(xi, seg, a, q), xi.npl);
        if ((threadIdx.x & 63) == 0) sh[q * kShRed + seg] = tot;
    }
    __syncthreads();
    double vbar = 0.0, vg = 0.0;
    for (int seg = 0; seg < xi.world; ++seg) {
        vbar = fma(h.fac[seg], sh[seg], vbar);
        vg += sh[kShRed + seg];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h.scal[a][S_SPARE0] = vbar;
        h.scal[a][S_SPARE1] = vg;
    }
    const double* __restrict__ v = h.v[a];
    const double* __restrict__ e = h.e;
    double* __restrict__ t = h.t[a];
    const SegPos sp = seg_pos(xi.npl, xi.segcols, n);
    // The walk covers the WHOLE segment, padding included: the adjoint pass of the previous product has left its output in
    // this buffer, finite but not zero beyond column n, and the forward pass multiplies the padding with the centred
    // operand (0 - centre), so every pair past the valid columns is written as zero here.
    const int jseg = sp.j0 + xi.segcols;
    for (int j = seg_first(sp); j < jseg; j += seg_step(xi.npl)) {
        d2 tv = {0.0, 0.0};
        if (j < sp.jend) {
            const d2 vv = ld_vec(v + j);
            const d2 ee = ld_vec(e + j);
            tv.x = ee.x * (vv.x - vbar);
            if (j + 1 < sp.jend) tv.y = ee.y * (vv.y - vbar);
        }
        st_vec<POLICY>(t + j, tv);
    }
}

// The hessp form of k_rows_combine (one block per direction): the segments' shares of yTilde . t_a enter with the
// point's factors, in segment order -> draw_i; the adjoint's operand (affine model: dr_eff = sc draw, stored
// pre-multiplied by sc as k_rows_combine stores r) compact in r_c, the point's raw ybar replicated into ybar_c, and the
// strip adjoint's constants S_B0 = sum_i center_i u_i, S_UY = sum_i ybar_i u_i into the direction's scalars.
__global__ __launch_bounds__(kBlock) void k_hessp_combine(Xch xi, int mp, int K, HesspArgs h,
                                                          const double* __restrict__ row_scale,
                                                          const double* __restrict__ center,
                                                          double* __restrict__ ybar_c, double* __restrict__ r_c) {
    __shared__ double sh[kWaves];
    __shared__ double fac[kShRed];
    const int a = blockIdx.y;
    for (int r = threadIdx.x; r < xi.world; r += kBlock) fac[r] = h.fac[r];
    __syncthreads();
    double b0 = 0.0, uy = 0.0;
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        double s = 0.0;
        for (int r = 0; r < xi.world; ++r) s = fma(fac[r], xi.base[(size_t)r * xi.payload + (size_t)row * K + a], s);
        const double sc = row_scale[row];
        const double u = (s * sc) * sc;
        const double raw = h.ybar[row];
        const double cen = center ? center[row] : 0.0;
        ybar_c[(size_t)row * K + a] = raw;
        r_c[(size_t)row * K + a] = u;
        b0 = fma(cen, u, b0);
        uy = fma(raw, u, uy);
    }
    b0 = block_sum(b0, sh);
    uy = block_sum(uy, sh);
    if (threadIdx.x == 0) {
        h.scal[a][S_B0] = b0;
        h.scal[a][S_UY] = uy;
    }
}

// (Hv)_k = (v_k - vbar) grad_k + w_k [ theta (v_k - vbar) + c_k - v . grad ],  w = e * S_INV of the block's segment
template <bool POLICY>
__global__ __launch_bounds__(kBlock) void k_hessp_epilogue(HesspArgs h, int n, SegMap sm) {
    const int a = blockIdx.y;
    const double* __restrict__ v = h.v[a];
    const double* __restrict__ e = h.e;
    const double* __restrict__ g = h.grad;
    double* tc = h.t[a];                        // holds c (the adjoint's output); H v replaces it element by element
    const double vbar = h.scal[a][S_SPARE0], vg = h.scal[a][S_SPARE1];
    const double theta = h.theta;
    const SegPos sp = seg_pos(sm.npl, sm.segcols, n);
    const double inv = h.pscal[S_INV + sp.v];
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(sm.npl)) {
        const d2 vv = ld_vec(v + j);
        const d2 ee = ld_vec(e + j);
        const d2 gg = ld_vec(g + j);
        const d2 cc = ld_vec(tc + j);
        const double dx = vv.x - vbar, dy = vv.y - vbar;
        d2 out;
        out.x = fma(dx, gg.x, (ee.x * inv) * ((fma(theta, dx, cc.x)) - vg));
        out.y = (j + 1 < sp.jend) ? fma(dy, gg.y, (ee.y * inv) * ((fma(theta, dy, cc.y)) - vg)) : 0.0;
        st_vec<POLICY>(tc + j, out);
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------
void launch_hessp_keep(bioen_hip_ctx* c, double* fac, double* ybar) {
    hipLaunchKernelGGL(k_hessp_keep, dim3(1), dim3(kBlock), 0, c->stream, make_xch(c, X_YBAR, ybar_payload(c, 1, true)),
                       c->mp, c->ybar_c, fac, ybar);
}

// the partials go into the X_GRAD stage (room for 3 K values per block: 2 K used), idle between evaluations
void launch_hessp_dots(bioen_hip_ctx* c, const HesspArgs& h) {
    TimedLaunch tl(c, 2, h.n);
    const Xch xo = make_xch(c, X_GRAD, 2 * h.n * vec_grid(c));
    if (c->nvec_nt) BIOEN_LAUNCH_TIMED(c, k_hessp_dots<true>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, h, c->n, xo);
    else BIOEN_LAUNCH_TIMED(c, k_hessp_dots<false>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, h, c->n, xo);
}

void launch_hessp_tangent(bioen_hip_ctx* c, const HesspArgs& h) {
    TimedLaunch tl(c, 3, h.n);
    const Xch xi = make_xch(c, X_GRAD, 2 * h.n * vec_grid(c));
    if (c->nvec_nt) BIOEN_LAUNCH_TIMED(c, k_hessp_tangent<true>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, h, c->n, xi);
    else BIOEN_LAUNCH_TIMED(c, k_hessp_tangent<false>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, h, c->n, xi);
}

void launch_hessp_combine(bioen_hip_ctx* c, const HesspArgs& h, const double* center) {
    TimedLaunch tl(c, 4, h.n);
    BIOEN_LAUNCH_TIMED(c, k_hessp_combine, dim3(1, h.n), dim3(kBlock), 0, make_xch(c, X_YBAR, ybar_payload(c, h.n, false)),
                       c->mp, h.n, h, c->row_scale, center, c->ybar_c, c->r_c);
}

void launch_hessp_epilogue(bioen_hip_ctx* c, const HesspArgs& h) {
    TimedLaunch tl(c, 5, h.n);
    if (c->nvec_nt) BIOEN_LAUNCH_TIMED(c, k_hessp_epilogue<true>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, h, c->n, seg_map(c));
    else BIOEN_LAUNCH_TIMED(c, k_hessp_epilogue<false>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, h, c->n, seg_map(c));
}

}  // namespace bioen

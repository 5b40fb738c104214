// Hessian-vector products of the forces objective at a kept point (gfx950): the M-vector and N-vector kernels around the
// two matrix passes of a product (M <= 1024: the SM_TANGENT / SM_PRODUCT forms of k_strip / k_strip2); DESIGN 6d.
// Notation of DESIGN 2: A_ij = o_i + s_i Y_ij, Y' = Y - centre, x' = Y'^T (f o s), w ~ w0 e^x', ybar' = Y' w,
// r = ybar - YTilde.  For a direction v:
//   dx_j    = sum_i (v o s)_i Y'_ij                             [pass 1, column sums]        dxbar = sum_i (v o s)_i ybar'_i
//   dy'_i   = sum_j Y'_ij w_j dx_j - ybar'_i sum_j w_j dx_j     [pass 1, row sums; the gradient's own finish]
//   c_j     = sum_i (dy' o s o s)_i Y'_ij                       [pass 2, column sums]        cbar  = sum_i (dy' o s o s)_i ybar'_i
//   s_j     = w_j [ (dx_j - dxbar) (q_j - qbar + theta) + c_j - cbar ]
//   (Hv)_i  = s_i [ sum_j Y'_ij s_j - ybar'_i sum_j s_j ]       [pass 2, row sums; the gradient's own finish]
// with q_j - qbar = theta x'_j + b'_j - (theta sum_j w_j x'_j + sum_i (r o s)_i ybar'_i), b' = Y'^T (r o s).  The averages
// dxbar, cbar and qbar are sums over the M rows of what the point holds (sum_j w_j Y'_ij = ybar'_i): no sum over
// structures is formed for them, so nothing about them depends on the number of ranks.  Constants added to x', q, dx or
// c cancel in the centred last line; each is taken off where it arises, so every sum stays at the scale of the data's
// spread.  One block per direction in the M-vector kernels: K directions in one call give the bits of K calls.
#include "device_utils.hpp"

namespace bioen {

// After the K = 1 evaluation that sets the point: ybar' (ybar_c of that round) and r o s (r_c) out of the round's arrays.
__global__ __launch_bounds__(kBlock) void k_fhp_keep(int mp, const double* __restrict__ ybar_c, const double* __restrict__ r_c,
                                                     double* __restrict__ ybar, double* __restrict__ rs) {
    for (int row = blockIdx.x * kBlock + threadIdx.x; row < mp; row += gridDim.x * kBlock) {
        ybar[row] = ybar_c[row];
        rs[row] = r_c[row];
    }
}

// q_j - qbar over the point's columns: qv holds b' (the column-sum pass on r o s), x the point's x'; every block forms
// qbar from the M rows in the same order.  The padding (j >= n) is zero.
__global__ __launch_bounds__(kBlock) void k_fhp_point_q(int mp, int n, size_t ld, const double* __restrict__ ybar,
                                                        const double* __restrict__ rs, const double* __restrict__ pscal,
                                                        double theta, const double* __restrict__ x, double* __restrict__ qv) {
    __shared__ double sh[kWaves];
    double ry = 0.0;
    for (int row = threadIdx.x; row < mp; row += kBlock) ry = fma(rs[row], ybar[row], ry);
    ry = block_sum(ry, sh);
    const double qbar = fma(theta, pscal[S_P], ry);
    for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < ld; j += (size_t)gridDim.x * kBlock)
        qv[j] = j < (size_t)n ? fma(theta, x[j], qv[j]) - qbar : 0.0;
}

// Before pass 1 (block a = direction a): ybar_c[row K + a] = ybar' (what the row-sum finish takes off), the direction's
// scalars: S_LOGS of the point, dxbar = sum_i um[row K + a] ybar'_i (um: v, on an affine model v o s already).
// center (the row panels, whose column sums run on Y itself): the averages of dx and c are those on Y, ybar' + centre.
__global__ __launch_bounds__(kBlock) void k_fhp_prepare(int mp, int K, const double* __restrict__ ybar, const double* __restrict__ um,
                                                        const double* __restrict__ pscal, const double* __restrict__ center,
                                                        double* __restrict__ ybar_c, double* __restrict__ hscal) {
    __shared__ double sh[kWaves];
    const int a = blockIdx.x;
    double s = 0.0;
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        const double yb = ybar[row];
        ybar_c[(size_t)row * K + a] = yb;
        s = fma(um[(size_t)row * K + a], center ? yb + center[row] : yb, s);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        double* sc = hscal + (size_t)a * kScalStride;
        sc[S_LOGS] = pscal[S_LOGS];
        sc[S_SPARE0] = s;
    }
}

// Between the passes (block a = direction a): gm holds dy' (the segments' shares added in segment order); the operand of
// pass 2's column sums -> u2[row K + a] = dy' (affine: o s o s, as r o s is the evaluation's), S_B0 = -cbar.
__global__ __launch_bounds__(kBlock) void k_fhp_combine(int mp, int K, const double* __restrict__ ybar, const double* __restrict__ gm,
                                                        const double* __restrict__ row_scale, bool affine,
                                                        const double* __restrict__ center,
                                                        double* __restrict__ u2, double* __restrict__ hscal) {
    __shared__ double sh[kWaves];
    const int a = blockIdx.x;
    double s = 0.0;
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        double u = gm[(size_t)row * K + a];
        if (affine) {
            const double sc = row_scale[row];
            u = (u * sc) * sc;
        }
        u2[(size_t)row * K + a] = u;
        s = fma(u, center ? ybar[row] + center[row] : ybar[row], s);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) hscal[(size_t)a * kScalStride + S_B0] = -s;
}

void launch_fhp_keep(bioen_hip_ctx* c, double* ybar, double* rs) {
    hipLaunchKernelGGL(k_fhp_keep, dim3((c->mp + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->mp, c->ybar_c, c->r_c, ybar, rs);
}

void launch_fhp_point_q(bioen_hip_ctx* c, const double* ybar, const double* rs, const double* pscal, double theta,
                        const double* x, double* qv) {
    hipLaunchKernelGGL(k_fhp_point_q, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, c->mp, c->n, c->ld, ybar, rs, pscal, theta, x, qv);
}

void launch_fhp_prepare(bioen_hip_ctx* c, int K, const double* ybar, const double* pscal, double* hscal, const double* center) {
    hipLaunchKernelGGL(k_fhp_prepare, dim3(K), dim3(kBlock), 0, c->stream, c->mp, K, ybar, c->um, pscal, center, c->ybar_c, hscal);
}

void launch_fhp_combine(bioen_hip_ctx* c, int K, const double* ybar, double* hscal, const double* center) {
    hipLaunchKernelGGL(k_fhp_combine, dim3(K), dim3(kBlock), 0, c->stream, c->mp, K, ybar, c->gm, c->row_scale, c->affine, center,
                       c->r_c, hscal);
}

// ---- M > 1024: the four passes over row panels (launch_adj_strip / launch_fwd_strip, as the evaluation there) ----------
// The point: slot 0 holds the normalised weights w and b = Y^T (r o s); q_j - qbar = theta log(w_j / w0_j) + b_j
// - (theta KL + sum_i (r o s)_i ybar_raw_i), the two sums being the point's S_KL and S_UY.  (The log as k_forces_seg_t
// takes it: nothing where a weight has underflowed.)
__global__ __launch_bounds__(kBlock) void k_fhp_seg_point_q(FhpVecArgs h, int n, SegMap sm) {
    const SegPos sp = seg_pos(sm.npl, sm.segcols, n);
    const double qbar = fma(h.theta, h.pscal[S_KL], h.pscal[S_UY]);
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(sm.npl)) {
        const d2 wv = ld_vec(h.w + j), w0v = ld_vec(h.w0 + j), bv = ld_vec(h.b + j);
        double l0 = 0.0, l1 = 0.0;
        if (wv.x >= DBL_MIN && w0v.x >= DBL_MIN) l0 = log(wv.x) - log(w0v.x);
        if (wv.y >= DBL_MIN && w0v.y >= DBL_MIN) l1 = log(wv.y) - log(w0v.y);
        d2 qv;
        qv.x = fma(h.theta, l0, bv.x) - qbar;
        qv.y = (j + 1 < sp.jend) ? fma(h.theta, l1, bv.y) - qbar : 0.0;
        *reinterpret_cast<d2*>(h.q + j) = qv;
    }
}

// PRODUCT = false: t = w dx (the operand of the first row-sum pass); true: t <- s = w [(dx - dxbar)(q - qbar + theta) +
// c - cbar], c in t.  The block's share of sum_j t_j goes to a one-array stage, as k_forces_seg_t's.
template <bool PRODUCT>
__global__ __launch_bounds__(kBlock) void k_fhp_seg_t(FhpVecArgs h, int n, Xch xo) {
    __shared__ double sh[kWaves];
    const int a = blockIdx.y;
    const double* __restrict__ dx = h.dx[a];
    double* __restrict__ t = h.t[a];
    const double dxbar = PRODUCT ? h.scal[a][S_SPARE0] : 0.0, b0 = PRODUCT ? h.scal[a][S_B0] : 0.0;
    double s = 0.0;
    const SegPos sp = seg_pos(xo.npl, xo.segcols, n);
    // The walk covers the WHOLE segment, padding included, as k_hessp_tangent's: t is one of the buffers the log-weights
    // products use, whose adjoint pass leaves its constant beyond column n, and the row-sum pass multiplies the padding
    // with the centred operand (0 - centre) -- the first product after a bioen_hip_logw_hessp call on the same context
    // was wrong by that (tests/test_hip_panel_loops.py: 16384 x 300).  Every pair past the valid columns is written as zero.
    const int jseg = sp.j0 + xo.segcols;
    for (int j = seg_first(sp); j < jseg; j += seg_step(xo.npl)) {
        if (j >= sp.jend) {
            *reinterpret_cast<d2*>(t + j) = d2{0.0, 0.0};
            continue;
        }
        const d2 wv = ld_vec(h.w + j), dv = ld_vec(dx + j);
        const bool two = j + 1 < sp.jend;
        d2 tv;
        if (PRODUCT) {
            const d2 qv = ld_vec(h.q + j), cv = ld_vec(t + j);
            tv.x = wv.x * fma(dv.x - dxbar, qv.x + h.theta, cv.x + b0);
            tv.y = two ? wv.y * fma(dv.y - dxbar, qv.y + h.theta, cv.y + b0) : 0.0;
        } else {
            tv.x = wv.x * dv.x;
            tv.y = two ? wv.y * dv.y : 0.0;
        }
        *reinterpret_cast<d2*>(t + j) = tv;
        s += tv.x;
        s += tv.y;
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) xput<1>(xo, a, 0, s);
}

// the total of a local segment's shares -> share 0 of that segment's `seg_sets` P_KL shares, the others zero
// (k_forces_seg_tsum's job; grid (directions, local segments))
__global__ __launch_bounds__(kBlock) void k_fhp_seg_tsum(Xch xi, FhpVecArgs h, int seg_sets) {
    const int a = blockIdx.x, v = blockIdx.y;
    const double s = xsum_seg<1>(xi, xi.rank + v, a, 0);
    double* share = h.part[a] + (size_t)P_KL * kPartStride + (size_t)v * seg_sets;
    for (int b = threadIdx.x; b < seg_sets; b += kBlock) share[b] = b == 0 ? s : 0.0;
}

void launch_fhp_seg_point_q(bioen_hip_ctx* c, const FhpVecArgs& h) {
    hipLaunchKernelGGL(k_fhp_seg_point_q, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, h, c->n, seg_map(c));
}

void launch_fhp_seg_t(bioen_hip_ctx* c, const FhpVecArgs& h, bool product, int seg_sets) {
    const Xch xo = make_xch(c, X_MAX, h.n * vec_grid(c));       // (free: the block maxima of the point's evaluation have been consumed)
    if (product) hipLaunchKernelGGL(k_fhp_seg_t<true>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, c->stream, h, c->n, xo);
    else hipLaunchKernelGGL(k_fhp_seg_t<false>, dim3(vec_blocks(c), h.n), dim3(kBlock), 0, c->stream, h, c->n, xo);
    hipLaunchKernelGGL(k_fhp_seg_tsum, dim3(h.n, c->vr), dim3(kBlock), 0, c->stream, xo, h, seg_sets);
}

}  // namespace bioen

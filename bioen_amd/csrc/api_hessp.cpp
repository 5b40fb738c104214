// Hessian-vector products of the log-weights objective (kernels: kernels_hessp.hip; the mathematics: DESIGN section 6b).
//
// A call with g != NULL is bioen_hip_logw_fdf with a gradient, after which the context keeps "the point": slot 0 holds e,
// the gradient and the scalars, c->fixed the prior G, point_ybar the raw averages, point_fac every segment's softmax
// factor.  A product at the kept point is then what a gradient costs: three N-vector sweeps around one forward and one
// centred adjoint pass -- the context's own pass family, for up to kMaxBatch directions at once.
// Whether a call sets the point or serves the kept one, and the refusal without one, is api_forces_point.cpp's
// logw_point_prologue, the dual Newton entries' too (api_logw_newton.cpp).
#include <algorithm>

#include "dense.hpp"

namespace bioen {

int hessp_buffers(bioen_hip_ctx* c, int k) {
    int rc;
    if (!c->point_ybar && (rc = dalloc_zero(&c->point_ybar, (size_t)c->mp, c->stream))) return rc;
    if (!c->point_fac && (rc = dalloc_zero(&c->point_fac, (size_t)std::max(c->nseg, (int)kMaxSeg), c->stream))) return rc;
    if (!c->hp_scal && (rc = dalloc_zero(&c->hp_scal, (size_t)kMaxBatch * kScalStride, c->stream))) return rc;
    for (int i = 0; i < 2 * k; ++i)
        if (!c->hp_vec[i] && (rc = dalloc_zero(&c->hp_vec[i], c->ld, c->stream))) return rc;      // (the padding stays zero)
    return 0;
}

void hessp_free(bioen_hip_ctx* c) {
    double* bufs[] = {c->point_ybar, c->point_fac, c->hp_scal, c->fpoint_ybar, c->fpoint_rs, c->fpoint_q};
    for (double* b : bufs)
        if (b) (void)hipFree(b);
    for (double*& b : c->hp_vec) {
        if (b) (void)hipFree(b);
        b = nullptr;
    }
    c->point_ybar = c->point_fac = c->hp_scal = nullptr;
    c->fpoint_ybar = c->fpoint_rs = c->fpoint_q = nullptr;
    c->point_valid = 0;
}

// hv_a = H(point) v_a, a < k
static int hessp_products(bioen_hip_ctx* c, int k, const double* v, double* hv) {
    int rc;
    if ((rc = hessp_buffers(c, k))) return rc;
    const ProblemSlot& s0 = c->slot[0];
    HesspArgs h{};
    h.n = k;
    for (int a = 0; a < k; ++a) {
        h.v[a] = c->hp_vec[2 * a];
        h.t[a] = c->hp_vec[2 * a + 1];
        h.scal[a] = c->hp_scal + (size_t)a * kScalStride;
        if ((rc = upload_n(c, c->hp_vec[2 * a], v + (size_t)a * c->n_global))) return rc;
    }
    h.e = s0.w;
    h.grad = s0.g;
    h.pscal = s0.scal;
    h.fac = c->point_fac;
    h.ybar = c->point_ybar;
    h.theta = c->point_theta;
    launch_hessp_dots(c, h);
    if ((rc = exchange(c, X_GRAD, 2 * (size_t)k * vec_grid(c)))) return rc;
    launch_hessp_tangent(c, h);
    Vec8 tv{};
    MVec8 out{}, sc{};
    for (int a = 0; a < k; ++a) {
        tv.p[a] = h.t[a];
        out.p[a] = h.t[a];              // the adjoint pass writes c over t: the forward pass has read it by then
        sc.p[a] = h.scal[a];
    }
    // the pass family is the one enqueue_logw_eval takes on this context (the point's evaluation has built the copies)
    int nblk;
    if ((rc = choose_logw_passes(c, true, 0, true, &nblk))) return rc;
    c->last_width = k;              // ybar_c: the point's raw averages in every column
    c->last_pos = 0;
    c->last_centered = false;
    if (nblk > 0) {
        launch_fwd_strip(c, k, tv);
        launch_fwd_rows_local(c, k, false, nblk, true);
        if ((rc = exchange(c, X_YBAR, (size_t)ybar_payload(c, k, false)))) return rc;
        launch_hessp_combine(c, h, c->strip_center);
        launch_adj_strip(c, k, c->r_c, out, sc);
    } else {
        launch_fwd_partial(c, k, tv);
        launch_fwd_rows_local(c, k, false);
        if ((rc = exchange(c, X_YBAR, (size_t)ybar_payload(c, k, false)))) return rc;
        launch_hessp_combine(c, h, nullptr);
        launch_adj(c, k, c->r_c, out, true);
    }
    launch_hessp_epilogue(c, h);
    if ((rc = check_launch())) return rc;
    for (int a = 0; a < k; ++a)
        if ((rc = download_n(c, hv + (size_t)a * c->n_global, h.t[a]))) return rc;
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return transport_error(c);
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_hip_logw_hessp(bioen_hip_ctx* c, const double* g, const double* G, double theta, int k,
                                    const double* v, double* hv, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone ...
    if (k < 0 || k > kMaxBatch) return fail(BIOEN_HIP_EINVAL, "k must be in [0, 8]");
    if (k > 0 && (!v || !hv)) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (g && !G) return fail(BIOEN_HIP_EINVAL, "g without G");
    int rc;
    // ONE point per context, of either method (api_forces_point.cpp) ... with g it is an evaluation
    if ((rc = logw_point_prologue(c, g, G, theta, 0, f, grad, __func__))) return rc;
    if (k == 0) return 0;
    rc = hessp_products(c, k, v, hv);
    if (rc) point_drop(c, "a product on it that failed");
    return rc;
}

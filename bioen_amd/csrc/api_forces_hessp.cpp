// Hessian-vector products of the forces objective (kernels: kernels_forces_hessp.hip and the SM_TANGENT / SM_PRODUCT forms
// of k_strip / k_strip2; the mathematics: DESIGN section 6d).
//
// A call with forces != NULL is bioen_hip_forces_fdf with a gradient, launch for launch, after which the context keeps
// "the point" (ctx.hpp: point_kind 1): slot 0 holds x' and the scalars, c->fixed the prior w0, fpoint_ybar / fpoint_rs the
// M-vectors ybar' and r o s, fpoint_q the N-vector q - qbar -- ONE column-sum pass more than the evaluation.  A product at
// the kept point is then two fused matrix passes, what a gradient costs, for up to kMaxBatch directions at once.
// Whether a call sets the point or serves the kept one, and the refusal without one, is api_forces_point.cpp's
// forces_point_prologue, shared with the dense entries.
#include <algorithm>
#include <vector>

#include "dense.hpp"

namespace bioen {

static int fhp_buffers(bioen_hip_ctx* c, int k) {
    int rc;
    if (!c->fpoint_ybar && (rc = dalloc_zero(&c->fpoint_ybar, (size_t)c->mp, c->stream))) return rc;
    if (!c->fpoint_rs && (rc = dalloc_zero(&c->fpoint_rs, (size_t)c->mp, c->stream))) return rc;
    if (!c->fpoint_q && (rc = dalloc_zero(&c->fpoint_q, c->ld, c->stream))) return rc;
    if (!c->hp_scal && (rc = dalloc_zero(&c->hp_scal, (size_t)kMaxBatch * kScalStride, c->stream))) return rc;
    for (int i = 0; i < (strip_panels(c) ? 2 : 1) * k; ++i) {      // dx of direction a (row panels: and its work vector)
        const int at = strip_panels(c) ? i : 2 * i;
        if (!c->hp_vec[at] && (rc = dalloc_zero(&c->hp_vec[at], c->ld, c->stream))) return rc;
    }
    return 0;
}

// what the entry refuses beyond forces_guard: everything but the fused strip passes on the FP64 copy
int fhp_guard(const bioen_hip_ctx* c) {
    if (c->storage)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_hessp is not served on the reduced-storage experiment's copies "
                                      "(bioen_hip_ctx_set_storage(0))");
    if (strip_panels(c) ? fwd_strip_blocks(c) <= 0 : forces_fused_blocks(c) <= 0)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_hessp needs the strip copies of the matrix (M > 1024: the row panels): "
                                      "the streaming kernels have no product");
    return 0;
}

// gm (compact [row k + a]) -> hv [k][m], through the pinned staging buffer
static int fhp_download(bioen_hip_ctx* c, int k, double* hv, double* gm_h) {
    int rc;
    const size_t cnt = (size_t)c->mp * k;
    if ((rc = check_launch())) return rc;
    BIOEN_HIP_CHECK(hipMemcpyAsync(gm_h, c->gm, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    if ((rc = transport_error(c))) return rc;
    for (int a = 0; a < k; ++a)
        for (int i = 0; i < c->m; ++i) hv[(size_t)a * c->m + i] = gm_h[(size_t)i * k + a];
    return 0;
}

// hv_a = H(point) v_a, a < k; v, hv: [k][m]
static int fhp_products(bioen_hip_ctx* c, int k, const double* v, double* hv) {
    int rc;
    if ((rc = fhp_buffers(c, k))) return rc;
    if ((rc = forces_staging(c))) return rc;            // (c->host_m; the live page is the engine's own business: api.hip)
    const int m = c->m;
    const size_t cnt = (size_t)c->mp * k;
    double* um_h = c->host_m;
    double* gm_h = c->host_m + (size_t)c->mp * kMaxBatch;
    std::fill(um_h, um_h + cnt, 0.0);
    for (int a = 0; a < k; ++a)
        for (int i = 0; i < m; ++i) um_h[(size_t)i * k + a] = v[(size_t)a * m + i];
    BIOEN_HIP_CHECK(hipMemcpyAsync(c->um, um_h, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const ProblemSlot& s0 = c->slot[0];
    if (strip_panels(c)) {
        // M > 1024: four passes over the row panels, the evaluation's own there -- two column-sum passes on Y, two row-sum
        // passes on Y', an N-vector kernel behind each column-sum pass
        const int psets = fwd_strip_blocks(c);
        if (psets <= 0) return fail(BIOEN_HIP_ESTATE, "the row panels no longer serve this context");
        if ((rc = ensure_strip_copy(c)) || (rc = ensure_strip_copy_colsum(c))) return rc;
        const StripSets ss = strip_sets(c);
        const int seg_sets = ss.gs * (ss.fold ? 1 : ss.nch);
        FhpVecArgs h{};
        ForcesRound fr{};
        MVec8 dxo{}, to{};
        Vec8 tv{};
        h.n = fr.n = k;
        h.w = s0.w;
        h.w0 = c->fixed;
        h.q = c->fpoint_q;
        h.theta = c->point_theta;
        for (int a = 0; a < k; ++a) {
            h.dx[a] = dxo.p[a] = c->hp_vec[2 * a];
            h.t[a] = to.p[a] = c->hp_vec[2 * a + 1];
            tv.p[a] = c->hp_vec[2 * a + 1];
            h.scal[a] = c->hp_scal + (size_t)a * kScalStride;
            h.part[a] = fr.part[a] = c->part + (size_t)a * P_COUNT * kPartStride;
        }
        c->last_width = k;
        c->last_pos = 0;
        c->last_centered = true;
        if (c->affine) launch_forces_affine_operand(c, k);
        launch_fhp_prepare(c, k, c->fpoint_ybar, s0.scal, c->hp_scal, c->strip_center);
        launch_adj_strip(c, k, c->um, dxo, MVec8{}, true);                  // dx = Y^T (v o s)                [matrix pass 1]
        launch_fhp_seg_t(c, h, false, seg_sets);                            // t = w dx ; its sum per segment
        launch_fwd_strip(c, k, tv);                                         // Y' . t                          [matrix pass 2]
        launch_fwd_rows_forces_grad_share(c, k, 0, &fr, false);             // ... - ybar' T_v, per segment
        if ((rc = exchange(c, X_YBAR, cnt))) return rc;
        launch_forces_grad_sum_ranks(c, k);                                 // dy' -> gm
        launch_fhp_combine(c, k, c->fpoint_ybar, c->hp_scal, c->strip_center);
        launch_adj_strip(c, k, c->r_c, to, MVec8{}, true);                  // c = Y^T (dy' o s o s)            [matrix pass 3]
        launch_fhp_seg_t(c, h, true, seg_sets);                             // s ; its sum per segment
        launch_fwd_strip(c, k, tv);                                         // Y' . s                          [matrix pass 4]
        launch_fwd_rows_forces_grad_share(c, k, 0, &fr, false);
        if ((rc = exchange(c, X_YBAR, cnt))) return rc;
        launch_forces_grad_sum_ranks(c, k);
        if (c->affine) launch_forces_affine_grad(c, k);
        return fhp_download(c, k, hv, gm_h);
    }
    const int nblk = forces_fused_blocks(c);
    if (nblk <= 0) return fail(BIOEN_HIP_ESTATE, "the strip passes no longer serve this context");
    if ((rc = ensure_strip_copy(c, 1))) return rc;
    ForcesRound fr{};
    fr.n = k;
    for (int a = 0; a < k; ++a) {
        fr.a[a] = s0.a;
        fr.w[a] = c->hp_vec[2 * a];
        fr.t[a] = c->fpoint_q;
        fr.scal[a] = c->hp_scal + (size_t)a * kScalStride;
        fr.part[a] = c->part + (size_t)a * P_COUNT * kPartStride;
        fr.theta[a] = c->point_theta;
    }
    c->last_width = k;              // ybar_c: the point's centred averages in every column
    c->last_pos = 0;
    c->last_centered = true;
    if (c->affine) launch_forces_affine_operand(c, k);                 // um <- v o s
    launch_fhp_prepare(c, k, c->fpoint_ybar, s0.scal, c->hp_scal, nullptr);
    launch_forces_hp_tangent(c, fr);                                   // dx, w dx, Y' . (w dx)          [matrix pass 1]
    launch_fwd_rows_forces_grad_share(c, k, nblk, &fr, true);          // every segment's share of dy'
    if ((rc = exchange(c, X_YBAR, cnt))) return rc;
    launch_forces_grad_sum_ranks(c, k);                                // ... added in segment order -> gm
    launch_fhp_combine(c, k, c->fpoint_ybar, c->hp_scal, nullptr);     // r_c <- dy' (o s o s), -cbar
    launch_forces_hp_product(c, fr);                                   // c, s, Y' . s                   [matrix pass 2]
    launch_fwd_rows_forces_grad_share(c, k, nblk, &fr, true);
    if ((rc = exchange(c, X_YBAR, cnt))) return rc;
    launch_forces_grad_sum_ranks(c, k);
    if (c->affine) launch_forces_affine_grad(c, k);
    return fhp_download(c, k, hv, gm_h);
}

// Evaluates the point and keeps it on the context, for the entry `who` (every entry that goes through
// api_forces_point.cpp's forces_point_prologue, and the Newton loop): the effects are declared under that name, so the
// reason recorded for a dropped point names the call the user made.
int fhp_set_point(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* f, double* grad,
                  const char* who) {
    int rc;
    if ((rc = enter(c, FX_EVALUATES, who))) return rc;
    c->point_lost = "a call that failed to set a new point";
    if ((rc = fhp_buffers(c, 0))) return rc;
    std::vector<double> own;
    if (!grad) {
        own.resize((size_t)c->m);
        grad = own.data();
    }
    // bioen_hip_forces_fdf's evaluation, launch for launch
    if ((rc = forces_eval(c, 1, forces, w0, &theta, f, grad))) return rc;
    if (strip_panels(c) ? fwd_strip_blocks(c) <= 0 : forces_fused_blocks(c) <= 0)
        return fail(BIOEN_HIP_ESTATE, "the strip copies could not be built: the streaming kernels have no product");
    const ProblemSlot& s0 = c->slot[0];
    launch_fhp_keep(c, c->fpoint_ybar, c->fpoint_rs);
    if (strip_panels(c)) {                                             // the evaluation has left w and b in the slot: no pass more
        FhpVecArgs h{};
        h.n = 1;
        h.w = s0.w;
        h.w0 = c->fixed;
        h.b = s0.a;
        h.pscal = s0.scal;
        h.q = c->fpoint_q;
        h.theta = theta;
        launch_fhp_seg_point_q(c, h);
    } else {
        launch_forces_colsum(c, c->fpoint_rs, c->fpoint_q);            // b' = Y'^T (r o s): the one pass more
        launch_fhp_point_q(c, c->fpoint_ybar, c->fpoint_rs, s0.scal, theta, s0.a, c->fpoint_q);
    }
    if ((rc = check_launch())) return rc;
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->point_theta = theta;
    c->point_kind = 1;
    c->point_valid = 1;
    c->point_lost = nullptr;
    return 0;
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_hip_forces_hessp(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, int k,
                                      const double* v, double* hv, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone ...
    if (k < 0 || k > kMaxBatch) return fail(BIOEN_HIP_EINVAL, "k must be in [0, 8]");
    if (k > 0 && (!v || !hv)) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (forces && !w0) return fail(BIOEN_HIP_EINVAL, "forces without w0");
    if (!forces && k == 0) return fail(BIOEN_HIP_EINVAL, "nothing to do: no forces and k = 0");
    int rc;
    if ((rc = forces_guard(c)) || (rc = fhp_guard(c))) return rc;
    if ((rc = forces_point_prologue(c, forces, w0, theta, f, grad, __func__))) return rc;      // ... with forces it is an evaluation
    if (k == 0) return 0;
    rc = fhp_products(c, k, v, hv);
    if (rc) point_drop(c, "a product on it that failed");
    return rc;
}

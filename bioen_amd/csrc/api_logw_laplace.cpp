// The Laplace error bars of the log-weights method at a kept point, without leaving the device (kernels:
// kernels_logw_laplace.hip).  Everything heavy is another section's, launched as it is: C from
// k_logw_gram (api_logw_newton.cpp: logwn_gram), C + theta I factorised by the Newton entries' kernels (fnewton_factor),
// P = (C + theta I)^-1 from the factor (launch_flaplace_inverse), one quadratic form per structure from k_forces_colquad, a
// held-out observable's c = Y' t from the forward strip pass and P c from the resident factor (launch_fnewton_solve).  The
// point is bioen_logwn_cov's (logw_point_prologue), the guard dense_guard with the dual Newton's reasons, the buffers
// SCRATCH_LOGW_GRAM, SCRATCH_NEWTON, SCRATCH_LAPLACE and SCRATCH_COLQUAD.  Only what the caller asks for is computed
// and comes down.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "dense.hpp"

namespace bioen {

// the parts of SCRATCH_LAPLACE's work matrix B (mp x mp >= 1024 doubles) this entry uses
struct LogwlWork {
    double *ybp, *keep, *out, *sc;      // ybar' (mp); the right-hand sides c (kMaxBatch x mp); obar | var (2 kMaxBatch); Var_w, obar (2 kMaxBatch)
};
static LogwlWork logwl_work(const bioen_hip_ctx* c) {
    LogwlWork w{};
    const size_t mp = (size_t)c->mp;
    w.ybp = flaplace_layout(c).B;
    w.keep = w.ybp + mp;
    w.out = w.keep + (size_t)kMaxBatch * mp;
    w.sc = w.out + 2 * kMaxBatch;
    return w;
}
static_assert((1 + kMaxBatch) * kRowAlign + 4 * kMaxBatch <= kRowAlign * kRowAlign, "the work matrix holds the parts at the smallest mp");

// var(obar_a) and obar_a of nobs <= kMaxBatch per-structure quantities at the kept point: t = e (o - obar) by the products'
// own kernels, c = S Y' t by the forward strip pass, x = P c on the resident factor of C + theta I
static int logwl_observables(bioen_hip_ctx* c, const double* observables, int nobs, double theta, double* obs_averages,
                             double* var_observables) {
    int rc;
    if ((rc = hessp_buffers(c, nobs))) return rc;
    const ProblemSlot& s0 = c->slot[0];
    HesspArgs h{};
    h.n = nobs;
    for (int a = 0; a < nobs; ++a) {
        h.v[a] = c->hp_vec[2 * a];
        h.t[a] = c->hp_vec[2 * a + 1];
        h.scal[a] = c->hp_scal + (size_t)a * kScalStride;
        if ((rc = upload_n(c, c->hp_vec[2 * a], observables + (size_t)a * c->n_global))) return rc;
    }
    h.e = s0.w;
    h.grad = s0.g;
    h.pscal = s0.scal;
    h.fac = c->point_fac;
    h.ybar = c->point_ybar;
    h.theta = theta;
    launch_hessp_dots(c, h);                  // sum e o (and grad . o, unused) -> X_GRAD
    launch_hessp_tangent(c, h);               // obar -> S_SPARE0; t = e (o - obar)
    launch_logwl_obs_var(c, h);               // sum e (o - obar)^2 -> X_GRAD
    int nblk = 0;                             // (the point's evaluation has built the copies)
    if ((rc = choose_logw_passes(c, true, 0, true, &nblk))) return rc;
    if (nblk <= 0) return fail(BIOEN_HIP_ESTATE, "bioen_logwn_laplace needs the strip copies of the matrix");
    Vec8 tv{};
    for (int a = 0; a < nobs; ++a) tv.p[a] = h.t[a];
    launch_fwd_strip(c, nobs, tv);            // sum t = 0: the strip centre drops out of Y' t
    launch_fwd_rows_local(c, nobs, false, nblk, true);
    const FNewtonBuf nb = fnewton_layout(c);
    const LogwlWork w = logwl_work(c);
    launch_logwl_obs_rhs(c, h, nb.X, w.keep, w.sc);
    launch_fnewton_solve(c, nb.L, nb.ldl, nobs, nb.X, c->mp);
    launch_logwl_obs_finish(c, nobs, theta, nb.X, w.keep, w.sc, w.out);
    if ((rc = check_launch())) return rc;
    double out[2 * kMaxBatch];
    BIOEN_HIP_CHECK(hipMemcpyAsync(out, w.out, sizeof out, hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int a = 0; a < nobs; ++a) {
        if (obs_averages) obs_averages[a] = out[a];
        if (var_observables) var_observables[a] = out[kMaxBatch + a];
    }
    return 0;
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_logwn_laplace(bioen_hip_ctx* c, const double* g, const double* G, double theta, const double* observables,
                                   int nobs, double* std_averages, double* cov_averages, double* w, double* leverage,
                                   double* var_logw, double* std_w, double* obs_averages, double* var_observables,
                                   double* logdet, double* min_pivot, int* info, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone
    if (!info) return fail(BIOEN_HIP_EINVAL, "info is NULL");
    if (g && !G) return fail(BIOEN_HIP_EINVAL, "g without G");
    if (!(theta > 0.0) || !std::isfinite(theta))
        return fail(BIOEN_HIP_EINVAL, "bioen_logwn_laplace needs theta > 0 (the error bars divide by theta)");
    if (nobs < 0 || nobs > kMaxBatch) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_laplace: nobs must be in [0, 8]");
    if (observables && nobs == 0) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_laplace: observables without nobs");
    if (!observables && nobs > 0) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_laplace: nobs without observables");
    int rc;
    if ((rc = dense_guard(c, __func__, kLogwnReasons, fwd_strip_blocks))) return rc;
    if ((rc = logw_point_prologue(c, g, G, theta, 1, f, grad, __func__, &kLogwnPoint))) return rc;
    if ((rc = logwn_copies(c, __func__))) return rc;
    // 1 - 4: C, chol(C + theta I), P, ln det
    const double* cov = nullptr;
    if ((rc = logwn_gram(c, 0, &cov, nullptr))) return rc;
    if ((rc = fnewton_buffers(c)) || (rc = flaplace_buffers(c))) return rc;
    if ((rc = fnewton_factor(c, cov, theta, info, nullptr)) || *info) return rc;      // a failed pivot: an ordinary result
    const int m = c->m, mps = (int)round_up((size_t)c->m, 16);      // the strips' rows (M <= 1024: one panel)
    const size_t pcount = (size_t)mps * mps, mbytes = (size_t)m * sizeof(double);
    const bool averages = std_averages || cov_averages, vectors = w || leverage || var_logw || std_w;
    const FNewtonBuf nb = fnewton_layout(c);
    const FLaplaceBuf b = flaplace_layout(c);
    const LogwlWork wk = logwl_work(c);
    std::vector<double> ldiag((size_t)m), dg((size_t)m, 0.0);
    if (averages || vectors || logdet || min_pivot) {
        launch_flaplace_inverse(c, nb.L, nb.ldl, b.W, b.ld, b.Hi, b.ldiag);
        if ((rc = check_launch())) return rc;
        BIOEN_HIP_CHECK(hipMemcpyAsync(ldiag.data(), b.ldiag, mbytes, hipMemcpyDeviceToHost, c->stream));
    }
    // 5 - 7: I - theta P and ybar'; P_eff = S P S where k_forces_colquad takes it; one quadratic form per structure; w,
    // leverage, var ln w, std w
    if (averages || vectors) {
        if ((rc = ensure_scratch(c, SCRATCH_COLQUAD, pcount + c->ld))) return rc;
        double* buf = c->scratch[SCRATCH_COLQUAD].p;
        launch_logwl_matrices(c, b.Hi, theta, c->point_ybar, b.Ca, wk.ybp);
        launch_flaplace_to_colquad(c, b.Hi, b.Ca, c->affine ? c->row_scale : nullptr, buf, mps, b.dg, b.ld);
        if (vectors) {
            if ((rc = hessp_buffers(c, 2))) return rc;
            double* const dw = w ? c->hp_vec[0] : nullptr;
            double* const dl = leverage ? c->hp_vec[1] : nullptr;
            double* const dv = var_logw ? c->hp_vec[2] : nullptr;
            double* const ds = std_w ? c->hp_vec[3] : nullptr;
            launch_forces_colquad(c, buf, wk.ybp, buf + pcount);
            launch_logwl_finish(c, c->slot[0].w, buf + pcount, c->slot[0].scal, theta, dw, dl, dv, ds);
            if ((rc = check_launch())) return rc;
            if (w && (rc = download_n(c, w, dw))) return rc;
            if (leverage && (rc = download_n(c, leverage, dl))) return rc;
            if (var_logw && (rc = download_n(c, var_logw, dv))) return rc;
            if (std_w && (rc = download_n(c, std_w, ds))) return rc;
        }
        if ((rc = check_launch())) return rc;
        if (std_averages) BIOEN_HIP_CHECK(hipMemcpyAsync(dg.data(), b.dg + b.ld, mbytes, hipMemcpyDeviceToHost, c->stream));
        if (cov_averages) BIOEN_HIP_CHECK(d2h_user(c->stream, cov_averages, b.Ca, (size_t)m * mbytes));
    }
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (logdet || min_pivot) flaplace_logdet(ldiag.data(), m, logdet, min_pivot);
    if (std_averages)
        for (int i = 0; i < m; ++i) std_averages[i] = std::sqrt(std::max(dg[i], 0.0));
    // 8: the held-out observables
    if (nobs > 0 && (obs_averages || var_observables)) return logwl_observables(c, observables, nobs, theta, obs_averages, var_observables);
    return 0;
}

// The log-weights method's dual Newton minimizer and the covariance it is built on (kernels: kernels_logw_newton.hip; DESIGN
// section 6j).  N unknowns through an M x M system: C of the kept log-weights point from k_logw_gram, C + theta I
// factorised and solved by section 6h's kernels (api_forces_newton.cpp: fnewton_factor, launch_fnewton_solve), the step from ONE centred adjoint pass on r + z.  Every N-vector stays in HBM; the
// loop is log_weights.py's dual_newton_bioen_log_posterior_base, decision for decision.  DESIGN section 6k: C may come from
// k_logw_gram_bf16 instead (split-BF16 products; -b, the gradient and every test of the loop stay FP64), and the loop runs a
// whole theta series behind one call (bioen_logwn_series), warm- or cold-started.  The point is bioen_hip_logw_hessp's:
// set, kept and refused by api_forces_point.cpp's logw_point_prologue / logw_keep_point, the entries guarded by its dense_guard.
#include <cmath>
#include <string>

#include "dense.hpp"

namespace bioen {

const PointWords kLogwnPoint = {"call with g", "set a log-weights point first (bioen_logwn_cov or bioen_hip_logw_hessp with g)"};

// After a point's evaluation the guard once more (dense_guard, on the copy the log-weights forward pass reads): the strip
// copies exist by now, or never will
int logwn_copies(const bioen_hip_ctx* c, const char* who, bool over_panels) {
    if (int rc = dense_guard(c, who, kLogwnReasons, fwd_strip_blocks, over_panels)) return rc;
    for (int p = 0; p * 1024 < c->m; ++p)                   // every row panel's (M <= 1024: the one)
        if (!c->Ys[p]) return fail(BIOEN_HIP_ESTATE, (std::string(who) + " needs the strip copies of the matrix").c_str());
    return 0;
}

// the loop's evaluations: what slot 0's x holds becomes the kept point (k = 1: hp_vec[0] takes the adjoint of r + z)
static int logwn_keep_point(bioen_hip_ctx* c, double theta, double* f, const char* who) {
    if (int rc = logw_keep_point(c, theta, 1, f, nullptr)) return rc;
    return logwn_copies(c, who, true);
}

// C of the kept log-weights point into SCRATCH_LOGW_GRAM, not downloaded; negb (may be NULL): -Yc grad for the solve (the
// same bits from either source)
int logwn_gram(bioen_hip_ctx* c, int source, const double** cov, double* negb) {
    int rc;
    const GramPlan p = logw_gram_plan(c);
    if ((rc = ensure_scratch(c, SCRATCH_LOGW_GRAM, p.doubles))) return rc;
    double* buf = c->scratch[SCRATCH_LOGW_GRAM].p;
    const ProblemSlot& s0 = c->slot[0];
    launch_logw_gram(c, p, buf, s0.w, s0.g, s0.scal, c->point_ybar, negb, source == LOGWN_BF16);
    if ((rc = check_launch())) return rc;
    if (cov) *cov = buf + p.cov_at;
    return 0;
}

// max |grad|, max w, max |gamma| of the point slot 0 was just evaluated at
static int logwn_stats(bioen_hip_ctx* c, double theta, double* gmax, double* wmax, double* gammamax) {
    int rc;
    const GramPlan p = logw_gram_plan(c);
    double* out = c->scratch[SCRATCH_LOGW_GRAM].p + p.tail_at;
    const ProblemSlot& s0 = c->slot[0];
    launch_logwn_stats(c, s0.x, s0.w, s0.g, s0.a, s0.scal, theta, out);
    if ((rc = check_launch())) return rc;
    double h[3];
    BIOEN_HIP_CHECK(hipMemcpyAsync(h, out + LN_GMAX, sizeof h, hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    *gmax = h[0], *wmax = h[1], *gammamax = h[2];
    return 0;
}

// bioen_logwn_cov and bioen_logwn_cov_bf16: one entry, the source apart
static int logwn_cov_entry(bioen_hip_ctx* c, const double* g, const double* G, double theta, double* C, double* f, double* grad,
                           int source, const char* who) {
    if (int rc = enter(c, FX_NONE, who)) return rc;           // a call rejected below leaves the point (and the device) alone
    if (g && !G) return fail(BIOEN_HIP_EINVAL, "g without G");
    if (!g && !C) return fail(BIOEN_HIP_EINVAL, "nothing to do: no g and no C");
    int rc;
    if ((rc = dense_guard(c, who, kLogwnReasons, fwd_strip_blocks, true))) return rc;
    if ((rc = logw_point_prologue(c, g, G, theta, 1, f, grad, who, &kLogwnPoint))) return rc;
    if (g && (rc = logwn_copies(c, who, true))) return rc;
    if (!C) return 0;
    const double* dcov = nullptr;
    if ((rc = logwn_gram(c, source, &dcov, nullptr))) return rc;
    BIOEN_HIP_CHECK(hipMemcpyAsync(C, dcov, (size_t)c->m * c->m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// what bioen_logwn_opt and bioen_logwn_series refuse before the device, the point or a session are touched
int logwn_check(const bioen_logwn_config* cfg, const double* thetas, int ntheta, const char* who) {
    if (!(cfg->gtol >= 0.0) || cfg->max_iterations < 0 || cfg->max_halvings < 1 || !(cfg->armijo > 0.0) || !(cfg->floor_ulps >= 0.0))
        return fail(BIOEN_HIP_EINVAL, "bioen_logwn_config: gtol >= 0, max_iterations >= 0, max_halvings >= 1, armijo > 0, floor_ulps >= 0");
    for (int k = 0; k < ntheta; ++k)
        if (!(thetas[k] > 0.0) || !std::isfinite(thetas[k]))
            return fail(BIOEN_HIP_EINVAL, (std::string(who) + " needs theta > 0 (the step divides by theta): use the L-BFGS for theta = 0").c_str());
    return 0;
}

// The loop for one theta and one covariance source, from the point slot 0's xp holds (c->fixed = G): DESIGN 6j, and 6k's
// switch -- with LOGWN_BF16 a step rejected at the rounding floor does not end the run: the kept point is restored and the
// FP64 pass serves the rest of this theta (once; res->switched).  Leaves the returned point in xp, evaluated and kept; every
// status returns 0.  While the context's profile selection is set (api_logw_profile.cpp) every evaluation forms the
// scales, and C and -b are projected behind the Gram finish: the loop is the same.
int logwn_loop(bioen_hip_ctx* c, double theta, const bioen_logwn_config* cfg, int source, bioen_logwn_series_result* res,
               const char* who) {
    int rc;
    const double eps = 2.220446049250313e-16;
    ProblemSlot& s0 = c->slot[0];
    *res = bioen_logwn_series_result{};
    // slot 0: xp = the accepted point, d = the step u, x = the trial (k_trial: x = xp + alpha d), w, g, a, scal = the
    // evaluation's; hp_vec[0] takes the adjoint of r + z
    BIOEN_HIP_CHECK(hipMemcpyAsync(s0.x, s0.xp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    BIOEN_HIP_CHECK(hipMemsetAsync(s0.d, 0, c->ld * sizeof(double), c->stream));
    double f = 0.0, ft = 0.0, gmax = 0.0, wmax = 0.0, cmax = 0.0;
    if ((rc = logwn_keep_point(c, theta, &f, who))) return rc;
    res->evaluations = 1;
    if ((rc = fnewton_buffers(c))) return rc;
    const GramPlan plan = logw_gram_plan(c);
    if ((rc = ensure_scratch(c, SCRATCH_LOGW_GRAM, plan.doubles))) return rc;
    double* const scal = c->scratch[SCRATCH_LOGW_GRAM].p + plan.tail_at;
    const FNewtonBuf nb = fnewton_layout(c);
    if ((rc = logwn_stats(c, theta, &gmax, &wmax, &cmax))) return rc;
    const int one[1] = {0};
    int status = -1, at_x = 1;
    for (;;) {
        // 1. the gradient test, and gamma's -- at a finite point: the maxima of a point that is not finite are not its own (fmax
        // passes over a NaN), and it goes on to 3, where C + theta I does not factorise
        if (std::isfinite(f) && gmax <= cfg->gtol * wmax && cmax <= theta) {
            status = 0;
            break;
        }
        if (res->iterations >= cfg->max_iterations) {        // 2.
            status = 1;
            break;
        }
        // 3. C and -b of the kept point (= xp), (C + theta I) z = -b, the operand r + z, its adjoint, u and grad . u
        const double* cov = nullptr;
        if ((rc = logwn_gram(c, source, &cov, nb.X))) return rc;
        if (source == LOGWN_BF16) ++res->bf16_passes;
        if (c->profile_groups > 0) launch_logw_project(c, c->point_ybar, const_cast<double*>(cov), nb.X);
        int info = 0;
        if ((rc = fnewton_factor(c, cov, theta, &info, nullptr))) return rc;
        ++res->factorisations;
        if (info != 0) {                                     // C is PSD and theta > 0: a pivot fails only on a point that is not finite
            status = 3;
            break;
        }
        launch_fnewton_solve(c, nb.L, nb.ldl, 1, nb.X, c->mp);
        launch_logwn_operand(c, nb.X, c->hp_scal);
        int nblk = 0;                                        // (the evaluation has built the copies the adjoint reads)
        if ((rc = choose_logw_passes(c, true, 0, true, &nblk))) return rc;
        if (nblk <= 0) return fail(BIOEN_HIP_ESTATE, (std::string(who) + " needs the strip copies of the matrix").c_str());
        MVec8 out{}, sc{};
        out.p[0] = c->hp_vec[0];
        sc.p[0] = c->hp_scal;
        c->last_width = 1;
        c->last_pos = 0;
        c->last_centered = false;
        launch_adj_strip(c, 1, c->r_c, out, sc);
        launch_logwn_step(c, s0.xp, c->hp_vec[0], s0.g, s0.scal, theta, s0.d, scal);
        if ((rc = check_launch())) return rc;
        double slope = 0.0;
        BIOEN_HIP_CHECK(hipMemcpyAsync(&slope, scal + LN_SLOPE, sizeof slope, hipMemcpyDeviceToHost, c->stream));
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
        // 4. alpha = 1, 1/2, ...
        double alpha = 1.0, gtmax = 0.0, wtmax = 0.0, ctmax = 0.0;
        bool accepted = false, go_over = false;
        for (int k = 0; k < cfg->max_halvings; ++k) {
            Round r = make_round(c, one, 1, &alpha, &theta);
            launch_trial(c, r);
            point_drop(c, who);
            if ((rc = logwn_keep_point(c, theta, &ft, who))) return rc;
            ++res->evaluations;
            at_x = 0;
            if ((rc = logwn_stats(c, theta, &gtmax, &wtmax, &ctmax))) return rc;
            const bool floor = std::fabs(alpha * slope) <= cfg->floor_ulps * eps * std::fabs(f);
            if (floor) {
                if (std::isfinite(ft) && gtmax < gmax) accepted = true;
                else if (source == LOGWN_BF16) go_over = true;       // 5. the step was the split pass's: FP64 from here on
                else status = 2;
                break;
            }
            if (std::isfinite(ft) && ft - f <= cfg->armijo * alpha * slope) {
                accepted = true;
                break;
            }
            alpha *= 0.5;
        }
        if (go_over) {                                       // the kept point again (one evaluation), then C anew
            source = LOGWN_FP64;
            res->switched = 1;
            BIOEN_HIP_CHECK(hipMemcpyAsync(s0.x, s0.xp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            point_drop(c, who);
            if ((rc = logwn_keep_point(c, theta, &f, who))) return rc;
            ++res->evaluations;
            if ((rc = logwn_stats(c, theta, &gmax, &wmax, &cmax))) return rc;
            at_x = 1;
            continue;
        }
        if (!accepted) {
            if (status < 0) status = 3;
            break;
        }
        BIOEN_HIP_CHECK(hipMemcpyAsync(s0.xp, s0.x, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        f = ft, gmax = gtmax, wmax = wtmax, cmax = ctmax;
        at_x = 1;
        ++res->iterations;
    }
    if (!at_x) {                                             // the returned point is the kept one
        BIOEN_HIP_CHECK(hipMemcpyAsync(s0.x, s0.xp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        point_drop(c, who);
        if ((rc = logwn_keep_point(c, theta, &f, who))) return rc;
        ++res->evaluations;
        if ((rc = logwn_stats(c, theta, &gmax, &wmax, &cmax))) return rc;
    }
    res->status = status;
    res->fmin = f;
    res->gmax = gmax;
    res->wmax = wmax;
    return 0;
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_logwn_cov(bioen_hip_ctx* c, const double* g, const double* G, double theta, double* C, double* f,
                               double* grad) {
    return logwn_cov_entry(c, g, G, theta, C, f, grad, LOGWN_FP64, __func__);
}

extern "C" int bioen_logwn_cov_bf16(bioen_hip_ctx* c, const double* g, const double* G, double theta, double* C, double* f,
                                    double* grad) {
    return logwn_cov_entry(c, g, G, theta, C, f, grad, LOGWN_BF16, __func__);
}

extern "C" int bioen_logwn_opt(bioen_hip_ctx* c, const double* g0, const double* G, double theta,
                               const bioen_logwn_config* cfg, double* gopt, bioen_logwn_result* res) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (!g0 || !G || !cfg || !gopt || !res) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    int rc;
    if ((rc = logwn_check(cfg, &theta, 1, __func__))) return rc;
    if ((rc = dense_guard(c, __func__, kLogwnReasons, fwd_strip_blocks, true))) return rc;
    if ((rc = enter(c, FX_EVALUATES, __func__))) return rc;
    *res = bioen_logwn_result{};
    if ((rc = upload_n(c, c->slot[0].xp, g0))) return rc;
    if ((rc = upload_n(c, c->fixed, G))) return rc;
    bioen_logwn_series_result r;
    if ((rc = logwn_loop(c, theta, cfg, LOGWN_FP64, &r, __func__))) return rc;
    if ((rc = download_n(c, gopt, c->slot[0].xp))) return rc;
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    res->status = r.status;
    res->fmin = r.fmin;
    res->gmax = r.gmax;
    res->wmax = r.wmax;
    res->iterations = r.iterations;
    res->evaluations = r.evaluations;
    res->factorisations = r.factorisations;
    return 0;
}

extern "C" int bioen_logwn_series(bioen_hip_ctx* c, const double* g0, const double* G, const double* thetas, int ntheta,
                                  const bioen_logwn_config* cfg, int source, int warm, double* gopt,
                                  bioen_logwn_series_result* results) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (!g0 || !G || !thetas || !cfg || !gopt || !results) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (ntheta < 1) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_series needs ntheta >= 1");
    if (source != LOGWN_FP64 && source != LOGWN_BF16) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_series: source is 0 (FP64) or 1 (split BF16)");
    if (warm != 0 && warm != 1) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_series: warm is 0 or 1");
    int rc;
    if ((rc = logwn_check(cfg, thetas, ntheta, __func__))) return rc;
    if ((rc = dense_guard(c, __func__, kLogwnReasons, fwd_strip_blocks, true))) return rc;
    if ((rc = enter(c, FX_EVALUATES, __func__))) return rc;
    ProblemSlot& s0 = c->slot[0];
    if ((rc = upload_n(c, s0.xp, g0))) return rc;
    if ((rc = upload_n(c, c->fixed, G))) return rc;
    // cold: g0 waits in slot 0's gp, which neither the evaluations nor the step write
    if (!warm) BIOEN_HIP_CHECK(hipMemcpyAsync(s0.gp, s0.xp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    for (int k = 0; k < ntheta; ++k) {
        if (!warm && k > 0) BIOEN_HIP_CHECK(hipMemcpyAsync(s0.xp, s0.gp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if ((rc = logwn_loop(c, thetas[k], cfg, source, &results[k], __func__))) return rc;
        if ((rc = download_n(c, gopt + (size_t)k * c->n, s0.xp))) return rc;
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

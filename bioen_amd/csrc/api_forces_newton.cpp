// The forces method's own Newton minimizer (kernels: kernels_forces_newton.hip).  The Hessian stays
// where bioen_hip_forces_gram / _gram_bf16 leave it (api_forces_gram.cpp: fgram_compute), is factorised and solved on the
// device; the M-vectors stay on the host, as in ForcesBatchEngine; the loop is forces.py's
// newton_bioen_log_posterior_base, decision for decision.  The guard, the refusal without a forces point and the buffer
// are api_forces_point.cpp's, with these entries' wording.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "dense.hpp"

namespace bioen {

// the refusal without a forces point, as these entries word it (need_point)
static const PointWords kFNewtonPoint = {"call with forces",
                                         "set a forces point first (bioen_hip_forces_hessp, bioen_hip_forces_gram with forces)"};

FNewtonBuf fnewton_layout(const bioen_hip_ctx* c) {
    FNewtonBuf b{};
    const size_t mp = (size_t)c->mp, m = (size_t)c->m;
    b.ldl = c->mp;
    b.L = c->scratch[SCRATCH_NEWTON].p;
    b.A = b.L + mp * mp;
    b.X = b.A + m * m;
    b.dg = b.X + (size_t)kMaxBatch * mp;
    b.info = reinterpret_cast<int*>(b.dg + mp);
    return b;
}

int fnewton_buffers(bioen_hip_ctx* c) {
    const size_t mp = (size_t)c->mp, m = (size_t)c->m;
    return ensure_scratch(c, SCRATCH_NEWTON, mp * mp + m * m + (size_t)kMaxBatch * mp + mp + 2);
}

// chol(lower(src) + lambda I) -> the context's L; *info as LAPACK's; dmax (may be NULL): max |diag src|
int fnewton_factor(bioen_hip_ctx* c, const double* src, double lambda, int* info, double* dmax) {
    int rc;
    const FNewtonBuf b = fnewton_layout(c);
    c->fnewton_state = 0;
    launch_fnewton_factor(c, src, c->m, lambda, b.L, b.ldl, b.dg, b.info);
    if ((rc = check_launch())) return rc;
    BIOEN_HIP_CHECK(hipMemcpyAsync(info, b.info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    std::vector<double> dg;
    if (dmax) {
        dg.resize((size_t)c->m);
        BIOEN_HIP_CHECK(hipMemcpyAsync(dg.data(), b.dg, (size_t)c->m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (dmax) {
        *dmax = 0.0;
        for (double v : dg) *dmax = std::max(*dmax, std::fabs(v));
    }
    c->fnewton_state = *info ? 2 : 1;
    c->fnewton_info = *info;
    return 0;
}

// X [k][m] <- (L L^T)^-1 B [k][m]
static int fnewton_solve(bioen_hip_ctx* c, int k, const double* B, double* X) {
    int rc;
    const FNewtonBuf b = fnewton_layout(c);
    const size_t row = (size_t)c->m * sizeof(double);
    for (int a = 0; a < k; ++a)
        if ((rc = h2d_user(c, b.X + (size_t)a * c->mp, B + (size_t)a * c->m, row))) return rc;
    launch_fnewton_solve(c, b.L, b.ldl, k, b.X, c->mp);
    if ((rc = check_launch())) return rc;
    for (int a = 0; a < k; ++a)
        BIOEN_HIP_CHECK(d2h_user(c->stream, X + (size_t)a * c->m, b.X + (size_t)a * c->mp, row));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_hip_forces_newton_factor(bioen_hip_ctx* c, const double* A, int source, double lambda, double* L, int* info) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves point, session and device alone
    if (!info) return fail(BIOEN_HIP_EINVAL, "info is NULL");
    if (!A && source != 0 && source != 1) return fail(BIOEN_HIP_EINVAL, "source must be 0 (gram) or 1 (gram_bf16)");
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(BIOEN_HIP_EINVAL, "lambda must be finite and >= 0");
    int rc;
    if ((rc = dense_guard(c, __func__, kNewtonReasons)) || (rc = forces_guard(c))) return rc;
    if (!A && (rc = need_point(c, 1, __func__, &kFNewtonPoint))) return rc;
    if ((rc = enter(c, FX_DEVICE, __func__))) return rc;
    if ((rc = fnewton_buffers(c))) return rc;
    const FNewtonBuf b = fnewton_layout(c);
    const double* src = b.A;
    if (A) {
        if ((rc = h2d_user(c, b.A, A, (size_t)c->m * c->m * sizeof(double)))) return rc;
    } else if ((rc = fgram_compute(c, source, nullptr, &src))) {
        return rc;
    }
    if ((rc = fnewton_factor(c, src, lambda, info, nullptr))) return rc;
    if (L && *info == 0) {
        BIOEN_HIP_CHECK(d2h_user_2d(c->stream, reinterpret_cast<char*>(L), (size_t)c->m * sizeof(double),
                                    reinterpret_cast<const char*>(b.L), (size_t)b.ldl * sizeof(double),
                                    (size_t)c->m * sizeof(double), (size_t)c->m));
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int bioen_hip_forces_newton_solve(bioen_hip_ctx* c, int k, const double* B, double* X) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (k < 1 || k > kMaxBatch) return fail(BIOEN_HIP_EINVAL, "k must be in [1, 8]");
    if (!B || !X) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    int rc;
    if ((rc = dense_guard(c, __func__, kNewtonReasons))) return rc;
    if (c->fnewton_state == 2) {
        const std::string m = "bioen_hip_forces_newton_solve: the last factorisation on this context ended with info = " +
                              std::to_string(c->fnewton_info) + " (no factor)";
        return fail(BIOEN_HIP_ESTATE, m.c_str());
    }
    if (c->fnewton_state != 1 || !c->scratch[SCRATCH_NEWTON].p)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_newton_solve: no factor on this context: call "
                                      "bioen_hip_forces_newton_factor first");
    if ((rc = enter(c, FX_DEVICE, __func__))) return rc;
    return fnewton_solve(c, k, B, X);
}

extern "C" int bioen_hip_opt_newton_forces(bioen_hip_ctx* c, const double* forces0, const double* w0, double theta,
                                           const bioen_newton_config* cfg, double* forces_out, double* weights_out,
                                           bioen_newton_result* res) {
    if (int rc = enter(c, FX_EVALUATES, __func__)) return rc;
    if (!forces0 || !w0 || !cfg || !forces_out || !res) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (cfg->hessian != 0 && cfg->hessian != 1) return fail(BIOEN_HIP_EINVAL, "config.hessian must be 0 (gram) or 1 (gram_bf16)");
    if (!(cfg->gtol >= 0.0) || cfg->max_iterations < 0 || !(cfg->lambda_factor > 1.0) || !(cfg->lambda_first > 0.0) ||
        !(cfg->lambda_max > cfg->lambda_first) || !(cfg->armijo > 0.0) || !(cfg->floor_ulps >= 0.0))
        return fail(BIOEN_HIP_EINVAL, "bioen_newton_config: gtol >= 0, max_iterations >= 0, lambda_factor > 1, 0 < lambda_first < "
                                      "lambda_max, armijo > 0, floor_ulps >= 0");
    int rc;
    if ((rc = dense_guard(c, __func__, kNewtonReasons)) || (rc = forces_guard(c)) || (rc = fhp_guard(c))) return rc;
    const int m = c->m;
    const double eps = 2.220446049250313e-16;
    std::vector<double> x(forces0, forces0 + m), g((size_t)m), xt((size_t)m), gt((size_t)m), p((size_t)m);
    double f = 0.0, ft = 0.0, lambda = 0.0, d = 1.0;
    int source = cfg->hessian, status = -1, need_h = 1, at_x = 1;
    const double* hess = nullptr;
    *res = bioen_newton_result{};
    auto gmax_of = [m](const std::vector<double>& v) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = std::fabs(v[i]) > s || std::isnan(v[i]) ? std::fabs(v[i]) : s;
        return s;
    };
    auto grow = [&]() {                                      // -> true: lambda has left the range (status 3)
        lambda = std::max(cfg->lambda_factor * lambda, cfg->lambda_first * d);
        return lambda > cfg->lambda_max * d;
    };
    if ((rc = fhp_set_point(c, x.data(), w0, theta, &f, g.data(), __func__))) return rc;
    res->evaluations = 1;
    if ((rc = dense_guard(c, __func__, kNewtonReasons)) || (rc = fnewton_buffers(c))) return rc;      // (the strip copies exist by now, or never will)
    double gmax = gmax_of(g);
    for (;;) {
        if (gmax <= cfg->gtol) {                             // 1. the gradient test
            status = 0;
            break;
        }
        if (res->iterations >= cfg->max_iterations) {        // 10.
            status = 1;
            break;
        }
        if (need_h) {                                        // 2. H at the kept point (= x), from `source`
            if (!at_x) {
                if ((rc = fhp_set_point(c, x.data(), w0, theta, &f, g.data(), __func__))) return rc;
                ++res->evaluations;
                at_x = 1;
            }
            if ((rc = fgram_compute(c, source, nullptr, &hess))) return rc;
            ++res->hessians;
        }
        int info = 0;                                        // 3. H + lambda I = L L^T
        for (;;) {
            double dm = 0.0;
            if ((rc = fnewton_factor(c, hess, lambda, &info, need_h ? &dm : nullptr))) return rc;
            ++res->factorisations;
            if (need_h) {
                d = dm > 0.0 && std::isfinite(dm) ? dm : 1.0;
                need_h = 0;
            }
            if (info == 0) break;
            if (grow()) {
                status = 3;
                break;
            }
        }
        if (status == 3) break;
        if ((rc = fnewton_solve(c, 1, g.data(), p.data()))) return rc;      // 4. p = -(L L^T)^-1 g: m doubles down, m up
        double gp = 0.0, pp = 0.0;
        for (int i = 0; i < m; ++i) {
            p[i] = -p[i];
            gp += g[i] * p[i];
            pp += p[i] * p[i];
            xt[i] = x[i] + p[i];
        }
        const double pred = 0.5 * (-gp) + 0.5 * lambda * pp;
        if ((rc = fhp_set_point(c, xt.data(), w0, theta, &ft, gt.data(), __func__))) return rc;      // 5. the trial, kept as the point
        ++res->evaluations;
        at_x = 0;
        const double gtmax = gmax_of(gt);
        const bool floor = pred <= cfg->floor_ulps * eps * std::fabs(f);      // 6.
        const bool accept = std::isfinite(ft) && (floor ? gtmax < gmax : ft - f <= -cfg->armijo * pred);
        if (accept) {                                        // 7.
            if (floor || (f - ft) / pred > cfg->rho_good) {
                lambda /= cfg->lambda_factor;
                if (lambda < cfg->lambda_zero * d) lambda = 0.0;
            }
            x.swap(xt);
            g.swap(gt);
            f = ft;
            gmax = gtmax;
            at_x = 1;
            need_h = 1;
            ++res->iterations;
            continue;
        }
        if (floor) {                                         // 8.
            if (source == 1) {
                source = 0;
                res->switched = 1;
                need_h = 1;                                  // (the point is restored at x where H is computed)
                continue;
            }
            status = 2;
            break;
        }
        if (grow()) {                                        // 9. no new Hessian: H of x is still in its buffer
            status = 3;
            break;
        }
    }
    if (!at_x) {                                             // the returned point is the kept one
        if ((rc = fhp_set_point(c, x.data(), w0, theta, &f, g.data(), __func__))) return rc;
        ++res->evaluations;
    }
    if (weights_out) {
        // an evaluation of f alone hands out the weights (slot 0); the point is set again behind it
        const double theta0 = 0.0;
        if ((rc = enter(c, FX_EVALUATES, __func__))) return rc;
        if ((rc = forces_eval(c, 1, x.data(), w0, &theta0, nullptr, nullptr))) return rc;
        if ((rc = download_n(c, weights_out, c->slot[0].w))) return rc;
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
        if ((rc = fhp_set_point(c, x.data(), w0, theta, &f, g.data(), __func__))) return rc;
        res->evaluations += 2;
    }
    std::copy(x.begin(), x.end(), forces_out);
    res->status = status;
    res->fmin = f;
    res->gmax = gmax;
    res->lambda = lambda;
    return 0;
}

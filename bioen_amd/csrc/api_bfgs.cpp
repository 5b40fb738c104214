// Dense inverse-Hessian BFGS session on a log-weights context (what it calls of the core: host.hpp; BfgsSession is an
// incomplete type everywhere else).
//
// The host driver (bioen_amd/bfgs.py) runs scipy's fmin_bfgs loop on scipy's own scalar line searches; this session
// is its vector backend: the point, the gradient, the direction, the step pairs and the N x N inverse Hessian H stay in
// HBM, and only scalars cross PCIe per trial.  Kernels and the algebra of the lazy update: kernels_bfgs.hip.
//
//   begin   x = g0, f and grad at x, p = -g               -> f0, |g| (the driver's norm), |g|_2, g.p
//   trial   f(x + alpha p) (forward pass only); with need_grad also the adjoint at the same point -> g(alpha).p
//   accept  s = alpha p, x += s, y = g(alpha) - g, g = g(alpha)  -> |g|, |p|_2, |x|_2 (the stopping tests)
//   update  one pass over H (pending update of the previous step + row sums H [y, g]), 4 dots, the next direction
//   end     w, chi^2, S at x; H is freed
//
// A session lives on an UNSHARDED context only.  Which other calls on the context end it is each entry's declaration to
// the guard (host.hpp: enter); every error inside a bfgs call ends it too, and bioen_hip_ctx_destroy.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>

#include "host.hpp"
#include "kernels.hpp"

namespace bioen {

struct BfgsSession {
    double theta = 0.0;
    size_t ldh = 0;                    // leading dimension of H (bfgs_ld)
    double* H = nullptr;               // ldh x ldh, row-major
    double *x = nullptr, *xt = nullptr, *g = nullptr, *gt = nullptr, *p = nullptr, *y = nullptr, *hg = nullptr;
    double* dx = nullptr;              // scratch: alpha p of a trial
    double* sb[2] = {};                // step pairs: the newest and the pending one
    double* ub[2] = {};                // u = H y: the newest and the pending one
    double* dsc = nullptr;             // 8 device doubles: reduction results
    int s_new = -1;                    // buffer of the newest accepted step
    int ps = -1, pu = -1;              // buffers of the pending update (-1: none)
    double rho = 0.0, cc = 0.0;        // its coefficients
    bool have_h = false;               // H holds a materialised matrix (a pass has run); else H_0 = I
    bool accepted = false;             // a step was accepted and awaits update
    double alpha = 0.0;                // the trial point whose forward (and maybe adjoint) state is in place
    bool has_f = false, has_g = false;
    double pp = 0.0;                   // p.p of the current direction
    long long passes = 0;              // H passes run
};

void bfgs_free(bioen_hip_ctx* c) {
    if (!c || !c->bfgs) return;
    BfgsSession* S = c->bfgs;
    if (c->stream) hipStreamSynchronize(c->stream);
    double* bufs[] = {S->H, S->dx, S->x, S->xt, S->g, S->gt, S->p, S->y, S->hg, S->sb[0], S->sb[1], S->ub[0], S->ub[1], S->dsc};
    for (double* b : bufs)
        if (b) hipFree(b);
    delete S;
    c->bfgs = nullptr;
    c->bfgs_hbytes = 0;
}

static int bfgs_error(bioen_hip_ctx* c, int rc) {     // every error path frees H
    bfgs_free(c);
    return rc;
}

static Round bfgs_round(bioen_hip_ctx* c, BfgsSession* S, double* x, double* g) {
    const int one[1] = {0};
    Round r = make_round(c, one, 1, nullptr, &S->theta);
    r.x[0] = x;
    r.g[0] = g;
    r.d[0] = S->p;          // the adjoint's g.d by-product is g(alpha).p = phi'(alpha)
    return r;
}

// k (x, y) pairs through the level-1 reduction (mode 0: dots; mode 1: out[1] = max |x1|) -> host
static int bfgs_reduce(bioen_hip_ctx* c, BfgsSession* S, int k, int mode, const double* const* xs,
                       const double* const* ys, double* out) {
    VDotArgs a{};
    a.k = k;
    a.mode = mode;
    for (int q = 0; q < k; ++q) {
        a.x[q] = xs[q];
        a.y[q] = ys[q];
    }
    launch_vdots_part(c, a);
    int rc = exchange(c, X_GRAD, 4 * (size_t)vec_grid(c));
    if (rc) return rc;
    launch_vdots_finish(c, a, S->dsc);
    if ((rc = check_launch())) return rc;
    double* host = c->host_scal + 2 * kScalStride;
    BIOEN_HIP_CHECK(hipMemcpyAsync(host, S->dsc, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int q = 0; q < k; ++q) out[q] = host[q];
    return 0;
}

static int bfgs_absmax(bioen_hip_ctx* c, BfgsSession* S, const double* v, double* out) {
    const double* xs[2] = {v, v};
    double o[2];
    const int rc = bfgs_reduce(c, S, 2, 1, xs, xs, o);
    *out = o[1];
    return rc;
}

// p = -(((hg - a1 s) - a2 u) + a3 s), -> g.p, p.p
static int bfgs_direction(bioen_hip_ctx* c, BfgsSession* S, const double* hg, const double* s, const double* u, double a1,
                          double a2, double a3, double* gp) {
    launch_bfgs_dir(c, hg, s, u, a1, a2, a3, S->g, S->p);
    int rc = exchange(c, X_GRAD, 4 * (size_t)vec_grid(c));
    if (rc) return rc;
    VDotArgs a{};
    a.k = 2;
    launch_vdots_finish(c, a, S->dsc);
    if ((rc = check_launch())) return rc;
    double* host = c->host_scal + 2 * kScalStride;
    BIOEN_HIP_CHECK(hipMemcpyAsync(host, S->dsc, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    *gp = host[0];
    S->pp = host[1];
    return 0;
}

static int bfgs_begin(bioen_hip_ctx* c, const double* g0, const double* G, double theta, int norm_inf, double* f0,
                      double* gnorm, double* gnorm2, double* dphi0) {
    BfgsSession* S = new (std::nothrow) BfgsSession;
    if (!S) return fail(BIOEN_HIP_ENOMEM, "BFGS session");
    c->bfgs = S;
    S->theta = theta;
    S->ldh = bfgs_ld(c->n);
    int rc;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&S->H), S->ldh * S->ldh * sizeof(double));   // never read before a pass writes it
    if (e != hipSuccess) {
        S->H = nullptr;
        hip_fail(e, "hipMalloc (BFGS inverse Hessian)", __FILE__, __LINE__);
        return BIOEN_HIP_ENOMEM;
    }
    c->bfgs_hbytes = (long long)(S->ldh * S->ldh * sizeof(double));
    double** vecs[] = {&S->dx, &S->x, &S->xt, &S->g, &S->gt, &S->p, &S->y, &S->hg, &S->sb[0], &S->sb[1], &S->ub[0], &S->ub[1]};
    for (double** v : vecs)
        if ((rc = dalloc_zero(v, c->ld, c->stream))) return rc;
    if ((rc = dalloc_zero(&S->dsc, 8, c->stream))) return rc;
    if ((rc = upload_n(c, S->x, g0))) return rc;
    if ((rc = upload_n(c, c->fixed, G))) return rc;
    if ((rc = eval_logw_point(c, bfgs_round(c, S, S->x, S->g), true, false, f0, nullptr))) return rc;
    const double gg = c->host_scal[S_GG];
    *gnorm2 = std::sqrt(gg);
    if (norm_inf) {
        if ((rc = bfgs_absmax(c, S, S->g, gnorm))) return rc;
    } else {
        *gnorm = std::sqrt(gg);
    }
    return bfgs_direction(c, S, S->g, S->sb[0], S->ub[0], 0.0, 0.0, 0.0, dphi0);     // p = -g (H_0 = I)
}

static int bfgs_trial(bioen_hip_ctx* c, BfgsSession* S, double alpha, int need_grad, double* f, double* dphi) {
    int rc;
    const Round r = bfgs_round(c, S, S->xt, S->gt);
    if (!(S->has_f && alpha == S->alpha)) {
        launch_vstep(c, S->x, S->p, alpha, S->xt, S->dx);     // x + alpha p
        launch_max(c, r);
        if ((rc = enqueue_logw_eval(c, r, false))) return rc;
        S->alpha = alpha;
        S->has_f = true;
        S->has_g = false;
    }
    if (need_grad && !S->has_g) {
        if ((rc = enqueue_logw_adjoint(c, r))) return rc;     // the forward state of this very point is in place
        S->has_g = true;
    }
    if ((rc = check_launch())) return rc;
    if ((rc = read_scalars(c))) return rc;
    *f = c->host_scal[S_F];
    if (dphi) *dphi = need_grad ? c->host_scal[S_DG] : 0.0;
    return 0;
}

static int bfgs_accept(bioen_hip_ctx* c, BfgsSession* S, double alpha, int norm_inf, double* gnorm, double* pnorm,
                       double* xnorm) {
    if (!(S->has_g && alpha == S->alpha) || S->accepted)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_bfgs_logw_accept: the gradient at this step has not been evaluated");
    const double gg = c->host_scal[S_GG], xx = c->host_scal[S_XX];     // of the trial point: read by the last trial
    const int ns = (S->ps == 0) ? 1 : 0;                                // not the pending step's buffer
    launch_vstep(c, S->x, S->p, alpha, S->xt, S->sb[ns]);               // s = alpha p ; x + s (the very bits of the trials)
    std::swap(S->x, S->xt);
    launch_bfgs_sub(c, S->gt, S->g, S->y);                              // y = g(alpha) - g
    std::swap(S->g, S->gt);
    int rc;
    if ((rc = check_launch())) return rc;
    S->s_new = ns;
    S->accepted = true;
    S->has_f = S->has_g = false;
    if (norm_inf) {
        if ((rc = bfgs_absmax(c, S, S->g, gnorm))) return rc;
    } else {
        *gnorm = std::sqrt(gg);
    }
    *pnorm = std::sqrt(S->pp);
    *xnorm = std::sqrt(xx);
    return 0;
}

static int bfgs_update(bioen_hip_ctx* c, BfgsSession* S, double* dphi0, int* rho_fallback) {
#pragma clang fp contract(off)
    if (!S->accepted) return fail(BIOEN_HIP_ESTATE, "bioen_hip_bfgs_logw_update: no accepted step");
    int rc;
    const int un = (S->pu == 0) ? 1 : 0;
    double* u = S->ub[un];
    const double* hg;
    if (S->ps < 0) {                     // first update: H_0 = I, so H_0 y = y and H_0 g = g
        BIOEN_HIP_CHECK(hipMemcpyAsync(u, S->y, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        hg = S->g;
    } else {                             // apply the pending update while streaming H, row sums H [y, g]
        launch_bfgs_hpass(c, S->H, S->ldh, !S->have_h, S->sb[S->ps], S->ub[S->pu], S->rho, S->cc, S->y, S->g, u, S->hg);
        S->have_h = true;
        ++S->passes;
        hg = S->hg;
    }
    const double* s = S->sb[S->s_new];
    const double* xs[4] = {S->y, S->y, u, s};
    const double* ys[4] = {s, u, S->g, S->g};
    double d[4];
    if ((rc = bfgs_reduce(c, S, 4, 0, xs, ys, d))) return rc;
    const double ys_ = d[0], yu = d[1], ug = d[2], sg = d[3];
    *rho_fallback = (ys_ == 0.0) ? 1 : 0;              // scipy: rhok = 1000 when y.s == 0
    const double rho = (ys_ == 0.0) ? 1000.0 : 1.0 / ys_;
    const double cc = rho * rho * yu + rho;
    if ((rc = bfgs_direction(c, S, hg, s, u, rho * ug, rho * sg, cc * sg, dphi0))) return rc;
    S->ps = S->s_new;
    S->pu = un;
    S->rho = rho;
    S->cc = cc;
    S->accepted = false;
    S->has_f = S->has_g = false;
    return 0;
}

}  // namespace bioen

using namespace bioen;

extern "C" {

int bioen_hip_bfgs_logw_begin(bioen_hip_ctx* c, const double* g0, const double* G, double theta, int norm_inf,
                              double* f0, double* gnorm, double* gnorm2, double* dphi0) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected for its arguments leaves point and session ...
    if (!g0 || !G || !f0 || !gnorm || !gnorm2 || !dphi0) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (c->world > 1) return fail(BIOEN_HIP_ESTATE, "the BFGS session needs an unsharded context (world = 1)");
    if (int rc = enter(c, FX_EVALUATES, __func__)) return rc;      // ... a valid one starts afresh
    c->bfgs_interrupted = 0;
    // memory check first: nothing is allocated for a matrix that cannot fit
    const size_t ldh = bfgs_ld(c->n);
    const double need = (double)ldh * (double)ldh * 8.0 + (double)(12 * c->ld + 8) * 8.0;
    size_t free_b = 0, total_b = 0;
    BIOEN_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need > (double)free_b) {
        char msg[320];
        std::snprintf(msg, sizeof msg,
                      "BFGS: the N x N inverse Hessian (N = %d, %.4g GB) and its work vectors exceed the %.4g GB of free "
                      "device memory",
                      c->n, (double)ldh * (double)ldh * 8e-9, (double)free_b * 1e-9);
        return fail(BIOEN_HIP_ENOMEM, msg);
    }
    const int rc = bfgs_begin(c, g0, G, theta, norm_inf, f0, gnorm, gnorm2, dphi0);
    return rc ? bfgs_error(c, rc) : 0;
}

int bioen_hip_bfgs_logw_trial(bioen_hip_ctx* c, double alpha, int need_grad, double* f, double* dphi) {
    if (int rc = enter(c, FX_SESSION_CALL, __func__)) return rc;
    if (!f) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    const int rc = bfgs_trial(c, c->bfgs, alpha, need_grad, f, dphi);
    return rc ? bfgs_error(c, rc) : 0;
}

int bioen_hip_bfgs_logw_accept(bioen_hip_ctx* c, double alpha, int norm_inf, double* gnorm, double* pnorm,
                               double* xnorm) {
    if (int rc = enter(c, FX_SESSION_CALL, __func__)) return rc;
    if (!gnorm || !pnorm || !xnorm) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    const int rc = bfgs_accept(c, c->bfgs, alpha, norm_inf, gnorm, pnorm, xnorm);
    return rc ? bfgs_error(c, rc) : 0;
}

int bioen_hip_bfgs_logw_update(bioen_hip_ctx* c, double* dphi0, int* rho_fallback) {
    if (int rc = enter(c, FX_SESSION_CALL, __func__)) return rc;
    if (!dphi0 || !rho_fallback) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    const int rc = bfgs_update(c, c->bfgs, dphi0, rho_fallback);
    return rc ? bfgs_error(c, rc) : 0;
}

int bioen_hip_bfgs_logw_end(bioen_hip_ctx* c, double* g_out, double* w_out, bioen_opt_result* info) {
    if (int rc = enter(c, FX_SESSION_CALL, __func__)) return rc;
    BfgsSession* S = c->bfgs;
    int rc = 0;
    do {
        const Round r = bfgs_round(c, S, S->x, S->gt);
        launch_max(c, r);
        if ((rc = enqueue_logw_eval(c, r, false))) break;      // w, chi^2, S at the result
        launch_scale_w(c, r);
        if ((rc = check_launch())) break;
        if ((rc = read_scalars(c))) break;
        if (g_out && (rc = download_n(c, g_out, S->x))) break;
        if (w_out && (rc = download_n(c, w_out, c->slot[0].w))) break;
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            rc = hip_fail(e, "bioen_hip_bfgs_logw_end", __FILE__, __LINE__);
            break;
        }
        if (info) {
            const double* h = c->host_scal;
            std::memset(info, 0, sizeof *info);
            info->fmin = h[S_F];
            info->chi2 = 0.5 * h[S_CHI];
            info->kl = h[S_P] - h[S_LOGS] + h[S_LOGS0];
            info->iterations = (int)S->passes;
        }
    } while (false);
    bfgs_free(c);
    return rc;
}

int bioen_hip_bfgs_logw_read_hinv(bioen_hip_ctx* c, int row0, int rows, int padded, double* out) {
    if (int rc = enter(c, FX_SESSION_CALL, __func__)) return rc;
    BfgsSession* S = c->bfgs;
    if (!out) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    const long long height = padded ? (long long)S->ldh : (long long)c->n;      // padded: the stored rows, pads included
    if (row0 < 0 || rows <= 0 || row0 + rows > height) return fail(BIOEN_HIP_EINVAL, "rows out of range");
    const size_t width = padded ? S->ldh : (size_t)c->n;
    double* stage = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&stage), (size_t)rows * S->ldh * sizeof(double));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (inverse Hessian read-back)", __FILE__, __LINE__);
    const bool pend = S->ps >= 0;
    launch_bfgs_hread(c, S->H, S->ldh, !S->have_h, pend ? S->sb[S->ps] : S->sb[0], pend ? S->ub[S->pu] : S->ub[0],
                      pend ? S->rho : 0.0, pend ? S->cc : 0.0, (size_t)row0, rows, stage);
    int rc = check_launch();
    if (!rc) {
        e = d2h_user_2d(c->stream, reinterpret_cast<char*>(out), width * sizeof(double),
                        reinterpret_cast<const char*>(stage), S->ldh * sizeof(double), width * sizeof(double),
                        (size_t)rows);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = hip_fail(e, "inverse Hessian read-back", __FILE__, __LINE__);
    }
    (void)hipFree(stage);
    return rc;
}

int bioen_hip_bfgs_logw_read_vec(bioen_hip_ctx* c, int which, double* out) {
    if (int rc = enter(c, FX_SESSION_CALL, __func__)) return rc;
    BfgsSession* S = c->bfgs;
    if (!out || which < 0 || which > 5) return fail(BIOEN_HIP_EINVAL, "bad argument");
    const double* v[6] = {S->x, S->g, S->p, S->s_new >= 0 ? S->sb[S->s_new] : S->sb[0], S->y,
                          S->pu >= 0 ? S->ub[S->pu] : S->ub[0]};
    if (int rc = download_n(c, out, v[which])) return rc;
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"

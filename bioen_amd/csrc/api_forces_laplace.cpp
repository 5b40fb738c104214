// The Laplace error bars of the forces method without leaving the device (kernels: kernels_forces_laplace.hip; DESIGN
// section 6i).  H stays where bioen_hip_forces_gram leaves it (fgram_compute, the FP64 pass), is factorised by the Newton
// entries' kernels (fnewton_factor, lambda = 0) and inverted from the factor; H^-1 is handed to k_forces_colquad where it
// stands.  Only what the caller asks for comes down.  The guard, the refusal without a forces point and the buffers are
// api_forces_point.cpp's, with these entries' wording.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dense.hpp"

namespace bioen {

static const DenseReasons kLaplaceReasons = {
    "the Hessian pass is not built there): use forces.laplace_error_bars' numpy path on the gathered matrix",
    " and there is no dense Hessian pass): the error bars are served for M <= 1024", "Gram product"};
static const PointWords kLaplacePoint = {"call with forces",
                                         "set a forces point first (bioen_laplace_forces, bioen_hip_forces_gram with forces)"};

// (FLaplaceBuf: dense.hpp -- here W = L^-1, B = W C, Hi = H^-1, Ca = C H^-1 C; the log-weights error bars share the buffer)
FLaplaceBuf flaplace_layout(const bioen_hip_ctx* c) {
    FLaplaceBuf b{};
    const size_t mp = (size_t)c->mp;
    b.ld = c->mp;
    b.W = c->scratch[SCRATCH_LAPLACE].p;
    b.Hi = b.W + mp * mp;
    b.B = b.Hi + mp * mp;
    b.Ca = b.B + mp * mp;
    b.ldiag = b.Ca + mp * mp;
    b.dg = b.ldiag + mp;
    return b;
}

int flaplace_buffers(bioen_hip_ctx* c) {
    const size_t mp = (size_t)c->mp;
    return ensure_scratch(c, SCRATCH_LAPLACE, 4 * mp * mp + 3 * mp);
}

// chol(lower(src)) -> the context's factor; with *info == 0: W, H^-1 (enqueued) and diag L (on the host).  With
// *info != 0 no kernel of the inverse has run.
static int flaplace_inverse(bioen_hip_ctx* c, const double* src, int* info, std::vector<double>& ldiag) {
    int rc;
    if ((rc = fnewton_factor(c, src, 0.0, info, nullptr)) || *info) return rc;
    const FNewtonBuf nb = fnewton_layout(c);
    const FLaplaceBuf b = flaplace_layout(c);
    launch_flaplace_inverse(c, nb.L, nb.ldl, b.W, b.ld, b.Hi, b.ldiag);
    if ((rc = check_launch())) return rc;
    ldiag.resize((size_t)c->m);
    BIOEN_HIP_CHECK(hipMemcpyAsync(ldiag.data(), b.ldiag, (size_t)c->m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// C and H of the kept forces point, FP64 pass: where the last bioen_hip_forces_gram pass left them if the point has not
// changed since (ctx.hpp: fgram_fresh -- the same bits a new pass would write), else computed now
static int flaplace_gram(bioen_hip_ctx* c, const double** cov, const double** hess) {
    if (!c->fgram_fresh || !c->scratch[SCRATCH_GRAM].p) return fgram_compute(c, 0, cov, hess);
    const GramPlan p = forces_gram_plan(c);
    *cov = c->scratch[SCRATCH_GRAM].p + p.cov_at;
    *hess = c->scratch[SCRATCH_GRAM].p + p.tail_at;
    return 0;
}

// ln det H = 2 sum_i ln L_ii, in index order; min_i L_ii^2
void flaplace_logdet(const double* ldiag, int m, double* logdet, double* min_pivot) {
    double s = 0.0, lo = m > 0 ? ldiag[0] : 0.0;
    for (int i = 0; i < m; ++i) {
        const double v = ldiag[i];
        s += std::log(v);
        lo = std::min(lo, v);
    }
    if (logdet) *logdet = 2.0 * s;
    if (min_pivot) *min_pivot = lo * lo;
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_laplace_forces_inverse(bioen_hip_ctx* c, const double* A, double* Ainv, double* logdet, int* info) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves point, session and device alone
    if (!info) return fail(BIOEN_HIP_EINVAL, "info is NULL");
    int rc;
    if ((rc = dense_guard(c, __func__, kLaplaceReasons)) || (rc = forces_guard(c))) return rc;
    if (!A && (rc = need_point(c, 1, __func__, &kLaplacePoint))) return rc;
    if ((rc = enter(c, FX_DEVICE, __func__))) return rc;
    if ((rc = fnewton_buffers(c)) || (rc = flaplace_buffers(c))) return rc;
    const double *src = fnewton_layout(c).A, *cov = nullptr;
    if (A) {
        if ((rc = h2d_user(c, fnewton_layout(c).A, A, (size_t)c->m * c->m * sizeof(double)))) return rc;
    } else if ((rc = flaplace_gram(c, &cov, &src))) {
        return rc;
    }
    std::vector<double> ldiag;
    if ((rc = flaplace_inverse(c, src, info, ldiag)) || *info) return rc;
    flaplace_logdet(ldiag.data(), c->m, logdet, nullptr);
    if (Ainv) {
        BIOEN_HIP_CHECK(d2h_user(c->stream, Ainv, flaplace_layout(c).Hi, (size_t)c->m * c->m * sizeof(double)));
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int bioen_laplace_forces(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* std_forces,
                                    double* std_averages, double* var_logw, double* cov_forces, double* cov_averages,
                                    double* logdet, double* min_pivot, int* info, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone ...
    if (forces && !w0) return fail(BIOEN_HIP_EINVAL, "forces without w0");
    if (!info) return fail(BIOEN_HIP_EINVAL, "info is NULL");
    int rc;
    if ((rc = dense_guard(c, __func__, kLaplaceReasons)) || (rc = forces_guard(c))) return rc;
    if ((rc = forces_point_prologue(c, forces, w0, theta, f, grad, __func__))) return rc;      // ... with forces it is an evaluation
    if ((rc = fnewton_buffers(c)) || (rc = flaplace_buffers(c))) return rc;
    const double *cov = nullptr, *hess = nullptr;
    if ((rc = flaplace_gram(c, &cov, &hess))) return rc;
    std::vector<double> ldiag;
    if ((rc = flaplace_inverse(c, hess, info, ldiag)) || *info) return rc;
    flaplace_logdet(ldiag.data(), c->m, logdet, min_pivot);
    const FLaplaceBuf b = flaplace_layout(c);
    const int m = c->m, mps = (int)round_up((size_t)c->m, 16);      // the strips' rows (M <= 1024: one panel)
    const size_t pcount = (size_t)mps * mps, mbytes = (size_t)m * sizeof(double);
    const bool averages = std_averages || cov_averages;
    if (averages) launch_flaplace_averages(c, b.W, b.ld, cov, b.B, b.ld, b.Ca);
    if ((rc = ensure_strip_copy(c, 1)) || (rc = ensure_scratch(c, SCRATCH_COLQUAD, pcount + c->ld))) return rc;
    double* buf = c->scratch[SCRATCH_COLQUAD].p;
    launch_flaplace_to_colquad(c, b.Hi, averages ? b.Ca : nullptr, c->affine ? c->row_scale : nullptr, buf, mps, b.dg, b.ld);
    if (var_logw) launch_forces_colquad(c, buf, c->fpoint_ybar, buf + pcount);
    if ((rc = check_launch())) return rc;
    std::vector<double> dg(2 * (size_t)m, 0.0);
    BIOEN_HIP_CHECK(hipMemcpyAsync(dg.data(), b.dg, mbytes, hipMemcpyDeviceToHost, c->stream));
    if (averages) BIOEN_HIP_CHECK(hipMemcpyAsync(dg.data() + m, b.dg + b.ld, mbytes, hipMemcpyDeviceToHost, c->stream));
    if (var_logw) BIOEN_HIP_CHECK(d2h_user(c->stream, var_logw, buf + pcount, (size_t)c->n * sizeof(double)));
    if (cov_forces) BIOEN_HIP_CHECK(d2h_user(c->stream, cov_forces, b.Hi, (size_t)m * mbytes));
    if (cov_averages) BIOEN_HIP_CHECK(d2h_user(c->stream, cov_averages, b.Ca, (size_t)m * mbytes));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; ++i) {
        if (std_forces) std_forces[i] = std::sqrt(dg[i]);
        if (std_averages) std_averages[i] = std::sqrt(std::max(dg[(size_t)m + i], 0.0));
    }
    return 0;
}

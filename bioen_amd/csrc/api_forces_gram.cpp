// The dense Hessian and the covariance of the forces objective in one pass, from FP64 operands -- bioen_hip_forces_gram; kernels: kernels_forces_gram.hip; DESIGN section 6e -- or
// from split-BF16 operands on the BF16 matrix cores, for a Newton minimizer -- bioen_hip_forces_gram_bf16; kernel:
// k_forces_gram_bf16, in the same file; DESIGN section 6g.  Two entries, not two modes of one: each pass has a buffer of its own,
// so that bioen_hip_forces_gram's results stay bitwise what they are.  Everything else is one function, fgram_entry; the
// point, the guard and the buffers are api_forces_point.cpp's.
#include "dense.hpp"

namespace bioen {

// C and H of the kept forces point into the buffer of `source` (0: the FP64 pass, SCRATCH_GRAM; 1: the split-BF16 pass,
// SCRATCH_GRAM16), not downloaded: *cov, *hess (either may be NULL) <- where they stand on the device.  The Newton
// entries (api_forces_newton.cpp) take their Hessian from here.
int fgram_compute(bioen_hip_ctx* c, int source, const double** cov, const double** hess) {
    int rc;
    if (!source) c->fgram_fresh = 0;
    if (forces_fused_blocks(c) <= 0) return fail(BIOEN_HIP_ESTATE, "the strip passes no longer serve this context");
    if ((rc = ensure_strip_copy(c, 1))) return rc;
    const GramPlan p = forces_gram_plan(c);
    const int which = source ? SCRATCH_GRAM16 : SCRATCH_GRAM;
    if ((rc = ensure_scratch(c, which, p.doubles))) return rc;
    double* buf = c->scratch[which].p;
    const ProblemSlot& s0 = c->slot[0];
    launch_forces_gram(c, p, buf, s0.a, s0.scal, c->fpoint_q, c->fpoint_ybar, c->point_theta, source != 0);
    if ((rc = check_launch())) return rc;
    if (!source) c->fgram_fresh = 1;                          // (bioen_laplace_forces at the same kept point takes them as they stand)
    if (cov) *cov = buf + p.cov_at;
    if (hess) *hess = buf + p.tail_at;
    return 0;
}

static int fgram_entry(bioen_hip_ctx* c, int source, const double* forces, const double* w0, double theta, double* cov,
                       double* hess, double* f, double* grad, const char* who) {
    if (int rc = enter(c, FX_NONE, who)) return rc;           // a call rejected below leaves the point (and the device) alone
    if (forces && !w0) return fail(BIOEN_HIP_EINVAL, "forces without w0");
    if (!forces && !cov && !hess) return fail(BIOEN_HIP_EINVAL, "nothing to do: no forces, no cov and no hess");
    int rc;
    if ((rc = dense_guard(c, who, kGramReasons)) || (rc = forces_guard(c))) return rc;
    if ((rc = forces_point_prologue(c, forces, w0, theta, f, grad, who))) return rc;
    if (!cov && !hess) return 0;
    const double *dcov = nullptr, *dhess = nullptr;
    if ((rc = fgram_compute(c, source, &dcov, &dhess))) return rc;
    const size_t bytes = (size_t)c->m * c->m * sizeof(double);
    if (cov) BIOEN_HIP_CHECK(hipMemcpyAsync(cov, dcov, bytes, hipMemcpyDeviceToHost, c->stream));
    if (hess) BIOEN_HIP_CHECK(hipMemcpyAsync(hess, dhess, bytes, hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace bioen

using namespace bioen;

extern "C" int bioen_hip_forces_gram(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* cov,
                                     double* hess, double* f, double* grad) {
    return fgram_entry(c, 0, forces, w0, theta, cov, hess, f, grad, __func__);
}

extern "C" int bioen_hip_forces_gram_bf16(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* cov,
                                          double* hess, double* f, double* grad) {
    return fgram_entry(c, 1, forces, w0, theta, cov, hess, f, grad, __func__);
}

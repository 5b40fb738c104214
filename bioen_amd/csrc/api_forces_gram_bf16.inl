// The dense Hessian of the forces objective for a Newton minimizer, from split-BF16 operands on the BF16 matrix cores
// (part of api.hip's translation unit: uses its static helpers; kernel: kernels_forces_gram_bf16.hip).
// An entry beside bioen_hip_forces_gram (api_forces_gram.inl), not a mode of it: point semantics and refusals are that
// entry's to the letter, the buffer is its own, and bioen_hip_forces_gram's results stay bitwise what they are.

namespace bioen {

// what the entry refuses, each with a message of its own (fgram_guard's set)
static int fgram16_guard(const bioen_hip_ctx* c) {
    if (c->world != 1)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_gram_bf16 is not served on a structure-sharded context (the all-gather "
                                      "of the segments' partial matrices is not built): use bioen_hip_forces_hessp there");
    if (c->m > 1024)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_gram_bf16 serves M <= 1024 only (beyond, the matrix is held as row "
                                      "panels): use bioen_hip_forces_hessp there");
    if (c->storage)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_gram_bf16 is not served on the reduced-storage experiment's copies "
                                      "(bioen_hip_ctx_set_storage(0))");
    if (forces_fused_blocks(c) <= 0)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_gram_bf16 needs the strip copies of the matrix: the streaming kernels "
                                      "have no Gram product");
    return 0;
}

}  // namespace bioen

extern "C" int bioen_hip_forces_gram_bf16(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* cov,
                                          double* hess, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone ...
    if (forces && !w0) return fail(BIOEN_HIP_EINVAL, "forces without w0");
    if (!forces && !cov && !hess) return fail(BIOEN_HIP_EINVAL, "nothing to do: no forces, no cov and no hess");
    int rc;
    if ((rc = fgram16_guard(c)) || (rc = forces_guard(c))) return rc;
    if (forces) {
        // ... with forces it is an evaluation: bioen_hip_forces_hessp's with k = 0, declared under this entry's name
        if ((rc = fhp_set_point(c, forces, w0, theta, f, grad, __func__))) return rc;
    } else {
        if (!c->point_valid || c->point_kind != 1) {
            std::string m;
            if (c->point_valid)
                m = "the point on this context is a log-weights point (set by bioen_hip_logw_hessp): call bioen_hip_forces_gram_bf16 with forces first";
            else if (c->point_lost)
                m = std::string("the point of the last call with forces (or g) is gone: dropped by ") + c->point_lost;
            else
                m = "no point on this context: call bioen_hip_forces_gram_bf16 with forces first";
            return fail(BIOEN_HIP_ESTATE, m.c_str());
        }
        if ((rc = enter(c, FX_DEVICE, __func__))) return rc;
    }
    if (!cov && !hess) return 0;
    if (forces_fused_blocks(c) <= 0) return fail(BIOEN_HIP_ESTATE, "the strip passes no longer serve this context");
    if ((rc = ensure_strip_copy(c, 1))) return rc;
    const ForcesGramPlan p = forces_gram_plan(c);
    if (!c->fgram16_buf) {
        if ((rc = dalloc_zero(&c->fgram16_buf, p.doubles, c->stream))) return rc;
        c->fgram16_bytes = (long long)(p.doubles * sizeof(double));
    }
    const ProblemSlot& s0 = c->slot[0];
    launch_forces_gram_bf16(c, p, c->fgram16_buf, s0.a, s0.scal, c->fpoint_q, c->fpoint_ybar, c->point_theta);
    if ((rc = check_launch())) return rc;
    const size_t bytes = (size_t)c->m * c->m * sizeof(double);
    if (cov) BIOEN_HIP_CHECK(hipMemcpyAsync(cov, c->fgram16_buf + p.cov_at, bytes, hipMemcpyDeviceToHost, c->stream));
    if (hess) BIOEN_HIP_CHECK(hipMemcpyAsync(hess, c->fgram16_buf + p.hess_at, bytes, hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// One quadratic form per structure at a kept forces point (part of api.hip's translation unit: uses its static helpers;
// kernel: kernels_forces_colquad.hip; the mathematics: DESIGN section 6f).  The point is bioen_hip_forces_hessp's
// (api_forces_hessp.inl: fhp_set_point), with bioen_hip_forces_gram's semantics.

namespace bioen {

// what the entry refuses, each with a message of its own (fgram_guard's set)
static int fcolquad_guard(const bioen_hip_ctx* c) {
    if (c->world != 1)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_colquad is not served on a structure-sharded context (a rank holds its "
                                      "own structures' columns only and the entry does not gather the results)");
    if (c->m > 1024)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_colquad serves M <= 1024 only (beyond, the matrix is held as row panels "
                                      "and a block cannot own all rows of its columns)");
    if (c->storage)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_colquad is not served on the reduced-storage experiment's copies "
                                      "(bioen_hip_ctx_set_storage(0))");
    if (forces_fused_blocks(c) <= 0)
        return fail(BIOEN_HIP_ESTATE, "bioen_hip_forces_colquad needs the strip copies of the matrix: the streaming kernels have "
                                      "no quadratic form");
    return 0;
}

// |P_ij - P_ji| <= 1e-12 max |P| (an inverse formed in floating point is symmetric to rounding, not bit for bit)
static bool fcolquad_symmetric(const double* P, int m) {
    double top = 0.0, skew = 0.0;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) {
            const double a = P[(size_t)i * m + j], b = P[(size_t)j * m + i];
            top = std::max(top, std::max(std::fabs(a), std::fabs(b)));
            skew = std::max(skew, std::fabs(a - b));
        }
    return !(skew > 1e-12 * top);      // (non-finite entries are the caller's business)
}

}  // namespace bioen

extern "C" int bioen_hip_forces_colquad(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, const double* P,
                                        double* out, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone ...
    if (forces && !w0) return fail(BIOEN_HIP_EINVAL, "forces without w0");
    if (!forces && !P) return fail(BIOEN_HIP_EINVAL, "nothing to do: no forces and no P");
    if (P && !out) return fail(BIOEN_HIP_EINVAL, "P without out");
    if (P && !fcolquad_symmetric(P, c->m)) return fail(BIOEN_HIP_EINVAL, "P is not symmetric");
    int rc;
    if ((rc = fcolquad_guard(c)) || (rc = forces_guard(c))) return rc;
    if (forces) {
        // ... with forces it is an evaluation: bioen_hip_forces_hessp's with k = 0, declared under this entry's name
        if ((rc = fhp_set_point(c, forces, w0, theta, f, grad, __func__))) return rc;
    } else {
        if (!c->point_valid || c->point_kind != 1) {
            std::string m;
            if (c->point_valid)
                m = "the point on this context is a log-weights point (set by bioen_hip_logw_hessp): call bioen_hip_forces_colquad with forces first";
            else if (c->point_lost)
                m = std::string("the point of the last call with forces (or g) is gone: dropped by ") + c->point_lost;
            else
                m = "no point on this context: call bioen_hip_forces_colquad with forces first";
            return fail(BIOEN_HIP_ESTATE, m.c_str());
        }
        if ((rc = enter(c, FX_DEVICE, __func__))) return rc;
    }
    if (!P) return 0;
    if (forces_fused_blocks(c) <= 0) return fail(BIOEN_HIP_ESTATE, "the strip passes no longer serve this context");
    if ((rc = ensure_strip_copy(c, 1))) return rc;
    const int m = c->m, mps = (int)round_up((size_t)c->m, 16);      // the strips' rows (M <= 1024: one panel)
    const size_t pcount = (size_t)mps * mps;
    if (!c->fcolquad_buf) {
        if ((rc = dalloc_zero(&c->fcolquad_buf, pcount + c->ld, c->stream))) return rc;
        c->fcolquad_bytes = (long long)((pcount + c->ld) * sizeof(double));
    }
    // P_eff = S P S on the symmetric part of P, padded with zeros to the strip rows: element (i, j) is
    // ((P_ij + P_ji) / 2) (s_i s_j) -- bitwise symmetric, and P_ij itself for an exactly symmetric P and scales of 1
    std::vector<double> sc((size_t)m, 1.0);
    if (c->affine) {
        BIOEN_HIP_CHECK(hipMemcpyAsync(sc.data(), c->row_scale, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    std::vector<double> pe(pcount, 0.0);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = (0.5 * (P[(size_t)i * m + j] + P[(size_t)j * m + i])) * (sc[i] * sc[j]);
            pe[(size_t)i * mps + j] = v;
            pe[(size_t)j * mps + i] = v;
        }
    BIOEN_HIP_CHECK(hipMemcpyAsync(c->fcolquad_buf, pe.data(), pcount * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));         // (pe is pageable and leaves scope)
    launch_forces_colquad(c, c->fcolquad_buf, c->fpoint_ybar, c->fcolquad_buf + pcount);
    if ((rc = check_launch())) return rc;
    BIOEN_HIP_CHECK(hipMemcpyAsync(out, c->fcolquad_buf + pcount, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

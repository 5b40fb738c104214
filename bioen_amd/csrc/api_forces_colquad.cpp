// One quadratic form per structure at a kept forces point (kernel: kernels_forces_colquad.hip; the mathematics: DESIGN
// section 6f).  The point, the guard and the buffer are api_forces_point.cpp's: forces_point_prologue, dense_guard with
// this entry's reasons, ensure_scratch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dense.hpp"

namespace bioen {

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

using namespace bioen;

extern "C" int bioen_hip_forces_colquad(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, const double* P,
                                        double* out, double* f, double* grad) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;      // a call rejected below leaves the point (and the device) alone ...
    if (forces && !w0) return fail(BIOEN_HIP_EINVAL, "forces without w0");
    if (!forces && !P) return fail(BIOEN_HIP_EINVAL, "nothing to do: no forces and no P");
    if (P && !out) return fail(BIOEN_HIP_EINVAL, "P without out");
    if (P && !fcolquad_symmetric(P, c->m)) return fail(BIOEN_HIP_EINVAL, "P is not symmetric");
    int rc;
    if ((rc = dense_guard(c, __func__, kColquadReasons)) || (rc = forces_guard(c))) return rc;
    if ((rc = forces_point_prologue(c, forces, w0, theta, f, grad, __func__))) return rc;      // ... with forces it is an evaluation
    if (!P) return 0;
    if (forces_fused_blocks(c) <= 0) return fail(BIOEN_HIP_ESTATE, "the strip passes no longer serve this context");
    if ((rc = ensure_strip_copy(c, 1))) return rc;
    const int m = c->m, mps = (int)round_up((size_t)c->m, 16);      // the strips' rows (M <= 1024: one panel)
    const size_t pcount = (size_t)mps * mps;
    if ((rc = ensure_scratch(c, SCRATCH_COLQUAD, pcount + c->ld))) return rc;
    double* buf = c->scratch[SCRATCH_COLQUAD].p;
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
    BIOEN_HIP_CHECK(hipMemcpyAsync(buf, pe.data(), pcount * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));         // (pe is pageable and leaves scope)
    launch_forces_colquad(c, buf, c->fpoint_ybar, buf + pcount);
    if ((rc = check_launch())) return rc;
    BIOEN_HIP_CHECK(hipMemcpyAsync(out, buf + pcount, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

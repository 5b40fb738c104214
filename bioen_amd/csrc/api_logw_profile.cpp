// The log-weights dual Newton theta series with the nuisance scales profiled out (kernels: kernels_logw_profile.hip; DESIGN
// section 6m).  The loop is api_logw_newton.cpp's logwn_loop as it is: while c->profile_groups is set every evaluation's
// launch_rows_combine forms the groups' least-squares scales from the raw averages and writes sigma into c->row_scale
// before the residual, and the loop projects C_A and -b_A behind k_lgram_finish.  The selection is set here on entry and
// cleared on every way out, so no other entry's launches change; what stays is the affine model (row_offset, sigma of the
// last theta's returned point) and that point as the context's kept log-weights point.
#include <cmath>
#include <vector>

#include "dense.hpp"

using namespace bioen;

namespace {

struct ProfileSelection {      // cleared on every way out of the entry
    bioen_hip_ctx* c;
    ProfileSelection(bioen_hip_ctx* ctx, int ngroups) : c(ctx) { c->profile_groups = ngroups; }
    ~ProfileSelection() { c->profile_groups = 0; }
};

}  // namespace

extern "C" int bioen_logwn_profile_series(bioen_hip_ctx* c, const double* g0, const double* G, const double* thetas, int ntheta,
                                          const bioen_logwn_config* cfg, int source, int warm, const double* row_offset,
                                          const int* group, int ngroups, double* gopt, double* scales, double* chi2,
                                          double* kl, bioen_logwn_series_result* results) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (!g0 || !G || !thetas || !cfg || !group || !gopt || !scales || !results) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (ntheta < 1) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_profile_series needs ntheta >= 1");
    if (source != LOGWN_FP64 && source != LOGWN_BF16)
        return fail(BIOEN_HIP_EINVAL, "bioen_logwn_profile_series: source is 0 (FP64) or 1 (split BF16)");
    if (warm != 0 && warm != 1) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_profile_series: warm is 0 or 1");
    if (ngroups < 1 || ngroups > 64) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_profile_series: ngroups is 1 .. 64");
    int rc;
    if ((rc = logwn_check(cfg, thetas, ntheta, __func__))) return rc;
    std::vector<int> grp(c->mp, -1), rows(ngroups, 0);
    for (int i = 0; i < c->m; ++i) {
        if (group[i] < -1 || group[i] >= ngroups)
            return fail(BIOEN_HIP_EINVAL, "bioen_logwn_profile_series: a group id outside -1 .. ngroups - 1");
        grp[i] = group[i];
        if (group[i] >= 0) ++rows[group[i]];
    }
    for (int k = 0; k < ngroups; ++k)
        if (!rows[k]) return fail(BIOEN_HIP_EINVAL, "bioen_logwn_profile_series: a group without rows");
    if ((rc = dense_guard(c, __func__, kLogwnReasons, fwd_strip_blocks))) return rc;
    if ((rc = enter(c, FX_EVALUATES, __func__))) return rc;

    if ((rc = ensure_scratch(c, SCRATCH_LOGW_PROFILE, logw_profile_doubles(c)))) return rc;
    const LogwProfileBuf pb = logw_profile_layout(c, c->scratch[SCRATCH_LOGW_PROFILE].p);
    // the model: the offset as given, the scales 1 until the first evaluation writes them
    std::vector<double> off(c->mp, 0.0), one(c->mp, 1.0);
    if (row_offset)
        for (int i = 0; i < c->m; ++i) off[i] = row_offset[i];
    BIOEN_HIP_CHECK(hipMemcpyAsync(pb.group, grp.data(), (size_t)c->mp * sizeof(int), hipMemcpyHostToDevice, c->stream));
    BIOEN_HIP_CHECK(hipMemcpyAsync(c->row_offset, off.data(), (size_t)c->mp * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BIOEN_HIP_CHECK(hipMemcpyAsync(c->row_scale, one.data(), (size_t)c->mp * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->affine = true;
    const ProfileSelection selected(c, ngroups);

    ProblemSlot& s0 = c->slot[0];
    if ((rc = upload_n(c, s0.xp, g0))) return rc;
    if ((rc = upload_n(c, c->fixed, G))) return rc;
    // cold: g0 waits in slot 0's gp, which neither the evaluations nor the step write
    if (!warm) BIOEN_HIP_CHECK(hipMemcpyAsync(s0.gp, s0.xp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    for (int k = 0; k < ntheta; ++k) {
        if (!warm && k > 0) BIOEN_HIP_CHECK(hipMemcpyAsync(s0.xp, s0.gp, c->ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if ((rc = logwn_loop(c, thetas[k], cfg, source, &results[k], __func__))) return rc;
        if ((rc = download_n(c, gopt + (size_t)k * c->n, s0.xp))) return rc;
        // the loop's last evaluation was the returned point's: its scales, and its scalars in host_scal
        BIOEN_HIP_CHECK(hipMemcpyAsync(scales + (size_t)k * ngroups, pb.scales, (size_t)ngroups * sizeof(double),
                                       hipMemcpyDeviceToHost, c->stream));
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (chi2) chi2[k] = 0.5 * c->host_scal[S_CHI];
        if (kl) kl[k] = c->host_scal[S_KL];
    }
    return 0;
}

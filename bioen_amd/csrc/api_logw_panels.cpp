// The switch of the log-weights dense entries' pass over row panels.  Off, every dense entry serves
// M <= 1024 and refuses beyond, as it always did; on, dense_guard (api_forces_point.cpp) lets bioen_logwn_cov,
// bioen_logwn_cov_bf16, bioen_logwn_opt and bioen_logwn_series through up to kDensePanelRows rows, where launch_logw_gram
// takes k_logw_gram_panels / k_logw_gram_bf16_panels (kernels_logw_newton.hip) and launch_fnewton_solve the wide solve
// (kernels_forces_newton.hip).  A setting only: the point and a session stay, nothing runs on the device.
#include "dense.hpp"

using namespace bioen;

extern "C" int bioen_hip_ctx_set_dense_panels(bioen_hip_ctx* c, int on) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (on != 0 && on != 1) return fail(BIOEN_HIP_EINVAL, "bioen_hip_ctx_set_dense_panels: on is 0 or 1");
    c->dense_panels = on;
    return 0;
}

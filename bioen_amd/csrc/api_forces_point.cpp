// What the entries that work at a kept point share (declared in dense.hpp, for api_hessp.cpp, the api_forces_*.cpp files
// and api_logw_newton.cpp): the refusal without a point of the right kind, the prologues of the entries that set a point or
// serve the kept one -- the forces entries' and the log-weights entries' --, the guard of the dense entries (M <= 1024, one
// GPU, the FP64 strip copies) and the scratch buffers the context keeps for them.  DESIGN section 6c has the rules.
#include <string>

#include "dense.hpp"

namespace bioen {

// 0 if the context keeps a point of `kind` (0: log-weights, 1: forces), else BIOEN_HIP_ESTATE and why there is none: it is
// the other method's, it was dropped (by what), or none was ever set
int need_point(const bioen_hip_ctx* c, int kind, const char* who, const PointWords* words) {
    if (c->point_valid && c->point_kind == kind) return 0;
    static const struct { const char *name, *setter, *arg, *last; } kKind[2] = {
        {"log-weights", "bioen_hip_logw_hessp", "g", "bioen_hip_logw_hessp call with g"},
        {"forces", "bioen_hip_forces_hessp", "forces", "call with forces (or g)"}};
    const std::string pre = words ? std::string(who) + ": " : std::string();
    const std::string remedy = words ? std::string(words->remedy) : std::string("call ") + who + " with " + kKind[kind].arg + " first";
    std::string m;
    if (c->point_valid)
        m = pre + "the point on this context is a " + kKind[!kind].name + " point (set by " + kKind[!kind].setter + "): " + remedy;
    else if (c->point_lost)
        m = pre + "the point of the last " + (words ? words->last : kKind[kind].last) + " is gone: dropped by " + c->point_lost;
    else
        m = pre + "no point on this context: " + remedy;
    return fail(BIOEN_HIP_ESTATE, m.c_str());
}

// The point of a forces entry `who`: with forces it is an evaluation -- bioen_hip_forces_hessp's with k = 0, declared under
// the entry's name -- that leaves a new point; without, the kept forces point serves, and the call only works on the device
int forces_point_prologue(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* f, double* grad,
                          const char* who) {
    if (forces) return fhp_set_point(c, forces, w0, theta, f, grad, who);
    if (int rc = need_point(c, 1, who)) return rc;
    return enter(c, FX_DEVICE, who);
}

// Slot 0's x (and c->fixed = G) hold a log-weights point: bioen_hip_logw_fdf's evaluation of it, launch for launch, after
// which it is the context's kept point.  k: the directions hessp_buffers provides for
int logw_keep_point(bioen_hip_ctx* c, double theta, int k, double* f, double* grad) {
    int rc;
    c->point_lost = "a call that failed to set a new point";
    if ((rc = hessp_buffers(c, k))) return rc;
    const int one[1] = {0};
    if ((rc = eval_logw_point(c, make_round(c, one, 1, nullptr, &theta), true, true, f, grad))) return rc;
    c->point_theta = theta;
    c->point_kind = 0;
    c->point_valid = 1;
    c->point_lost = nullptr;
    return 0;
}

// The point of a log-weights entry `who`, as forces_point_prologue: with g it is an evaluation at (g, G), declared under the
// entry's name, that leaves a new point; without, the kept log-weights point serves
int logw_point_prologue(bioen_hip_ctx* c, const double* g, const double* G, double theta, int k, double* f, double* grad,
                        const char* who, const PointWords* words) {
    int rc;
    if (!g) return (rc = need_point(c, 0, who, words)) ? rc : enter(c, FX_DEVICE, who);
    if ((rc = enter(c, FX_EVALUATES, who))) return rc;
    ProblemSlot& s0 = c->slot[0];
    if ((rc = upload_n(c, s0.x, g)) || (rc = upload_n(c, c->fixed, G))) return rc;
    BIOEN_HIP_CHECK(hipMemsetAsync(s0.d, 0, c->ld * sizeof(double), c->stream));
    return logw_keep_point(c, theta, k, f, grad);
}

// What the dense entries refuse, each with a message of its own: the frame is shared, an entry's reasons fill it
const DenseReasons kGramReasons = {
    "the all-gather of the segments' partial matrices is not built): use bioen_hip_forces_hessp there",
    "): use bioen_hip_forces_hessp there", "Gram product"};
const DenseReasons kColquadReasons = {
    "a rank holds its own structures' columns only and the entry does not gather the results)",
    " and a block cannot own all rows of its columns)", "quadratic form"};
const DenseReasons kNewtonReasons = {
    "the Hessian pass is not built there): use the L-BFGS, or bioen_hip_forces_hessp with a host driver",
    " and there is no dense Hessian pass): use the L-BFGS there", "Gram product"};
const DenseReasons kLogwnReasons = {
    "the all-gather of the segments' partial matrices is not built): use the L-BFGS there",
    " and there is no Gram pass over them): use the L-BFGS there", "Gram product"};

// strip_blocks: the strip passes whose copy the entry reads -- the forces method's, or fwd_strip_blocks for the log-weights
// entries
int dense_guard(const bioen_hip_ctx* c, const char* who, const DenseReasons& why, int (*strip_blocks)(const bioen_hip_ctx*),
                bool over_panels) {
    const std::string w(who);
    if (c->world != 1)
        return fail(BIOEN_HIP_ESTATE, (w + " is not served on a structure-sharded context (" + why.sharded).c_str());
    if (c->m > 1024 && !(over_panels && c->dense_panels))
        return fail(BIOEN_HIP_ESTATE, (w + " serves M <= 1024 only (beyond, the matrix is held as row panels" + why.panels).c_str());
    if (c->m > kDensePanelRows)
        return fail(BIOEN_HIP_ESTATE, (w + " serves M <= 4096 over row panels (bioen_hip_ctx_set_dense_panels): use the L-BFGS "
                                           "beyond").c_str());
    if (c->storage)
        return fail(BIOEN_HIP_ESTATE, (w + " is not served on the reduced-storage experiment's copies "
                                           "(bioen_hip_ctx_set_storage(0))").c_str());
    if (strip_blocks(c) <= 0)
        return fail(BIOEN_HIP_ESTATE, (w + " needs the strip copies of the matrix: the streaming kernels have no " +
                                       why.product).c_str());
    return 0;
}

// A scratch buffer of the context (ctx.hpp: CtxScratch): allocated, zeroed, at its first use, kept until the context goes
int ensure_scratch(bioen_hip_ctx* c, int which, size_t doubles) {
    CtxScratchBuf& s = c->scratch[which];
    if (s.p) return 0;
    if (int rc = dalloc_zero(&s.p, doubles, c->stream)) return rc;
    s.bytes = (long long)(doubles * sizeof(double));
    return 0;
}

}  // namespace bioen

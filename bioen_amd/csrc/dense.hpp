// What the second-order entries share among their translation units (api_hessp.cpp, api_forces_*.cpp, api_logw_newton.cpp),
// beyond host.hpp: the kept point's refusal and prologues, the guard and the scratch buffers of the dense entries
// (definitions: api_forces_point.cpp), and the pieces one entry's file lends to another's -- the forces point and its guard,
// the Hessian pass, the Cholesky factor.  Hidden, like host.hpp; what a file does not share is static in it.  DESIGN
// section 6c has the rules.
#pragma once

#include "host.hpp"
#include "kernels.hpp"

#pragma GCC visibility push(hidden)
namespace bioen {

// ---- the kept point (api_forces_point.cpp) ----------------------------------------------------------------------------------
// Where an entry's refusal without a point reads differently from the kind's own, it stands behind "<who>: " with these
// words: last, the call whose point is gone; remedy, what to do about it
struct PointWords {
    const char *last, *remedy;
};

// 0 if the context keeps a point of `kind` (0: log-weights, 1: forces), else BIOEN_HIP_ESTATE and why there is none: it is
// the other method's, it was dropped (by what), or none was ever set
int need_point(const bioen_hip_ctx* c, int kind, const char* who, const PointWords* words = nullptr);

// The point of a forces entry `who`: with forces it is an evaluation -- bioen_hip_forces_hessp's with k = 0, declared under
// the entry's name -- that leaves a new point; without, the kept forces point serves, and the call only works on the device
int forces_point_prologue(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* f, double* grad,
                          const char* who);

// Slot 0's x (and c->fixed = G) hold a log-weights point: bioen_hip_logw_fdf's evaluation of it, launch for launch, after
// which it is the context's kept point.  k: the directions hessp_buffers provides for
int logw_keep_point(bioen_hip_ctx* c, double theta, int k, double* f, double* grad);

// The point of a log-weights entry `who`, as forces_point_prologue: with g it is an evaluation at (g, G), declared under the
// entry's name, that leaves a new point; without, the kept log-weights point serves
int logw_point_prologue(bioen_hip_ctx* c, const double* g, const double* G, double theta, int k, double* f, double* grad,
                        const char* who, const PointWords* words = nullptr);

// ---- the dense entries' guard and buffers (api_forces_point.cpp) ------------------------------------------------------------
// What the dense entries refuse, each with a message of its own: the frame is shared, an entry's reasons fill it
struct DenseReasons {
    const char *sharded, *panels, *product;
};
extern const DenseReasons kGramReasons, kColquadReasons, kNewtonReasons, kLogwnReasons;

// M <= 1024, one GPU, the FP64 strip copies.  strip_blocks: the strip passes whose copy the entry reads -- the forces
// method's, or fwd_strip_blocks for the log-weights entries.  over_panels: the entry has a pass over row panels (DESIGN 6n:
// the log-weights covariance and dual Newton entries) -- on a context with bioen_hip_ctx_set_dense_panels it serves
// M <= kDensePanelRows
int dense_guard(const bioen_hip_ctx* c, const char* who, const DenseReasons& why,
                int (*strip_blocks)(const bioen_hip_ctx*) = forces_fused_blocks, bool over_panels = false);

// A scratch buffer of the context (ctx.hpp: CtxScratch): allocated, zeroed, at its first use, kept until the context goes
int ensure_scratch(bioen_hip_ctx* c, int which, size_t doubles);

// ---- the log-weights point's buffers (api_hessp.cpp) ------------------------------------------------------------------------
int hessp_buffers(bioen_hip_ctx* c, int k);      // what the kept point and k directions of products on it need

// ---- the forces point (api_forces_hessp.cpp) --------------------------------------------------------------------------------
// Evaluates the point and keeps it on the context, for the entry `who`: the effects are declared under that name
int fhp_set_point(bioen_hip_ctx* c, const double* forces, const double* w0, double theta, double* f, double* grad,
                  const char* who);
// what bioen_hip_forces_hessp refuses beyond forces_guard: everything but the fused strip passes on the FP64 copy
int fhp_guard(const bioen_hip_ctx* c);

// ---- the Hessian pass (api_forces_gram.cpp) ---------------------------------------------------------------------------------
// C and H of the kept forces point into the buffer of `source` (0: the FP64 pass, SCRATCH_GRAM; 1: the split-BF16 pass,
// SCRATCH_GRAM16), not downloaded: *cov, *hess (either may be NULL) <- where they stand on the device
int fgram_compute(bioen_hip_ctx* c, int source, const double** cov, const double** hess);

// ---- the Cholesky factor on the device (api_forces_newton.cpp) --------------------------------------------------------------
struct FNewtonBuf {
    double *L, *A, *X, *dg;
    int* info;
    int ldl;
};
FNewtonBuf fnewton_layout(const bioen_hip_ctx* c);      // where the parts of SCRATCH_NEWTON stand
int fnewton_buffers(bioen_hip_ctx* c);
// chol(lower(src) + lambda I) -> the context's L; *info as LAPACK's; dmax (may be NULL): max |diag src|
int fnewton_factor(bioen_hip_ctx* c, const double* src, double lambda, int* info, double* dmax);

// ---- from the factor to its inverse (api_forces_laplace.cpp) ----------------------------------------------------------------
struct FLaplaceBuf {
    double *W, *Hi, *B, *Ca;      // L^-1 and a work matrix (leading dimension ld); the inverse and a covariance (m x m, dense)
    double *ldiag, *dg;           // diag L; diag of the inverse, then (at dg + ld) diag of the covariance
    int ld;
};
FLaplaceBuf flaplace_layout(const bioen_hip_ctx* c);      // where the parts of SCRATCH_LAPLACE stand
int flaplace_buffers(bioen_hip_ctx* c);
// ln det = 2 sum_i ln L_ii, in index order; min_i L_ii^2 (either may be NULL); ldiag: m values on the host
void flaplace_logdet(const double* ldiag, int m, double* logdet, double* min_pivot);

// ---- the covariance of the kept log-weights point (api_logw_newton.cpp) -----------------------------------------------------
extern const PointWords kLogwnPoint;      // the refusal without a log-weights point, as the bioen_logwn_* entries word it
// after a point's evaluation the guard once more (the strip copies exist by now, or never will)
// (over_panels: dense_guard's)
int logwn_copies(const bioen_hip_ctx* c, const char* who, bool over_panels = false);
// C of the kept log-weights point into SCRATCH_LOGW_GRAM, not downloaded (source 0: the FP64 pass, 1: the split-BF16 one);
// negb (may be NULL): -Yc grad
int logwn_gram(bioen_hip_ctx* c, int source, const double** cov, double* negb);
// the covariance's source: the FP64 pass (k_logw_gram) or the split-BF16 one (k_logw_gram_bf16)
enum LogwnSource : int { LOGWN_FP64 = 0, LOGWN_BF16 = 1 };
// what the dual Newton entries refuse before the device, the point or a session are touched: the config, a theta <= 0
int logwn_check(const bioen_logwn_config* cfg, const double* thetas, int ntheta, const char* who);
// the dual Newton loop for one theta from the point slot 0's xp holds (c->fixed = G); leaves the returned point in xp,
// evaluated and kept; every status returns 0
int logwn_loop(bioen_hip_ctx* c, double theta, const bioen_logwn_config* cfg, int source, bioen_logwn_series_result* res,
               const char* who);

}  // namespace bioen
#pragma GCC visibility pop

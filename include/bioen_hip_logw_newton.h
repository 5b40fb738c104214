/* bioen_hip_logw_newton.h -- the log-weights method's dual Newton minimizer: the N log-weights through an M x M system that
 * is formed, factorised (FP64 Cholesky) and solved in device memory, and the covariance of the observables under the
 * refined weights it is built on.  The part of the C ABI of libbioen_hip that is declared beside bioen_hip.h and the six
 * forces headers (same library, same conventions: plain C, host buffers owned by the caller, 0 or a negative BIOEN_HIP_E*
 * code).  The bioen_hip_* and bioen_laplace_* names are closed over the earlier headers; this one's entries are
 * bioen_logwn_*, bound by bioen_amd/_lib.py in a table of their own (_SIGNATURES_LOGW_NEWTON).  DESIGN section 6j.
 *
 * Both entries are refused with BIOEN_HIP_ESTATE, each case with a message of its own, on m > 1024 (row panels), on contexts
 * without the strip copies, on the reduced-storage experiment's copies and on structure-sharded contexts.
 */
#ifndef BIOEN_HIP_LOGW_NEWTON_H
#define BIOEN_HIP_LOGW_NEWTON_H

#include "bioen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C = sum_j w_j (y_j - ybar)(y_j - ybar)^T, w = softmax(g): the covariance of the (affine model: effective) observables
 * under the weights of a log-weights point, m x m row-major, bitwise symmetric; the same bits call after call.
 *   g != NULL: an evaluation (bioen_hip_logw_hessp's with k = 0: the same f and grad, both optional) that leaves g as the
 *              context's kept log-weights point; G [n] is required then.  C may be NULL: the call only sets the point.
 *   g == NULL: serves the kept log-weights point (set by this entry, by bioen_hip_logw_hessp or by bioen_logwn_opt);
 *              BIOEN_HIP_ESTATE without one, naming what dropped it.  G, theta, f and grad are ignored.
 * The device buffer of the pass is this header's own, allocated at the first call that computes C and freed with the
 * context (bioen_hip_ctx_footprint: bit 10). */
int bioen_logwn_cov(bioen_hip_ctx* ctx, const double* g, const double* G, double theta, double* C, double* f, double* grad);

typedef struct {
    double gtol;            /* ends with status 0 when max |grad_k| <= gtol * max w_k (and max |gamma_k| <= theta) */
    double armijo;          /* a step alpha u is accepted when f+ - f <= armijo * alpha * grad . u                (1e-4) */
    double floor_ulps;      /* |alpha grad . u| <= floor_ulps * epsilon * |f|: f cannot judge the step, max |grad| does (8) */
    int max_iterations;     /* accepted steps; status 1 when reached */
    int max_halvings;       /* trials of one step, alpha = 1, 1/2, ...; status 3 when exhausted                   (60) */
} bioen_logwn_config;

typedef struct {
    double fmin;            /* objective at the returned log-weights */
    double gmax;            /* max |grad_k| there */
    double wmax;            /* max w_k there */
    int status;             /* 0: the gradient test; 1: max_iterations; 2: a step at the rounding floor of f did not lower
                               max |grad|; 3: the step was exhausted elsewhere (or C + theta I did not factorise) */
    int iterations;         /* accepted steps */
    int evaluations;        /* evaluations of f and grad (status 2, 3: one more than the trials, to restore the point) */
    int factorisations;
} bioen_logwn_result;

/* The dual Newton minimizer of the log-weights objective from g0 [n] with the prior G [n] (DESIGN 6j has the loop;
 * log_weights.py's dual_newton_bioen_log_posterior_base restates it in numpy, decision for decision): per iteration one
 * covariance pass, one factorisation of C + theta I and one solve on the device, one centred adjoint pass, and one
 * evaluation per trial; every N-vector stays in device memory.  theta > 0 is required (BIOEN_HIP_EINVAL otherwise: the step
 * divides by theta).  gopt [n] (required) is in the gauge the steps leave it in: compare weights, not g.  Returns 0 with
 * every status; the returned point is then the context's kept log-weights point (bioen_logwn_cov and bioen_hip_logw_hessp
 * without g serve it at once).  Ends a BFGS session. */
int bioen_logwn_opt(bioen_hip_ctx* ctx, const double* g0, const double* G, double theta, const bioen_logwn_config* config,
                    double* gopt, bioen_logwn_result* result);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_LOGW_NEWTON_H */

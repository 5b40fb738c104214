/* bioen_hip_forces_newton.h -- the forces method's own Newton minimizer: the dense Hessian stays in device memory, is
 * factorised (FP64 Cholesky) and solved there, and the loop runs behind one call.  The part of the C ABI of libbioen_hip
 * that is declared beside bioen_hip.h and the four forces headers (same library, same conventions: plain C, host buffers
 * owned by the caller, 0 or a negative BIOEN_HIP_E* code).  INTEGRATION.md says why it is a header of its own;
 * bioen_amd/_lib.py binds it in a sixth table (_SIGNATURES_FORCES_NEWTON).
 *
 * All three entries are refused with BIOEN_HIP_ESTATE, each case with a message of its own, where
 * bioen_hip_forces_gram_bf16 is: m > 1024 (row panels), contexts without the strip copies, the reduced-storage
 * experiment's copies, structure-sharded contexts.
 */
#ifndef BIOEN_HIP_FORCES_NEWTON_H
#define BIOEN_HIP_FORCES_NEWTON_H

#include "bioen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A + lambda I = L L^T, L lower triangular, on the device (blocked, right-looking, panels of 64; the trailing update on
 * the FP64 matrix cores).  Only the lower triangle of the matrix is read.
 *   A != NULL: an m x m row-major host matrix (source is ignored).
 *   A == NULL: the Hessian of the kept forces point, computed now on the device and not downloaded -- source 0:
 *              bioen_hip_forces_gram's H, source 1: bioen_hip_forces_gram_bf16's.  Refused with BIOEN_HIP_ESTATE without
 *              a forces point.
 * *info (required) is LAPACK dpotrf's: 0 and L is complete, or k + 1 where pivot k was <= 0 or not finite -- an ordinary
 * result (the call returns 0), after which no kernel of the factorisation has touched the rest of the matrix.  L (may be
 * NULL): m x m row-major, zeros above the diagonal; written only when *info == 0.  The order of every sum is a function
 * of m alone: the same bits in give the same bits out.  Keeps point and session.  The device buffer of L is this
 * header's own, allocated at the first call and freed with the context (bioen_hip_ctx_footprint: bit 8). */
int bioen_hip_forces_newton_factor(bioen_hip_ctx* ctx, const double* A, int source, double lambda, double* L, int* info);

/* X = (L L^T)^-1 B with the factor of the last bioen_hip_forces_newton_factor call; B, X: [k][m], 1 <= k <= 8 (they may
 * be the same buffer).  A right-hand side's result does not depend on k.  BIOEN_HIP_ESTATE if there is no factor, or if
 * the last factorisation ended with info != 0.  Keeps point and session. */
int bioen_hip_forces_newton_solve(bioen_hip_ctx* ctx, int k, const double* B, double* X);

typedef struct {
    double gtol;            /* ends with status 0 when max |g_i| <= gtol */
    double armijo;          /* a step is accepted when f+ - f <= -armijo * pred                          (1e-4) */
    double rho_good;        /* lambda shrinks after a step with (f - f+) / pred above this               (0.75) */
    double lambda_factor;   /* lambda grows and shrinks by this factor                                   (4)    */
    double lambda_first;    /* the first lambda > 0, in units of d = max |diag H|                        (1e-10) */
    double lambda_max;      /* status 3 when lambda exceeds this many d                                  (1e10) */
    double lambda_zero;     /* a lambda below this many d becomes 0                                      (1e-12) */
    double floor_ulps;      /* pred <= floor_ulps * epsilon * |f|: f cannot judge the step, max |g| does  (8)    */
    int max_iterations;     /* accepted steps; status 1 when reached */
    int hessian;            /* 0: bioen_hip_forces_gram's H, 1: bioen_hip_forces_gram_bf16's */
} bioen_newton_config;

typedef struct {
    double fmin;            /* objective at the returned forces */
    double gmax;            /* max |g_i| there */
    double lambda;          /* the final damping */
    int status;             /* 0: max|g| <= gtol; 1: max_iterations; 2: at the minimum to the rounding of f (a step at the
                               rounding floor did not lower max|g|); 3: lambda grew beyond lambda_max * d */
    int iterations;         /* accepted steps */
    int evaluations;        /* evaluations of f and g (each two matrix passes and the point's one) */
    int hessians;           /* Hessian passes */
    int factorisations;
    int switched;           /* 1: the run began with hessian = 1 and went over to 0 at the rounding floor */
} bioen_newton_result;

/* Regularised Newton on the forces objective from forces0 [m] (DESIGN 6h has the loop; forces.py's
 * newton_bioen_log_posterior_base restates it in numpy, decision for decision): H at the kept point from `hessian`,
 * H + lambda I factorised and solved on the device -- only m doubles go down and m come up per step --, the trial
 * evaluated as bioen_hip_forces_hessp evaluates a point, so that an accepted trial is the kept point of the next Hessian.
 * forces_out [m] (required), weights_out [n] (may be NULL), result (required).  Returns 0 with every status; the
 * returned point is then the context's kept point (bioen_hip_forces_gram and bioen_hip_forces_colquad serve it at once).
 * Ends a BFGS session. */
int bioen_hip_opt_newton_forces(bioen_hip_ctx* ctx, const double* forces0, const double* w0, double theta,
                                const bioen_newton_config* config, double* forces_out, double* weights_out,
                                bioen_newton_result* result);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_FORCES_NEWTON_H */

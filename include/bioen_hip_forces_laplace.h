/* bioen_hip_forces_laplace.h -- the Laplace error bars of the forces method without leaving the device: the dense Hessian
 * of bioen_hip_forces_gram is factorised where it stands (the kernels of bioen_hip_forces_newton_factor), inverted from
 * the factor, and the inverse is handed to the quadratic-form pass of bioen_hip_forces_colquad in device memory.  Only
 * what the caller asks for is downloaded: O(M + N) doubles per point for the error bars themselves.  The part of the C
 * ABI of libbioen_hip that is declared beside bioen_hip.h and the five forces headers (same library, same conventions:
 * plain C, host buffers owned by the caller, 0 or a negative BIOEN_HIP_E* code).  bioen_amd/_lib.py binds it in a seventh
 * table (_SIGNATURES_FORCES_LAPLACE).
 *
 * The two entries carry the prefix bioen_laplace_, not bioen_hip_: the set of exported bioen_hip_* symbols is closed over
 * the six earlier tables.
 *
 * With H = L L^T and W = L^-1:
 *   cov_forces   = H^-1     = W^T W
 *   cov_averages = C H^-1 C = B^T B,  B = W C
 *   var_logw_j   = a_j^T H^-1 a_j
 *   logdet       = 2 sum_i ln L_ii
 * Both covariances are bitwise symmetric, and the same bits in give the same bits out.
 *
 * Both entries are refused with BIOEN_HIP_ESTATE, each case with a message of its own, where bioen_hip_forces_gram is:
 * m > 1024 (row panels), contexts without the strip copies, the reduced-storage experiment's copies, structure-sharded
 * contexts.  A rejected call leaves point, session and device alone.  The device buffers (W, H^-1, B, C H^-1 C) are this
 * header's own, allocated at the first call and freed with the context (bioen_hip_ctx_footprint: bit 9, value 512).
 */
#ifndef BIOEN_HIP_FORCES_LAPLACE_H
#define BIOEN_HIP_FORCES_LAPLACE_H

#include "bioen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* H^-1 of a caller's symmetric positive definite m x m row-major matrix A (only the lower triangle is read), or with
 * A == NULL of the Hessian (bioen_hip_forces_gram's, FP64) of the kept forces point (BIOEN_HIP_ESTATE without one).  The
 * factor becomes the context's factor: bioen_hip_forces_newton_solve afterwards solves with it.  Ainv (m x m) and logdet
 * may be NULL: the inverse stays resident.  *info (required) as LAPACK's dpotrf: 0, or k + 1 where pivot k was <= 0 or
 * not finite -- an ordinary result (the call returns 0) after which nothing is written, neither Ainv nor logdet nor the
 * resident inverse.  Keeps point and session. */
int bioen_laplace_forces_inverse(bioen_hip_ctx* ctx, const double* A, double* Ainv, double* logdet, int* info);

/* The error bars at a forces point.  With forces [m] (and w0 [n], theta) the point is evaluated and kept, as by
 * bioen_hip_forces_gram with forces: *f and grad [m] (either may be NULL) are bioen_hip_forces_fdf's bits, and a BFGS
 * session ends.  With forces == NULL the kept forces point is served (BIOEN_HIP_ESTATE without one; point and session
 * stay).  Every output may be NULL, and only what is asked for is computed and downloaded:
 *   std_forces [m], std_averages [m]      the roots of the covariances' diagonals (averages in the units of yTilde)
 *   var_logw [n]                          the Laplace variance of every ln w_j
 *   cov_forces, cov_averages [m x m]      row-major
 *   *logdet                               ln det H
 *   *min_pivot                            min_i L_ii^2: the caller judges definiteness against the scale of H
 * *info (required) as LAPACK's dpotrf; with *info != 0 the call returns 0 and writes nothing else (f and grad apart). */
int bioen_laplace_forces(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta, double* std_forces,
                         double* std_averages, double* var_logw, double* cov_forces, double* cov_averages, double* logdet,
                         double* min_pivot, int* info, double* f, double* grad);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_FORCES_LAPLACE_H */

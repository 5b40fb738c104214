/* bioen_hip_forces_gram.h -- the dense Hessian of the forces objective and the covariance of the observables in one pass
 * over the matrix: the part of the C ABI of libbioen_hip that is declared beside bioen_hip.h and
 * bioen_hip_forces_hessp.h (same library, same conventions: plain C, host buffers owned by the caller, 0 or a negative
 * BIOEN_HIP_E* code).  INTEGRATION.md says why it is a header of its own; bioen_amd/_lib.py binds it in a third table
 * (_SIGNATURES_FORCES_GRAM).
 */
#ifndef BIOEN_HIP_FORCES_GRAM_H
#define BIOEN_HIP_FORCES_GRAM_H

#include "bioen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cov = C, the covariance of the observables under the weights of the point (= d ybar / d forces), and hess = H, the
 * exact Hessian of L(f) = theta KL(w || w0) + 0.5 |ybar - YTilde|^2 at it (of the affine model if
 * bioen_hip_ctx_set_affine has set one); both m x m, row-major, bitwise symmetric; either may be NULL.  With
 * a_j = A_:j - ybar and q_j = theta x_j + b_j:  C = sum_j w_j a_j a_j^T,  H = theta C + C C + sum_j w_j (q_j - qbar) a_j a_j^T
 * -- ONE compute-bound pass over the matrix on the FP64 matrix cores for both, where bioen_hip_forces_hessp needs
 * 2 ceil(m / 8) bandwidth-bound ones for H.  No reference counterpart.
 *
 * The point is bioen_hip_forces_hessp's.  forces != NULL (with w0): evaluates the point first -- bioen_hip_forces_fdf
 * with a gradient, launch for launch: f and grad (optional outputs) are its bits --, keeps it on the context and ends
 * a BFGS session.  forces == NULL: serves the kept forces point (w0, theta ignored), keeps point and session; refused
 * with BIOEN_HIP_ESTATE on a log-weights point or without a point.  A call rejected for its arguments
 * (BIOEN_HIP_EINVAL: forces without w0; nothing asked for) or refused for the context's state leaves point, session
 * and device alone.
 *
 * Two calls at one point give the same bits (fixed summation order, no atomics); a call that sets the point gives the
 * bits of a call that serves it.  Refused with BIOEN_HIP_ESTATE: m > 1024 (row panels), contexts without the strip
 * copies, the reduced-storage experiment's copies, structure-sharded contexts.  The device buffer of the partial
 * sums is allocated at the first call and freed with the context (bioen_hip_ctx_footprint: bit 5).  Its size is
 * O(sets x m^2) whatever n is -- sets = 8 segments x ceil(512 / (8 tiles)) groups, each holding the lower triangle's 64 x 64
 * sub-tiles of both matrices: 117 MB at m = 256, 139 MB at m = 512, 168 MB at m = 1024, 4 MB at m = 7 -- so a small
 * matrix does not make it small: callers that keep many small contexts should use bioen_hip_forces_hessp there. */
int bioen_hip_forces_gram(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                          double* cov, double* hess, double* f, double* grad);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_FORCES_GRAM_H */

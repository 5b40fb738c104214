/* bioen_hip_forces_colquad.h -- one quadratic form per structure at a kept forces point, in one pass over the matrix: the
 * part of the C ABI of libbioen_hip that is declared beside bioen_hip.h, bioen_hip_forces_hessp.h and
 * bioen_hip_forces_gram.h (same library, same conventions: plain C, host buffers owned by the caller, 0 or a negative
 * BIOEN_HIP_E* code).  INTEGRATION.md says why it is a header of its own; bioen_amd/_lib.py binds it in a fourth table
 * (_SIGNATURES_FORCES_COLQUAD).
 */
#ifndef BIOEN_HIP_FORCES_COLQUAD_H
#define BIOEN_HIP_FORCES_COLQUAD_H

#include "bioen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_j = a_j^T P a_j, j = 0 .. n - 1, with a_j = A_:j - ybar the j-th structure's observables (of the affine model if
 * bioen_hip_ctx_set_affine has set one: a_j = S (Y_:j - ybar), S = diag(scale)) centred on the averages under the
 * weights of the point, and P a symmetric m x m matrix, row-major.  Because d ln w_j / d forces = a_j:
 *   P = H^-1 (bioen_hip_forces_gram's H)  the Laplace variance of ln w_j around an optimum,
 *   P = C^-1                              the structure's Mahalanobis distance from the refined ensemble,
 *   P = I                                 its spread |a_j|^2.
 * ONE compute-bound pass over the matrix on the FP64 matrix cores (2 m^2 n flops), where the column sums of
 * bioen_hip_forces_hessp's passes would need ceil(m / 8) bandwidth-bound ones.  No reference counterpart.
 *
 * The point is bioen_hip_forces_hessp's, with bioen_hip_forces_gram's semantics.  forces != NULL (with w0): evaluates
 * the point first -- bioen_hip_forces_fdf with a gradient, launch for launch: f and grad (optional outputs) are its
 * bits --, keeps it on the context and ends a BFGS session; P == NULL then only sets the point (out is not written).
 * forces == NULL: serves the kept forces point (w0, theta ignored), keeps point and session; refused with
 * BIOEN_HIP_ESTATE on a log-weights point or without a point.  A call rejected for its arguments (BIOEN_HIP_EINVAL:
 * forces without w0; neither forces nor P; P without out; "P is not symmetric": |P_ij - P_ji| > 1e-12 max |P|) or
 * refused for the context's state leaves point, session and device alone.  Non-finite entries of P are the caller's
 * business.  What is computed is the form of the symmetric part (P + P^T) / 2.
 *
 * Two calls at one point give the same bits (every out_j has one writer, fixed summation order, no atomics).  Refused
 * with BIOEN_HIP_ESTATE: m > 1024 (row panels), contexts without the strip copies, the reduced-storage experiment's
 * copies, structure-sharded contexts.  The device buffer -- P padded to a multiple of 16 rows, and the n results -- is
 * allocated at the first call that computes and freed with the context (bioen_hip_ctx_footprint: bit 6). */
int bioen_hip_forces_colquad(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                             const double* P, double* out, double* f, double* grad);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_FORCES_COLQUAD_H */

/* bioen_hip_forces_gram_bf16.h -- the dense Hessian of the forces objective for a Newton minimizer, from split-BF16
 * operands on the BF16 matrix cores: the part of the C ABI of libbioen_hip that is declared beside bioen_hip.h and the
 * three forces headers (same library, same conventions: plain C, host buffers owned by the caller, 0 or a negative
 * BIOEN_HIP_E* code).  INTEGRATION.md says why it is a header of its own; bioen_amd/_lib.py binds it in a fifth table
 * (_SIGNATURES_FORCES_GRAM_BF16).
 */
#ifndef BIOEN_HIP_FORCES_GRAM_BF16_H
#define BIOEN_HIP_FORCES_GRAM_BF16_H

#include "bioen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cov = C~ and hess = H~: bioen_hip_forces_gram's C and H (bioen_hip_forces_gram.h: the same formulas, arguments, layout
 * and point semantics) with the two M x M x N products formed from split-BF16 operands -- every operand is hi + lo, two
 * bfloat16 numbers, the products hi hi + hi lo + lo hi are accumulated in f32 -- at 32 x the matrix rate of FP64.
 * Everything else (the point, its weights, the row sums, the rank corrections, theta C + G2 + C C) stays FP64.  The
 * result is a MINIMIZER's Hessian, good to about 1e-5 .. 1e-4 of max|H|: it shapes a Newton step, whose gradient (f and
 * grad of this entry are bioen_hip_forces_fdf's bits) decides the optimum.  Error bars and anything else that needs C
 * or H themselves take them from bioen_hip_forces_gram, which this entry leaves bitwise alone.
 *
 * Both matrices are m x m, row-major, bitwise symmetric; either may be NULL.  forces != NULL (with w0): evaluates the
 * point first, keeps it on the context and ends a BFGS session.  forces == NULL: serves the kept forces point (w0,
 * theta ignored), keeps point and session; refused with BIOEN_HIP_ESTATE on a log-weights point or without a point.  A
 * call rejected for its arguments (BIOEN_HIP_EINVAL: forces without w0; nothing asked for) or refused for the
 * context's state leaves point, session and device alone.
 *
 * Two calls at one point give the same bits (fixed summation order, no atomics; the sets' f32 sums are added in FP64).
 * Refused with BIOEN_HIP_ESTATE: m > 1024 (row panels), contexts without the strip copies, the reduced-storage
 * experiment's copies, structure-sharded contexts.  The device buffer of the partial sums is this entry's own, of
 * bioen_hip_forces_gram's size, allocated at the first computing call and freed with the context
 * (bioen_hip_ctx_footprint: bit 7). */
int bioen_hip_forces_gram_bf16(bioen_hip_ctx* ctx, const double* forces, const double* w0, double theta,
                               double* cov, double* hess, double* f, double* grad);

#ifdef __cplusplus
}
#endif
#endif /* BIOEN_HIP_FORCES_GRAM_BF16_H */

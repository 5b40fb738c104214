/* A C99 caller of include/bioen_hip.h: a caller's matrix inverted on the device from its Cholesky factor (A
 * Ainv = I and the symmetry checked), a pivot failure reported as LAPACK's info with nothing written, then a small forces
 * problem minimised by the device-resident Newton loop and the Laplace error bars taken at the optimum, which the loop
 * leaves as the kept point: only the M + N numbers of the error bars come down.  Leaves with 0 and "ok", with 77 where
 * there is no HIP device (there is no CPU path), with 1 on a failure. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bioen_hip.h"

#define M 24
#define N 300

static double unit(unsigned* s) {
    *s = *s * 1664525u + 1013904223u;
    return (double)(*s >> 8) / 16777216.0;
}

int main(void) {
    int count = 0;
    if (bioen_hip_device_count(&count) != 0 || count == 0) {
        printf("no HIP device: bioen_laplace_forces needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], w0[N], f0[M], fopt[M], A[M * M], Ainv[M * M], sf[M], sa[M], vl[N], cov[M * M];
    unsigned s = 12345u;
    int i, j, k, info = -1;
    double logdet = 0.0, pivot = 0.0;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        f0[i] = 0.0;
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
    }
    for (j = 0; j < N; ++j) w0[j] = 1.0 / N;
    for (i = 0; i < M; ++i)
        for (j = 0; j <= i; ++j) A[i * M + j] = A[j * M + i] = (i == j ? 2.0 : 0.0) + 0.5 * unit(&s) / M;
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    /* a caller's matrix */
    if (bioen_laplace_forces_inverse(ctx, A, Ainv, &logdet, &info) != 0 || info != 0) {
        printf("inverse: %s (info %d)\n", bioen_hip_last_error(), info);
        return 1;
    }
    double worst = 0.0;
    for (i = 0; i < M; ++i)
        for (j = 0; j < M; ++j) {
            double r = i == j ? -1.0 : 0.0;
            for (k = 0; k < M; ++k) r += A[i * M + k] * Ainv[k * M + j];
            if (fabs(r) > worst) worst = fabs(r);
            if (Ainv[i * M + j] != Ainv[j * M + i]) worst = 1.0;
        }
    if (!(worst <= 1e-13) || !(logdet > 0.0)) {
        printf("max |A Ainv - I| = %.3g, logdet = %.6g\n", worst, logdet);
        return 1;
    }
    /* a pivot that is not positive: an ordinary result, nothing written */
    A[5 * M + 5] = -1.0;
    logdet = -7.0;
    if (bioen_laplace_forces_inverse(ctx, A, NULL, &logdet, &info) != 0 || info != 6 || logdet != -7.0) {
        printf("info = %d where 6 was expected (logdet %.3g)\n", info, logdet);
        return 1;
    }
    /* without a forces point the error bars are refused */
    if (bioen_laplace_forces(ctx, NULL, NULL, 0.0, sf, NULL, NULL, NULL, NULL, NULL, NULL, &info, NULL, NULL) != BIOEN_HIP_ESTATE) {
        printf("error bars without a point were not refused\n");
        return 1;
    }
    /* the loop, then the error bars at the point it leaves */
    bioen_newton_config cfg;
    bioen_newton_result res;
    memset(&cfg, 0, sizeof cfg);
    cfg.gtol = 1e-8;
    cfg.armijo = 1e-4;
    cfg.rho_good = 0.75;
    cfg.lambda_factor = 4.0;
    cfg.lambda_first = 1e-10;
    cfg.lambda_max = 1e10;
    cfg.lambda_zero = 1e-12;
    cfg.floor_ulps = 8.0;
    cfg.max_iterations = 50;
    cfg.hessian = 0;
    if (bioen_hip_opt_newton_forces(ctx, f0, w0, 10.0, &cfg, fopt, NULL, &res) != 0 || (res.status != 0 && res.status != 2)) {
        printf("opt_newton_forces: %s (status %d)\n", bioen_hip_last_error(), res.status);
        return 1;
    }
    if (bioen_laplace_forces(ctx, NULL, NULL, 0.0, sf, sa, vl, NULL, NULL, &logdet, &pivot, &info, NULL, NULL) != 0 || info != 0) {
        printf("error bars: %s (info %d)\n", bioen_hip_last_error(), info);
        return 1;
    }
    /* with the forces given the point is evaluated anew: the same numbers, and the covariance with them */
    double f = 0.0;
    static double sf2[M];
    if (bioen_laplace_forces(ctx, fopt, w0, 10.0, sf2, NULL, NULL, cov, NULL, NULL, NULL, &info, &f, NULL) != 0 || info != 0) {
        printf("error bars with forces: %s (info %d)\n", bioen_hip_last_error(), info);
        return 1;
    }
    for (i = 0; i < M; ++i)
        if (!(sf[i] > 0.0) || !(sa[i] > 0.0) || sf2[i] != sf[i] || sf[i] != sqrt(cov[i * M + i])) {
            printf("std_forces[%d] = %.17g (%.17g with forces), std_averages = %.17g\n", i, sf[i], sf2[i], sa[i]);
            return 1;
        }
    for (j = 0; j < N; ++j)
        if (!(vl[j] >= 0.0)) {
            printf("var_logw[%d] = %.17g\n", j, vl[j]);
            return 1;
        }
    if (f != res.fmin || !(pivot > 0.0)) {
        printf("f = %.17g, fmin = %.17g, min pivot %.3g\n", f, res.fmin, pivot);
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("fmin = %.12g, ln det H = %.12g, min pivot = %.6g, std_forces[0] = %.6g, std_averages[0] = %.6g\nok\n", res.fmin,
           logdet, pivot, sf[0], sa[0]);
    return 0;
}

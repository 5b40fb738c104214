/* A C99 caller of include/bioen_hip.h: a caller's matrix factorised and solved on the device (the residual
 * checked), a pivot failure reported as LAPACK's info and the solve behind it refused, then a small forces problem
 * minimised by the device-resident Newton loop and the Hessian of the optimum, which the loop leaves as the kept point,
 * factorised in place.  Leaves with 0 and "ok", with 77 where there is no HIP device (there is no CPU path), with 1 on a
 * failure. */
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
        printf("no HIP device: bioen_hip_opt_newton_forces needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], w0[N], f0[M], fopt[M], A[M * M], L[M * M], b[2 * M], x[2 * M], H[M * M];
    unsigned s = 12345u;
    int i, j, k, info = -1;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        f0[i] = 0.0;
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
    }
    for (j = 0; j < N; ++j) w0[j] = 1.0 / N;
    for (i = 0; i < M; ++i)
        for (j = 0; j <= i; ++j) A[i * M + j] = A[j * M + i] = (i == j ? 2.0 : 0.0) + 0.5 * unit(&s) / M;
    for (i = 0; i < 2 * M; ++i) b[i] = unit(&s) - 0.5;
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    /* a caller's matrix */
    if (bioen_hip_forces_newton_factor(ctx, A, 0, 0.0, L, &info) != 0 || info != 0 ||
        bioen_hip_forces_newton_solve(ctx, 2, b, x) != 0) {
        printf("factor / solve: %s (info %d)\n", bioen_hip_last_error(), info);
        return 1;
    }
    double worst = 0.0;
    for (k = 0; k < 2; ++k)
        for (i = 0; i < M; ++i) {
            double r = -b[k * M + i];
            for (j = 0; j < M; ++j) r += A[i * M + j] * x[k * M + j];
            if (fabs(r) > worst) worst = fabs(r);
        }
    if (!(worst <= 1e-13)) {
        printf("max |A x - b| = %.3g\n", worst);
        return 1;
    }
    /* a pivot that is not positive: an ordinary result, and no factor to solve with */
    A[5 * M + 5] = -1.0;
    if (bioen_hip_forces_newton_factor(ctx, A, 0, 0.0, NULL, &info) != 0 || info != 6) {
        printf("info = %d where 6 was expected\n", info);
        return 1;
    }
    if (bioen_hip_forces_newton_solve(ctx, 1, b, x) != BIOEN_HIP_ESTATE) {
        printf("a solve without a factor was not refused\n");
        return 1;
    }
    /* the loop */
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
    if (bioen_hip_opt_newton_forces(ctx, f0, w0, 10.0, &cfg, fopt, NULL, &res) != 0) {
        printf("opt_newton_forces: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (res.status != 0 && res.status != 2) {
        printf("status %d after %d iterations, max|g| = %.3g\n", res.status, res.iterations, res.gmax);
        return 1;
    }
    /* the optimum is the kept point: its Hessian, downloaded and factorised where it lies */
    if (bioen_hip_forces_gram(ctx, NULL, NULL, 0.0, NULL, H, NULL, NULL) != 0 ||
        bioen_hip_forces_newton_factor(ctx, NULL, 0, 0.0, L, &info) != 0 || info != 0) {
        printf("the Hessian at the optimum: %s (info %d)\n", bioen_hip_last_error(), info);
        return 1;
    }
    if (fabs(L[0] * L[0] - H[0]) > 1e-12 * fabs(H[0])) {
        printf("L[0][0]^2 = %.17g, H[0][0] = %.17g\n", L[0] * L[0], H[0]);
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("fmin = %.12g, max|g| = %.3g, status %d, %d iterations, %d evaluations, %d Hessians, %d factorisations\nok\n",
           res.fmin, res.gmax, res.status, res.iterations, res.evaluations, res.hessians, res.factorisations);
    return 0;
}

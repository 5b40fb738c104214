/* A C99 caller of include/bioen_hip.h: a small forces problem, the point set with the spread of every
 * structure (P = I) in one call, the result checked against |a_j|^2 formed here from the weights, the call at the kept
 * point for the same bits, an unsymmetric P rejected, a call refused after another evaluation.  Leaves with 0 and "ok",
 * with 77 where there is no HIP device (there is no CPU path), with 1 on a failure. */
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
        printf("no HIP device: bioen_hip_forces_colquad needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], w0[N], f[M], grad[M], g2[M], P[M * M], v[N], v2[N], w[N], ybar[M];
    unsigned s = 12345u;
    int i, j;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        f[i] = 0.02 * (unit(&s) - 0.5);
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
        P[i * M + i] = 1.0;
    }
    for (j = 0; j < N; ++j) w0[j] = 1.0 / N;
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    double fv = 0.0, f2 = 0.0;
    int rc = bioen_hip_forces_colquad(ctx, f, w0, 10.0, P, v, &fv, grad);     /* sets the point */
    if (rc == 0) rc = bioen_hip_forces_colquad(ctx, NULL, NULL, 0.0, P, v2, NULL, NULL);
    if (rc != 0) {
        printf("forces_colquad: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (memcmp(v, v2, sizeof v) != 0) {
        printf("the call at the kept point gives other bits\n");
        return 1;
    }
    /* the spread from the weights: w ~ w0 exp(f . y_j), a_j = y_j - ybar */
    double z = 0.0, worst = 0.0;
    for (j = 0; j < N; ++j) {
        double x = 0.0;
        for (i = 0; i < M; ++i) x += f[i] * y[i * N + j];
        w[j] = w0[j] * exp(x);
        z += w[j];
    }
    for (i = 0; i < M; ++i) {
        ybar[i] = 0.0;
        for (j = 0; j < N; ++j) ybar[i] += y[i * N + j] * w[j] / z;
    }
    for (j = 0; j < N; ++j) {
        double q = 0.0;
        for (i = 0; i < M; ++i) q += (y[i * N + j] - ybar[i]) * (y[i * N + j] - ybar[i]);
        if (fabs(v[j] - q) > worst) worst = fabs(v[j] - q);
        if (!(v[j] > 0.0)) {
            printf("v[%d] = %.17g is no squared length\n", j, v[j]);
            return 1;
        }
    }
    if (worst > 1e-10 * M) {
        printf("the spread is off by %.3g\n", worst);
        return 1;
    }
    P[1] = 0.5;                                                               /* P[0][1] != P[1][0] */
    if (bioen_hip_forces_colquad(ctx, NULL, NULL, 0.0, P, v2, NULL, NULL) != BIOEN_HIP_EINVAL) {
        printf("an unsymmetric P was not rejected\n");
        return 1;
    }
    P[1] = 0.0;
    if (bioen_hip_forces_colquad(ctx, NULL, NULL, 0.0, P, v2, NULL, NULL) != 0 || memcmp(v, v2, sizeof v) != 0) {
        printf("the rejected call did not leave the point alone\n");
        return 1;
    }
    if (bioen_hip_forces_fdf(ctx, f, w0, 10.0, &f2, g2) != 0 || f2 != fv) {
        printf("forces_fdf disagrees with the point-setting call\n");
        return 1;
    }
    if (bioen_hip_forces_colquad(ctx, NULL, NULL, 0.0, P, v2, NULL, NULL) != BIOEN_HIP_ESTATE) {
        printf("a call after another evaluation was not refused\n");
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("v[0] = %.12g, largest |v - |a|^2| = %.3g\nok\n", v[0], worst);
    return 0;
}

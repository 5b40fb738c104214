/* A C99 caller of include/bioen_hip.h: a small forces problem, the point set, two products at it checked
 * for symmetry (v1 . H v0 = v0 . H v1), a product refused after another evaluation.  Leaves with 0 and "ok", with 77
 * where there is no HIP device (there is no CPU path), with 1 on a failure. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

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
        printf("no HIP device: bioen_hip_forces_hessp needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], w0[N], f[M], v[2 * M], hv[2 * M], grad[M], g2[M];
    unsigned s = 12345u;
    int i, j;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        f[i] = 0.02 * (unit(&s) - 0.5);
        v[i] = unit(&s) - 0.5;
        v[M + i] = unit(&s) - 0.5;
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
    }
    for (j = 0; j < N; ++j) w0[j] = 1.0 / N;
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    double fv = 0.0, f2 = 0.0, a = 0.0, b = 0.0;
    int rc = bioen_hip_forces_hessp(ctx, f, w0, 10.0, 0, NULL, NULL, &fv, grad);     /* sets the point */
    if (rc == 0) rc = bioen_hip_forces_hessp(ctx, NULL, NULL, 0.0, 2, v, hv, NULL, NULL);
    if (rc != 0) {
        printf("forces_hessp: %s\n", bioen_hip_last_error());
        return 1;
    }
    for (i = 0; i < M; ++i) {
        a += v[M + i] * hv[i];
        b += v[i] * hv[M + i];
    }
    if (!(fabs(a - b) <= 1e-10 * (fabs(a) + fabs(b)) && fabs(a) > 0.0)) {
        printf("H is not symmetric: %.17g %.17g\n", a, b);
        return 1;
    }
    if (bioen_hip_forces_fdf(ctx, f, w0, 10.0, &f2, g2) != 0 || f2 != fv) {
        printf("forces_fdf disagrees with the point-setting call\n");
        return 1;
    }
    if (bioen_hip_forces_hessp(ctx, NULL, NULL, 0.0, 1, v, hv, NULL, NULL) != BIOEN_HIP_ESTATE) {
        printf("a product after another evaluation was not refused\n");
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("v1.Hv0 = %.12g\nok\n", a);
    return 0;
}

/* A C99 caller of include/bioen_hip.h: a small forces problem, the point set with the covariance and the
 * Hessian in one call, both checked for exact symmetry, the covariance for a non-negative diagonal, the call at the kept
 * point for the same bits, a call refused after another evaluation.  Leaves with 0 and "ok", with 77 where there is no
 * HIP device (there is no CPU path), with 1 on a failure. */
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
        printf("no HIP device: bioen_hip_forces_gram needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], w0[N], f[M], grad[M], g2[M], C[M * M], H[M * M], C2[M * M], H2[M * M];
    unsigned s = 12345u;
    int i, j;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        f[i] = 0.02 * (unit(&s) - 0.5);
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
    }
    for (j = 0; j < N; ++j) w0[j] = 1.0 / N;
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    double fv = 0.0, f2 = 0.0;
    int rc = bioen_hip_forces_gram(ctx, f, w0, 10.0, C, H, &fv, grad);     /* sets the point */
    if (rc == 0) rc = bioen_hip_forces_gram(ctx, NULL, NULL, 0.0, C2, H2, NULL, NULL);
    if (rc != 0) {
        printf("forces_gram: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (memcmp(C, C2, sizeof C) != 0 || memcmp(H, H2, sizeof H) != 0) {
        printf("the call at the kept point gives other bits\n");
        return 1;
    }
    for (i = 0; i < M; ++i) {
        if (!(C[i * M + i] > 0.0)) {
            printf("C[%d][%d] = %.17g is no variance\n", i, i, C[i * M + i]);
            return 1;
        }
        for (j = 0; j < i; ++j)
            if (C[i * M + j] != C[j * M + i] || H[i * M + j] != H[j * M + i]) {
                printf("not symmetric at (%d, %d)\n", i, j);
                return 1;
            }
    }
    if (bioen_hip_forces_fdf(ctx, f, w0, 10.0, &f2, g2) != 0 || f2 != fv) {
        printf("forces_fdf disagrees with the point-setting call\n");
        return 1;
    }
    if (bioen_hip_forces_gram(ctx, NULL, NULL, 0.0, C2, NULL, NULL, NULL) != BIOEN_HIP_ESTATE) {
        printf("a call after another evaluation was not refused\n");
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("C[0][0] = %.12g, H[0][0] = %.12g\nok\n", C[0], H[0]);
    return 0;
}

/* A C99 caller of include/bioen_hip.h: a small forces problem, the point set with the split-BF16
 * covariance and Hessian in one call, both checked for exact symmetry and against bioen_hip_forces_gram's FP64 results at
 * the same kept point (1e-3 of the largest entry: what a minimizer's Hessian may be off by), the call at the kept point
 * for the same bits, a call refused after another evaluation.  Leaves with 0 and "ok", with 77 where there is no HIP
 * device (there is no CPU path), with 1 on a failure. */
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
        printf("no HIP device: bioen_hip_forces_gram_bf16 needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], w0[N], f[M], grad[M], g2[M], C[M * M], H[M * M], C2[M * M], H2[M * M], C64[M * M], H64[M * M];
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
    double fv = 0.0, f2 = 0.0, scale = 0.0, worst = 0.0;
    int rc = bioen_hip_forces_gram_bf16(ctx, f, w0, 10.0, C, H, &fv, grad);     /* sets the point */
    if (rc == 0) rc = bioen_hip_forces_gram_bf16(ctx, NULL, NULL, 0.0, C2, H2, NULL, NULL);
    if (rc == 0) rc = bioen_hip_forces_gram(ctx, NULL, NULL, 0.0, C64, H64, NULL, NULL);      /* FP64, at the same point */
    if (rc != 0) {
        printf("forces_gram_bf16: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (memcmp(C, C2, sizeof C) != 0 || memcmp(H, H2, sizeof H) != 0) {
        printf("the call at the kept point gives other bits\n");
        return 1;
    }
    for (i = 0; i < M; ++i)
        for (j = 0; j < M; ++j) {
            if (C[i * M + j] != C[j * M + i] || H[i * M + j] != H[j * M + i]) {
                printf("not symmetric at (%d, %d)\n", i, j);
                return 1;
            }
            if (fabs(H64[i * M + j]) > scale) scale = fabs(H64[i * M + j]);
            if (fabs(H[i * M + j] - H64[i * M + j]) > worst) worst = fabs(H[i * M + j] - H64[i * M + j]);
        }
    if (!(worst <= 1e-3 * scale)) {
        printf("max |H~ - H| = %.3g against max |H| = %.3g\n", worst, scale);
        return 1;
    }
    if (bioen_hip_forces_fdf(ctx, f, w0, 10.0, &f2, g2) != 0 || f2 != fv || memcmp(grad, g2, sizeof grad) != 0) {
        printf("forces_fdf disagrees with the point-setting call\n");
        return 1;
    }
    if (bioen_hip_forces_gram_bf16(ctx, NULL, NULL, 0.0, C2, NULL, NULL, NULL) != BIOEN_HIP_ESTATE) {
        printf("a call after another evaluation was not refused\n");
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("H~[0][0] = %.12g, H[0][0] = %.12g, max |H~ - H| = %.3g max|H|\nok\n", H[0], H64[0], worst / scale);
    return 0;
}

/* A C99 caller of include/bioen_hip.h: a small log-weights problem minimised for a descending theta series by the
 * device-resident dual Newton loop in ONE call (bioen_logwn_series), warm-started, with the covariance of every step from
 * the split-BF16 pass; the same series from the FP64 pass, which must equal chained bioen_logwn_opt calls bit for bit; and
 * the covariance of the last optimum from both passes (bioen_logwn_cov, bioen_logwn_cov_bf16), which must differ by a
 * little and by no more than the split allows.
 * Leaves with 0 and "ok", with 77 where there is no HIP device (there is no CPU path), with 1 on a failure. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bioen_hip.h"

#define M 24
#define N 300
#define K 4

static double unit(unsigned* s) {
    *s = *s * 1664525u + 1013904223u;
    return (double)(*s >> 8) / 16777216.0;
}

int main(void) {
    int count = 0;
    if (bioen_hip_device_count(&count) != 0 || count == 0) {
        printf("no HIP device: bioen_logwn_series needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], G[N], g0[N], gs[K * N], gw[K * N], gc[N], C[M * M], Cb[M * M];
    const double thetas[K] = {100.0, 10.0, 1.0, 0.1}, bad[2] = {10.0, 0.0};
    unsigned s = 12345u;
    int i, j, k;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
    }
    for (j = 0; j < N; ++j) G[j] = g0[j] = 0.0;
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    bioen_logwn_config cfg;
    bioen_logwn_series_result rs[K], rw[K];
    bioen_logwn_result r1;
    memset(&cfg, 0, sizeof cfg);
    cfg.gtol = 1e-8;
    cfg.armijo = 1e-4;
    cfg.floor_ulps = 8.0;
    cfg.max_iterations = 50;
    cfg.max_halvings = 60;
    if (bioen_logwn_series(ctx, g0, G, thetas, 0, &cfg, 1, 1, gs, rs) != BIOEN_HIP_EINVAL ||
        bioen_logwn_series(ctx, g0, G, bad, 2, &cfg, 1, 1, gs, rs) != BIOEN_HIP_EINVAL ||
        bioen_logwn_series(ctx, g0, G, thetas, K, &cfg, 2, 1, gs, rs) != BIOEN_HIP_EINVAL) {
        printf("an empty series, theta = 0 or source = 2 was not refused\n");
        return 1;
    }
    /* warm, split-BF16 covariances */
    if (bioen_logwn_series(ctx, g0, G, thetas, K, &cfg, 1, 1, gs, rs) != 0) {
        printf("bioen_logwn_series: %s\n", bioen_hip_last_error());
        return 1;
    }
    /* warm, FP64 covariances: the chained single calls, bit for bit */
    if (bioen_logwn_series(ctx, g0, G, thetas, K, &cfg, 0, 1, gw, rw) != 0) {
        printf("bioen_logwn_series: %s\n", bioen_hip_last_error());
        return 1;
    }
    for (k = 0; k < K; ++k) {
        if (bioen_logwn_opt(ctx, k ? gc : g0, G, thetas[k], &cfg, gc, &r1) != 0) {
            printf("bioen_logwn_opt: %s\n", bioen_hip_last_error());
            return 1;
        }
        if (memcmp(gc, gw + k * N, sizeof gc) != 0 || r1.fmin != rw[k].fmin || r1.iterations != rw[k].iterations ||
            r1.evaluations != rw[k].evaluations || rw[k].bf16_passes != 0 || rw[k].switched != 0) {
            printf("theta %g: the FP64 series and the chained call differ\n", thetas[k]);
            return 1;
        }
        if (rs[k].status != 0 || rw[k].status != 0 || fabs(rs[k].fmin - rw[k].fmin) > 1e-9 * fabs(rw[k].fmin)) {
            printf("theta %g: status %d / %d, fmin %.17g / %.17g\n", thetas[k], rs[k].status, rw[k].status, rs[k].fmin, rw[k].fmin);
            return 1;
        }
        printf("theta %5g: fmin = %.12g, split BF16 %d iterations / %d evaluations (%d BF16 passes%s), FP64 %d / %d\n", thetas[k],
               rs[k].fmin, rs[k].iterations, rs[k].evaluations, rs[k].bf16_passes, rs[k].switched ? ", switched" : "",
               rw[k].iterations, rw[k].evaluations);
    }
    /* the last optimum is the kept point: its covariance from both passes */
    if (bioen_logwn_cov(ctx, NULL, NULL, 0.0, C, NULL, NULL) != 0 || bioen_logwn_cov_bf16(ctx, NULL, NULL, 0.0, Cb, NULL, NULL) != 0) {
        printf("bioen_logwn_cov: %s\n", bioen_hip_last_error());
        return 1;
    }
    double worst = 0.0, scale = 0.0;
    for (i = 0; i < M; ++i) {
        double g2 = C[i * M + i];       /* G'_ii >= C_ii; the centre is Y, so G'_ii = C_ii + (ybar_i - Y_i)^2 <= C_ii + 4 here */
        scale = g2 + 4.0 > scale ? g2 + 4.0 : scale;
        for (j = 0; j < M; ++j) worst = fabs(Cb[i * M + j] - C[i * M + j]) > worst ? fabs(Cb[i * M + j] - C[i * M + j]) : worst;
    }
    if (!(worst > 0.0) || worst > 5e-5 * scale) {
        printf("max |C_bf16 - C| = %.3g against a scale of %.3g\n", worst, scale);
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("max |C_bf16 - C| = %.3g (scale %.3g)\nok\n", worst, scale);
    return 0;
}

/* A C99 caller of include/bioen_hip.h: a small log-weights problem minimised by the device-resident dual Newton
 * loop, then the covariance of the observables under the refined weights, served at the point the loop leaves and again by
 * an evaluation of the returned log-weights (the same bits), with its trace checked against the weighted variances.
 * Leaves with 0 and "ok", with 77 where there is no HIP device (there is no CPU path), with 1 on a failure. */
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
        printf("no HIP device: bioen_logwn_opt needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], G[N], g0[N], gopt[N], w[N], C[M * M], C2[M * M];
    unsigned s = 12345u;
    int i, j;
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
    if (bioen_logwn_cov(ctx, NULL, NULL, 0.0, C, NULL, NULL) != BIOEN_HIP_ESTATE) {
        printf("a covariance without a point was not refused\n");
        return 1;
    }
    bioen_logwn_config cfg;
    bioen_logwn_result res;
    memset(&cfg, 0, sizeof cfg);
    cfg.gtol = 1e-8;
    cfg.armijo = 1e-4;
    cfg.floor_ulps = 8.0;
    cfg.max_iterations = 50;
    cfg.max_halvings = 60;
    if (bioen_logwn_opt(ctx, g0, G, 0.0, &cfg, gopt, &res) != BIOEN_HIP_EINVAL) {
        printf("theta = 0 was not refused\n");
        return 1;
    }
    if (bioen_logwn_opt(ctx, g0, G, 10.0, &cfg, gopt, &res) != 0) {
        printf("bioen_logwn_opt: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (res.status != 0) {
        printf("status %d after %d iterations, max|grad| = %.3g\n", res.status, res.iterations, res.gmax);
        return 1;
    }
    /* the optimum is the kept point: its covariance, and the same from an evaluation of gopt */
    double f2 = 0.0;
    if (bioen_logwn_cov(ctx, NULL, NULL, 0.0, C, NULL, NULL) != 0 || bioen_logwn_cov(ctx, gopt, G, 10.0, C2, &f2, NULL) != 0) {
        printf("bioen_logwn_cov: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (memcmp(C, C2, sizeof C) != 0 || f2 != res.fmin) {
        printf("the covariance at the kept point and at gopt differ (f %.17g, %.17g)\n", res.fmin, f2);
        return 1;
    }
    double gm = gopt[0], sw = 0.0, trace = 0.0, var = 0.0;
    for (j = 1; j < N; ++j) gm = gopt[j] > gm ? gopt[j] : gm;
    for (j = 0; j < N; ++j) sw += (w[j] = exp(gopt[j] - gm));
    for (i = 0; i < M; ++i) {
        double mean = 0.0, sq = 0.0;
        for (j = 0; j < N; ++j) mean += w[j] / sw * y[i * N + j];
        for (j = 0; j < N; ++j) sq += w[j] / sw * (y[i * N + j] - mean) * (y[i * N + j] - mean);
        var += sq;
        trace += C[i * M + i];
    }
    if (fabs(trace - var) > 1e-12 * var) {
        printf("trace C = %.17g, the weighted variances add up to %.17g\n", trace, var);
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("fmin = %.12g, max|grad| = %.3g max w, status %d, %d iterations, %d evaluations, %d factorisations\nok\n", res.fmin,
           res.gmax / res.wmax, res.status, res.iterations, res.evaluations, res.factorisations);
    return 0;
}

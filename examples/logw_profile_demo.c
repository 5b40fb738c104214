/* A C99 caller of include/bioen_hip.h: a small scattering-like problem -- two curves, each with a scale factor of its own
 * that nobody knows, and a few rows whose scale is fixed at 1 -- refined for a descending theta series by the dual Newton
 * minimizer with the scales profiled out (bioen_logwn_profile_series), in ONE call, with no alternation between optimising
 * and refitting.  Checked here: the returned scales are the least-squares refit at the returned point's raw averages; the
 * objective of the affine model the call leaves on the context, evaluated at the returned log-weights, is the entry's fmin;
 * the split-BF16 covariance reaches the same optimum; what the entry refuses.
 * Leaves with 0 and "ok", with 77 where there is no HIP device (there is no CPU path), with 1 on a failure. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bioen_hip.h"

#define M 40
#define N 300
#define K 3
#define P 2

static double unit(unsigned* s) {
    *s = *s * 1664525u + 1013904223u;
    return (double)(*s >> 8) / 16777216.0;
}

int main(void) {
    int count = 0;
    if (bioen_hip_device_count(&count) != 0 || count == 0) {
        printf("no HIP device: bioen_logwn_profile_series needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], G[N], g0[N], g[K * N], gb[K * N], wt[N], yraw[M], yeff[M];
    static int group[M];
    const double thetas[K] = {100.0, 10.0, 1.0}, bad[2] = {10.0, 0.0}, truth[P] = {1.7, 0.6};
    double sc[K * P], scb[K * P], chi2[K], kl[K], f = 0.0, wsum = 0.0;
    unsigned s = 2024u;
    int i, j, k;
    for (j = 0; j < N; ++j) {
        G[j] = g0[j] = 0.0;
        wt[j] = unit(&s) < 0.2 ? 4.0 * unit(&s) : 0.1 * unit(&s);
        wsum += wt[j];
    }
    for (i = 0; i < M; ++i) {
        group[i] = i < 16 ? 0 : i < 34 ? 1 : -1;          /* the last six rows: no scale to fit */
        Y[i] = 0.0;
        for (j = 0; j < N; ++j) {
            y[i * N + j] = 20.0 * exp(-0.05 * (i % 17) * (1.0 + 2.0 * (double)j / N)) + unit(&s);
            Y[i] += y[i * N + j] * wt[j] / wsum;
        }
        Y[i] = (group[i] >= 0 ? truth[group[i]] : 1.0) * Y[i] + 0.05 * (unit(&s) - 0.5);
    }
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    bioen_logwn_config cfg;
    bioen_logwn_series_result r[K], rb[K];
    memset(&cfg, 0, sizeof cfg);
    cfg.gtol = 1e-8;
    cfg.armijo = 1e-4;
    cfg.floor_ulps = 8.0;
    cfg.max_iterations = 100;
    cfg.max_halvings = 60;
    group[3] = P;
    if (bioen_logwn_profile_series(ctx, g0, G, thetas, K, &cfg, 0, 1, NULL, group, P, g, sc, chi2, kl, r) != BIOEN_HIP_EINVAL) {
        printf("a group id out of range was not refused\n");
        return 1;
    }
    group[3] = 0;
    if (bioen_logwn_profile_series(ctx, g0, G, thetas, K, &cfg, 0, 1, NULL, group, P + 1, g, sc, chi2, kl, r) != BIOEN_HIP_EINVAL ||
        bioen_logwn_profile_series(ctx, g0, G, thetas, K, &cfg, 0, 1, NULL, group, 65, g, sc, chi2, kl, r) != BIOEN_HIP_EINVAL ||
        bioen_logwn_profile_series(ctx, g0, G, bad, 2, &cfg, 0, 1, NULL, group, P, g, sc, chi2, kl, r) != BIOEN_HIP_EINVAL ||
        bioen_logwn_profile_series(ctx, g0, G, thetas, 0, &cfg, 0, 1, NULL, group, P, g, sc, chi2, kl, r) != BIOEN_HIP_EINVAL ||
        bioen_logwn_profile_series(ctx, g0, G, thetas, K, &cfg, 0, 1, NULL, group, P, g, NULL, chi2, kl, r) != BIOEN_HIP_EINVAL) {
        printf("an empty group, 65 groups, theta = 0, an empty series or scales = NULL was not refused\n");
        return 1;
    }
    /* warm, FP64 covariances; then the split-BF16 ones */
    if (bioen_logwn_profile_series(ctx, g0, G, thetas, K, &cfg, 0, 1, NULL, group, P, g, sc, chi2, kl, r) != 0 ||
        bioen_logwn_profile_series(ctx, g0, G, thetas, K, &cfg, 1, 1, NULL, group, P, gb, scb, NULL, NULL, rb) != 0) {
        printf("bioen_logwn_profile_series: %s\n", bioen_hip_last_error());
        return 1;
    }
    for (k = 0; k < K; ++k) {
        if (r[k].status != 0 || rb[k].status != 0 || fabs(rb[k].fmin - r[k].fmin) > 1e-9 * fabs(r[k].fmin) ||
            fabs(r[k].fmin - (thetas[k] * kl[k] + chi2[k])) > 1e-12 * fabs(r[k].fmin)) {
            printf("theta %g: status %d / %d, fmin %.17g / %.17g, theta kl + chi2 = %.17g\n", thetas[k], r[k].status, rb[k].status,
                   r[k].fmin, rb[k].fmin, thetas[k] * kl[k] + chi2[k]);
            return 1;
        }
        for (i = 0; i < P; ++i)
            if (fabs(scb[k * P + i] - sc[k * P + i]) > 1e-6 * fabs(sc[k * P + i])) {
                printf("theta %g: scale %d is %.17g from the FP64 covariance, %.17g from the split-BF16 one\n", thetas[k], i,
                       sc[k * P + i], scb[k * P + i]);
                return 1;
            }
        printf("theta %5g: fmin = %.12g, scales %.6f %.6f (truth %.1f %.1f), %d iterations / %d evaluations, split BF16 %d / %d\n",
               thetas[k], r[k].fmin, sc[k * P], sc[k * P + 1], truth[0], truth[1], r[k].iterations, r[k].evaluations,
               rb[k].iterations, rb[k].evaluations);
    }
    /* the context keeps the model (no offset, sigma of the last theta): the plain evaluation there gives the entry's fmin,
     * and the scales are the refit of its raw averages */
    if (bioen_hip_logw_fdf(ctx, gb + (K - 1) * N, G, thetas[K - 1], &f, NULL) != 0 || bioen_hip_last_average(ctx, yraw, yeff) != 0) {
        printf("bioen_hip_logw_fdf: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (fabs(f - rb[K - 1].fmin) > 1e-12 * fabs(f)) {
        printf("f of the model the call left = %.17g, fmin = %.17g\n", f, rb[K - 1].fmin);
        return 1;
    }
    for (k = 0; k < P; ++k) {
        double num = 0.0, den = 0.0;
        for (i = 0; i < M; ++i)
            if (group[i] == k) {
                num += yraw[i] * Y[i];
                den += yraw[i] * yraw[i];
            }
        if (fabs(num / den - scb[(K - 1) * P + k]) > 1e-12 * fabs(num / den)) {
            printf("scale %d: %.17g, the refit of the raw averages gives %.17g\n", k, scb[(K - 1) * P + k], num / den);
            return 1;
        }
    }
    for (i = 34; i < M; ++i)
        if (yeff[i] != yraw[i]) {
            printf("row %d belongs to no group and has the scale %.17g\n", i, yeff[i] / yraw[i]);
            return 1;
        }
    bioen_hip_ctx_set_affine(ctx, NULL, NULL);
    bioen_hip_ctx_destroy(ctx);
    printf("ok\n");
    return 0;
}

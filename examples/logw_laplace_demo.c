/* A C99 caller of include/bioen_hip.h: a small log-weights problem minimised by the device-resident dual Newton loop, then
 * the Laplace error bars at the point the loop leaves (bioen_logwn_laplace without g) and again by an evaluation of the
 * returned log-weights (the same bits), with three identities checked on the host: sum_j leverage_j = trace cov_averages
 * (both are trace (C P)), the leverages lie in [0, 1 - w_j), and a held-out observable that is constant over the structures
 * has variance zero.
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
        printf("no HIP device: bioen_logwn_laplace needs one\n");
        return 77;
    }
    static double y[M * N], Y[M], G[N], g0[N], gopt[N], obs[2 * N];
    static double sa[M], ca[M * M], w[N], lev[N], vl[N], sw[N], sa2[M], ca2[M * M], w2[N], lev2[N], vl2[N], sw2[N];
    double oa[2], vo[2], oa2[2], vo2[2], logdet = 0.0, pivot = 0.0, logdet2 = 0.0, pivot2 = 0.0, f2 = 0.0;
    const double theta = 10.0;
    unsigned s = 12345u;
    int i, j, info = -1, info2 = -1;
    for (i = 0; i < M; ++i) {
        Y[i] = 5.0 + unit(&s);
        for (j = 0; j < N; ++j) y[i * N + j] = 5.0 + 2.0 * (unit(&s) - 0.5);
    }
    for (j = 0; j < N; ++j) {
        G[j] = g0[j] = 0.0;
        obs[j] = unit(&s);          /* a quantity that was not fitted */
        obs[N + j] = 3.0;           /* and one every structure shares: no variance */
    }
    bioen_hip_ctx* ctx = NULL;
    if (bioen_hip_ctx_create(M, N, y, Y, 0, &ctx) != 0) {
        printf("ctx_create: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (bioen_logwn_laplace(ctx, NULL, NULL, theta, NULL, 0, sa, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &info, NULL,
                            NULL) != BIOEN_HIP_ESTATE) {
        printf("error bars without a point were not refused\n");
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
    if (bioen_logwn_opt(ctx, g0, G, theta, &cfg, gopt, &res) != 0 || res.status != 0) {
        printf("bioen_logwn_opt: status %d: %s\n", res.status, bioen_hip_last_error());
        return 1;
    }
    if (bioen_logwn_laplace(ctx, NULL, NULL, 0.0, NULL, 0, sa, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &info, NULL,
                            NULL) != BIOEN_HIP_EINVAL ||
        bioen_logwn_laplace(ctx, NULL, NULL, theta, obs, 9, sa, NULL, NULL, NULL, NULL, NULL, oa, vo, NULL, NULL, &info, NULL,
                            NULL) != BIOEN_HIP_EINVAL) {
        printf("theta = 0 or nobs = 9 was not refused\n");
        return 1;
    }
    /* the optimum is the kept point: its error bars, and the same from an evaluation of gopt */
    if (bioen_logwn_laplace(ctx, NULL, NULL, theta, obs, 2, sa, ca, w, lev, vl, sw, oa, vo, &logdet, &pivot, &info, NULL, NULL) != 0 ||
        bioen_logwn_laplace(ctx, gopt, G, theta, obs, 2, sa2, ca2, w2, lev2, vl2, sw2, oa2, vo2, &logdet2, &pivot2, &info2, &f2,
                            NULL) != 0) {
        printf("bioen_logwn_laplace: %s\n", bioen_hip_last_error());
        return 1;
    }
    if (info != 0 || info2 != 0) {
        printf("info = %d, %d\n", info, info2);
        return 1;
    }
    if (memcmp(sa, sa2, sizeof sa) || memcmp(ca, ca2, sizeof ca) || memcmp(w, w2, sizeof w) || memcmp(lev, lev2, sizeof lev) ||
        memcmp(vl, vl2, sizeof vl) || memcmp(sw, sw2, sizeof sw) || memcmp(oa, oa2, sizeof oa) || memcmp(vo, vo2, sizeof vo) ||
        logdet != logdet2 || pivot != pivot2 || f2 != res.fmin) {
        printf("the error bars at the kept point and at gopt differ (f %.17g, %.17g)\n", res.fmin, f2);
        return 1;
    }
    double trace = 0.0, levsum = 0.0, wsum = 0.0;
    for (i = 0; i < M; ++i) {
        trace += ca[i * M + i];
        if (fabs(sa[i] * sa[i] - ca[i * M + i]) > 1e-14 || !(ca[i * M + i] >= 0.0 && ca[i * M + i] < 1.0)) {
            printf("std_averages[%d] = %.17g, cov_averages = %.17g\n", i, sa[i], ca[i * M + i]);
            return 1;
        }
        for (j = 0; j < i; ++j)
            if (ca[i * M + j] != ca[j * M + i]) {
                printf("cov_averages is not symmetric at (%d, %d)\n", i, j);
                return 1;
            }
    }
    for (j = 0; j < N; ++j) {
        levsum += lev[j];
        wsum += w[j];
        if (!(lev[j] >= 0.0 && lev[j] < 1.0 - w[j]) ||
            fabs(vl[j] - (1.0 - w[j] - lev[j]) / (theta * w[j])) > 1e-12 * vl[j] || fabs(sw[j] * sw[j] - w[j] * w[j] * vl[j]) > 1e-12 * sw[j] * sw[j]) {
            printf("structure %d: w = %.17g, leverage = %.17g, var_logw = %.17g, std_w = %.17g\n", j, w[j], lev[j], vl[j], sw[j]);
            return 1;
        }
    }
    if (fabs(levsum - trace) > 1e-10 * trace || fabs(wsum - 1.0) > 1e-12) {      /* sum_j w_j a_j^T P a_j = trace (C P) */
        printf("sum leverage = %.17g, trace cov_averages = %.17g, sum w = %.17g\n", levsum, trace, wsum);
        return 1;
    }
    if (fabs(oa[1] - 3.0) > 1e-14 || fabs(vo[1]) > 1e-16 || !(vo[0] > 0.0)) {
        printf("held-out: averages %.17g, %.17g, variances %.3g, %.3g\n", oa[0], oa[1], vo[0], vo[1]);
        return 1;
    }
    bioen_hip_ctx_destroy(ctx);
    printf("fmin = %.12g, ln det (C + theta I) = %.12g, sum leverage = %.6g of %d, held-out average %.6g +- %.3g\nok\n", res.fmin,
           logdet, levsum, M, oa[0], sqrt(vo[0]));
    return 0;
}

#!/usr/bin/env python3
"""Refine an ensemble with the log-weights method's dual Newton minimizer on one MI355X, then put Laplace error bars on the
result without a further evaluation: the standard deviations of the refined averages, and the refined averages of two
observables that were NOT fitted with theirs (needs the built library and a GPU; there is no CPU path).

    make -C bioen_amd/csrc && python examples/logw_error_bars.py [N] [M] [theta]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bioen_amd                                   # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 64
theta = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0

# synthetic ensemble after bioen/optimize/log_weights.py's tests; two more observables of the same kind are held out
rng = np.random.default_rng(12345)
YTrue = rng.uniform(1, 10, M + 2)
sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
y = rng.normal(YTrue[:, None], sig_sim[:, None], (M + 2, N))
yTilde = y[:M] / sig_exp[:M, None]
YTilde = rng.normal(YTrue[:M], sig_exp[:M]) / sig_exp[:M]
held_out = y[M:]                                   # per-structure values, in their own units
G = np.full(N, -np.log(N))

with bioen_amd.Context(yTilde, YTilde) as ctx:
    # 1. refine: the dual Newton ends on the gradient, which is what a Laplace expansion wants
    res = ctx.opt_dual_newton_logw(G, G, theta, dict(gtol=1e-8))
    print("theta %g: L = %.6f after %d iterations, max|grad| = %.2e max w" % (theta, res["fmin"], res["iterations"],
                                                                             res["gmax"] / res["wmax"]))
    # 2. error bars at the kept point: C + theta I factorised and inverted on the device, one pass over the matrix
    eb = ctx.logw_laplace(theta=theta, observables=held_out, matrices=False)
    assert eb["info"] == 0
print("ln det (C + theta I) = %.6f" % eb["logdet"])
print("averages: standard deviations of ybar (units of yTilde) %.3g ... %.3g" % (eb["std_averages"].min(), eb["std_averages"].max()))
for k in range(2):
    print("held-out observable %d: prior average %.4f, refined %.4f +- %.4f" % (k, held_out[k].mean(), eb["obs_averages"][k],
                                                                               np.sqrt(eb["var_observables"][k])))
# a single weight is poorly determined whenever theta w_j << 1: the information is in the averages
rel = eb["std_w"] / eb["w"]
print("weights: std(w_j) / w_j = %.3g ... %.3g (1 / sqrt(theta w_j) = %.3g ... %.3g); leverage %.3g ... %.3g, sum %.4g of M = %d"
      % (rel.min(), rel.max(), (1.0 / np.sqrt(theta * eb["w"])).min(), (1.0 / np.sqrt(theta * eb["w"])).max(),
         eb["leverage"].min(), eb["leverage"].max(), eb["leverage"].sum(), M))

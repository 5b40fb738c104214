#!/usr/bin/env python3
"""Refine an ensemble with the log-weights method's dual Newton minimizer on one MI355X -- N log-weights through an M x M
system formed, factorised and solved on the device --, compare it with the device L-BFGS, and read the covariance of the
observables under the refined weights (needs the built library and a GPU; there is no CPU path).

    make -C bioen_amd/csrc && python examples/logw_dual_newton.py [N] [M] [theta]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bioen_amd                                   # noqa: E402
from bioen_amd import optimize                     # noqa: E402  (drop-in for `from bioen import optimize`)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 64
theta = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0

# synthetic ensemble after bioen/optimize/log_weights.py's tests
rng = np.random.default_rng(12345)
YTrue = rng.uniform(1, 10, M)
sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
y = rng.normal(YTrue[:, None], sig_sim[:, None], (M, N))
yTilde = y / sig_exp[:, None]
YTilde = (rng.normal(YTrue, sig_exp) / sig_exp)[None, :]
w0 = np.full((N, 1), 1.0 / N)
_, _, G, GInit = optimize.log_weights.init_log_weights(w0)

with optimize.resident(yTilde):                    # one upload for both runs
    for name, mod in (("dual_newton", ""), ("lbfgs", "lbfgs:epsilon=1e-9,lbfgs:delta=0,lbfgs:past=0,lbfgs:max_iterations=200000")):
        params = optimize.minimize.Parameters(name, mod)
        params["verbose"] = False
        t0 = time.perf_counter()
        wopt, yopt, gopt, f0, fmin = optimize.log_weights.find_optimum(GInit, G, y, yTilde, YTilde, theta, params)
        print("%-12s L %.6f -> %.12f in %.4f s, max w = %.3e" % (name, f0, fmin, time.perf_counter() - t0, wopt.max()))
        if name == "dual_newton":
            info, w_newton, f_newton = optimize.ext.c_bioen.last_opt_info, wopt, fmin
            print("             %d iterations, %d evaluations, %d factorisations, max|grad| = %.2e max w"
                  % (info["iterations"], info["evaluations"], info["factorisations"], info["gmax"] / info["wmax"]))
        else:                                      # the L-BFGS ends on its epsilon (or its line search), not on the gradient
            info = optimize.ext.c_bioen.last_opt_info
            print("             %d iterations, %d evaluations, liblbfgs status %d" % (info.iterations, info.evaluations, info.lbfgs_code))
    # liblbfgs's test is |grad| <= epsilon max(1, |g|): it passes while structures of small weight are still far from theirs
    print("the L-BFGS ends %.3g above the Newton minimum; max |w_newton - w_lbfgs| = %.2e max w"
          % (fmin - f_newton, np.abs(w_newton - wopt).max() / wopt.max()))

# the covariance of the observables under the refined weights: error bars on the refined averages for free
with bioen_amd.Context(yTilde, YTilde.reshape(-1)) as ctx:
    res = ctx.opt_dual_newton_logw(GInit.reshape(-1), G.reshape(-1), theta)
    C = ctx.logw_cov()                             # the loop leaves its optimum as the kept point
    spread = np.sqrt(np.diag(C)) * sig_exp
    print("spread of the observables under the refined weights: %.3g ... %.3g (sigma_sim %.3g ... %.3g)"
          % (spread.min(), spread.max(), sig_sim.min(), sig_sim.max()))

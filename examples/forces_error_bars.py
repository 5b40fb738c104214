#!/usr/bin/env python3
"""Refine an ensemble with the forces method on one MI355X, then put Laplace error bars on the result: the standard
deviations of the forces and of the refined averages, and the five structures whose refined weights are least certain
(needs the built library and a GPU; there is no CPU path).

    make -C bioen_amd/csrc && python examples/forces_error_bars.py [--on-device] [N] [M] [theta]

--on-device: the Hessian is factorised and inverted in device memory and handed to the quadratic-form pass there
(laplace_error_bars(on_device=True, matrices=False)): only the M + N numbers of the error bars and ln det H come down.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bioen_amd import optimize                     # noqa: E402  (drop-in for `from bioen import optimize`)

on_device = "--on-device" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--on-device"]
N = int(argv[0]) if len(argv) > 0 else 20000
M = int(argv[1]) if len(argv) > 1 else 64
theta = float(argv[2]) if len(argv) > 2 else 10.0

# synthetic ensemble after bioen/optimize/forces.py:19-68
rng = np.random.default_rng(12345)
YTrue = rng.uniform(1, 10, M)
sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
y = rng.normal(YTrue[:, None], sig_sim[:, None], (M, N))
yTilde = y / sig_exp[:, None]
YTilde = (rng.normal(YTrue, sig_exp) / sig_exp)[None, :]
w0 = np.full((N, 1), 1.0 / N)

# 1. refine: Newton with the dense Hessian of one Gram pass ends on the gradient, which is what a Laplace expansion wants
params = optimize.minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:hessian=gram,scipy:gtol=1e-8")
params["verbose"] = False
wopt, yopt, fopt, f0, fmin, chi2, S = optimize.forces.find_optimum(np.zeros((M, 1)), w0, y, yTilde, YTilde, theta, params)
print("theta %g: L %.6f -> %.6f, chi2/2 = %.4f, S = %.4f" % (theta, f0, fmin, chi2, S))

# 2. error bars at the optimum: C and H from forces_gram, Var(ln w_j) = a_j^T inv(H) a_j from forces_colquad, one kept point
if on_device:
    eb = optimize.forces.laplace_error_bars(fopt, w0, y, yTilde, YTilde, theta, on_device=True, matrices=False)
    print("on the device: ln det H = %.6f" % eb["logdet_H"])
else:
    eb = optimize.forces.laplace_error_bars(fopt, w0, y, yTilde, YTilde, theta)
print("forces:   largest |f| = %.4g, standard deviations %.3g ... %.3g" % (np.abs(fopt).max(), eb["std_forces"].min(),
                                                                          eb["std_forces"].max()))
print("averages: standard deviations of ybar (units of yTilde) %.3g ... %.3g" % (eb["std_averages"].min(),
                                                                                 eb["std_averages"].max()))
rel = np.sqrt(eb["var_logw"])                      # std(w_j) / w_j
print("the five largest relative weight uncertainties:")
for j in np.argsort(rel)[::-1][:5]:
    print("  structure %7d   w = %.4e +- %.2e   (%.1f %%)" % (j, eb["w"][j], eb["std_w"][j], 100.0 * rel[j]))

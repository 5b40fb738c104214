#!/usr/bin/env python3
"""What the log-weights method's Laplace error bars cost (Context.logw_laplace), in ONE process per
case, at the dual Newton's optimum (cold start from the prior g = G = 0, gtol 1e-6) of the synthetic problem M x N:

    python3 tools/logw_laplace_probe.py --once [M] [N] [calls] [theta]   # `calls` (default 3) full logw_laplace() calls with
                                        # 8 held-out observables at the kept optimum: for a kernel-trace run of its own.
                                        # Condition: what the entry adds per call -- the k_logwl_* kernels and, for the 8
                                        # observables, k_hessp_dots, k_hessp_tangent, the forward strip pass, its row sums
                                        # and the solve -- stays below the k_forces_colquad launch of the same call
    python3 tools/logw_laplace_probe.py --wall [M] [N] [reps] [theta]    # wall time of one call at the kept optimum,
                                        # alternating, `reps` repetitions (default 7), median and min ... max: (a) every
                                        # output, (b) vectors=False (M + M^2 numbers down), (c) matrices=False,
                                        # vectors=False (M numbers down), (d) as (a) with 8 held-out observables; for
                                        # context the dual Newton run that produced the optimum
Defaults 512 x 1e6, theta = 10.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]


def spread(x):
    x = np.asarray(x)
    return {"median_s": round(float(np.median(x)), 5), "min_s": round(float(x.min()), 5), "max_s": round(float(x.max()), 5)}


def run(M, N, reps, theta, wall):
    import bioen_amd
    rng = np.random.default_rng(20260)
    YTrue = rng.uniform(1, 10, M)
    sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
    YTilde = rng.normal(YTrue, sig_exp) / sig_exp
    G = np.zeros(N)
    obs = rng.standard_normal((8, N))
    out = {"M": M, "N": N, "theta": theta, "reps": reps}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        ctx.logw_cov(g=G, G=G, theta=theta)                  # warm-up: the copies, the sets' buffer
        ctx.synchronize()
        t0 = time.perf_counter()
        res = ctx.opt_dual_newton_logw(G, G, theta, dict(gtol=1e-6))
        ctx.synchronize()
        out["dual_newton"] = {"seconds": round(time.perf_counter() - t0, 4), "status": res["status"],
                              "iterations": res["iterations"], "evaluations": res["evaluations"], "fmin": res["fmin"]}
        legs = {"d_full_with_8_observables": lambda: ctx.logw_laplace(theta=theta, observables=obs)}
        if wall:
            legs = dict({"a_full": lambda: ctx.logw_laplace(theta=theta),
                         "b_no_vectors": lambda: ctx.logw_laplace(theta=theta, vectors=False),
                         "c_no_vectors_no_matrices": lambda: ctx.logw_laplace(theta=theta, vectors=False, matrices=False)}, **legs)
        first = ctx.logw_laplace(theta=theta, observables=obs)           # the buffers' first use
        assert first["info"] == 0
        ctx.synchronize()
        times = {name: [] for name in legs}
        for rep in range(reps):                              # alternating
            for name, call in legs.items():
                t0 = time.perf_counter()
                r = call()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
                assert r["info"] == 0
        for name in legs:
            out[name] = spread(times[name])
        rest = (1.0 - first["w"]) - first["leverage"]
        out["at_the_optimum"] = {"logdet": first["logdet"], "min_pivot": first["min_pivot"],
                                 "sum_leverage": float(first["leverage"].sum()), "min_1_minus_w_minus_leverage": float(rest.min()),
                                 "std_averages": [float(first["std_averages"].min()), float(first["std_averages"].max())],
                                 "std_observables": [float(v) for v in np.sqrt(first["var_observables"])]}
    return out


M = int(args[0]) if len(args) > 0 else 512
N = int(args[1]) if len(args) > 1 else 1000000
wall = "--wall" in flags
reps = int(args[2]) if len(args) > 2 else (7 if wall else 3)
theta = float(args[3]) if len(args) > 3 else 10.0
print(json.dumps(run(M, N, reps, theta, wall)))

#!/usr/bin/env python3
"""What the log-weights theta series by dual Newton costs (Context.logw_cov_bf16 / opt_dual_newton_logw_series, DESIGN
section 6k), in ONE process per case:

    python3 tools/logw_series_probe.py --once [M] [N] [calls]      # k_logw_gram_bf16 (logw_cov_bf16) and k_logw_gram
                                        # (logw_cov) alternately at the kept point g = G, `calls` times each (default 3):
                                        # for a kernel-trace run of its own.  Condition: the split-BF16 kernel faster by
                                        # more than the two spreads
    python3 tools/logw_series_probe.py --series [M] [N] [reps] [theta ...]   # whole-series wall time, cold start from the
                                        # prior g = G = 0, gtol 1e-6, alternating, `reps` repetitions (default 5): median and
                                        # min ... max of (a) opt_dual_newton_logw_series warm with hessian=gram_bf16, (b) the
                                        # same with gram, (c) cold per-theta opt_dual_newton_logw calls; per-theta iterations,
                                        # evaluations and switched.  Default 256 x 1e5 and the eight thetas 1000 ... 0.316;
                                        # `--headline`: np.logspace(3, -0.5, 8), the benchmark's.  Condition: (a) below (c)
                                        # by more than the two spreads
    ... --lbfgs                         # with --series: the L-BFGS sweep at the yaml defaults once, for context (it stops
                                        # above the optimum)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]
THETAS = [1000.0, 316.0, 100.0, 31.6, 10.0, 3.16, 1.0, 0.316]
LBFGS_YAML = dict(linesearch=2, max_iterations=5000, delta=1e-6, epsilon=1e-6, ftol=1e-5, gtol=0.9, wolfe=0.9, past=10,
                  max_linesearch=100)         # config/bioen_optimize.yaml: lbfgs


def targets(M, rng):
    YTrue = rng.uniform(1, 10, M)
    sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
    return YTrue, sig_sim, sig_exp, rng.normal(YTrue, sig_exp) / sig_exp


def spread(x):
    x = np.asarray(x)
    return {"median_s": round(float(np.median(x)), 4), "min_s": round(float(x.min()), 4), "max_s": round(float(x.max()), 4)}


def once(M, N, calls):
    import bioen_amd
    rng = np.random.default_rng(12345)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G = np.zeros(N)
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        ctx.logw_cov(g=G, G=G, theta=10.0)                   # the point, the copies and the sets' buffer
        worst, scale = 0.0, None
        for _ in range(calls):                               # the kernels alternately, from one process
            Cb = ctx.logw_cov_bf16()
            C = ctx.logw_cov()
            worst = max(worst, float(np.abs(Cb - C).max()))
            scale = float(np.abs(C).max())
        flops = 2.0 * M * (M + 64) / 2 * N                   # the 64 x 64 sub-tiles of the lower triangle (M a multiple of 64)
    return {"M": M, "N": N, "calls": calls, "max_dC": worst, "max_C": scale, "flops_one_matrix_lower_triangle": flops,
            "library": os.environ.get("BIOEN_HIP_LIBRARY", "default")}


def per_theta(res):
    return {"iterations": [r["iterations"] for r in res], "evaluations": [r["evaluations"] for r in res],
            "status": [r["status"] for r in res], "switched": [int(bool(r.get("switched", False))) for r in res],
            "fmin": [r["fmin"] for r in res]}


def series(M, N, reps, thetas, with_lbfgs):
    import bioen_amd
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G, x0 = np.zeros(N), np.zeros(N)
    prm = dict(gtol=1e-6)
    out = {"M": M, "N": N, "thetas": thetas, "reps": reps}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        legs = {
            "a_series_warm_gram_bf16": lambda: ctx.opt_dual_newton_logw_series(thetas, x0, G, prm, hessian="gram_bf16"),
            "b_series_warm_gram": lambda: ctx.opt_dual_newton_logw_series(thetas, x0, G, prm),
            "c_cold_single_calls": lambda: [ctx.opt_dual_newton_logw(x0, G, t, prm) for t in thetas],
        }
        ctx.logw_cov_bf16(g=x0, G=G, theta=thetas[0])        # warm-up: the copies, the sets' buffer
        ctx.opt_dual_newton_logw(x0, G, thetas[0], dict(max_iterations=1))      # ... and the factor's
        ctx.synchronize()
        times = {name: [] for name in legs}
        for rep in range(reps):                              # alternating
            for name, run in legs.items():
                t0 = time.perf_counter()
                res = run()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
                out[name] = per_theta(res)
                print("repetition %d %s: %.4f s" % (rep, name, times[name][-1]), file=sys.stderr, flush=True)
        for name in legs:
            out[name].update(spread(times[name]))
        a, b, c = (out[k] for k in legs)
        out["max_dfmin_a_minus_c"] = max(abs(x - y) for x, y in zip(a["fmin"], c["fmin"]))
        out["a_over_c"] = round(a["median_s"] / c["median_s"], 4)
        out["b_over_c"] = round(b["median_s"] / c["median_s"], 4)
        out["a_below_c_by_more_than_the_spreads"] = bool(
            c["median_s"] - a["median_s"] > (a["max_s"] - a["min_s"]) + (c["max_s"] - c["min_s"]))
        if with_lbfgs:
            t0 = time.perf_counter()
            infos = [ctx.opt_lbfgs_logw(x0, G, t, LBFGS_YAML, want_weights=False)[2] for t in thetas]
            ctx.synchronize()
            out["lbfgs_yaml_defaults"] = {"seconds": round(time.perf_counter() - t0, 4), "fmin": [i.fmin for i in infos],
                                          "iterations": [i.iterations for i in infos],
                                          "above_the_dual_newton_optimum": [i.fmin - f for i, f in zip(infos, a["fmin"])]}
    return out


if "--series" in flags:
    M = int(args[0]) if len(args) > 0 else 256
    N = int(args[1]) if len(args) > 1 else 100000
    reps = int(args[2]) if len(args) > 2 else 5
    thetas = [float(t) for t in args[3:]] or ([float(t) for t in np.logspace(3, -0.5, 8)] if "--headline" in flags else THETAS)
    print(json.dumps(series(M, N, reps, thetas, "--lbfgs" in flags)))
else:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 1000000
    print(json.dumps(once(M, N, int(args[2]) if len(args) > 2 else 3)))

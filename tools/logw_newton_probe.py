#!/usr/bin/env python3
"""What the log-weights method's dual Newton minimizer costs (Context.logw_cov / opt_dual_newton_logw),
in ONE process per case:

    python3 tools/logw_newton_probe.py --once [M] [N] [calls]         # k_logw_gram (logw_cov at g = G) and k_forces_gram
                                        # (forces_gram at forces = 0, w0 = softmax(G): the same weights) alternately,
                                        # `calls` times each (default 3): for a kernel-trace run of its own.  Condition:
                                        # k_logw_gram below k_forces_gram (half the matrix instructions on the same loads)
    python3 tools/logw_newton_probe.py --minimizer [M] [N] [theta] [reps] [budget_s]   # whole-run wall time, cold start from g = G = 0:
                                        # the device L-BFGS at epsilon = 1e-9 with no plateau test and the dual Newton at
                                        # gtol 1e-6, alternating, `reps` repetitions (default 5): median and min ... max
                                        # (default 256 x 1e5, theta 10).  Condition: the dual Newton is faster by more than
                                        # the two min ... max spreads.  Every leg reports to stderr as it ends; no repetition is
                                        # begun after budget_s seconds (reps_done says how many ran)
    python3 tools/logw_newton_probe.py --small-theta [M] [N] [theta]  # which of the dual Newton, the forces Newton and the
                                        # L-BFGS ends lowest, and with what status (default 300 x 9000, theta 0.1; run it
                                        # with BIOEN_HIP_SEGMENTS=1 for one canonical segment)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]
CONV = dict(linesearch=2, max_iterations=200000, delta=0.0, epsilon=1e-9, ftol=1e-5, gtol=0.9, wolfe=0.9, past=0,
            max_linesearch=100)


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
    G, w0, f0 = np.zeros(N), np.full(N, 1.0 / N), np.zeros(M)
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        worst = 0.0
        for _ in range(calls):                               # the kernels alternately, from one process
            C = ctx.logw_cov(g=G, G=G, theta=10.0)[0]
            Cf = ctx.forces_gram(forces=f0, w0=w0, theta=10.0, hess=False)[0]
            worst = max(worst, float(np.abs(C - Cf).max() / np.abs(Cf).max()))
        flops = 2.0 * M * (M + 64) / 2 * N                   # the 64 x 64 sub-tiles of the lower triangle (M a multiple of 64): for the fraction of the peak
    return {"M": M, "N": N, "calls": calls, "max_dC_over_max_C": worst, "flops_one_matrix_lower_triangle": flops}


def minimizer_record(M, N, theta, reps, budget=None):
    import bioen_amd
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G, x0 = np.zeros(N), np.zeros(N)
    out = {"M": M, "N": N, "theta": theta, "reps": reps}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        kept = {}

        def lbfgs():
            gl, wl, info = ctx.opt_lbfgs_logw(x0, G, theta, CONV)
            kept["w_lbfgs"] = wl
            return {"status": info.lbfgs_code, "iterations": info.iterations, "evaluations": info.evaluations, "fmin": info.fmin}

        def dual():
            r = ctx.opt_dual_newton_logw(x0, G, theta, dict(gtol=1e-6))
            kept["g_dual"] = r["g"]
            return {"status": r["status"], "iterations": r["iterations"], "evaluations": r["evaluations"],
                    "factorisations": r["factorisations"], "fmin": r["fmin"], "gmax_over_wmax": r["gmax"] / r["wmax"]}

        legs = {"lbfgs": lbfgs, "dual_newton": dual}
        ctx.logw_cov(g=x0, G=G, theta=theta)                 # warm-up: the copies, the sets' buffer
        ctx.opt_dual_newton_logw(x0, G, theta, dict(max_iterations=1))      # ... and the factor's
        ctx.synchronize()
        times = {name: [] for name in legs}
        start = time.perf_counter()
        for rep in range(reps):                              # alternating; every run a cold start from x0
            if budget is not None and rep > 0 and time.perf_counter() - start > budget:
                break
            for name, run in legs.items():
                t0 = time.perf_counter()
                out[name] = run()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
                print("repetition %d %s: %.4f s %s" % (rep, name, times[name][-1], json.dumps(out[name])), file=sys.stderr, flush=True)
        out["reps_done"] = len(times["lbfgs"])
        for name in legs:
            out[name].update(spread(times[name]))
        wd = np.exp(kept["g_dual"] - kept["g_dual"].max())
        wd /= wd.sum()
        n, t = out["dual_newton"], out["lbfgs"]
        out["dfmin_dual_minus_lbfgs"] = n["fmin"] - t["fmin"]
        out["max_dw_over_max_w"] = float(np.abs(wd - kept["w_lbfgs"]).max() / kept["w_lbfgs"].max())
        out["dual_newton_over_lbfgs"] = round(n["median_s"] / t["median_s"], 4)
        out["dual_newton_faster_by_more_than_the_spreads"] = bool(
            t["median_s"] - n["median_s"] > (n["max_s"] - n["min_s"]) + (t["max_s"] - t["min_s"]))
    return out


def small_theta(M, N, theta):
    import bioen_amd
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G, x0, w0 = np.zeros(N), np.zeros(N), np.full(N, 1.0 / N)
    out = {"M": M, "N": N, "theta": theta, "segments": os.environ.get("BIOEN_HIP_SEGMENTS", "8")}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        t0 = time.perf_counter()
        r = ctx.opt_dual_newton_logw(x0, G, theta, dict(gtol=1e-6))
        out["dual_newton"] = {"seconds": round(time.perf_counter() - t0, 4), "status": r["status"], "iterations": r["iterations"],
                              "evaluations": r["evaluations"], "factorisations": r["factorisations"], "fmin": r["fmin"],
                              "gmax_over_wmax": r["gmax"] / r["wmax"], "wmax": r["wmax"]}
        t0 = time.perf_counter()
        fn = ctx.opt_newton_forces(np.zeros(M), w0, theta, dict(gtol=1e-6), want_weights=False)
        out["forces_newton"] = {"seconds": round(time.perf_counter() - t0, 4), "status": fn["status"], "iterations": fn["iterations"],
                                "evaluations": fn["evaluations"], "fmin": fn["fmin"], "gmax": fn["gmax"]}
        t0 = time.perf_counter()
        gl, wl, info = ctx.opt_lbfgs_logw(x0, G, theta, CONV)
        out["lbfgs"] = {"seconds": round(time.perf_counter() - t0, 4), "status": info.lbfgs_code, "iterations": info.iterations,
                        "evaluations": info.evaluations, "fmin": info.fmin}
        fmins = {k: out[k]["fmin"] for k in ("dual_newton", "forces_newton", "lbfgs")}
        out["lowest"] = min(fmins, key=fmins.get)
        out["above_the_lowest"] = {k: v - min(fmins.values()) for k, v in fmins.items()}
    return out


if "--minimizer" in flags:
    M = int(args[0]) if len(args) > 0 else 256
    N = int(args[1]) if len(args) > 1 else 100000
    theta = float(args[2]) if len(args) > 2 else 10.0
    print(json.dumps(minimizer_record(M, N, theta, int(args[3]) if len(args) > 3 else 5, float(args[4]) if len(args) > 4 else None)))
elif "--small-theta" in flags:
    M = int(args[0]) if len(args) > 0 else 300
    N = int(args[1]) if len(args) > 1 else 9000
    print(json.dumps(small_theta(M, N, float(args[2]) if len(args) > 2 else 0.1)))
else:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 1000000
    print(json.dumps(once(M, N, int(args[2]) if len(args) > 2 else 3)))

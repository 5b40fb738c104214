#!/usr/bin/env python3
"""What a Hessian-vector product costs (Context.logw_hessp) next to the yardstick it is built from, logw_fdf with a
gradient, in ONE process: wall time per call (each ends synchronised; the call shapes alternate) and the kernel times of
the two matrix passes and the four hessp kernels (kernel_stats).  Condition: a k = 1 product at the kept
point takes no longer than 1.10 x logw_fdf with gradient.

    python3 tools/hessp_probe.py [M] [N] [reps]              # GPU box; default 1024 x 1e6, 20 repetitions
    python3 tools/hessp_probe.py --minimizer [M] [N] [theta] [seconds]   # scipy Newton-CG on the device objective (driven
                                        # as find_optimum drives it) against the converged device L-BFGS, one seeded problem
                                        # (default 256 x 1e5, theta 10); Newton-CG is stopped after `seconds` (300), warnflag -1
"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402
import bioen_amd            # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
minimizer = "--minimizer" in sys.argv[1:]


def targets(M, rng):
    YTrue = rng.uniform(1, 10, M)
    sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
    return YTrue, sig_sim, sig_exp, rng.normal(YTrue, sig_exp) / sig_exp


def stats(x):
    x = np.asarray(x) * 1e3
    return {"mean_ms": round(float(x.mean()), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4),
            "std_ms": round(float(x.std()), 4)}


def timing(M, N, reps):
    rng = np.random.default_rng(12345)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G = np.zeros(N)
    x = 0.1 * rng.standard_normal(N)
    V = rng.standard_normal((8, N))
    theta = 10.0
    out = {"M": M, "N": N, "reps": reps, "theta": theta}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        shapes = {
            "logw_fdf_grad": lambda: ctx.logw_fdf(x, G, theta),
            "hessp_set_point_k1": lambda: ctx.logw_hessp(V[0], g=x, G=G, theta=theta),
            "hessp_kept_k1": lambda: ctx.logw_hessp(V[0]),
            "hessp_kept_k8": lambda: ctx.logw_hessp(V),
        }
        order = ["logw_fdf_grad", "hessp_set_point_k1", "hessp_kept_k1", "hessp_kept_k8"]     # a kept point follows a set one
        for _ in range(3):                                   # warm-up of every call shape (strip copies, work vectors)
            for name in order:
                shapes[name]()
        ctx.synchronize()
        times = {name: [] for name in order}
        for _ in range(reps):                                # alternating
            for name in order:
                t0 = time.perf_counter()
                shapes[name]()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
        out["wall"] = {name: stats(times[name]) for name in order}
        base = out["wall"]["logw_fdf_grad"]["mean_ms"]
        out["ratio_kept_k1_to_fdf"] = round(out["wall"]["hessp_kept_k1"]["mean_ms"] / base, 4)
        out["ratio_kept_k8_to_fdf"] = round(out["wall"]["hessp_kept_k8"]["mean_ms"] / base, 4)
        out["condition_k1_within_1.10"] = bool(out["ratio_kept_k1_to_fdf"] <= 1.10)
        # kernel times, per call shape: the two passes and the four new kernels
        ctx.kernel_stats_enable(True)
        out["kernels"] = {}
        for name in order:
            ctx.kernel_stats_reset()                         # (in this order the kept point is the one set just before)
            for _ in range(reps):
                shapes[name]()
            st = ctx.kernel_stats()
            out["kernels"][name] = {key: {"launches_per_call": v["launches"] / reps,
                                          "ms_per_call": round(v["total_ms"] / reps, 4)} for key, v in st.items()}
        ctx.kernel_stats_enable(False)
    return out


def minimizer_record(M, N, theta, budget):
    import scipy.optimize as sopt
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G = np.zeros(N)
    x0 = np.zeros(N)
    conv = dict(linesearch=2, max_iterations=200000, delta=0.0, epsilon=1e-9, ftol=1e-5, gtol=0.9, wolfe=0.9, past=0,
                max_linesearch=100)
    out = {"M": M, "N": N, "theta": theta}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        ctx.logw_fdf(x0, G, theta)
        t0 = time.perf_counter()
        gl, wl, info = ctx.opt_lbfgs_logw(x0, G, theta, conv)
        out["lbfgs_converged"] = {"seconds": round(time.perf_counter() - t0, 3), "iterations": info.iterations,
                                  "evaluations": info.evaluations, "code": info.lbfgs_code, "fmin": info.fmin}
        state = {"x": None, "f": None, "g": None, "evals": 0, "products": 0}
        t_stop = time.perf_counter() + budget

        def ev(x):                                           # as _DeviceFdf under the Newton drivers: the k = 0 call sets
            if state["x"] is None or not np.array_equal(x, state["x"]):        # the point, so a product at x repeats nothing
                _, state["f"], state["g"] = ctx.logw_hessp(None, g=x, G=G, theta=theta)
                state["x"] = x.copy()
                state["evals"] += 1

        def f(x):
            ev(x)
            return state["f"]

        def fp(x):
            ev(x)
            return state["g"]

        def hp(x, p):
            if time.perf_counter() > t_stop:
                raise TimeoutError
            state["products"] += 1
            if state["x"] is not None and np.array_equal(x, state["x"]):
                return ctx.logw_hessp(p)
            hv, state["f"], state["g"] = ctx.logw_hessp(p, g=x, G=G, theta=theta)
            state["x"] = x.copy()
            state["evals"] += 1
            return hv

        t0 = time.perf_counter()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = sopt.fmin_ncg(f, x0, fp, fhess_p=hp, avextol=1e-10, maxiter=400, full_output=True, disp=False)
        except TimeoutError:                                 # stopped at the budget: the counts so far, the last point seen
            res = (state["x"], state["f"], None, None, None, -1)
        dt = time.perf_counter() - t0
        wn = np.exp(res[0] - res[0].max())
        wn /= wn.sum()
        out["newton_cg"] = {"seconds": round(dt, 3), "evaluations": state["evals"], "products": state["products"],
                            "warnflag": int(res[5]), "fmin": float(res[1]),
                            "dfmin_vs_lbfgs": float(res[1] - info.fmin),
                            "max_dw_over_max_w": float(np.abs(wn - wl).max() / wl.max())}
    return out


if minimizer:
    M = int(args[0]) if len(args) > 0 else 256
    N = int(args[1]) if len(args) > 1 else 100000
    theta = float(args[2]) if len(args) > 2 else 10.0
    budget = float(args[3]) if len(args) > 3 else 300.0
    print(json.dumps(minimizer_record(M, N, theta, budget)))
else:
    M = int(args[0]) if len(args) > 0 else 1024
    N = int(args[1]) if len(args) > 1 else 1000000
    reps = int(args[2]) if len(args) > 2 else 20
    print(json.dumps(timing(M, N, reps)))

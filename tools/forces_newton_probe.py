#!/usr/bin/env python3
"""What the forces method's device-resident Newton minimizer costs (Context.opt_newton_forces), in ONE
process per case:

    python3 tools/forces_newton_probe.py --once [M] [N] [calls]          # point set, then k_forces_gram_bf16 and one
                                        # factorisation + one solve alternately, `calls` times each (default 3): for a
                                        # kernel-trace run of its own.  Condition: the summed kernel time of one
                                        # factorisation plus one solve <= one k_forces_gram_bf16 launch of the same run
    python3 tools/forces_newton_probe.py --lapack [M] [reps]             # host dpotrf + dpotrs wall time (no GPU), for information
    python3 tools/forces_newton_probe.py --minimizer [M] [N] [theta] [reps]   # whole-run wall time, cold start, gtol 1e-6:
                                        # the device L-BFGS, scipy's trust-exact with hessian = gram / gram_bf16 (driven as
                                        # find_optimum drives it) and newton with each source, alternating, `reps`
                                        # repetitions (default 5): median and min ... max (default 256 x 1e5, theta 10).
                                        # Condition: newton is faster than trust-exact with the same source by more than
                                        # the min ... max spread of the two
"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]


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
    w0 = np.full(N, 1.0 / N)
    f = 1e-3 * rng.standard_normal(M)
    b = rng.standard_normal(M)
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        H = ctx.forces_gram(cov=False)[1]                    # a caller's matrix: the factorisation alone, no Hessian pass in it
        lam = max(0.0, -np.linalg.eigvalsh(H).min()) + 1e-6 * np.abs(np.diag(H)).max()
        infos = []
        for _ in range(calls):                               # the kernels alternately, from one process
            ctx.forces_gram_bf16(cov=False)
            infos.append(ctx.forces_newton_factor(H, lam=lam, want_L=False)[1])
            x = ctx.forces_newton_solve(b)
        resid = float(np.abs((H + lam * np.eye(M)).dot(x) - b).max() / (np.abs(H).max() * np.abs(x).max()))
    return {"M": M, "N": N, "calls": calls, "infos": infos, "lambda": lam, "solve_residual_over_A_x": resid}


def lapack(M, reps):
    import scipy.linalg.lapack as la
    rng = np.random.default_rng(1)
    B = rng.standard_normal((M, M))
    A = B.dot(B.T) / M + np.eye(M)
    b = rng.standard_normal(M)
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        c, info = la.dpotrf(A, lower=1)
        x, info2 = la.dpotrs(c, b, lower=1)
        ts.append(time.perf_counter() - t0)
    return {"M": M, "host_dpotrf_plus_dpotrs": spread(ts[1:]), "threads": os.environ.get("OMP_NUM_THREADS")}


def minimizer_record(M, N, theta, reps):
    import bioen_amd
    import scipy.optimize as sopt
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    w0 = np.full(N, 1.0 / N)
    x0 = np.zeros(M)
    conv = dict(linesearch=2, max_iterations=200000, delta=0.0, epsilon=1e-9, ftol=1e-5, gtol=0.9, wolfe=0.9, past=0,
                max_linesearch=100)
    out = {"M": M, "N": N, "theta": theta, "reps": reps, "gtol": 1e-6}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:

        def lbfgs():
            fl, wl, info = ctx.opt_lbfgs_forces(x0, w0, theta, conv, want_weights=False)
            g = ctx.forces_fdf(fl, w0, theta)[1]
            return {"status": info.lbfgs_code, "iterations": info.iterations, "evaluations": info.evaluations,
                    "fmin": info.fmin, "max_abs_grad": float(np.abs(g).max())}

        def trust(source):
            state = {"x": None, "evals": 0, "hessians": 0}

            def ev(x):                                       # as _DeviceFdf under trust-exact: every evaluation sets the point
                if state["x"] is None or not np.array_equal(x, state["x"]):
                    _, state["f"], state["g"] = ctx.forces_hessp(None, forces=x, w0=w0, theta=theta)
                    state["x"] = x.copy()
                    state["evals"] += 1

            def f(x):
                ev(x)
                return state["f"]

            def fp(x):
                ev(x)
                return state["g"]

            def hess(x):
                ev(x)
                state["hessians"] += 1
                return (ctx.forces_gram_bf16 if source == "gram_bf16" else ctx.forces_gram)(cov=False)[1]

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = sopt.minimize(f, x0, method="trust-exact", jac=fp, hess=hess, options={"gtol": 1e-6, "maxiter": 200})
            return {"status": int(res.status), "iterations": int(res.nit), "evaluations": state["evals"],
                    "hessians": state["hessians"], "fmin": float(res.fun), "max_abs_grad": float(np.abs(res.jac).max())}

        def newton(source):
            r = ctx.opt_newton_forces(x0, w0, theta, dict(gtol=1e-6, hessian=source), want_weights=False)
            return {"status": r["status"], "iterations": r["iterations"], "evaluations": r["evaluations"],
                    "hessians": r["hessians"], "factorisations": r["factorisations"], "switched": r["switched"],
                    "fmin": r["fmin"], "max_abs_grad": r["gmax"], "lambda": r["lam"]}

        legs = {"lbfgs": lbfgs, "trust_exact_gram": lambda: trust("gram"), "trust_exact_gram_bf16": lambda: trust("gram_bf16"),
                "newton_gram": lambda: newton("gram"), "newton_gram_bf16": lambda: newton("gram_bf16")}
        ctx.forces_hessp(None, forces=x0, w0=w0, theta=theta)    # warm-up: the copies, the sets' buffers, the factor's buffer
        ctx.forces_gram(cov=False)
        ctx.forces_gram_bf16(cov=False)
        ctx.forces_newton_factor(None, source="gram", lam=1.0, want_L=False)
        ctx.synchronize()
        times = {name: [] for name in legs}
        for _ in range(reps):                                # alternating; every run a cold start from x0
            for name, run in legs.items():
                t0 = time.perf_counter()
                out[name] = run()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
        for name in legs:
            out[name].update(spread(times[name]))
        for source in ("gram", "gram_bf16"):
            n, t = out["newton_" + source], out["trust_exact_" + source]
            gap = t["median_s"] - n["median_s"]
            out["newton_%s_faster_by_more_than_the_spreads" % source] = bool(
                gap > (n["max_s"] - n["min_s"]) + (t["max_s"] - t["min_s"]))
            out["newton_%s_over_lbfgs" % source] = round(n["median_s"] / out["lbfgs"]["median_s"], 3)
            out["newton_%s_over_trust_exact" % source] = round(n["median_s"] / t["median_s"], 3)
    return out


if "--minimizer" in flags:
    M = int(args[0]) if len(args) > 0 else 256
    N = int(args[1]) if len(args) > 1 else 100000
    theta = float(args[2]) if len(args) > 2 else 10.0
    print(json.dumps(minimizer_record(M, N, theta, int(args[3]) if len(args) > 3 else 5)))
elif "--lapack" in flags:
    print(json.dumps(lapack(int(args[0]) if len(args) > 0 else 512, int(args[1]) if len(args) > 1 else 10)))
else:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 1000000
    print(json.dumps(once(M, N, int(args[2]) if len(args) > 2 else 3)))

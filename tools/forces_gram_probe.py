#!/usr/bin/env python3
"""What the dense Hessian of the forces objective costs in ONE compute-bound pass (Context.forces_gram) next to the method
it replaces, ceil(M / 8) batched products at the same kept point (Context.forces_hessian), in ONE process: wall time per
call, each ending synchronised, the call shapes alternating -- and, as a third leg, the same pass from split-BF16 operands
(Context.forces_gram_bf16) with one forces_fdf evaluation, the memory floor, as a fourth.  Conditions:
forces_gram(cov, hess) takes at most 0.5 x forces_hessian() and forces_gram_bf16 at most 0.5 x forces_gram
(by kernel time: a --once run under a kernel trace) at 512 x 1e6 and 1024 x 1e5.

    python3 tools/forces_gram_probe.py [M] [N] [reps]                # GPU box; default 512 x 1e6, 5 repetitions
    python3 tools/forces_gram_probe.py --once [M] [N] [calls]        # point set, then forces_gram and forces_gram_bf16 alternately, `calls` times each (default 2): for a counter or kernel-trace run
    python3 tools/forces_gram_probe.py --minimizer [M] [N] [theta]   # trust-exact with hessian = gram_bf16 / gram / products (--skip-products: without the last; driven as
                                        # find_optimum drives it), cold start, against the converged device L-BFGS on one
                                        # seeded problem (default 256 x 1e5, theta 10)
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
flags = [a for a in sys.argv[1:] if a.startswith("--")]
FP64_MATRIX_PEAK = 78.6e12


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
    w0 = np.full(N, 1.0 / N)
    f = 1e-3 * rng.standard_normal(M)
    theta = 10.0
    out = {"M": M, "N": N, "reps": reps, "theta": theta}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)
        shapes = {"forces_hessian_products": lambda: ctx.forces_hessian(),
                  "forces_gram_cov_hess": lambda: ctx.forces_gram(),
                  "forces_gram_bf16_cov_hess": lambda: ctx.forces_gram_bf16(),
                  "forces_hessp_point_only": lambda: ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)}   # = one forces_fdf
        order = list(shapes)
        Hp = shapes[order[0]]()                              # warm-up of the call shapes (work vectors, the sets' buffers)
        C, H = shapes[order[1]]()
        Cb, Hb = shapes[order[2]]()
        ctx.synchronize()
        times = {name: [] for name in order}
        for _ in range(reps):                                # alternating
            for name in order:
                t0 = time.perf_counter()
                shapes[name]()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
        out["wall"] = {name: stats(times[name]) for name in order}
        out["ratio_gram_to_products"] = round(out["wall"][order[1]]["mean_ms"] / out["wall"][order[0]]["mean_ms"], 4)
        out["condition_at_most_0.5"] = bool(out["ratio_gram_to_products"] <= 0.5)
        out["ratio_gram_bf16_to_gram"] = round(out["wall"][order[2]]["mean_ms"] / out["wall"][order[1]]["mean_ms"], 4)
        out["ratio_gram_bf16_to_one_evaluation"] = round(out["wall"][order[2]]["mean_ms"] / out["wall"][order[3]]["mean_ms"], 4)
        out["bf16_max_dH_over_max_H"] = float(np.abs(Hb - H).max() / np.abs(H).max())
        out["bf16_max_dC_over_max_C"] = float(np.abs(Cb - C).max() / np.abs(C).max())
        # the flops the pass performs: two M x M x N products on the lower triangle's 64 x 64 sub-tiles; of the floor 2 . 2 M^2 N
        nsl = -(-M // 64)
        done = 2 * 2 * (nsl * (nsl + 1) // 2) * 64 * 64 * float(N)
        out["fraction_of_fp64_matrix_peak"] = {
            "of_flops_performed": round(done / (out["wall"][order[1]]["min_ms"] * 1e-3) / FP64_MATRIX_PEAK, 4),
            "of_full_square_2x2MMN": round(4.0 * M * M * N / (out["wall"][order[1]]["min_ms"] * 1e-3) / FP64_MATRIX_PEAK, 4)}
        out["max_dH_over_max_H"] = float(np.abs(H - Hp).max() / np.abs(Hp).max())
        out["footprint"] = {"forms": sorted(ctx.footprint()[0]), "bytes": ctx.footprint()[1],
                            "matrix_bytes": 8 * (-(-M // 16) * 16) * N}
    return out


def once(M, N, calls=2):
    rng = np.random.default_rng(12345)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    w0 = np.full(N, 1.0 / N)
    f = 1e-3 * rng.standard_normal(M)
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        for _ in range(calls):                               # the two kernels alternately, from one process
            ctx.forces_gram()
            ctx.forces_gram_bf16()
    return {"M": M, "N": N, "forces_gram_calls": calls, "forces_gram_bf16_calls": calls}


def minimizer_record(M, N, theta):
    import scipy.optimize as sopt
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    w0 = np.full(N, 1.0 / N)
    x0 = np.zeros(M)
    conv = dict(linesearch=2, max_iterations=200000, delta=0.0, epsilon=1e-9, ftol=1e-5, gtol=0.9, wolfe=0.9, past=0,
                max_linesearch=100)
    out = {"M": M, "N": N, "theta": theta}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        ctx.forces_fdf(x0, w0, theta)
        t0 = time.perf_counter()
        fl, wl, info = ctx.opt_lbfgs_forces(x0, w0, theta, conv)
        out["lbfgs_converged"] = {"seconds": round(time.perf_counter() - t0, 3), "iterations": info.iterations,
                                  "evaluations": info.evaluations, "code": info.lbfgs_code, "fmin": info.fmin}
        for source in ("gram_bf16", "gram") + (() if "--skip-products" in flags else ("products",)):
            state = {"x": None, "f": None, "g": None, "evals": 0, "hessians": 0, "device_s": 0.0}

            def ev(x):                                       # as _DeviceFdf under trust-exact: every evaluation sets the point
                if state["x"] is None or not np.array_equal(x, state["x"]):
                    t = time.perf_counter()
                    _, state["f"], state["g"] = ctx.forces_hessp(None, forces=x, w0=w0, theta=theta)
                    state["device_s"] += time.perf_counter() - t
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
                t = time.perf_counter()
                try:
                    if source == "gram_bf16":
                        return ctx.forces_gram_bf16(cov=False)[1]
                    return ctx.forces_gram(cov=False)[1] if source == "gram" else ctx.forces_hessian()
                finally:
                    state["device_s"] += time.perf_counter() - t

            hess(x0)                                         # warm-up (the sets' buffer, the directions' work vectors)
            state.update(x=None, evals=0, hessians=0, device_s=0.0)
            t0 = time.perf_counter()
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    res = sopt.minimize(f, x0, method="trust-exact", jac=fp, hess=hess, options={"gtol": 1e-6, "maxiter": 200})
            except bioen_amd.BioenHipError as e:             # (forces_hessian refuses products that are not symmetric to 1e-10)
                out["trust_exact_" + source] = {"seconds": round(time.perf_counter() - t0, 3), "evaluations": state["evals"],
                                                "hessians": state["hessians"], "error": str(e)}
                continue
            dt = time.perf_counter() - t0
            wn = ctx.forces_weights(res.x, w0)
            out["trust_exact_" + source] = {"seconds": round(dt, 3), "seconds_in_device_calls": round(state["device_s"], 3),
                                            "seconds_in_scipy_on_the_host": round(dt - state["device_s"], 3), "iterations": int(res.nit), "evaluations": state["evals"],
                                            "hessians": state["hessians"], "success": bool(res.success),
                                            "status": int(res.status), "message": str(res.message), "fmin": float(res.fun),
                                            "max_abs_grad": float(np.abs(res.jac).max()),
                                            "dfmin_vs_lbfgs": float(res.fun - info.fmin),
                                            "max_dw_over_max_w": float(np.abs(wn - wl).max() / wl.max())}
        if "fmin" in out["trust_exact_gram"] and "fmin" in out["trust_exact_gram_bf16"]:
            out["dfmin_gram_bf16_vs_gram"] = out["trust_exact_gram_bf16"]["fmin"] - out["trust_exact_gram"]["fmin"]
        if "fmin" in out["trust_exact_gram"] and "fmin" in out.get("trust_exact_products", {}):
            out["dfmin_gram_vs_products"] = out["trust_exact_gram"]["fmin"] - out["trust_exact_products"]["fmin"]
    return out


if "--minimizer" in flags:
    M = int(args[0]) if len(args) > 0 else 256
    N = int(args[1]) if len(args) > 1 else 100000
    theta = float(args[2]) if len(args) > 2 else 10.0
    print(json.dumps(minimizer_record(M, N, theta)))
elif "--once" in flags:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 1000000
    print(json.dumps(once(M, N, int(args[2]) if len(args) > 2 else 2)))
else:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 1000000
    reps = int(args[2]) if len(args) > 2 else 5
    print(json.dumps(timing(M, N, reps)))

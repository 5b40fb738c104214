#!/usr/bin/env python3
"""What a Hessian-vector product of the forces objective costs (Context.forces_hessp) next to the yardstick it is built
from, forces_fdf with a gradient, in ONE process: wall time per call (each ends synchronised; the call shapes alternate)
and the kernel times of the matrix passes (kernel_stats).  Condition: a k = 1 product at the kept point
takes no longer than 1.10 x forces_fdf with gradient.

    python3 tools/forces_hessp_probe.py [M] [N] [reps]       # GPU box; default 512 x 1e6, 20 repetitions
    python3 tools/forces_hessp_probe.py --hessian [M] [N]    # one dense Hessian at the kept point (default 512 x 1e5)
    python3 tools/forces_hessp_probe.py --minimizer [M] [N] [theta]   # scipy trust-exact on the device objective (driven as
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
    V = rng.standard_normal((8, M))
    theta = 10.0
    out = {"M": M, "N": N, "reps": reps, "theta": theta}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        shapes = {
            "forces_fdf_grad": lambda: ctx.forces_fdf(f, w0, theta),
            "hessp_set_point_k0": lambda: ctx.forces_hessp(None, forces=f, w0=w0, theta=theta),
            "hessp_kept_k1": lambda: ctx.forces_hessp(V[0]),
            "hessp_kept_k8": lambda: ctx.forces_hessp(V),
        }
        order = ["forces_fdf_grad", "hessp_set_point_k0", "hessp_kept_k1", "hessp_kept_k8"]     # a kept point follows a set one
        for _ in range(3):                                   # warm-up of every call shape (strip copy, work vectors)
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
        base = out["wall"]["forces_fdf_grad"]["mean_ms"]
        out["ratio_kept_k1_to_fdf"] = round(out["wall"]["hessp_kept_k1"]["mean_ms"] / base, 4)
        out["ratio_kept_k8_to_fdf"] = round(out["wall"]["hessp_kept_k8"]["mean_ms"] / base, 4)
        out["ratio_set_point_to_fdf"] = round(out["wall"]["hessp_set_point_k0"]["mean_ms"] / base, 4)
        out["condition_k1_within_1.10"] = bool(out["ratio_kept_k1_to_fdf"] <= 1.10)
        ctx.kernel_stats_enable(True)
        out["kernels"] = {}
        for name in order:
            ctx.kernel_stats_reset()                         # (in this order the kept point is the one set just before)
            for _ in range(reps):
                shapes[name]()
            st = ctx.kernel_stats()
            out["kernels"][name] = {key: {"launches_per_call": v["launches"] / reps,
                                          "ms_per_call": round(v["total_ms"] / reps, 4)}
                                    for key, v in st.items() if v["launches"]}
        ctx.kernel_stats_enable(False)
    return out


def hessian_record(M, N):
    rng = np.random.default_rng(12345)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    w0 = np.full(N, 1.0 / N)
    f = 1e-3 * rng.standard_normal(M)
    out = {"M": M, "N": N, "theta": 10.0}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        ctx.forces_hessian()                                 # warm-up
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            H = ctx.forces_hessian()
            ts.append(time.perf_counter() - t0)
        raw = np.array([ctx.forces_hessp(np.eye(M)[i0:i0 + 8]) for i0 in range(0, M, 8)]).reshape(M, M)
        out["dense_hessian"] = stats(ts)
        out["products_per_hessian"] = -(-M // 8)
        out["asymmetry_over_max"] = float(np.abs(raw - raw.T).max() / np.abs(raw).max())
        ev = np.linalg.eigvalsh(H)
        out["eigenvalues_min_max"] = [float(ev[0]), float(ev[-1])]
    return out


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
        state = {"x": None, "f": None, "g": None, "evals": 0, "hessians": 0}

        def ev(x):                                           # as _DeviceFdf under trust-exact: every evaluation sets the point
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
            return ctx.forces_hessian()

        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = sopt.minimize(f, x0, method="trust-exact", jac=fp, hess=hess, options={"gtol": 1e-6, "maxiter": 200})
        dt = time.perf_counter() - t0
        wn = ctx.forces_weights(res.x, w0)
        per = -(-M // 8)
        out["trust_exact"] = {"seconds": round(dt, 3), "iterations": int(res.nit), "evaluations": state["evals"],
                              "hessians": state["hessians"], "products": state["hessians"] * per,
                              "matrix_passes": 3 * state["evals"] + 2 * per * state["hessians"],
                              "success": bool(res.success), "fmin": float(res.fun),
                              "dfmin_vs_lbfgs": float(res.fun - info.fmin),
                              "max_dw_over_max_w": float(np.abs(wn - wl).max() / wl.max())}
        out["lbfgs_converged"]["matrix_passes"] = 2 * info.evaluations
    return out


if "--minimizer" in flags:
    M = int(args[0]) if len(args) > 0 else 256
    N = int(args[1]) if len(args) > 1 else 100000
    theta = float(args[2]) if len(args) > 2 else 10.0
    print(json.dumps(minimizer_record(M, N, theta)))
elif "--hessian" in flags:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 100000
    print(json.dumps(hessian_record(M, N)))
else:
    M = int(args[0]) if len(args) > 0 else 512
    N = int(args[1]) if len(args) > 1 else 1000000
    reps = int(args[2]) if len(args) > 2 else 20
    print(json.dumps(timing(M, N, reps)))

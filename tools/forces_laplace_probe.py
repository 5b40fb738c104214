#!/usr/bin/env python3
"""What the Laplace error bars cost through the host and on the device (forces.laplace_error_bars, Context.forces_laplace;
DESIGN section 6i), in ONE process per case:

    python3 tools/forces_laplace_probe.py --wall [M] [N] [reps]     # laplace_error_bars(use_c=True) at one converged optimum
                                        # (theta = 10, the device Newton minimizer, gtol 1e-8) on one resident copy of the
                                        # matrix: the path through the host, on_device=True and on_device=True with
                                        # matrices=False, alternating, `reps` repetitions (default 10) after a warm-up:
                                        # median and min ... max.  Condition: the device path is faster than the host path
                                        # by more than the min ... max spread of the two
    python3 tools/forces_laplace_probe.py --parts [M] [N] [reps]    # where the wall time of the paths goes: the Context
                                        # calls they are made of, each alone at the same optimum, synchronised, median
    python3 tools/forces_laplace_probe.py --once [M] [N] [calls]    # the optimum set, then Context.forces_laplace() at the
                                        # kept point `calls` times (default 3): for a kernel-trace run of its own
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]
THETA = 10.0


def problem(M, N):
    """the generator of the tests (tests/test_hip_forces_laplace.py: optimum), filled row by row"""
    rng = np.random.default_rng(M * N)
    centre = rng.normal(0.0, 2.0, M)
    yT = np.empty((M, N))
    for i in range(M):
        yT[i] = rng.standard_normal(N)
        yT[i] += centre[i]
    w0 = rng.uniform(0.5, 1.5, N)
    w0 /= w0.sum()
    YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
    return yT, YT, w0


def spread(x):
    x = np.asarray(x)
    return {"median_ms": round(1e3 * float(np.median(x)), 3), "min_ms": round(1e3 * float(x.min()), 3),
            "max_ms": round(1e3 * float(x.max()), 3)}


def wall(M, N, reps):
    from bioen_amd.optimize import forces
    from bioen_amd.optimize.ext import c_bioen
    yT, YT, w0 = problem(M, N)
    out = {"M": M, "N": N, "theta": THETA, "reps": reps}
    with c_bioen.hold(yT, YT):
        ctx, _ = c_bioen._context_for(yT, YT)
        res = ctx.opt_newton_forces(np.zeros(M), w0, THETA, dict(gtol=1e-8), want_weights=False)
        fopt = res["forces"]
        out["optimum"] = {"status": res["status"], "iterations": res["iterations"], "max_abs_grad": res["gmax"]}
        legs = {"host_path": dict(), "on_device": dict(on_device=True), "on_device_no_matrices": dict(on_device=True, matrices=False)}
        results = {}
        for name, kw in legs.items():                        # warm-up: every buffer of every path
            results[name] = forces.laplace_error_bars(fopt, w0, yT, yT, YT, THETA, use_c=True, **kw)
        ctx.synchronize()
        times = {name: [] for name in legs}
        for _ in range(reps):
            for name, kw in legs.items():
                t0 = time.perf_counter()
                forces.laplace_error_bars(fopt, w0, yT, yT, YT, THETA, use_c=True, **kw)
                times[name].append(time.perf_counter() - t0)
        for name in legs:
            out[name] = spread(times[name])
        ref = results["host_path"]
        out["max_difference_of_largest_entry"] = {
            k: float(np.abs(results["on_device"][k] - ref[k]).max() / np.abs(ref[k]).max()) for k in sorted(ref)}
        for name in ("on_device", "on_device_no_matrices"):
            h, d = out["host_path"], out[name]
            gap = h["median_ms"] - d["median_ms"]
            out[name + "_faster_by_more_than_the_spreads"] = bool(gap > (h["max_ms"] - h["min_ms"]) + (d["max_ms"] - d["min_ms"]))
            out[name + "_over_host_path"] = round(d["median_ms"] / h["median_ms"], 3)
    return out


def parts(M, N, reps):
    import bioen_amd
    from bioen_amd.optimize import forces
    yT, YT, w0 = problem(M, N)
    out = {"M": M, "N": N, "reps": reps}
    with bioen_amd.Context(yT, YT) as ctx:
        fopt = ctx.opt_newton_forces(np.zeros(M), w0, THETA, dict(gtol=1e-8), want_weights=False)["forces"]
        C, H, _, _ = ctx.forces_gram(forces=fopt, w0=w0, theta=THETA)
        Hi = forces._laplace_inverse(H, THETA)
        legs = {
            "forces_gram(forces): point, pass, C and H down": lambda: ctx.forces_gram(forces=fopt, w0=w0, theta=THETA),
            "forces_gram(): pass, C and H down": lambda: ctx.forces_gram(),
            "host: _laplace_inverse(H)": lambda: forces._laplace_inverse(H, THETA),
            "host: C inv(H) C": lambda: C.dot(Hi).dot(C),
            "forces_colquad(inv(H)): inverse up, pass, n down": lambda: ctx.forces_colquad(Hi),
            "forces_laplace(): kept point, resident C and H, two covariances down": lambda: ctx.forces_laplace(),
            "forces_laplace(matrices=False): kept point": lambda: ctx.forces_laplace(matrices=False),
            "forces_laplace(forces, matrices=False): point, pass": lambda: ctx.forces_laplace(forces=fopt, w0=w0, theta=THETA,
                                                                                             matrices=False),
            "forces_weights": lambda: ctx.forces_weights(fopt, w0),
        }
        for name, run in legs.items():
            ctx.forces_gram(forces=fopt, w0=w0, theta=THETA)     # every leg from the same state: the point kept, the pass fresh
            run()
            ts = []
            for _ in range(reps):
                if name == "forces_weights":
                    ctx.forces_gram(forces=fopt, w0=w0, theta=THETA)
                ctx.synchronize()
                t0 = time.perf_counter()
                run()
                ts.append(time.perf_counter() - t0)
            out[name] = spread(ts)
    return out


def once(M, N, calls):
    import bioen_amd
    yT, YT, w0 = problem(M, N)
    with bioen_amd.Context(yT, YT) as ctx:
        res = ctx.opt_newton_forces(np.zeros(M), w0, THETA, dict(gtol=1e-8), want_weights=False)
        infos = [ctx.forces_laplace(matrices=False)["info"] for _ in range(calls)]
        ctx.forces_colquad(np.eye(M))                        # the host path's quadratic-form call, for its kernel beside them
    return {"M": M, "N": N, "calls": calls, "status": res["status"], "infos": infos}


M = int(args[0]) if len(args) > 0 else 1024
N = int(args[1]) if len(args) > 1 else 100000
if "--parts" in flags:
    print(json.dumps(parts(M, N, int(args[2]) if len(args) > 2 else 5), indent=1))
elif "--wall" in flags:
    print(json.dumps(wall(M, N, int(args[2]) if len(args) > 2 else 10)))
else:
    print(json.dumps(once(M, N, int(args[2]) if len(args) > 2 else 3)))

#!/usr/bin/env python3
"""What the DEER refinement with a modulation-depth nuisance parameter costs with the scale profiled out
(nuisance.series_profiled / Context.opt_dual_newton_logw_profile_series), at BASELINE configs[3] as
bench.deer_record builds it (N = 5e5 x M = 205, the bench's three thetas, one group), in ONE process:

    python3 tools/logw_profile_probe.py --series [N] [reps]     # wall time, the variants alternating, `reps` repetitions
                                        # (default 5): median and min ... max of
                                        #   (a) nuisance.series as bench.deer_record calls it: 10 x (L-BFGS, refit) per theta
                                        #   (b) the same alternation with opt_dual_newton_logw as the inner solver
                                        #   (c) series_profiled, warm, with gram and with gram_bf16
                                        # with Gram passes, evaluations, the final scales, fmin against (a), and (c)'s scale
                                        # against a 30-round (b).  Condition: (c) faster than (a) and than (b) by more than
                                        # the sum of the two spreads
    python3 tools/logw_profile_probe.py --once [N] [calls]      # for a kernel-trace run of its own: `calls` profiled
                                        # series and as many plain dual Newton series on the affine model they leave, so
                                        # that k_rows_combine_profile stands beside k_rows_combine<true> and the
                                        # k_lproj_* kernels beside k_lgram_finish and k_logw_gram
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]
THETAS, ITERATIONS, M0 = [100.0, 10.0, 1.0], 10, 0.15       # bench.deer_record's
PRM = dict(gtol=1e-6)


def spread(x):
    x = np.asarray(x)
    return {"median_s": round(float(np.median(x)), 4), "min_s": round(float(x.min()), 4), "max_s": round(float(x.max()), 4)}


def alternation_newton(ctx, thetas, G, YT, off, rounds, scale0=M0, tol=None):
    """nuisance.series's protocol with the dual Newton as the inner solver: `rounds` x (optimise at the fixed scale, refit)
    per theta, cold-started weights, the scale carried over; tol: stop a theta once the scale moves by less"""
    from bioen_amd import nuisance
    scale, out = scale0, []
    groups = [np.arange(ctx.m)]
    for theta in thetas:
        passes = evals = used = 0
        for _ in range(rounds):
            ctx.set_affine(off, np.full(ctx.m, scale))
            r = ctx.opt_dual_newton_logw(G, G, theta, PRM)
            passes += r["factorisations"]
            evals += r["evaluations"]
            used += 1
            yraw, _ = ctx.last_average()
            new = nuisance.refit_scales(yraw, YT, off, groups)[0]
            moved, scale = abs(new - scale), new
            if tol is not None and moved < tol:
                break
        out.append({"theta": theta, "fmin": r["fmin"], "scale": scale, "gram_passes": passes, "evaluations": evals,
                    "rounds": used, "status": r["status"]})
    ctx.set_affine(None, None)
    return out


def inputs(N):
    import bench
    Ft, YT, off = bench.deer_inputs(N, bench.SEED)
    return bench, Ft, YT, off


def series(N, reps):
    import bioen_amd
    from bioen_amd import nuisance
    bench, Ft, YT, off = inputs(N)
    G = np.zeros(N)
    out = {"M": int(Ft.shape[0]), "N": N, "thetas": THETAS, "reps": reps}
    with bioen_amd.Context(Ft, YT) as ctx:
        def leg_a():
            res = nuisance.series(ctx, THETAS, G, G, bench.LBFGS_DEFAULTS, YT, row_offset=off, scale0=M0, iterations=ITERATIONS)
            return {"fmin": [r["fmin"] for r in res], "scales": [r["scales"][0] for r in res],
                    "evaluations": [sum(t["evaluations"] for t in r["trace"]) for r in res], "gram_passes": [0] * len(res)}

        def leg_b():
            res = alternation_newton(ctx, THETAS, G, YT, off, ITERATIONS)
            return {"fmin": [r["fmin"] for r in res], "scales": [r["scale"] for r in res],
                    "evaluations": [r["evaluations"] for r in res], "gram_passes": [r["gram_passes"] for r in res]}

        def leg_c(hessian):
            def run():
                res = nuisance.series_profiled(ctx, THETAS, G, G, PRM, row_offset=off, hessian=hessian, warm=True)
                return {"fmin": [r["fmin"] for r in res], "scales": [r["scales"][0] for r in res],
                        "evaluations": [r["evaluations"] for r in res], "gram_passes": [r["factorisations"] for r in res],
                        "iterations": [r["iterations"] for r in res], "switched": [int(r["switched"]) for r in res]}
            return run

        legs = {"a_series_lbfgs": leg_a, "b_alternation_dual_newton": leg_b, "c_profiled_gram": leg_c("gram"),
                "c_profiled_gram_bf16": leg_c("gram_bf16")}
        # warm-up: the strip copies, the Gram buffers, the factor's, the profile's
        nuisance.series(ctx, THETAS[:1], G, G, bench.LBFGS_DEFAULTS, YT, row_offset=off, scale0=M0, iterations=1)
        ctx.opt_dual_newton_logw_profile_series(THETAS[:1], G, G, dict(PRM, max_iterations=1), row_offset=off, hessian="gram_bf16")
        ctx.set_affine(None, None)
        ctx.synchronize()
        times = {name: [] for name in legs}
        for rep in range(reps):                              # alternating
            for name, run in legs.items():
                t0 = time.perf_counter()
                res = run()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
                out[name] = res
                print("repetition %d %s: %.4f s" % (rep, name, times[name][-1]), file=sys.stderr, flush=True)
        for name in legs:
            out[name].update(spread(times[name]))
        ref = alternation_newton(ctx, THETAS, G, YT, off, 30, tol=1e-10)
        out["b_30_rounds"] = {"scales": [r["scale"] for r in ref], "fmin": [r["fmin"] for r in ref], "rounds": [r["rounds"] for r in ref]}
    a, b = out["a_series_lbfgs"], out["b_alternation_dual_newton"]
    for name in ("c_profiled_gram", "c_profiled_gram_bf16"):
        c = out[name]
        c["fmin_minus_a"] = [x - y for x, y in zip(c["fmin"], a["fmin"])]
        c["scale_vs_b_30_rounds_rel"] = [abs(x - y) / abs(y) for x, y in zip(c["scales"], out["b_30_rounds"]["scales"])]
        c["scale_agrees_to_1e-6"] = bool(max(c["scale_vs_b_30_rounds_rel"]) <= 1e-6)
        for other, key in ((a, "a"), (b, "b")):
            c["over_" + key] = round(c["median_s"] / other["median_s"], 4)
            c["below_%s_by_more_than_the_spreads" % key] = bool(
                other["median_s"] - c["median_s"] > (c["max_s"] - c["min_s"]) + (other["max_s"] - other["min_s"]))
    b["fmin_minus_a"] = [x - y for x, y in zip(b["fmin"], a["fmin"])]
    return out


def once(N, calls):
    import bioen_amd
    _, Ft, YT, off = inputs(N)
    G = np.zeros(N)
    with bioen_amd.Context(Ft, YT) as ctx:
        for _ in range(calls):
            res = ctx.opt_dual_newton_logw_profile_series(THETAS, G, G, PRM, row_offset=off)
            plain = ctx.opt_dual_newton_logw_series(THETAS[-1:], G, G, PRM)      # on the model (off, sigma) the call left
        ctx.set_affine(None, None)
    return {"M": int(Ft.shape[0]), "N": N, "calls": calls, "profiled_gram_passes": [r["factorisations"] for r in res],
            "profiled_evaluations": [r["evaluations"] for r in res], "plain_gram_passes": plain[0]["factorisations"],
            "plain_evaluations": plain[0]["evaluations"], "scales": [r["scales"][0] for r in res]}


N = int(args[0]) if len(args) > 0 else 500000
if "--series" in flags:
    print(json.dumps(series(N, int(args[1]) if len(args) > 1 else 5)))
else:
    print(json.dumps(once(N, int(args[1]) if len(args) > 1 else 2)))

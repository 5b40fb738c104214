#!/usr/bin/env python3
"""What the log-weights dual Newton over row panels costs (Context.set_dense_panels), ONE process per case:

    python3 tools/logw_panels_probe.py --once [calls] [N] [M ...]
                                        # per M (default 1024 2048 4096, N = 1e5): logw_cov_bf16 and logw_cov alternately at
                                        # the kept point g = G, `calls` times each (default 5), then one iteration of
                                        # opt_dual_newton_logw (one factorisation, one solve) -- for a kernel-trace run of its
                                        # own and, separately, a counter run (FETCH_SIZE).  M = 1024 runs k_logw_gram /
                                        # k_logw_gram_bf16, beyond it k_logw_gram_panels / k_logw_gram_bf16_panels: the same
                                        # session, the same process.  Prints the flops of the lower triangle's 64 x 64
                                        # sub-tiles and the bytes of the matrix per M
    python3 tools/logw_panels_probe.py --summarize DIR
                                        # the kernel-trace (and counter) CSVs under DIR: per kernel name and grid median
                                        # (min ... max) of its dispatches' durations; with the flops above the fraction of
                                        # the matrix peak; FETCH_SIZE per dispatch
    python3 tools/logw_panels_probe.py --runs [M] [N] [reps] [theta]
                                        # whole cold-start runs from g = G = 0 (default 2048 x 1e5, theta 10, 5
                                        # repetitions, alternating): opt_dual_newton_logw with gram and with gram_bf16
                                        # against the device L-BFGS at converged settings (epsilon 1e-9, no plateau test),
                                        # the only minimizer of the library at that shape without the switch.  Condition:
                                        # each dual Newton leg faster than the L-BFGS by more than the two spreads
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]
LBFGS_CONV = dict(linesearch=2, max_iterations=200000, delta=0.0, epsilon=1e-9, ftol=1e-5, gtol=0.9, wolfe=0.9, past=0,
                  max_linesearch=100)         # tests/conftest.py: LBFGS_CONV
PEAK_FP64, PEAK_BF16 = 78.6e12, 2516.6e12     # MI355X matrix peaks, dense, flop/s


def targets(M, rng):
    YTrue = rng.uniform(1, 10, M)
    sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
    return YTrue, sig_sim, sig_exp, rng.normal(YTrue, sig_exp) / sig_exp


def spread(x):
    x = np.asarray(x, dtype=float)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "count": int(x.size)}


def lower_triangle_flops(M, N):
    nsl = -(-M // 64)
    return 2.0 * (nsl * (nsl + 1) // 2) * 64 * 64 * N


def once(calls, N, Ms):
    import bioen_amd
    out = []
    for M in Ms:
        rng = np.random.default_rng(12345)
        YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
        G = np.zeros(N)
        with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
            if M > 1024:
                ctx.set_dense_panels()
            ctx.logw_cov(g=G, G=G, theta=10.0)               # the point, the copies and the sets' buffer
            worst = 0.0
            for _ in range(calls):                           # the kernels alternately
                Cb = ctx.logw_cov_bf16()
                C = ctx.logw_cov()
                worst = max(worst, float(np.abs(Cb - C).max()))
            res = ctx.opt_dual_newton_logw(G, G, 10.0, dict(max_iterations=1))
            forms, nbytes = ctx.footprint()
        out.append({"M": M, "N": N, "calls": calls, "max_dC": worst, "max_C": float(np.abs(C).max()),
                    "flops_lower_triangle": lower_triangle_flops(M, N), "matrix_bytes": 8.0 * M * N,
                    "footprint_bytes": nbytes, "forms": sorted(forms), "one_iteration": [res["status"], res["evaluations"]]})
        print(json.dumps(out[-1]), flush=True)
    return out


def summarize(root):
    """{kernel name | grid: spread of the durations in microseconds}, and FETCH_SIZE per dispatch where a counter CSV lies"""
    out = {"kernels_us": {}, "fetch_size_kb": {}}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        rows = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0]
                if "gram" in name or "fnewton" in name:
                    key = "%s | grid %s" % (name, r.get("Grid_Size", r.get("Grid_Size_X", "?")))
                    rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for key, v in rows.items():
            out["kernels_us"].setdefault(key, []).extend(v)
    for path in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0]
                if "logw_gram" in name and r["Counter_Name"] == "FETCH_SIZE":
                    key = "%s | grid %s" % (name, r.get("Grid_Size", "?"))
                    out["fetch_size_kb"].setdefault(key, []).append(float(r["Counter_Value"]))
    out["kernels_us"] = {k: spread(v) for k, v in sorted(out["kernels_us"].items())}
    out["fetch_size_kb"] = {k: spread(v) for k, v in sorted(out["fetch_size_kb"].items())}
    return out


def runs(M, N, reps, theta):
    import bioen_amd
    rng = np.random.default_rng(20260)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    G, x0 = np.zeros(N), np.zeros(N)
    prm = dict(gtol=1e-6)
    out = {"M": M, "N": N, "theta": theta, "reps": reps}
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=20260) as ctx:
        ctx.set_dense_panels()

        def lbfgs():
            info = ctx.opt_lbfgs_logw(x0, G, theta, LBFGS_CONV, want_weights=False)[2]
            return dict(fmin=info.fmin, iterations=info.iterations, evaluations=info.evaluations, status=info.lbfgs_code)

        legs = {"dual_newton_gram": lambda: ctx.opt_dual_newton_logw(x0, G, theta, prm),
                "dual_newton_gram_bf16": lambda: ctx.opt_dual_newton_logw(x0, G, theta, dict(prm, hessian="gram_bf16")),
                "lbfgs_converged": lbfgs}
        ctx.logw_cov_bf16(g=x0, G=G, theta=theta)            # warm-up: the copies, the sets' buffer
        ctx.opt_dual_newton_logw(x0, G, theta, dict(max_iterations=1))      # ... and the factor's
        ctx.synchronize()
        times = {name: [] for name in legs}
        for rep in range(reps):                              # alternating
            for name, run in legs.items():
                t0 = time.perf_counter()
                res = run()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
                out[name] = {k: res[k] for k in ("fmin", "iterations", "evaluations", "status", "factorisations", "bf16_passes",
                                                 "switched") if k in res}
                print("repetition %d %s: %.4f s" % (rep, name, times[name][-1]), file=sys.stderr, flush=True)
        for name in legs:
            out[name]["seconds"] = spread(times[name])
        lb = out["lbfgs_converged"]
        for name in ("dual_newton_gram", "dual_newton_gram_bf16"):
            a = out[name]
            a["fmin_minus_lbfgs"] = a["fmin"] - lb["fmin"]
            a["lbfgs_over_this"] = round(lb["seconds"]["median"] / a["seconds"]["median"], 2)
            a["margin_s"] = lb["seconds"]["median"] - a["seconds"]["median"]
            a["faster_by_more_than_the_spreads"] = bool(
                a["margin_s"] > (a["seconds"]["max"] - a["seconds"]["min"]) + (lb["seconds"]["max"] - lb["seconds"]["min"]))
    return out


if "--summarize" in flags:
    print(json.dumps(summarize(args[0]), indent=1))
elif "--runs" in flags:
    M = int(args[0]) if len(args) > 0 else 2048
    N = int(args[1]) if len(args) > 1 else 100000
    reps = int(args[2]) if len(args) > 2 else 5
    print(json.dumps(runs(M, N, reps, float(args[3]) if len(args) > 3 else 10.0)))
else:
    calls = int(args[0]) if len(args) > 0 else 5
    N = int(args[1]) if len(args) > 1 else 100000
    once(calls, N, [int(a) for a in args[2:]] or [1024, 2048, 4096])

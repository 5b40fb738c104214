#!/usr/bin/env python3
"""What one quadratic form per structure, v_j = a_j^T P a_j, costs in ONE compute-bound pass (Context.forces_colquad) next
to the yardstick of the code before it: without the kernel the N numbers cost one column-sum pass per 8 directions,
ceil(M / 8) passes -- half of what Context.forces_hessian() runs (2 ceil(M / 8)) at the same kept point.  ONE process, wall
time per call, each ending synchronised, the two call shapes alternating.  P is the inverse of the point's own Hessian
(forces_gram), shifted by a multiple of I where H is not positive definite.  Condition: the median of
forces_colquad is at most 0.5 x the median of forces_hessian at 512 x 1e6 and 1024 x 1e5.

    python3 tools/forces_colquad_probe.py [M] [N] [reps]            # GPU box; default 512 x 1e6, 10 repetitions
    python3 tools/forces_colquad_probe.py --once [M] [N] [calls]    # point set, forces_gram once, then forces_colquad `calls`
                                                                    # times (default 2): for a counter or kernel-trace run
"""
import json
import os
import sys
import time

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
    return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4),
            "max_ms": round(float(x.max()), 4), "mean_ms": round(float(x.mean()), 4)}


def inverse_of_the_hessian(ctx):
    """-> (P, shift): inv(H + shift I) at the kept point, shift = 0 where H is positive definite"""
    H = ctx.forces_gram(cov=False)[1]
    lo = float(np.linalg.eigvalsh(H)[0])
    shift = 0.0 if lo > 0 else 1e-3 * float(np.abs(H).max()) - lo
    P = np.linalg.inv(H + shift * np.eye(H.shape[0]))
    return 0.5 * (P + P.T), shift


def setup(M, N):
    rng = np.random.default_rng(12345)
    YTrue, sig_sim, sig_exp, YTilde = targets(M, rng)
    return (YTrue, sig_sim, sig_exp, YTilde), np.full(N, 1.0 / N), 1e-3 * rng.standard_normal(M)


def timing(M, N, reps):
    syn, w0, f = setup(M, N)
    theta = 10.0
    out = {"M": M, "N": N, "reps": reps, "theta": theta}
    with bioen_amd.Context.synthetic(M, N, *syn, seed=12345) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)
        P, out["shift"] = inverse_of_the_hessian(ctx)
        shapes = {"forces_hessian_products": lambda: ctx.forces_hessian(),
                  "forces_colquad": lambda: ctx.forces_colquad(P)}
        order = list(shapes)
        shapes[order[0]]()                                   # warm-up of both call shapes (work vectors, the entry's buffer)
        v = shapes[order[1]]()
        ctx.synchronize()
        times = {name: [] for name in order}
        for _ in range(reps):                                # alternating
            for name in order:
                t0 = time.perf_counter()
                shapes[name]()
                ctx.synchronize()
                times[name].append(time.perf_counter() - t0)
        out["wall"] = {name: stats(times[name]) for name in order}
        out["ratio_of_medians_colquad_to_products"] = round(out["wall"][order[1]]["median_ms"] / out["wall"][order[0]]["median_ms"], 4)
        out["condition_at_most_0.5"] = bool(out["ratio_of_medians_colquad_to_products"] <= 0.5)
        # the flops the pass performs: per panel of 32 columns and slice s of 64 rows, every wave multiplies its blocks
        # kb >= s (the lower triangle of P in 16-row blocks; a block of the slice above the wave's own is multiplied by
        # zero: counted) -- two matrix instructions of 2048 flops per block and step of four rows
        mps = -(-M // 16) * 16
        nsl, nst = -(-mps // 64), mps // 4
        done = float(sum(min(16, nst - 16 * s) * (nsl - s) for s in range(nsl)) * 2 * 4 * 2048) * -(-N // 32)
        best = out["wall"][order[1]]["min_ms"] * 1e-3
        out["wall_fraction_of_fp64_matrix_peak"] = {"of_flops_performed": round(done / best / FP64_MATRIX_PEAK, 4),
                                                    "of_2MMN": round(2.0 * M * M * N / best / FP64_MATRIX_PEAK, 4)}
        out["flops_performed"] = done
        out["v_min_max"] = [float(v.min()), float(v.max())]
        out["footprint"] = {"forms": sorted(ctx.footprint()[0]), "bytes": ctx.footprint()[1],
                            "matrix_bytes": 8 * (-(-M // 16) * 16) * N}
    return out


def once(M, N, calls=2):
    syn, w0, f = setup(M, N)
    with bioen_amd.Context.synthetic(M, N, *syn, seed=12345) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        P, shift = inverse_of_the_hessian(ctx)               # (one forces_gram call: k_forces_gram is in the same trace)
        for _ in range(calls):
            ctx.forces_colquad(P)
    return {"M": M, "N": N, "forces_colquad_calls": calls, "shift": shift}


M = int(args[0]) if len(args) > 0 else 512
N = int(args[1]) if len(args) > 1 else 1000000
if "--once" in flags:
    print(json.dumps(once(M, N, int(args[2]) if len(args) > 2 else 2)))
else:
    print(json.dumps(timing(M, N, int(args[2]) if len(args) > 2 else 10)))

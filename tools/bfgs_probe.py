"""Per-iteration cost of the dense inverse-Hessian BFGS session (bioen_amd/bfgs.py, csrc/kernels_bfgs.hip) on one GPU:
the H pass (bioen_hip_bfgs_logw_update: one read + one write of ld^2 doubles, the four dots and the direction), one
evaluation (a trial with its gradient: forward + adjoint matrix passes) and the host driver's own time per iteration,
at M = 1024 and N = 1e4, 3e4, 1e5 (H = 0.8, 7.2, 80 GB: the first is ~3 x the Infinity Cache, the others far past it).
The H pass's achieved rate 2 ld^2 8 B / t is printed beside the box's read probe (a plain read stream over the
resident matrix).

    python tools/bfgs_probe.py [--n 10000 30000 100000] [--m 1024] [--iters 6]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def probe(n, m, iters):
    import bioen_amd
    from bioen_amd import bfgs
    rng = np.random.default_rng(1)
    ytrue = rng.uniform(1, 10, m)
    ctx = bioen_amd.Context.synthetic(m, n, ytrue, 0.5 * ytrue, 0.1 * ytrue, rng.normal(ytrue, 0.1 * ytrue) / (0.1 * ytrue))
    try:
        G = np.zeros(n)
        g0 = 0.01 * rng.standard_normal(n)
        ld = (n + 15) // 16 * 16
        read_gbs, _ = ctx.read_probe(reps=5)
        ctx.bfgs_begin(g0, G, 10.0, True)
        t_pass, t_eval = [], []
        for k in range(iters):
            t0 = time.perf_counter()
            ctx.bfgs_trial(0.5, True)
            t_eval.append(time.perf_counter() - t0)
            ctx.bfgs_accept(0.5, True)
            t0 = time.perf_counter()
            ctx.bfgs_update()
            if k >= 1:                 # k = 0: H_0 = I, no pass; k = 1: the pass synthesises I (writes only)
                t_pass.append(time.perf_counter() - t0)
        ctx.bfgs_end()
        # the host driver's own time per iteration: a short real run, minus its device calls
        t0 = time.perf_counter()
        backend = bfgs.DeviceBackend(ctx, g0, G, 10.0)
        calls = {"dev": 0.0}
        for name in ("bfgs_trial", "bfgs_accept", "bfgs_update"):
            fn = getattr(ctx, name)

            def timed(*a, _fn=fn):
                s = time.perf_counter()
                try:
                    return _fn(*a)
                finally:
                    calls["dev"] += time.perf_counter() - s
            setattr(ctx, name, timed)
        res = bfgs.minimize(backend, n, gtol=1e-30, maxiter=4)
        total = time.perf_counter() - t0
        ctx.bfgs_end()
        host = (total - calls["dev"]) / max(1, res.iterations)
    finally:
        ctx.close()
    tp = float(np.median(t_pass))
    te = float(np.median(t_eval))
    rate = 2.0 * ld * ld * 8 / tp / 1e9
    print("N = %-7d M = %d  H %.2f GB  pass %.3f ms (%.0f GB/s; read probe %.0f GB/s)  evaluation %.3f ms  host %.3f ms"
          % (n, m, ld * ld * 8e-9, tp * 1e3, rate, read_gbs, te * 1e3, host * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 30000, 100000])
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    for n in a.n:
        probe(n, a.m, a.iters)


if __name__ == "__main__":
    main()

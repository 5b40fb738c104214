#!/usr/bin/env python3
"""DEER refinement with the modulation depth profiled out, on one MI355X (needs the built library and a GPU; there is no CPU
path): the measured trace exp-370-292 against N seeded rotamer distances, the modulation depth a nuisance parameter that
enters the model affinely, y~(m) = 1/sigma + m (F - 1)/sigma.  The reference's protocol alternates ten times per theta
between a BioEn optimisation and a least-squares refit of m (nuisance.series); nuisance.series_profiled makes the refit
part of every evaluation of ONE dual Newton run per theta and ends at the alternation's fixed point.

    make -C bioen_amd/csrc && python examples/deer_profiled.py [N]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                       # noqa: E402  (deer_inputs: the matrix (F - 1) / sigma, the target, 1 / sigma)
import bioen_amd                                   # noqa: E402
from bioen_amd import nuisance                     # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
thetas = [100.0, 10.0, 1.0]
Ft, YT, off = bench.deer_inputs(N, bench.SEED)
G = np.zeros(N)

with bioen_amd.Context(Ft, YT) as ctx:
    for name, run in (
            ("alternation, 10 x (L-BFGS, refit)", lambda: nuisance.series(ctx, thetas, G, G, bench.LBFGS_DEFAULTS, YT,
                                                                        row_offset=off, scale0=0.15, iterations=10)),
            ("profiled, dual Newton", lambda: nuisance.series_profiled(ctx, thetas, G, G, dict(gtol=1e-6), row_offset=off)),
            ("profiled, split-BF16 covariance", lambda: nuisance.series_profiled(ctx, thetas, G, G, dict(gtol=1e-6),
                                                                                 row_offset=off, hessian="gram_bf16"))):
        run()                                      # (the first call builds the copies and the buffers)
        ctx.synchronize()
        t0 = time.perf_counter()
        res = run()
        ctx.synchronize()
        print("%-34s %.4f s" % (name, time.perf_counter() - t0))
        for r in res:
            extra = ("%d iterations, %d evaluations" % (r["iterations"], r["evaluations"])) if "iterations" in r else \
                ("%d evaluations" % sum(t["evaluations"] for t in r["trace"]))
            print("    theta %5g: modulation depth %.9f, fmin %.9f, chi2 %.6f, S %.6f  (%s)"
                  % (r["theta"], r["scales"][0], r["fmin"], r["chi2"], r["S"], extra))

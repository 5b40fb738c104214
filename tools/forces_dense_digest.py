#!/usr/bin/env python3
"""SHA-256 of the bytes of every output of the dense forces entries (forces_gram, forces_gram_bf16, forces_colquad,
opt_newton_forces, forces_newton_factor / _solve, forces_inverse, forces_laplace) and of the log-weights
dense entries (logw_cov, opt_dual_newton_logw, with logw_hessp at their point; logw_cov_bf16 and
opt_dual_newton_logw_series over three theta from both covariance sources, its statuses and `switched` in clear)
on seeded synthetic contexts, as JSON: two builds of the library that print the same digests compute the same bits.

    python3 tools/forces_dense_digest.py > new.json
    BIOEN_HIP_LIBRARY=/path/to/other/libbioen_hip.so python3 tools/forces_dense_digest.py > old.json

One process, whatever library BIOEN_HIP_LIBRARY selects.  Cases (M x N): 28 x 300, 65 x 257, 129 x 257, 205 x 1000,
513 x 1537, 1024 x 2049; 129 x 257 and 513 x 1537 once more with an affine model set, 129 x 257 once more with
BIOEN_HIP_SEGMENTS=1 (one column segment).  `--cases 65x257,129x257:affine` runs a selection.
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402

THETA = 10.0
SERIES_THETAS = [1000.0, 10.0, 0.316]
CASES = ["28x300", "65x257", "129x257", "205x1000", "513x1537", "1024x2049", "129x257:affine", "513x1537:affine",
         "129x257:segments1"]


def problem(M, N):
    """the generator of tools/forces_laplace_probe.py"""
    rng = np.random.default_rng(M * N)
    centre = rng.normal(0.0, 2.0, M)
    yT = rng.standard_normal((M, N)) + centre[:, None]
    w0 = rng.uniform(0.5, 1.5, N)
    w0 /= w0.sum()
    YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
    return rng, yT, YT, w0


def sha(*values):
    """one digest over arrays (their bytes) and scalars (repr: exact for floats)"""
    h = hashlib.sha256()
    for v in values:
        h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()


def run_case(case):
    import bioen_amd
    shape, _, variant = case.partition(":")
    M, N = (int(x) for x in shape.split("x"))
    rng, yT, YT, w0 = problem(M, N)
    segments = os.environ.get("BIOEN_HIP_SEGMENTS")          # the caller's, put back below
    if variant == "segments1":
        os.environ["BIOEN_HIP_SEGMENTS"] = "1"              # read when the context is created
    out = {}
    try:
        with bioen_amd.Context(yT, YT) as ctx:
            if variant == "affine":
                ctx.set_affine(rng.normal(0.0, 0.5, M), rng.uniform(0.5, 2.0, M))
            point = 1e-2 * rng.standard_normal(M)
            C, H, f, grad = ctx.forces_gram(forces=point, w0=w0, theta=THETA)
            out["forces_gram"] = sha(C, H, f, grad)
            out["forces_gram_bf16"] = sha(*ctx.forces_gram_bf16(forces=point, w0=w0, theta=THETA))
            out["forces_colquad(C)"] = sha(ctx.forces_colquad(C))
            res = None
            for source in ("gram_bf16", "gram"):                # the FP64 source last: its optimum is the kept point below
                res = ctx.opt_newton_forces(np.zeros(M), w0, THETA, dict(gtol=1e-8, hessian=source))
                out["opt_newton_forces(%s)" % source] = sha(*(res[k] for k in sorted(res)))
            for source in ("gram", "gram_bf16"):
                L, info = ctx.forces_newton_factor(source=source)
                out["forces_newton_factor(%s)" % source] = sha(L if L is not None else "none", info)
            B = rng.standard_normal((8, M))
            ctx.forces_newton_factor(source="gram", want_L=False)
            out["forces_newton_solve(k=1)"] = sha(ctx.forces_newton_solve(B[0]))
            out["forces_newton_solve(k=8)"] = sha(ctx.forces_newton_solve(B))
            _, logdet, info = ctx.forces_inverse()
            out["forces_inverse()"] = sha(logdet, info)
            _, Hopt = ctx.forces_gram(cov=False)
            Ainv, logdet, info = ctx.forces_inverse(Hopt)
            out["forces_inverse(H)"] = sha(Ainv if Ainv is not None else "none", logdet, info)
            for matrices in (True, False):
                lap = ctx.forces_laplace(matrices=matrices)
                out["forces_laplace(matrices=%s)" % matrices] = sha(*(lap[k] if lap[k] is not None else "none" for k in sorted(lap)))
            A = Hopt.copy()
            A[M // 2, M // 2] = -1.0                             # indefinite: the factorisation ends at that pivot
            L, info = ctx.forces_newton_factor(A)
            out["forces_newton_factor(indefinite)"] = sha("none" if L is None else L, info)
            out["info_indefinite"] = info
            out["newton_status"] = res["status"]
            # the log-weights dense entries, on the same context (draws of their own: the digests above stay what they were)
            lrng = np.random.default_rng(M * N + 1)
            G = np.log(w0)
            g = G + 0.1 * lrng.standard_normal(N)
            out["logw_cov(g)"] = sha(*ctx.logw_cov(g=g, G=G, theta=THETA))
            out["logw_cov()"] = sha(ctx.logw_cov())
            V = lrng.standard_normal((8, N))
            out["logw_hessp(k=1)"] = sha(ctx.logw_hessp(V[0]))
            out["logw_hessp(k=8)"] = sha(ctx.logw_hessp(V))
            dn = ctx.opt_dual_newton_logw(g, G, THETA, dict(gtol=1e-8))
            out["opt_dual_newton_logw"] = sha(*(dn[k] for k in sorted(dn)))
            out["logw_cov() at the optimum"] = sha(ctx.logw_cov())
            out["dual_newton_status"] = dn["status"]
            # the split-BF16 covariance and the theta series, draws of their own again
            srng = np.random.default_rng(M * N + 2)
            g = G + 0.1 * srng.standard_normal(N)
            out["logw_cov_bf16(g)"] = sha(*ctx.logw_cov_bf16(g=g, G=G, theta=THETA))
            out["logw_cov_bf16()"] = sha(ctx.logw_cov_bf16())
            for source, warm in (("gram_bf16", True), ("gram_bf16", False), ("gram", True)):
                tag = "%s, %s" % (source, "warm" if warm else "cold")
                ser = ctx.opt_dual_newton_logw_series(SERIES_THETAS, g, G, dict(gtol=1e-8), hessian=source, warm=warm)
                out["opt_dual_newton_logw_series(%s)" % tag] = sha(*(r[k] for r in ser for k in sorted(r)))
                out["series_status(%s)" % tag] = [r["status"] for r in ser]
                out["series_switched(%s)" % tag] = [int(r["switched"]) for r in ser]
    finally:
        if segments is None:
            os.environ.pop("BIOEN_HIP_SEGMENTS", None)
        else:
            os.environ["BIOEN_HIP_SEGMENTS"] = segments
    return out


def main():
    cases = CASES
    if "--cases" in sys.argv:
        cases = sys.argv[sys.argv.index("--cases") + 1].split(",")
    from bioen_amd import _lib
    out = {"library": os.environ.get("BIOEN_HIP_LIBRARY", "default"), "cases": {}}
    _lib.lib()
    for case in cases:
        out["cases"][case] = run_case(case)
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

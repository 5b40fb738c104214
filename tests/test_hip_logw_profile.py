"""GPU tests of the dual Newton minimizer with the nuisance scales profiled out (csrc/kernels_logw_profile.hip,
csrc/api_logw_profile.cpp, Context.opt_dual_newton_logw_profile_series, nuisance.series_profiled) against
its numpy statement (log_weights.dual_newton_profile_base) and, for the step, against 80-bit arithmetic.

The shapes are the smallest at which the new kernels can go wrong:

  deer105    105 x 400,    two contiguous groups (60 + 45 rows: the second starts inside a 64-row slice), an offset
  deer205    205 x 20000,  one group, an offset: the measured DEER trace of BASELINE configs[3]; eight segments and one
  scat130    130 x 400,    two INTERLEAVED groups (even / odd rows of the first 120) and ten rows in no group, no offset,
                           one canonical segment
  big1024    1024 x 400,   three groups -- one 64-row slice exactly, rows 64 .. 499 across seven slices, the rest --, every
                           thread of the one-block kernels with four rows, mp = m

What is compared: the evaluation (the scales are refit_scales of the raw averages, f is the affine model's at those
scales), ONE accepted step against g0 + u in numpy.longdouble, the whole loop count for count, the optimum from both
covariance sources, warm against cold, and what the entry refuses and leaves behind."""
import numpy as np
import pytest

from test_logw_profile import deer_fixture, deer_problem

from bioen_amd import nuisance
from bioen_amd.optimize import log_weights as lw

pytestmark = pytest.mark.gpu

L = np.longdouble
PARAMS = dict(gtol=1e-6, max_iterations=60)
# the device's scales against the restatement's at the optimum: ten times the largest relative difference measured on these
# cases (7.3e-14, deer205 on one segment from the split-BF16 covariance; from the FP64 one 5.8e-15: DESIGN 6m)
SCALE_GATE = 7.3e-13
# two runs that reach the same optimum by different paths (warm and cold starts), each to gtol: the issue's bound
OPTIMUM_GATE = 1e-6


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


def _intensities(M, N, seed, groups, truth):
    """scattering-like curves I_ij > 0 in units of sigma; the target is truth_k x a mixture's average in group k, the
    average itself in the rows of no group, plus unit noise"""
    rng = np.random.default_rng(seed)
    q = np.linspace(0.05, 1.0, M)
    rg = rng.uniform(1.0, 3.0, N)
    Y = np.exp(-(q[:, None] * rg[None, :]) ** 2 / 3.0) / 0.02
    target = Y.dot(rng.dirichlet(np.ones(N)))
    for t, ix in zip(truth, groups):
        target[ix] *= t
    return Y, target + rng.standard_normal(M)


_CASES = {}


def case(name):
    """-> dict(Y, YT, off, groups, G, g0, theta, segments): theta is large enough that the restatement accepts alpha = 1 in
    its first iteration (asserted where it matters)"""
    if name not in _CASES:
        if name == "deer105":
            Y, YT, off, groups = deer_problem()
            c = dict(Y=Y, YT=YT, off=off, groups=groups, theta=50.0, segments=8)
        elif name in ("deer205", "deer205_1seg"):
            Y, YT, off = deer_fixture(20000, seed=7)
            c = dict(Y=Y, YT=YT, off=off, groups=None, theta=100.0, segments=1 if name.endswith("1seg") else 8)
        elif name == "scat130":
            groups = [np.arange(0, 120, 2), np.arange(1, 120, 2)]
            Y, YT = _intensities(130, 400, 5, groups, (1.7, 0.6))
            c = dict(Y=Y, YT=YT, off=None, groups=groups, theta=20.0, segments=1)
        elif name == "big1024":
            groups = [np.arange(0, 64), np.arange(64, 500), np.arange(500, 1024)]
            Y, YT = _intensities(1024, 400, 9, groups, (1.7, 0.6, 1.2))
            c = dict(Y=Y, YT=YT, off=None, groups=groups, theta=100.0, segments=8)
        n = c["Y"].shape[1]
        c["G"] = np.zeros(n)
        c["g0"] = 0.1 * np.random.default_rng(21).standard_normal(n)
        _CASES[name] = c
    return _CASES[name]


CASES = ["deer105", "deer205", "deer205_1seg", "scat130", "big1024"]
_HOST = {}


def host_run(name, **over):
    key = (name, tuple(sorted(over.items())))
    if key not in _HOST:
        c = case(name)
        _HOST[key] = lw.dual_newton_profile_base(c["g0"], c["G"], c["Y"], c["YT"], c["theta"], dict(PARAMS, **over), c["groups"],
                                                 c["off"])
    return _HOST[key]


def context(bioen_amd, monkeypatch, c):
    if c["segments"] == 1:
        monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")
    ctx = bioen_amd.Context(c["Y"], c["YT"])
    return ctx


def sigma_of(c, scales):
    m = c["Y"].shape[0]
    sg = np.ones(m)
    for s, ix in zip(scales, c["groups"] if c["groups"] is not None else [np.arange(m)]):
        sg[ix] = s
    return sg


def device_run(ctx, c, **over):
    p = dict(PARAMS, **over)
    return ctx.opt_dual_newton_logw_profile_series([c["theta"]], c["g0"], c["G"], p, groups=c["groups"], row_offset=c["off"])[0]


# ---- the evaluation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_evaluation(bioen_amd, monkeypatch, name):
    c = case(name)
    m = c["Y"].shape[0]
    groups = c["groups"] if c["groups"] is not None else [np.arange(m)]
    with context(bioen_amd, monkeypatch, c) as ctx:
        assert ctx.strip_plan(0)["local_segments"] == c["segments"]
        r = device_run(ctx, c, max_iterations=0)
        assert r["status"] == 1 and r["iterations"] == 0 and r["evaluations"] == 1 and r["factorisations"] == 0
        assert np.array_equal(r["g"], c["g0"])
        yraw, yeff = ctx.last_average()
        want = nuisance.refit_scales(yraw, c["YT"], c["off"], groups)
        rel = max(abs(a - b) / abs(b) for a, b in zip(r["scales"], want))
        sg = sigma_of(c, r["scales"])
        # the model the call left is (off, sigma): the effective averages, and f of the plain evaluation there
        off = np.zeros(m) if c["off"] is None else c["off"]
        assert (np.abs(yeff - (off + sg * yraw)) <= 4 * np.finfo(float).eps * (np.abs(off) + np.abs(sg * yraw))).all()
        f_left, _ = ctx.logw_fdf(c["g0"], c["G"], c["theta"])
        ctx.set_affine(c["off"], sg)
        f_set, _ = ctx.logw_fdf(c["g0"], c["G"], c["theta"])
        print("%s: scales %s, |scale - refit| / |refit| = %.2e, |f - fmin| / |fmin| = %.2e" %
              (name, r["scales"], rel, abs(f_set - r["fmin"]) / abs(r["fmin"])))
        assert rel <= 1e-12
        assert f_left == f_set
        assert abs(f_set - r["fmin"]) <= 1e-12 * abs(r["fmin"])
        assert abs(r["fmin"] - (c["theta"] * r["kl"] + r["chi2"])) <= 1e-14 * abs(r["fmin"])
        again = device_run(ctx, c, max_iterations=0)
        assert again["fmin"] == r["fmin"] and again["scales"] == r["scales"] and again["chi2"] == r["chi2"]
        host = host_run(name, max_iterations=0)
        assert abs(host["fmin"] - r["fmin"]) <= 1e-12 * abs(host["fmin"])
        assert "logw_profile" in ctx.footprint()[0]


# ---- one step ------------------------------------------------------------------------------------------------------------
def step_longdouble(c):
    """the profiled step at the case's g0 in 80-bit arithmetic: (Pi C_A Pi + theta I) z = -Pi b_A by iterative refinement,
    the operator applied in longdouble in O(MN), the preconditioner the float64 Cholesky factor of the restatement's matrix.
    -> dict(u, w, sweeps, last: max|du| / max|u| of the last correction)"""
    import scipy.linalg
    Y, theta = c["Y"].astype(L), L(c["theta"])
    m = Y.shape[0]
    groups = c["groups"] if c["groups"] is not None else [np.arange(m)]
    off = np.zeros(m, dtype=L) if c["off"] is None else c["off"].astype(L)
    YT, g, G = c["YT"].astype(L), c["g0"].astype(L), c["G"].astype(L)
    e = np.exp(g - g.max())
    w = e / e.sum()
    ybar = Y @ w
    sg = np.ones(m, dtype=L)
    V = np.zeros((m, len(groups)), dtype=L)
    for k, ix in enumerate(groups):
        sg[ix] = ybar[ix] @ (YT[ix] - off[ix]) / (ybar[ix] @ ybar[ix])
        V[ix, k] = ybar[ix] / np.sqrt(ybar[ix] @ ybar[ix])
    r = off + sg * ybar - YT
    dev = g - G
    P = w @ dev

    def adjoint(v):                                           # Yc^T v
        return v @ Y - ybar @ v

    def forward(t):                                           # Yc t
        return Y @ t - ybar * t.sum()

    def proj(v):
        return v - V @ (V.T @ v)

    grad = w * (theta * (dev - P) + adjoint(sg * r))

    def A(v):
        pv = proj(v)
        return proj(sg * forward(w * adjoint(sg * pv))) + theta * v

    rhs = -proj(sg * forward(grad))
    p64 = lw._dual_newton_profile_point(c["g0"], c["G"], c["Y"], c["YT"], c["theta"], 0.0, groups, off.astype(np.float64))
    CP, _, _ = lw.dual_newton_profile_covariance(p64, c["Y"], groups)
    factor = scipy.linalg.cho_factor(CP + c["theta"] * np.eye(m), lower=True)
    z, sweeps, last = np.zeros(m, dtype=L), 0, np.inf
    u0 = -((dev - P) + adjoint(sg * r) / theta)
    while sweeps < 10 and last > 1e-15:
        res = rhs - A(z) if sweeps else rhs
        dz = scipy.linalg.cho_solve(factor, res.astype(np.float64)).astype(L)
        z = z + dz
        sweeps += 1
        u = u0 - adjoint(sg * z) / theta
        last = float(np.abs(adjoint(sg * dz) / theta).max() / np.abs(u).max())      # what the correction moved u by
    return dict(u=u, w=w, sweeps=sweeps, last=last)


@pytest.mark.parametrize("name", CASES)
def test_one_accepted_step(bioen_amd, monkeypatch, name):
    c = case(name)
    host = host_run(name, max_iterations=1)
    assert host["status"] == 1 and host["iterations"] == 1 and host["evaluations"] == 2       # alpha = 1 accepted
    ref = step_longdouble(c)
    # the reference's own condition: its last correction moved u by five orders less than the gate
    assert ref["last"] <= 1e-15, (ref["sweeps"], ref["last"])
    with context(bioen_amd, monkeypatch, c) as ctx:
        r = device_run(ctx, c, max_iterations=1)
    assert (r["status"], r["iterations"], r["evaluations"], r["factorisations"]) == (1, 1, 2, 1)
    u = r["g"] - c["g0"]
    umax = float(np.abs(ref["u"]).max())
    err = float(np.abs(u.astype(L) - ref["u"]).max())
    err_host = float(np.abs((host["g"] - c["g0"]).astype(L) - ref["u"]).max())
    print("%s: max|u| = %.3g, |u - u_ref| / max|u| = %.2e (the restatement: %.2e), |w . u| / max|u| = %.2e" %
          (name, umax, err / umax, err_host / umax, abs(float(ref["w"] @ u.astype(L))) / umax))
    assert err <= 1e-10 * umax


# ---- the loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_loop_equals_the_restatement(bioen_amd, monkeypatch, name):
    c = case(name)
    host = host_run(name)
    assert host["status"] == 0
    with context(bioen_amd, monkeypatch, c) as ctx:
        r = device_run(ctx, c)
        b = device_run(ctx, c, hessian="gram_bf16")
    counts = ("iterations", "evaluations", "factorisations")
    rel = max(abs(a - h) / abs(h) for a, h in zip(r["scales"], host["scales"]))
    rel16 = max(abs(a - h) / abs(h) for a, h in zip(b["scales"], host["scales"]))
    print("%s: status %d / %d, counts %s (restatement %s; split BF16 %s, %d passes%s), |dfmin| / |fmin| = %.2e (BF16 %.2e), "
          "scales %s, |dscale| / |scale| = %.2e (BF16 %.2e)" %
          (name, r["status"], b["status"], [r[k] for k in counts], [host[k] for k in counts], [b[k] for k in counts],
           b["bf16_passes"], ", switched" if b["switched"] else "", abs(r["fmin"] - host["fmin"]) / abs(host["fmin"]),
           abs(b["fmin"] - host["fmin"]) / abs(host["fmin"]), r["scales"], rel, rel16))
    assert r["status"] == 0 and b["status"] == 0
    assert [r[k] for k in counts] == [host[k] for k in counts]
    assert r["bf16_passes"] == 0 and not r["switched"]
    assert abs(r["fmin"] - host["fmin"]) <= 1e-9 * abs(host["fmin"])
    assert abs(b["fmin"] - host["fmin"]) <= 1e-9 * abs(host["fmin"])
    assert rel <= SCALE_GATE and rel16 <= SCALE_GATE
    w, wh = np.exp(r["g"] - r["g"].max()), np.exp(host["g"] - host["g"].max())
    assert np.abs(w / w.sum() - wh / wh.sum()).max() <= 1e-5 * (wh / wh.sum()).max()


def test_warm_series_and_series_profiled(bioen_amd, monkeypatch):
    c = case("deer205")
    thetas = [100.0, 10.0, 1.0]
    with context(bioen_amd, monkeypatch, c) as ctx:
        f_plain, _ = ctx.logw_fdf(c["g0"], c["G"], 10.0)
        warm = ctx.opt_dual_newton_logw_profile_series(thetas, c["G"], c["G"], PARAMS, row_offset=c["off"], warm=True)
        cold = ctx.opt_dual_newton_logw_profile_series(thetas, c["G"], c["G"], PARAMS, row_offset=c["off"], warm=False)
        print("iterations warm %s, cold %s; scales %s" % ([r["iterations"] for r in warm], [r["iterations"] for r in cold],
                                                       [r["scales"][0] for r in warm]))
        assert [r["status"] for r in warm + cold] == [0] * 6
        assert np.array_equal(warm[0]["g"], cold[0]["g"]) and warm[0]["scales"] == cold[0]["scales"]
        assert sum(r["iterations"] for r in warm) <= sum(r["iterations"] for r in cold)
        for a, b in zip(warm, cold):
            assert a["iterations"] <= b["iterations"]
            assert abs(a["fmin"] - b["fmin"]) <= 1e-9 * abs(b["fmin"])
            assert abs(a["scales"][0] - b["scales"][0]) <= OPTIMUM_GATE * abs(b["scales"][0])
        # after the call the model is (off, sigma of the last theta) and the returned point the kept one
        sg = sigma_of(c, cold[-1]["scales"])
        f_left, _ = ctx.logw_fdf(cold[-1]["g"], c["G"], thetas[-1])
        assert abs(f_left - cold[-1]["fmin"]) <= 1e-12 * abs(f_left)
        ctx.set_affine(c["off"], sg)
        assert ctx.logw_fdf(cold[-1]["g"], c["G"], thetas[-1])[0] == f_left
        # nuisance.series_profiled: series' dicts, and the model is gone afterwards -- also after a raised status
        out = nuisance.series_profiled(ctx, thetas, c["G"], c["G"], PARAMS, row_offset=c["off"])
        assert [o["theta"] for o in out] == thetas and all(o["status"] == 0 for o in out)
        for o, a in zip(out, warm):
            assert o["fmin"] == a["fmin"] and o["scales"] == a["scales"] and np.array_equal(o["g"], a["g"])
            assert abs(o["w"].sum() - 1.0) <= 1e-12 and abs(o["fmin"] - (o["theta"] * -o["S"] + o["chi2"])) <= 1e-12 * abs(o["fmin"])
        assert ctx.logw_fdf(c["g0"], c["G"], 10.0)[0] == f_plain
        with pytest.raises(RuntimeError, match="return code 1"):
            nuisance.series_profiled(ctx, thetas, c["G"], c["G"], dict(PARAMS, max_iterations=1), row_offset=c["off"])
        assert ctx.logw_fdf(c["g0"], c["G"], 10.0)[0] == f_plain


# ---- refusals and state --------------------------------------------------------------------------------------------------
def test_refusals_leave_point_session_and_model_alone(bioen_amd, monkeypatch):
    import ctypes as C
    from bioen_amd import _lib
    from bioen_amd._lib import BioenHipError
    c = case("deer105")
    m, n = c["Y"].shape
    v = np.random.default_rng(4).standard_normal(n)
    th = np.array([10.0, 1.0])
    cfg = _lib.logw_newton_config(PARAMS)
    group = np.zeros(m, dtype=np.int32)
    group[60:] = 1
    out, sc = np.empty((2, n)), np.empty((2, 2))
    res = (_lib.LogwNewtonSeriesResult * 2)()

    def call(ctx, thetas=th, ntheta=2, config=cfg, source=0, warm=1, grp=group, ngroups=2, gopt=out, scales=sc):
        return _lib.lib().bioen_logwn_profile_series(
            ctx._h, _lib.ptr(c["g0"]), _lib.ptr(c["G"]), _lib.ptr(thetas), ntheta, C.byref(config) if config else None, source,
            warm, _lib.ptr(c["off"]), grp.ctypes.data_as(_lib.ip) if grp is not None else None, ngroups,
            _lib.ptr(gopt) if gopt is not None else None, _lib.ptr(scales) if scales is not None else None, None, None, res)

    bad_group, no_rows = group.copy(), group.copy()
    bad_group[7] = 2
    no_rows[60:] = -1
    bad_cfg = _lib.logw_newton_config(dict(PARAMS, max_halvings=0))
    refused = [dict(ntheta=0), dict(thetas=np.array([10.0, 0.0])), dict(thetas=np.array([np.inf, 1.0])), dict(ngroups=0),
               dict(ngroups=65), dict(grp=bad_group), dict(grp=-2 * np.ones(m, dtype=np.int32)), dict(grp=no_rows),
               dict(ngroups=3), dict(config=bad_cfg), dict(config=None), dict(grp=None), dict(gopt=None), dict(scales=None),
               dict(source=2), dict(warm=2)]
    with context(bioen_amd, monkeypatch, c) as ctx:
        hv, _, _ = ctx.logw_hessp(v, g=c["g0"], G=c["G"], theta=10.0)
        for kw in refused:
            assert call(ctx, **kw) == -1, kw
        assert np.array_equal(ctx.logw_hessp(v), hv)                       # the kept point serves
        assert "logw_profile" not in ctx.footprint()[0]
        ctx.bfgs_begin(c["g0"], c["G"], 10.0)
        f1, _ = ctx.bfgs_trial(1e-3, True)
        for kw in refused:
            assert call(ctx, **kw) == -1, kw
        f2, _ = ctx.bfgs_trial(2e-3, False)                                # the session lives
        assert np.isfinite(f1) and np.isfinite(f2)
        assert call(ctx) == 0                                              # ... and the accepted call ends it
        with pytest.raises(BioenHipError, match="ended by another call"):
            ctx.bfgs_trial(3e-3, False)
        # the selection is cleared: the plain series on the model the call left is the chained single call's
        a = ctx.opt_dual_newton_logw_series([10.0], c["g0"], c["G"], PARAMS)[0]
        ctx.set_affine(c["off"], sigma_of(c, list(sc[1])))
        b = ctx.opt_dual_newton_logw(c["g0"], c["G"], 10.0, PARAMS)
        assert np.array_equal(a["g"], b["g"]) and a["fmin"] == b["fmin"]
        ctx.set_affine(None, None)
        # a scale that is not finite (on the device the raw averages of a zero row are rounding, not zero: the numerator
        # is made NaN instead) makes f not finite at the start point: status 3 behind one failed factorisation, as the
        # restatement
        off = c["off"].copy()
        off[70] = np.nan
        r = ctx.opt_dual_newton_logw_profile_series([10.0], c["g0"], c["G"], PARAMS, groups=c["groups"], row_offset=off)[0]
        assert (r["status"], r["iterations"], r["evaluations"], r["factorisations"]) == (3, 0, 1, 1) and np.isnan(r["fmin"])
        assert np.isfinite(r["scales"][0]) and np.isnan(r["scales"][1])
        h = lw.dual_newton_profile_base(c["g0"], c["G"], c["Y"], c["YT"], 10.0, PARAMS, c["groups"], off)
        assert (h["status"], h["iterations"], h["evaluations"], h["factorisations"]) == (3, 0, 1, 1)
        ctx.set_affine(None, None)

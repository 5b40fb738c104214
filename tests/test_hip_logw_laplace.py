"""GPU tests of the log-weights method's Laplace error bars (csrc/kernels_logw_laplace.hip, csrc/api_logw_laplace.cpp,
Context.logw_laplace, log_weights.laplace_error_bars): the entry against its numpy restatement at the dual
Newton's optimum on the shapes of tests/test_hip_forces_laplace.py, the conditions under which the gates are meaningful
asserted from the restatement, the bitwise invariants, the kept-point rules, the lean calls, the affine model, the forces
method's cov_averages at the shared optimum, and the refusals.

The ratios measured on the MI355X are in tests/README_logw_laplace.md."""
import ctypes as C

import numpy as np
import pytest

from test_hip_forces_hessp import estate
from test_hip_forces_laplace import ENTRY_SHAPES
from test_hip_strip_loops import on_thread_ranks

from bioen_amd.optimize import log_weights
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

THETAS = (10.0, 1.0)
VECTORS = ("w", "leverage", "var_logw", "std_w")
_CTX, _DATA, _OPT, _REF = {}, {}, {}, {}


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()
    c_bioen.clear_cache()


def data(shape):
    """tests/test_hip_forces_laplace.py's generator, seeded by the shape; G = ln w0; three held-out observables"""
    if shape not in _DATA:
        M, N = shape
        rng = np.random.default_rng(M * N)
        yT = rng.normal(rng.normal(0.0, 2.0, (M, 1)), 1.0, (M, N))
        w0 = rng.uniform(0.5, 1.5, N)
        w0 /= w0.sum()
        YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
        obs = np.random.default_rng(M * N + 1).standard_normal((11, N))
        _DATA[shape] = (yT, YT, w0, np.log(w0), obs)
    return _DATA[shape]


def context(bioen_amd, shape):
    if shape not in _CTX:
        yT, YT = data(shape)[:2]
        _CTX[shape] = bioen_amd.Context(yT, YT)
    return _CTX[shape]


def optimum(bioen_amd, shape, theta):
    """the dual Newton's optimum (gtol 1e-8) on the shape's context, found once"""
    if (shape, theta) not in _OPT:
        G = data(shape)[3]
        res = context(bioen_amd, shape).opt_dual_newton_logw(G, G, theta, dict(gtol=1e-8))
        assert res["status"] in (0, 2) and res["gmax"] <= 1e-6 * res["wmax"]
        _OPT[shape, theta] = res
    return _OPT[shape, theta]


def restatement(key, g, G, yT, YT, theta, obs):
    """log_weights.laplace_error_bars(use_c=False), once per case, with the conditions the gates rest on: -> (ref, rest_j =
    1 - w_j - leverage_j, ratio_k = c^T P c / Var_w)"""
    if key not in _REF:
        ref = log_weights.laplace_error_bars(g, G, None, yT, YT, theta, observables=obs, use_c=False)
        w = ref["w"]
        rest = (1.0 - w) - ref["leverage"]
        d = obs - ref["obs_averages"][:, None]
        ratio = 1.0 - theta * ref["std_observables"] ** 2 / (d * d).dot(w)
        cond = np.linalg.cond(ref["C"] + theta * np.eye(yT.shape[0]))
        print("%s: min(1 - w - leverage) = %.3g, max c'Pc / Var_w = %.3g, cond(C + theta I) = %.3g" % (key, rest.min(), ratio.max(), cond))
        assert rest.min() >= 0.05 and ratio.max() <= 0.9 and cond <= 23.0
        _REF[key] = (ref, rest, ratio)
    return _REF[key]


def held_to_the_restatement(label, got, C, ref, rest, ratio):
    """the gates of the issue: 1e-8 of the largest entry for C, cov_averages, std_averages and leverage; the others below"""
    assert got["info"] == 0 and got["min_pivot"] > 0.0
    for k, dev in (("C", C), ("cov_averages", got["cov_averages"]), ("std_averages", got["std_averages"]),
                   ("leverage", got["leverage"])):
        err = np.abs(dev - ref[k]).max() / np.abs(ref[k]).max()
        print("%s %s: %.3g of its largest entry (gate 1e-8)" % (label, k, err))
        assert dev.shape == ref[k].shape and err <= 1e-8
    ew = np.abs(got["w"] / ref["w"] - 1.0).max()
    el = abs(got["logdet"] / ref["logdet"] - 1.0)
    print("%s w: %.3g relative (gate 1e-12); logdet: %.3g relative (gate 1e-12)" % (label, ew, el))
    assert ew <= 1e-12 and el <= 1e-12
    gate = (0.5 * 1e-8 * ref["leverage"].max() / rest + 1e-12)
    es = np.abs(got["std_w"] - ref["std_w"]) / (gate * ref["std_w"])
    ev = np.abs(got["var_logw"] - ref["var_logw"]) / (2.0 * gate * ref["var_logw"])
    print("%s std_w: %.3g of its gate; var_logw: %.3g of its gate" % (label, es.max(), ev.max()))
    assert es.max() <= 1.0 and ev.max() <= 1.0
    k = len(got["obs_averages"])
    vref = ref["std_observables"][:k] ** 2
    eo = np.abs(got["var_observables"] / vref - 1.0) / (1e-8 * ratio[:k] / (1.0 - ratio[:k]) + 1e-12)
    ea = np.abs(got["obs_averages"] / ref["obs_averages"][:k] - 1.0)
    print("%s var_observables: %.3g of its gate; obs_averages: %.3g relative (gate 1e-13)" % (label, eo.max(), ea.max()))
    assert eo.max() <= 1.0 and ea.max() <= 1e-13
    assert np.array_equal(got["cov_averages"], got["cov_averages"].T)


CASES = [(s, t) for s in ENTRY_SHAPES for t in THETAS]


@pytest.mark.parametrize("shape,theta", CASES, ids=["%dx%d-theta%g" % (s + (t,)) for s, t in CASES])
def test_error_bars_against_the_restatement(bioen_amd, shape, theta):
    yT, YT, w0, G, obs = data(shape)
    ctx = context(bioen_amd, shape)
    gopt = optimum(bioen_amd, shape, theta)["g"]
    ref, rest, ratio = restatement("%dx%d theta %g" % (shape + (theta,)), gopt, G, yT, YT, theta, obs[:3])
    got = ctx.logw_laplace(g=gopt, G=G, theta=theta, observables=obs[:3])
    held_to_the_restatement("%dx%d theta %g" % (shape + (theta,)), got, ctx.logw_cov(), ref, rest, ratio)
    again = ctx.logw_laplace(g=gopt, G=G, theta=theta, observables=obs[:3])      # the same bits in, the same bits out
    assert set(again) == set(got)
    for k in got:
        assert np.array_equal(np.asarray(again[k]), np.asarray(got[k])), k


def test_through_laplace_error_bars(bioen_amd):
    """log_weights.laplace_error_bars(use_c=True): Context.logw_laplace's numbers under the restatement's keys"""
    shape, theta = (65, 300), 10.0
    yT, YT, w0, G, obs = data(shape)
    gopt = optimum(bioen_amd, shape, theta)["g"]
    ref = restatement("65x300 theta 10", gopt, G, yT, YT, theta, obs[:3])[0]
    dev = log_weights.laplace_error_bars(gopt, G, None, yT, YT, theta, observables=obs[:3])
    lean = log_weights.laplace_error_bars(gopt, G, None, yT, YT, theta, matrices=False)
    assert set(dev) == set(ref) and set(lean) == set(ref) - {"obs_averages", "std_observables"}
    for k in ref:
        assert np.abs(dev[k] - ref[k]).max() <= 1e-8 * np.abs(ref[k]).max(), k
    assert lean["C"] is None and lean["cov_averages"] is None
    for k in VECTORS + ("std_averages", "logdet"):
        assert np.array_equal(lean[k], dev[k]), k
    bad = gopt.copy()
    bad[5] = np.nan                                                       # reported by the pivot test, not a fault
    with bioen_amd.Context(yT, YT) as ctx:
        r = ctx.logw_laplace(g=bad, G=G, theta=theta, observables=obs[:1])
        assert r["info"] != 0 and r["w"] is None and r["cov_averages"] is None and np.isnan(r["logdet"])
    with pytest.raises(ValueError, match="did not factorise"):
        log_weights.laplace_error_bars(bad, G, None, yT, YT, theta)


@pytest.mark.parametrize("shape", [(65, 300), (513, 1537)], ids=["65x300", "513x1537"])
def test_observables_in_one_call_are_those_of_single_calls(bioen_amd, shape):
    theta = 10.0
    yT, YT, w0, G, obs = data(shape)
    ctx = context(bioen_amd, shape)
    ctx.logw_cov(g=optimum(bioen_amd, shape, theta)["g"], G=G, theta=theta, cov=False)
    single = [ctx.logw_laplace(theta=theta, observables=o, matrices=False, vectors=False) for o in obs]
    for k in (1, 3, 8, 11):                                               # 11: two chunks through Context.logw_laplace
        r = ctx.logw_laplace(theta=theta, observables=obs[:k], matrices=False, vectors=False)
        assert r["obs_averages"].shape == r["var_observables"].shape == (k,)
        for a in range(k):
            assert r["obs_averages"][a] == single[a]["obs_averages"][0], (k, a)
            assert r["var_observables"][a] == single[a]["var_observables"][0], (k, a)


def test_the_kept_point_is_served_and_kept(bioen_amd):
    shape, theta = (65, 300), 10.0
    yT, YT, w0, G, obs = data(shape)
    v = np.random.default_rng(4).standard_normal(shape[1])
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.logw_laplace(theta=theta), "no point on this context", "bioen_logwn_laplace")
        res = ctx.opt_dual_newton_logw(G, G, theta, dict(gtol=1e-8))
        C = ctx.logw_cov()
        hv = ctx.logw_hessp(v)
        kept = ctx.logw_laplace(theta=theta, observables=obs[:3])         # the optimum, without g
        assert kept["info"] == 0 and "f" not in kept
        assert np.array_equal(ctx.logw_cov(), C) and np.array_equal(ctx.logw_hessp(v), hv)
        given = ctx.logw_laplace(g=res["g"], G=G, theta=theta, observables=obs[:3])
        assert given["f"] == res["fmin"] and np.abs(given["grad"]).max() == res["gmax"]
        for k in kept:
            assert np.array_equal(np.asarray(kept[k]), np.asarray(given[k])), k
        assert np.array_equal(ctx.logw_cov(), C) and np.array_equal(ctx.logw_hessp(v), hv)
        # lean calls: what is left out is None, what stays keeps its bits
        for matrices, vectors in ((False, True), (True, False), (False, False)):
            lean = ctx.logw_laplace(theta=theta, matrices=matrices, vectors=vectors)
            assert "obs_averages" not in lean
            for k in ("std_averages", "logdet", "min_pivot") + (("cov_averages",) if matrices else ()) + (VECTORS if vectors else ()):
                assert np.array_equal(np.asarray(lean[k]), np.asarray(kept[k])), k
            assert matrices or lean["cov_averages"] is None
            assert vectors or all(lean[k] is None for k in VECTORS)
        assert {"logw_gram", "forces_newton", "forces_laplace", "forces_colquad"} <= set(ctx.footprint()[0])
        ctx.logw_fdf(G, G, theta)                                         # an evaluation drops the point
        estate(lambda: ctx.logw_laplace(theta=theta), "is gone", "bioen_hip_logw_fdf")


def test_error_bars_with_an_affine_model(bioen_amd):
    """129 x 700 with the offsets and scales of tests/test_hip_forces_laplace.py's affine test on the context: the device
    against the restatement on the explicitly transformed matrix"""
    shape, theta = (129, 700), 10.0
    yT, YT, w0, G, obs = data(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, 129), rng.uniform(0.5, 1.5, 129)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        res = ctx.opt_dual_newton_logw(G, G, theta, dict(gtol=1e-8))
        assert res["status"] in (0, 2)
        ref, rest, ratio = restatement("affine 129x700 theta 10", res["g"], G, off[:, None] + sc[:, None] * yT, YT, theta, obs[:3])
        got = ctx.logw_laplace(theta=theta, observables=obs[:3])
        held_to_the_restatement("affine 129x700 theta 10", got, ctx.logw_cov(), ref, rest, ratio)


def test_cov_averages_is_the_forces_methods_on_the_device(bioen_amd):
    shape, theta = (129, 700), 10.0
    yT, YT, w0, G, obs = data(shape)
    ctx = context(bioen_amd, shape)
    fres = ctx.opt_newton_forces(np.zeros(shape[0]), w0, theta, dict(gtol=1e-8), want_weights=False)
    assert fres["status"] in (0, 2)
    fb = ctx.forces_laplace()
    lb = ctx.logw_laplace(g=optimum(bioen_amd, shape, theta)["g"], G=G, theta=theta, vectors=False)
    assert fb["info"] == 0 and lb["info"] == 0
    err = np.abs(lb["cov_averages"] - fb["cov_averages"]).max() / np.abs(fb["cov_averages"]).max()
    print("129x700 theta 10: cov_averages of the two methods differ by %.3g of the largest entry (gate 1e-8)" % err)
    assert err <= 1e-8


def raw_call(ctx, theta, nobs, observables):
    from bioen_amd import _lib
    info = C.c_int(0)
    return _lib.lib().bioen_logwn_laplace(ctx._h, None, None, theta, _lib.ptr(observables) if observables is not None else None,
                                          nobs, *([None] * 10 + [C.byref(info), None, None]))


def test_refusals(bioen_amd):
    from bioen_amd import _lib
    from bioen_amd._lib import BioenHipError
    shape, theta = (65, 300), 10.0
    yT, YT, w0, G, obs = data(shape)
    v = np.random.default_rng(4).standard_normal(shape[1])
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.logw_hessp(v, g=G, G=G, theta=theta)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(BioenHipError, match="theta > 0"):
                ctx.logw_laplace(theta=bad)
        with pytest.raises(ValueError, match="needs theta"):
            ctx.logw_laplace()
        with pytest.raises(ValueError, match="observables must be"):
            ctx.logw_laplace(theta=theta, observables=obs[:, :-1])
        nine = np.ascontiguousarray(obs[:9])
        for nobs, o, needle in ((9, nine, "nobs must be in [0, 8]"), (-1, nine, "nobs must be in [0, 8]"),
                                (0, nine, "observables without nobs"), (2, None, "nobs without observables")):
            assert raw_call(ctx, theta, nobs, o) == -1 and needle in _lib.lib().bioen_hip_last_error().decode()
        assert np.array_equal(ctx.logw_hessp(v), hv)                      # a rejected call leaves the point alone
        ctx.set_storage("fp32")                                           # the reduced-storage copies
        estate(lambda: ctx.logw_laplace(g=G, G=G, theta=theta), "bioen_logwn_laplace", "reduced-storage")
        ctx.set_storage("f64")
        assert "forces_laplace" not in ctx.footprint()[0]
    rng = np.random.default_rng(1040)
    tall = rng.standard_normal((1040, 384))                               # row panels
    with bioen_amd.Context(tall, tall.mean(axis=1)) as ctx:
        Gt = np.full(384, -np.log(384.0))
        estate(lambda: ctx.logw_laplace(g=Gt, G=Gt, theta=theta), "bioen_logwn_laplace", "M <= 1024")


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, w0, G, obs = data((129, 700))

    def workload(ctx, local_segments):
        estate(lambda: ctx.logw_laplace(g=G, G=G, theta=10.0), "bioen_logwn_laplace", "structure-sharded")
        estate(lambda: ctx.logw_laplace(theta=10.0), "bioen_logwn_laplace", "structure-sharded")
        return True

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))

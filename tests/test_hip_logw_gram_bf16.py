"""GPU tests of the log-weights theta series by dual Newton on a split-BF16 covariance (csrc/kernels_logw_newton.hip:
k_logw_gram_bf16; csrc/api_logw_newton.cpp: bioen_logwn_cov_bf16, bioen_logwn_series; Context.logw_cov_bf16,
opt_dual_newton_logw_series).

Tolerances of the pass, derived and not tuned.  With a = Y' - centre (the affine model: its scaled rows), G' = sum_j w_j a_j
a_j^T formed in FP64 on the host and s_ik = sqrt(G'_ii G'_kk), every summand of element (i, k) is bounded relative to s_ik
(Cauchy-Schwarz), and tg is the shape's longest Gram chain, from Context.strip_plan as assert_newton_regime computes it:

  (ii) against the restatement (log_weights.dual_newton_covariance_bf16, the same split products summed in FP64):
       |C~_dev - C~_rest|_ik <= 48 tg 2^-23 s_ik -- 48 f32 additions per strip and accumulator (3 instructions of depth 16),
       one unit of the last place each, which also covers a sum inside the instruction that is not IEEE's;
  (i)  against logw_cov at the same kept point: 3 * 2^-16 s_ik + (ii) -- each operand keeps 16 significant bits, lo lo is
       dropped.

Both comparisons carry an FP64 floor besides, 4 n eps max_j|y_ij| max_j|y_kj| (scale_matrix): the two sides form ybar in FP64
in different orders and ybar' ybar'^T carries that, which is all there is to compare where a row equals its centre and s_ik = 0
(808 x 10's first row: the device leaves 0, the restatement -4e-16).

The measured ratios are printed; tests/README_logw_series.md has them."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_hip_forces_gram import GATE as FORCES_GATE
from test_hip_forces_hessp import estate, problem
from test_hip_logw_dual_newton import SHAPES as COV_SHAPES, logw_problem
from test_hip_logw_newton_loops import (AFFINE_SHAPES, L, PARAMS, SHAPES as LOOP_SHAPES, THETA, assert_newton_regime, bits, case,
                                        case_id, converged, counts, golden_vectors, point_longdouble, rows_times, times_columns)
from test_hip_strip_loops import enter_regime, on_thread_ranks
from test_logw_dual_newton import GOOD, M808, case_args
from test_logw_series import BF16, THETAS, host_dual_newton_bf16, host_series, series_problem, weights

from bioen_amd.optimize import log_weights, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

PASS_SHAPES = [s for s in COV_SHAPES if s != (1, 37)]       # 7 x 37, 808 x 10, 129 x 257, 64 x 2000, 513 x 1537, 1024 x 528
CHAIN_SHAPES = [(300, 9000), (600, 33700), (1024, 33700)]
STEP_CASES = [((300, 9000), False), ((1024, 9000), False), ((600, 33700), True)]
U16, U23 = 2.0 ** -16, 2.0 ** -23


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    c_bioen.clear_cache()


def gram_tg(ctx, m):
    """the longest chain of strips a set of the Gram pass adds up, from the plan (assert_newton_regime's arithmetic)"""
    p = ctx.strip_plan(0)
    t = (-(-m // 64) + 1) // 2
    gs = max(1, min(p["sps"], -(-512 // (p["local_segments"] * (t * (t + 1) // 2)))))
    return -(-p["sps"] // gs)


def scale_matrix(yT, YT, g, sc=None):
    """-> (s_ik = sqrt(G'_ii G'_kk), G' = sum_j w_j a_j a_j^T in FP64 on the host, a = (yT - YT) (affine: times the row's
    scale); the FP64 floor 4 n eps max_j|y_ij| max_j|y_kj|: the two sides form ybar in FP64 in different orders, each to
    n eps max|y_i|, and ybar' ybar'^T carries that -- all there is to compare where a row equals its centre and s_ik = 0:
    808 x 10's first row)"""
    e = np.exp(g - g.max())
    w = e / e.sum()
    a = yT - YT[:, None]
    top = np.abs(yT).max(axis=1)
    if sc is not None:
        a, top = a * sc[:, None], top * sc
    s = np.sqrt(np.einsum("ij,j,ij->i", a, w, a))
    return np.outer(s, s), 4 * yT.shape[1] * np.finfo(np.float64).eps * np.outer(top, top)


def restated(yT, YT, G, g, theta):
    p = log_weights._dual_newton_point(g, G, yT, YT, theta, 0.0)
    return log_weights.dual_newton_covariance_bf16(p, yT, YT)


def held(label, Cb, Cfp, Crest, S, tg):
    """(i), (ii), not the FP64 pass under another name, bitwise symmetric"""
    S, floor = S
    bound_ii = 48 * tg * U23

    def ratio(D):                                  # the measured figure, over the elements that have a scale
        return float((np.abs(D)[S > 0] / S[S > 0]).max())
    print("%s: tg %d; (i) |C~ - C| = %.3g s_ik (bound %.3g)" % (label, tg, ratio(Cb - Cfp), 3 * U16 + bound_ii))
    if Crest is not None:
        print("%s: (ii) |C~ - C~_rest| = %.3g s_ik (bound %.3g)" % (label, ratio(Cb - Crest), bound_ii))
        assert (np.abs(Cb - Crest) <= bound_ii * S + floor).all()
    assert (np.abs(Cb - Cfp) <= (3 * U16 + bound_ii) * S + floor).all()
    assert np.abs(Cb - Cfp).max() > 0.0
    assert np.array_equal(Cb, Cb.T)


# ---- the pass --------------------------------------------------------------------------------------------------------------
def spread_point(shape):
    """-> yT, YT, G, g = G + 3 sigma: logw_problem's direction (standard deviation 1) three times as far"""
    yT, YT, G, g = logw_problem(shape)
    return yT, YT, G, G + 3.0 * (g - G)


@pytest.mark.parametrize("shape", PASS_SHAPES, ids=case_id)
def test_pass_against_the_fp64_pass_and_the_restatement(bioen_amd, shape):
    yT, YT, G, g = spread_point(shape)
    S = scale_matrix(yT, YT, g)
    with bioen_amd.Context(yT, YT) as ctx:
        _, f0, g0 = ctx.logw_hessp(None, g=g, G=G, theta=THETA)
        Cb, fv, grad = ctx.logw_cov_bf16(g=g, G=G, theta=THETA)
        assert fv == f0 and np.array_equal(grad, g0)                     # the point-setting call is logw_hessp's evaluation
        held("%dx%d" % shape, Cb, ctx.logw_cov(), restated(yT, YT, G, g, THETA), S, gram_tg(ctx, shape[0]))
        for _ in range(2):                                               # the same bits, call after call
            assert np.array_equal(ctx.logw_cov_bf16(), Cb)
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))            # (o, s) = (0, 1): the plain model's bits
        assert np.array_equal(ctx.logw_cov_bf16(g=g, G=G, theta=THETA)[0], Cb)


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=case_id)
def test_pass_on_long_chains(bioen_amd, monkeypatch, shape):
    """sets that chain 7, 53 and 132 strips: the f32 accumulators at their deepest"""
    enter_regime(monkeypatch, shape)
    c = case(shape)
    S = scale_matrix(c["yT"], c["YT"], c["g0"])
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        plan = assert_newton_regime(ctx, shape)
        assert plan["gram_tg"] == gram_tg(ctx, shape[0])
        Cb, _, _ = ctx.logw_cov_bf16(g=c["g0"], G=c["G"], theta=THETA)
        held("%dx%d" % shape, Cb, ctx.logw_cov(), restated(c["yT"], c["YT"], c["G"], c["g0"], THETA), S, plan["gram_tg"])
        assert np.array_equal(ctx.logw_cov_bf16(), Cb)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=case_id)
def test_pass_under_the_affine_model(bioen_amd, shape):
    """against logw_cov on the same model: the scales multiply both passes' results, and the bound's s_ik"""
    yT, YT, G, g = spread_point(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    with bioen_amd.Context(yT, YT) as ctx:
        plain, _, _ = ctx.logw_cov_bf16(g=g, G=G, theta=THETA)
        ctx.set_affine(off, sc)
        Cb, _, _ = ctx.logw_cov_bf16(g=g, G=G, theta=THETA)
        assert not np.array_equal(Cb, plain)
        held("affine %dx%d" % shape, Cb, ctx.logw_cov(), None, scale_matrix(yT, YT, g, sc), gram_tg(ctx, shape[0]))
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))
        assert np.array_equal(ctx.logw_cov_bf16(g=g, G=G, theta=THETA)[0], plain)


def test_the_fp64_pass_keeps_its_bits_beside_this_one(bioen_amd):
    """both orders in one buffer, and a fresh context"""
    yT, YT, G, g = spread_point((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        Cf, _, _ = ctx.logw_cov(g=g, G=G, theta=THETA)                    # alone
    with bioen_amd.Context(yT, YT) as ctx:
        Cb, _, _ = ctx.logw_cov_bf16(g=g, G=G, theta=THETA)
        assert np.array_equal(ctx.logw_cov(), Cf)                        # after the BF16 pass, at its point
        assert np.array_equal(ctx.logw_cov_bf16(), Cb)                   # ... and the other way round
        assert np.array_equal(ctx.logw_cov(g=g, G=G, theta=THETA)[0], Cf)
    with bioen_amd.Context(yT, YT) as ctx:
        assert np.array_equal(ctx.logw_cov_bf16(g=g, G=G, theta=THETA)[0], Cb)


@pytest.mark.parametrize("shape", [(7, 37), (129, 257), (513, 1537)], ids=case_id)
def test_cov_bf16_equals_forces_gram_bf16s_at_the_same_weights(bioen_amd, shape):
    """g = G against forces = 0 with w0 = softmax(G): the same weights, the two instances of the one split-BF16 loop
    (fgram.hpp: fgram16_pass) held to each other.  Each lies within (ii) of its restatement (the same loop, the same
    derivation) and the two restatements (forces.hessian_gram_bf16_bioen_log_posterior_base, log_weights.
    dual_newton_covariance_bf16) agree to the rounding of the weights, at most 1.2e-15 max|C| at these shapes on the host:
    |C~_logw - C~_forces|_ik <= 2 . 48 tg 2^-23 s_ik + GATE max|C| + the FP64 floor"""
    yT, YT, G, _ = logw_problem(shape)
    w0 = np.exp(G - G.max())
    w0 /= w0.sum()
    S, floor = scale_matrix(yT, YT, G)
    with bioen_amd.Context(yT, YT) as ctx:
        fg_before = ctx.forces_gram_bf16(forces=np.zeros(shape[0]), w0=w0, theta=THETA)
        Cb, _, _ = ctx.logw_cov_bf16(g=G, G=G, theta=THETA)
        tg = gram_tg(ctx, shape[0])
        D, top = np.abs(Cb - fg_before[0]), float(np.abs(fg_before[0]).max())
        print("%dx%d: tg %d; |C~_logw - C~_forces| = %.3g s_ik (bound %.3g), %.3g max|C|"
              % (shape + (tg, float((D[S > 0] / S[S > 0]).max()), 2 * 48 * tg * U23, float(D.max()) / top)))
        assert (D <= 2 * 48 * tg * U23 * S + FORCES_GATE * top + floor).all()
        fg_after = ctx.forces_gram_bf16(forces=np.zeros(shape[0]), w0=w0, theta=THETA)  # forces_gram_bf16's bits stay what they are
        assert all(np.array_equal(a, b) for a, b in zip(fg_before, fg_after))


# ---- the step, exactly ---------------------------------------------------------------------------------------------------
def step_from(c, Ct):
    """u of (Ct + theta I) z = -b at the case's g0 with no float64 on its path but Ct itself and the preconditioner: the
    point, b = Yc grad and the adjoint in longdouble (tests/test_hip_logw_newton_loops.py), z by iterative refinement on a
    float64 Cholesky factor of Ct + theta I with the residual in longdouble"""
    import scipy.linalg
    y, theta = c["y"], L(THETA)
    p = point_longdouble(y, c["YT"], c["G"], c["g0"], THETA)
    ybar, Cl = p["ybar"], Ct.astype(L)
    factor = scipy.linalg.cho_factor(Ct + THETA * np.eye(Ct.shape[0]), lower=True)
    negb = -(rows_times(y, p["grad"]) - ybar * p["grad"].sum())
    z, sweeps, last = np.zeros(Ct.shape[0], dtype=L), 0, np.inf
    while sweeps < 5 and last > 1e-17:
        res = negb - (Cl @ z + theta * z) if sweeps else negb
        dz = scipy.linalg.cho_solve(factor, res.astype(np.float64)).astype(L)
        z = z + dz
        sweeps += 1
        last = float(np.abs(dz).max() / np.abs(z).max())
    v = p["r"] + z
    u = -((p["dev"] - p["P"]) + (times_columns(v, y) - ybar @ v) / theta)
    return dict(u=u, w=p["w"], sweeps=sweeps, last=last)


@pytest.mark.parametrize("shape,affine", STEP_CASES, ids=["300x9000", "1024x9000", "600x33700-affine"])
def test_step_from_the_devices_own_covariance(bioen_amd, monkeypatch, shape, affine):
    """C~ is the device's, downloaded at the kept point g0: -b, the solve, the operand, the adjoint and k_logwn_step are held
    to the truth, u of a one-iteration gram_bf16 run within 1e-10 max|u| of it"""
    enter_regime(monkeypatch, shape)
    c = case(shape, affine)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        assert_newton_regime(ctx, shape)
        if affine:
            ctx.set_affine(c["off"], c["sc"])
        Ct, _, _ = ctx.logw_cov_bf16(g=c["g0"], G=c["G"], theta=THETA)
        res = ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, dict(PARAMS, max_iterations=1, hessian="gram_bf16"))
        plain = ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, dict(PARAMS, max_iterations=1))
    ref = step_from(c, Ct)
    converged(ref)
    assert res["status"] == 1 and res["iterations"] == 1 and res["factorisations"] == 1 and res["bf16_passes"] == 1
    alpha = 2.0 ** -(res["evaluations"] - 2)
    u_dev = (res["g"] - c["g0"]) / alpha
    S = float(np.abs(ref["u"]).max())
    err = float(np.abs(u_dev.astype(L) - ref["u"]).max()) / S
    gauge = abs(float(ref["w"] @ u_dev.astype(L))) / S
    du = float(np.abs(res["g"] - plain["g"]).max()) / (alpha * S)
    print("%dx%d%s: alpha %g, |u - u_ld(C~)| = %.3g max|u|, |w . u| = %.3g max|u|, |u - u_fp64 run| = %.3g max|u|; reference: "
          "%d sweeps, last correction %.3g max|z|" % (shape + (" affine" if affine else "", alpha, err, gauge, du,
                                                       ref["sweeps"], ref["last"])))
    assert err <= 1e-10
    assert gauge <= 1e-12
    assert not np.array_equal(res["g"], plain["g"])                       # the step is the split pass's


# ---- the loop ------------------------------------------------------------------------------------------------------------
def check_loop(label, ctx, g0, G, theta, host):
    res = ctx.opt_dual_newton_logw(g0, G, theta, BF16)
    ref = ctx.opt_dual_newton_logw(g0, G, theta, PARAMS)
    dw = float(np.abs(weights(res["g"]) - weights(ref["g"])).max() / weights(ref["g"]).max())
    print("%s: device gram_bf16 status %d, %d / %d / %d, %d BF16 passes, switched %s; restatement status %d, %d / %d / %d; device "
          "FP64 %d / %d / %d; fmin %.15g, restatement %.15g; max|dw| = %.3g max w against the device's FP64 run"
          % ((label, res["status"]) + counts(res) + (res["bf16_passes"], res["switched"], host["status"]) + counts(host)
             + counts(ref) + (res["fmin"], host["fmin"], dw)))
    assert (res["status"],) + counts(res) == (host["status"],) + counts(host)
    assert (res["bf16_passes"], res["switched"]) == (host["bf16_passes"], host["switched"])
    assert abs(res["fmin"] - host["fmin"]) <= 1e-9 * abs(host["fmin"])
    assert dw <= 1e-5
    assert "bf16_passes" not in ref and "switched" not in ref            # today's entry, today's dict
    return res


@pytest.mark.parametrize("name", GOOD)
def test_loop_on_the_goldens(bioen_amd, name):
    d, host = host_dual_newton_bf16(name)
    g0, G, yT, YT, theta = golden_vectors(d)
    with bioen_amd.Context(yT, YT) as ctx:
        check_loop(name, ctx, g0, G, theta, host)


_HOST16 = {}


def host_run_bf16(shape, affine=False):
    key = (shape, affine)
    if key not in _HOST16:
        c = case(shape, affine)
        _HOST16[key] = log_weights.dual_newton_bioen_log_posterior_base(c["g0"], c["G"], c["y64"], c["YT"], THETA, BF16)
    return _HOST16[key]


@pytest.mark.parametrize("shape,affine", [(s, False) for s in LOOP_SHAPES] + [(AFFINE_SHAPES[0], True)],
                         ids=[case_id(s) for s in LOOP_SHAPES] + [case_id(AFFINE_SHAPES[0]) + "-affine"])
def test_loop_at_production_geometry(bioen_amd, monkeypatch, shape, affine):
    """(under the affine model the restatement splits the model's matrix, the device the resident one times the scales: the
    counts are what is compared, and they hold)"""
    enter_regime(monkeypatch, shape)
    c = case(shape, affine)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        assert_newton_regime(ctx, shape)
        if affine:
            ctx.set_affine(c["off"], c["sc"])
        check_loop("%dx%d%s" % (shape + (" affine" if affine else "",)), ctx, c["g0"], c["G"], THETA, host_run_bf16(shape, affine))


# ---- the series ----------------------------------------------------------------------------------------------------------
SERIES = [("synth_logw_M64xN2000", [100.0, 10.0, 1.0]), ("recipe_300x9000", THETAS)]


@pytest.mark.parametrize("name,thetas", SERIES, ids=[s[0] for s in SERIES])
def test_series_from_the_fp64_pass_is_the_chained_and_the_single_calls(bioen_amd, name, thetas):
    yT, YT, G, g0 = series_problem(name)
    with bioen_amd.Context(yT, YT) as ctx:
        warm = ctx.opt_dual_newton_logw_series(thetas, g0, G, PARAMS)
        C_kept = ctx.logw_cov()                                           # the kept point is the last theta's returned point
        assert np.array_equal(C_kept, ctx.logw_cov(g=warm[-1]["g"], G=G, theta=thetas[-1])[0])
        cold = ctx.opt_dual_newton_logw_series(thetas, g0, G, PARAMS, warm=False)
        g = g0
        for t, w_, c_ in zip(thetas, warm, cold):
            chained = ctx.opt_dual_newton_logw(g, G, t, PARAMS)
            single = ctx.opt_dual_newton_logw(g0, G, t, PARAMS)
            assert bits(w_) == bits(chained) and bits(c_) == bits(single)
            assert (w_["bf16_passes"], w_["switched"], c_["bf16_passes"], c_["switched"]) == (0, False, 0, False)
            g = chained["g"]
    print("%s: warm evaluations %s, cold %s" % (name, [r["evaluations"] for r in warm], [r["evaluations"] for r in cold]))
    assert all(r["status"] == 0 for r in warm + cold)
    assert sum(r["evaluations"] for r in warm) <= sum(r["evaluations"] for r in cold)


@pytest.mark.parametrize("name,thetas", SERIES, ids=[s[0] for s in SERIES])
def test_series_from_the_bf16_pass_takes_the_restatements_counts(bioen_amd, name, thetas):
    yT, YT, G, g0 = series_problem(name)
    host = host_series(name, True, BF16, thetas)
    with bioen_amd.Context(yT, YT) as ctx:
        res = ctx.opt_dual_newton_logw_series(thetas, g0, G, PARAMS, hessian="gram_bf16")
        ref = ctx.opt_dual_newton_logw_series(thetas, g0, G, PARAMS)
    for t, r, h, f in zip(thetas, res, host, ref):
        print("%s theta %g: device %d / %d / %d status %d switched %s, restatement %d / %d / %d; |fmin - FP64 series'| = %.3g"
              % ((name, t) + counts(r) + (r["status"], r["switched"]) + counts(h) + (abs(r["fmin"] - f["fmin"]),)))
        assert (r["status"],) + counts(r) == (h["status"],) + counts(h) and r["switched"] == h["switched"]
        assert r["bf16_passes"] == h["bf16_passes"]
        assert abs(r["fmin"] - h["fmin"]) <= 1e-9 * abs(h["fmin"])
        assert np.abs(weights(r["g"]) - weights(f["g"])).max() <= 1e-5 * weights(f["g"]).max()


def test_a_theta_that_fails_is_reported_and_the_next_one_runs(bioen_amd):
    """potra part 1 (808 x 80) with its theta = 0.001 in the middle: the unsolved M >> N, theta -> 0 case ends with the status
    of the single call, and the theta after it is served -- cold bit for bit as the one before it, warm as the chained calls"""
    d = load_golden(M808[0])
    g0, G, yT, YT, theta = golden_vectors(d)
    thetas = [10.0, theta, 10.0]
    with bioen_amd.Context(yT, YT) as ctx:
        single = ctx.opt_dual_newton_logw(g0, G, theta, PARAMS)
        cold = ctx.opt_dual_newton_logw_series(thetas, g0, G, PARAMS, warm=False)
        warm = ctx.opt_dual_newton_logw_series(thetas, g0, G, PARAMS)
        g = g0
        for t, w_ in zip(thetas, warm):
            chained = ctx.opt_dual_newton_logw(g, G, t, PARAMS)
            assert bits(w_) == bits(chained)
            g = chained["g"]
    print("potra part 1: cold statuses %s, warm statuses %s" % ([r["status"] for r in cold], [r["status"] for r in warm]))
    assert single["status"] != 0 and bits(cold[1]) == bits(single)
    assert cold[0]["status"] == 0 and bits(cold[2]) == bits(cold[0])
    assert warm[0]["status"] == 0 and np.isfinite(warm[2]["fmin"])


def _find_args(d):
    return (np.asarray(d["GInit"], dtype=np.float64).reshape(-1, 1), d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1))


@pytest.mark.parametrize("mod", ["", "dual_newton:series=cold", "dual_newton:hessian=gram_bf16"])
def test_find_optimum_series_on_the_device(bioen_amd, mod):
    d = load_golden("synth_logw_M64xN2000.npz")
    thetas = [100.0, 10.0, 1.0]
    cfg = minimize.Parameters("dual_newton", mod)
    cfg.update(verbose=False)
    plain = minimize.Parameters("dual_newton")
    plain.update(verbose=False)
    series = log_weights.find_optimum_series(*_find_args(d), thetas, cfg)
    info = list(c_bioen.last_opt_info)
    assert len(series) == len(info) == 3 and all(("gram_bf16" in mod) == (r["bf16_passes"] > 0) for r in info)
    for t, got in zip(thetas, series):
        ref = log_weights.find_optimum(*_find_args(d), t, plain)
        assert got[3] == ref[3] and abs(got[4] - ref[4]) <= 1e-6
        assert np.abs(got[0] - ref[0]).max() <= 1e-5 * ref[0].max()
        assert np.abs(got[1] - ref[1]).max() <= 1e-5 * np.abs(ref[1]).max()
        if mod == "dual_newton:series=cold":
            assert got[4] == ref[4] and np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
    with pytest.raises(RuntimeError, match=r"theta = 1\.0.*return code 1"):
        log_weights.find_optimum_series(*_find_args(d), [1.0, 0.1], minimize.Parameters("dual_newton", "dual_newton:max_iterations=1"))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def raw_series(ctx, g0, G, thetas, source=1, warm=1):
    """the raw binding: -> the return code"""
    from bioen_amd import _lib
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    cfg = _lib.logw_newton_config(PARAMS)
    out = np.empty((max(len(th), 1), ctx.n))
    res = (_lib.LogwNewtonSeriesResult * max(len(th), 1))()
    return _lib.lib().bioen_logwn_series(ctx._h, _lib.ptr(g0), _lib.ptr(G), _lib.ptr(th), len(th), C.byref(cfg), source, warm,
                                         _lib.ptr(out), res)


def test_bad_arguments_leave_the_point_and_a_session_alone(bioen_amd):
    from bioen_amd._lib import BioenHipError
    yT, YT, G, g = logw_problem((64, 2000))
    v = np.random.default_rng(1).standard_normal(2000)
    bad = (dict(thetas=[10.0, 0.0]), dict(thetas=[-1.0, 10.0]), dict(thetas=[10.0, float("nan")]), dict(thetas=[float("inf")]),
           dict(thetas=[]), dict(thetas=[10.0], source=2), dict(thetas=[10.0], source=-1), dict(thetas=[10.0], warm=2))
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.logw_hessp(v, g=g, G=G, theta=THETA)
        for kw in bad:
            assert raw_series(ctx, g, G, **kw) == -1, kw                  # BIOEN_HIP_EINVAL
        with pytest.raises(BioenHipError, match="theta > 0"):
            ctx.opt_dual_newton_logw_series([10.0, 0.0], g, G)
        with pytest.raises(BioenHipError, match="ntheta >= 1"):
            ctx.opt_dual_newton_logw_series([], g, G)
        with pytest.raises(RuntimeError, match="dual_newton:hessian=fp32 not recognized"):
            ctx.opt_dual_newton_logw_series([10.0], g, G, hessian="fp32")
        with pytest.raises(RuntimeError, match="dual_newton:hessian=fp32 not recognized"):
            ctx.opt_dual_newton_logw(g, G, THETA, dict(hessian="fp32"))
        assert np.array_equal(ctx.logw_hessp(v), hv)                      # the point is served as before
        ctx.logw_fdf(g, G, THETA)
        ctx.bfgs_begin(g, G, THETA)
        ctx.bfgs_trial(1e-3, True)
        for kw in bad:
            assert raw_series(ctx, g, G, **kw) == -1, kw
        fv, _ = ctx.bfgs_trial(2e-3, False)                               # the session goes on
        assert np.isfinite(fv)


def test_refusals_of_the_state(bioen_amd, monkeypatch):
    yT, YT, G, g = logw_problem((64, 2000))
    v = np.random.default_rng(1).standard_normal(2000)
    calls = ((lambda c: c.logw_cov_bf16(g=g, G=G, theta=THETA), "bioen_logwn_cov_bf16"),
             (lambda c: c.opt_dual_newton_logw_series([10.0, 1.0], g, G, hessian="gram_bf16"), "bioen_logwn_series"))
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.logw_cov_bf16(), "no point on this context", "bioen_logwn_cov")
        ctx.set_storage("fp32")                                          # the reduced-storage copies
        for call, name in calls:
            estate(lambda: call(ctx), name, "reduced-storage")
        ctx.set_storage("f64")
        assert "logw_gram" not in ctx.footprint()[0]
    t = problem((1100, 2000))                                            # row panels
    with bioen_amd.Context(t[0], t[1]) as ctx:
        Gt = np.log(t[2])
        hv, _, _ = ctx.logw_hessp(np.ones(2000), g=Gt, G=Gt, theta=THETA)
        for name, call in (("bioen_logwn_cov_bf16", lambda: ctx.logw_cov_bf16(g=Gt, G=Gt, theta=THETA)),
                           ("bioen_logwn_series", lambda: ctx.opt_dual_newton_logw_series([10.0], Gt, Gt))):
            estate(call, name, "M <= 1024")
        assert np.array_equal(ctx.logw_hessp(np.ones(2000)), hv)          # the point is left alone
        assert "logw_gram" not in ctx.footprint()[0]
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")           # the streaming fallback: no strip copies
    with bioen_amd.Context(yT, YT) as ctx:
        f0, _ = ctx.logw_fdf(g, G, THETA)
        assert np.isfinite(f0) and ctx.footprint()[0] == {"rowmajor"}
        for call, name in calls:
            estate(lambda: call(ctx), name, "strip copies")
        assert "logw_gram" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, G, g = logw_problem((129, 1000))

    def workload(ctx, local_segments):
        estate(lambda: ctx.logw_cov_bf16(g=g, G=G, theta=THETA), "bioen_logwn_cov_bf16", "structure-sharded")
        estate(lambda: ctx.opt_dual_newton_logw_series([10.0, 1.0], g, G), "bioen_logwn_series", "structure-sharded")
        return True

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))

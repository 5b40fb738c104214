"""GPU tests of the log-weights dual Newton minimizer (csrc/kernels_logw_newton.hip, csrc/api_logw_newton.cpp,
Context.opt_dual_newton_logw) WHERE ITS LOOPS RUN LONG and in the regimes the five small fixtures of
tests/test_hip_logw_dual_newton.py never enter:

  the step itself        -b = -Yc grad with its rank correction (k_lgram_finish, the sg quad-sum of k_logw_gram), the operand
                         r_c + row_scale o z (k_logwn_operand), the centred adjoint on it, u and grad . u (k_logwn_step), the
                         three maxima (k_logwn_stats) -- a Newton loop forgives a wrong direction, so the DIRECTION is compared
  long chains            sets of k_logw_gram that chain 7 ... 132 strips, N-vector kernels with several blocks per segment,
                         the folded forward chunks and the strip adjoint at production geometry
  regimes                the affine model inside the loop, one canonical segment, M = 1024 and mp > m, a rejected first trial
                         (alpha = 1/2), status 2 on the device

The step is observed through the existing call: opt_dual_newton_logw with max_iterations = 1 returns g1 = g0 + alpha u with
alpha = 2^-(evaluations - 2), a power of two, so (g1 - g0) / alpha is the device's u up to the rounding of the sum
(<= eps max|g| / alpha, 1e-14 here).

The truth has no float64 on its path: w, ybar, r, dev, P, grad in numpy.longdouble from g0; (C + theta I) z = -b by iterative
refinement -- the operator A v = Yc (w o (Yc^T v)) + theta v and b = Yc grad applied in longdouble (O(MN), C never formed),
the preconditioner a float64 Cholesky factor of the restatement's covariance + theta I --; u = -[(dev - P) + Yc^T (r + z) /
theta].  Every comparison first asserts that the refinement converged: the last correction <= 1e-17 max|z| within 5 sweeps.

Every test asserts its regime through Context.strip_plan before it computes (tests/test_hip_strip_loops.py: REGIMES), and
the depth of the Gram chains computed from the plan (GRAM_CHAIN).  tests/README.md has the table and the measured errors."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import load_golden
from test_hip_forces_gram import GATE, _gram_ld
from test_hip_strip_loops import L, REGIMES, assert_forward_regime, enter_regime, logw_problem
from test_logw_dual_newton import M808, PARAMS, case_args

from bioen_amd.optimize import log_weights, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

THETA = 10.0
SHAPES = [(64, 131500), (300, 9000), (600, 33700), (1024, 9000), (1024, 33700)]
AFFINE_SHAPES = [(300, 9000), (600, 33700)]
# shape -> the most strips a set of k_logw_gram chains (tg), by hand from logw_gram_plan: ntiles = t (t + 1) / 2 with
# t = ceil(ceil(M / 64) / 2), gs = max(1, min(sps, ceil(512 / (segments ntiles)))), tg = ceil(sps / gs)
GRAM_CHAIN = {(64, 131500): 17, (300, 9000): 7, (600, 33700): 53, (1024, 9000): 38, (1024, 33700): 132}
# shape -> evaluations of the restatement's one-iteration run (2: alpha = 1 accepted; 3: the first trial rejected), and
# (iterations, evaluations, factorisations) of its whole run -- measured on the CPU; the tests assert that the restatement
# still gives them, then that the device does
FIRST_STEP = {(64, 131500): 2, (300, 9000): 2, (600, 33700): 3, (1024, 9000): 3, (1024, 33700): 3}
COUNTS = {(64, 131500): (3, 4, 3), (300, 9000): (6, 7, 6), (600, 33700): (7, 9, 7), (1024, 9000): (7, 10, 7),
          (1024, 33700): (7, 10, 7)}
AFFINE_COUNTS = {(300, 9000): (9, 13, 9), (600, 33700): (9, 16, 9)}


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    c_bioen.clear_cache()


# ---- regimes -----------------------------------------------------------------------------------------------------------
def assert_newton_regime(ctx, shape, local_segments=None):
    """the forward plan of tests/test_hip_strip_loops.py's table, and the depth of k_logw_gram's chains from it"""
    p = assert_forward_regime(ctx, shape, local_segments=local_segments)
    nsl = -(-shape[0] // 64)
    t = (nsl + 1) // 2
    ntiles = t * (t + 1) // 2
    gs = max(1, min(p["sps"], -(-512 // (p["local_segments"] * ntiles))))
    tg = -(-p["sps"] // gs)
    if local_segments is None:
        assert tg == GRAM_CHAIN[shape] and tg >= 7, (p, gs, tg)
    return dict(p, gram_gs=gs, gram_tg=tg)


# ---- data, the restatement's runs and the truth, once per case -----------------------------------------------------------
_CASES, _HOST, _STEP = {}, {}, {}


def case(shape, affine=False):
    """-> dict(y: the model's matrix in longdouble, y64: its float64 rounding (what the restatement runs on), yT, YT, G, g0,
    off, sc); g0 = logw_problem(shape)'s point G + 0.3 sigma.  The affine model: off ~ N(0, 0.5), sc ~ U(0.5, 1.5), seed 3
    (tests/test_hip_logw_dual_newton.py: test_cov_with_an_affine_model), folded into the matrix in longdouble"""
    key = (shape, affine)
    if key not in _CASES:
        yT, YT, G, g0, _ = logw_problem(shape)
        c = dict(yT=yT, YT=YT, G=G, g0=g0, off=None, sc=None)
        if affine:
            rng = np.random.default_rng(3)
            c["off"], c["sc"] = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
            c["y"] = c["off"][:, None].astype(L) + c["sc"][:, None].astype(L) * yT.astype(L)
            c["y64"] = c["y"].astype(np.float64)
        else:
            c["y"], c["y64"] = yT.astype(L), yT
        _CASES[key] = c
    return _CASES[key]


def host_run(shape, affine=False, max_iterations=None):
    """log_weights.dual_newton_bioen_log_posterior_base on the case's data, once per module"""
    key = (shape, affine, max_iterations)
    if key not in _HOST:
        c = case(shape, affine)
        params = PARAMS if max_iterations is None else dict(PARAMS, max_iterations=max_iterations)
        _HOST[key] = log_weights.dual_newton_bioen_log_posterior_base(c["g0"], c["G"], c["y64"], c["YT"], THETA, params)
    return _HOST[key]


def _threads(n):
    return [b for b in np.array_split(np.arange(n), 8) if b.size]


def rows_times(y, t):
    """y t in longdouble, row blocks on eight threads (numpy's longdouble products release the interpreter lock)"""
    with ThreadPoolExecutor(8) as workers:
        return np.concatenate(list(workers.map(lambda rows: y[rows[0]:rows[-1] + 1] @ t, _threads(y.shape[0]))))


def times_columns(v, y):
    """v y in longdouble, column blocks on eight threads"""
    with ThreadPoolExecutor(8) as workers:
        return np.concatenate(list(workers.map(lambda cols: v @ y[:, cols[0]:cols[-1] + 1], _threads(y.shape[1]))))


def point_longdouble(y, YT, G, g, theta):
    """the pieces of a log-weights point in 80-bit arithmetic (tests/test_hip_strip_loops.py: logw_truth)"""
    gl, Gl, Yl = g.astype(L), G.astype(L), YT.astype(L)
    e = np.exp(gl - gl.max())
    w = e / e.sum()
    ybar = rows_times(y, w)
    r = ybar - Yl
    dev = gl - Gl
    P = w @ dev
    gamma = L(theta) * (dev - P) + (times_columns(r, y) - ybar @ r)
    return dict(w=w, ybar=ybar, r=r, dev=dev, P=P, gamma=gamma, grad=w * gamma)


def step_longdouble(shape, affine=False):
    """-> dict(u, w, sweeps, last: max|dz| / max|z| of the last correction): the dual Newton step at the case's g0 in
    80-bit arithmetic, (C + theta I) z = -b by iterative refinement on a float64 Cholesky factor"""
    import scipy.linalg
    key = (shape, affine)
    if key in _STEP:
        return _STEP[key]
    c = case(shape, affine)
    y, theta = c["y"], L(THETA)
    p = point_longdouble(y, c["YT"], c["G"], c["g0"], THETA)
    w, ybar = p["w"], p["ybar"]

    def centred_adjoint(v):                                   # Yc^T v
        return times_columns(v, y) - ybar @ v

    def centred_forward(t):                                   # Yc t
        return rows_times(y, t) - ybar * t.sum()

    def A(v):
        return centred_forward(w * centred_adjoint(v)) + theta * v

    p64 = log_weights._dual_newton_point(c["g0"], c["G"], c["y64"], c["YT"], THETA, 0.0)
    factor = scipy.linalg.cho_factor(log_weights.dual_newton_covariance(p64, c["y64"]) + THETA * np.eye(shape[0]), lower=True)
    negb = -centred_forward(p["grad"])
    z, sweeps, last = np.zeros(shape[0], dtype=L), 0, np.inf
    while sweeps < 5 and last > 1e-17:
        res = negb - A(z) if sweeps else negb
        dz = scipy.linalg.cho_solve(factor, res.astype(np.float64)).astype(L)
        z = z + dz
        sweeps += 1
        last = float(np.abs(dz).max() / np.abs(z).max())
    u = -((p["dev"] - p["P"]) + centred_adjoint(p["r"] + z) / theta)
    _STEP[key] = dict(u=u, w=w, sweeps=sweeps, last=last, bmax=float(np.abs(negb).max()))
    return _STEP[key]


def converged(ref):
    """the reference's own condition, asserted before anything is compared with it"""
    assert ref["last"] <= 1e-17 and ref["sweeps"] <= 5, (ref["sweeps"], ref["last"])


# ---- 1, 2. the step ------------------------------------------------------------------------------------------------------
def one_step(ctx, c):
    return ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, dict(PARAMS, max_iterations=1))


def check_step(ctx, shape, affine, plan):
    c, ref = case(shape, affine), step_longdouble(shape, affine)
    converged(ref)
    host = host_run(shape, affine, max_iterations=1)
    assert host["status"] == 1 and host["iterations"] == 1
    if not affine:
        assert host["evaluations"] == FIRST_STEP[shape]       # the regime: the first trial accepted or rejected
    # k_lgram_finish's rank correction of b is -s_i (ybar - centre)_i sum_j grad_j on the resident matrix (centre = YTilde,
    # s the model's scales): a sum that is zero in exact arithmetic.  What a build WITHOUT it loses is below the step's gate
    # by construction -- it passes this file (tests/README.md) --, and this holds the premise: the correction stays the
    # rounding it is meant to remove
    _, _, grad0 = ctx.logw_cov(g=c["g0"], G=c["G"], theta=THETA, cov=False)
    offset = (c["yT"] @ ref["w"].astype(np.float64) - c["YT"]) * (c["sc"] if affine else 1.0)
    rank_term = float(np.abs(offset).max()) * abs(float(grad0.sum())) / ref["bmax"]
    print("%dx%d%s: max|ybar - centre| |sum grad| = %.3g max|b|" % (shape + (" affine" if affine else "", rank_term)))
    assert rank_term <= 1e-10
    res = one_step(ctx, c)
    assert res["status"] == 1 and res["iterations"] == 1 and res["factorisations"] == 1
    alpha = 2.0 ** -(res["evaluations"] - 2)
    u_dev = (res["g"] - c["g0"]) / alpha
    S = float(np.abs(ref["u"]).max())
    err = float(np.abs(u_dev.astype(L) - ref["u"]).max()) / S
    gauge = abs(float(ref["w"] @ u_dev.astype(L))) / S
    print("%dx%d%s: %d segment(s), plan %s; alpha %g, |u - u_ld| = %.3g max|u|, |w . u| = %.3g max|u|; reference: %d sweeps, "
          "last correction %.3g max|z|" % (shape + (" affine" if affine else "", plan["local_segments"], plan, alpha, err, gauge,
                                            ref["sweeps"], ref["last"])))
    assert err <= 1e-10
    assert gauge <= 1e-12
    assert res["evaluations"] == host["evaluations"]
    # the returned point is the kept point; gmax, fmin and wmax are that point's
    C_kept = ctx.logw_cov()
    C, f, grad = ctx.logw_cov(g=res["g"], G=c["G"], theta=THETA)
    assert np.array_equal(C_kept, C)
    assert res["gmax"] == np.abs(grad).max() and res["fmin"] == f
    g1 = res["g"].astype(L)
    e = np.exp(g1 - g1.max())
    wmax = float((e / e.sum()).max())
    assert abs(res["wmax"] - wmax) <= 1e-12 * wmax
    return res


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_step_against_longdouble(bioen_amd, monkeypatch, shape):
    """u of one iteration within 1e-10 max|u| of the 80-bit step, w . u = 0, the trial count the restatement's (alpha = 1 at
    300 x 9000 and 64 x 131500, 1/2 at the three others: the device loop's rejection path), the returned point kept"""
    enter_regime(monkeypatch, shape)
    c = case(shape)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        plan = assert_newton_regime(ctx, shape)
        check_step(ctx, shape, False, plan)


@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=case_id)
def test_step_under_the_affine_model(bioen_amd, monkeypatch, shape):
    """row offsets and scales set on the context, folded into the truth's matrix in longdouble: C_A = S C S, b_A = S b, the
    operand r_c + row_scale o z; (0, 1) afterwards gives the plain model's step bit for bit"""
    enter_regime(monkeypatch, shape)
    c = case(shape, True)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        plan = assert_newton_regime(ctx, shape)
        plain = one_step(ctx, c)
        ctx.set_affine(c["off"], c["sc"])
        res = check_step(ctx, shape, True, plan)
        assert not np.array_equal(res["g"], plain["g"])
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))
        again = one_step(ctx, c)
        assert np.array_equal(again["g"], plain["g"]) and again["fmin"] == plain["fmin"]
        assert again["evaluations"] == plain["evaluations"]


def test_step_and_loop_on_one_strip_copy(bioen_amd):
    """1024 x 33700 with one strip copy resident: the centred adjoint on r + z is the forces kernels' ADJ form on the row-sum
    order copy (tests/test_hip_strip_loops.py: one_copy), Gram chains of 132 strips beside it"""
    shape = (1024, 33700)
    c, host = case(shape), host_run(shape)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        ctx.set_one_copy(True)
        plan = assert_newton_regime(ctx, shape)
        check_step(ctx, shape, False, plan)
        assert ctx.layout()["one_copy"] == 1
        res = ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, PARAMS)
    assert res["status"] == 0 and counts(res) == counts(host) == COUNTS[shape]
    assert abs(res["fmin"] - host["fmin"]) <= 1e-9 * abs(host["fmin"])


def gamma_threshold(c, g):
    """gamma = theta d + a with d = dev - P and a = Yc^T r, neither depending on theta: -> (the theta at which max|gamma| =
    theta, by bisection on 80-bit values; d; a).  Needs max|d| < 1: below the root the stopping test's second half fails,
    above it holds"""
    p = point_longdouble(c["y"], c["YT"], c["G"], g, 1.0)
    d = p["dev"] - p["P"]
    a = p["gamma"] - d
    assert float(np.abs(d).max()) < 0.9

    def excess(theta):
        return float(np.abs(L(theta) * d + a).max()) - theta
    lo, hi = 1e-3, 1e9
    assert excess(lo) > 0.0 > excess(hi)
    for _ in range(100):
        mid = np.sqrt(lo * hi)
        if excess(mid) > 0.0:
            lo = mid
        else:
            hi = mid
    return float(hi), d, a


@pytest.mark.parametrize("shape", [(64, 131500), (1024, 9000)], ids=case_id)
def test_gamma_maximum_decides_at_its_threshold(bioen_amd, monkeypatch, shape):
    """k_logwn_stats's third maximum is returned nowhere; with gtol out of the way and no iteration allowed the status IS the
    comparison max|gamma| <= theta.  At G + 0.25 (g0 - G) that comparison changes sides at one theta (80-bit bisection);
    1e-6 below it the device says 1, 1e-6 above it 0 -- four decades clear of the 1e-10 max|gamma| an N-vector out of the
    matrix passes is held to.  Several blocks per segment at 64 x 131500, one segment at 1024 x 9000"""
    enter_regime(monkeypatch, shape)
    c = case(shape)
    g = c["G"] + 0.25 * (c["g0"] - c["G"])
    theta, d, a = gamma_threshold(c, g)
    decide = dict(gtol=1e300, max_iterations=0)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        assert_newton_regime(ctx, shape)
        for side, status in ((1.0 - 1e-6, 1), (1.0 + 1e-6, 0)):
            t = theta * side
            margin = float(np.abs(L(t) * d + a).max()) / t - 1.0
            print("%dx%d: theta %.17g, 80-bit max|gamma| / theta - 1 = %.3g" % (shape + (t, margin)))
            assert (margin >= 1e-8) if status else (margin <= -1e-8)         # the truth is clear of the threshold itself
            res = ctx.opt_dual_newton_logw(g, c["G"], t, decide)
            assert (res["status"], res["iterations"], res["evaluations"]) == (status, 0, 1)


def test_cov_on_the_deepest_affordable_chain(bioen_amd):
    """logw_cov at 64 x 131500 (sets of 16 and 17 strips, 64 sets per segment) against the centred formula in longdouble"""
    shape = (64, 131500)
    c = case(shape)
    p = point_longdouble(c["y"], c["YT"], c["G"], c["g0"], THETA)
    ref = _gram_ld(c["y"] - p["ybar"][:, None], p["w"]).astype(np.float64)
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        assert_newton_regime(ctx, shape)
        C, _, _ = ctx.logw_cov(g=c["g0"], G=c["G"], theta=THETA)
        d = float(np.abs(C - ref).max() / np.abs(ref).max())
        print("64x131500: |C - C_ld| = %.3g max|C|" % d)
        assert np.array_equal(C, C.T)
        assert d <= GATE
        assert np.array_equal(ctx.logw_cov(), C)


# ---- 3. the whole loop ---------------------------------------------------------------------------------------------------
def counts(res):
    return res["iterations"], res["evaluations"], res["factorisations"]


def bits(res):
    return res["g"].tobytes(), res["fmin"], res["gmax"], res["wmax"], res["status"], counts(res)


def check_loop(bioen_amd, shape, affine):
    c = case(shape, affine)
    host = host_run(shape, affine)
    assert host["status"] == 0 and counts(host) == (AFFINE_COUNTS if affine else COUNTS)[shape]
    with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
        plan = assert_newton_regime(ctx, shape)
        if affine:
            ctx.set_affine(c["off"], c["sc"])
        res = ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, PARAMS)
        second = ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, PARAMS)
    with bioen_amd.Context(c["yT"], c["YT"]) as fresh:
        if affine:
            fresh.set_affine(c["off"], c["sc"])
        third = fresh.opt_dual_newton_logw(c["g0"], c["G"], THETA, PARAMS)
    p = point_longdouble(c["y"], c["YT"], c["G"], res["g"], THETA)
    gmax, wmax, cmax = float(np.abs(p["grad"]).max()), float(p["w"].max()), float(np.abs(p["gamma"]).max())
    w_host, _ = log_weights.getWeights(host["g"])
    dw = float(np.abs(p["w"].astype(np.float64) - np.asarray(w_host).reshape(-1)).max() / np.asarray(w_host).max())
    print("%dx%d%s: %d segment(s), Gram chains of %d; device %d / %d / %d, restatement %d / %d / %d; fmin %.15g, restatement "
          "%.15g; 80-bit max|grad| = %.3g max w, max|gamma| = %.3g; max|dw| = %.3g max w"
          % (shape + (" affine" if affine else "", plan["local_segments"], plan["gram_tg"]) + counts(res) + counts(host)
             + (res["fmin"], host["fmin"], gmax / wmax, cmax, dw)))
    assert res["status"] == 0
    assert counts(res) == counts(host)
    assert abs(res["fmin"] - host["fmin"]) <= 1e-9 * abs(host["fmin"])
    assert gmax <= PARAMS["gtol"] * wmax * (1 + 1e-6) and cmax <= THETA
    assert dw <= 1e-5
    assert bits(second) == bits(res)                          # the same context again: the same bits
    assert bits(third) == bits(res)                           # and a fresh one
    return res


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_loop_against_the_restatement(bioen_amd, monkeypatch, shape):
    """status 0 with the restatement's iterations / evaluations / factorisations, its fmin to 1e-9 and its weights to 1e-5
    max w; the 80-bit gradient at the returned point passes the stopping test on its own; run again and on a fresh context:
    the same bits"""
    enter_regime(monkeypatch, shape)
    check_loop(bioen_amd, shape, False)


@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=case_id)
def test_loop_under_the_affine_model(bioen_amd, monkeypatch, shape):
    """the nuisance refits' regime: set_affine holds inside the loop"""
    enter_regime(monkeypatch, shape)
    check_loop(bioen_amd, shape, True)


def test_eight_segments_reach_the_one_segment_minimum(bioen_amd, monkeypatch):
    """300 x 9000: the canonical segments change the bits (by design) and nothing else"""
    shape = (300, 9000)
    c = case(shape)
    out = {}
    for segments in (1, 8):
        if segments == 1:
            monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")
        else:
            monkeypatch.delenv("BIOEN_HIP_SEGMENTS", raising=False)
        with bioen_amd.Context(c["yT"], c["YT"]) as ctx:
            assert ctx.strip_plan(0)["local_segments"] == segments
            out[segments] = ctx.opt_dual_newton_logw(c["g0"], c["G"], THETA, PARAMS)
    assert out[1]["status"] == 0 and out[8]["status"] == 0
    assert abs(out[8]["fmin"] - out[1]["fmin"]) <= 1e-9 * abs(out[1]["fmin"])


# ---- 4. the unsolved regime ------------------------------------------------------------------------------------------------
def golden_vectors(d):
    return (np.asarray(d["GInit"], dtype=np.float64).reshape(-1), np.asarray(d["G"], dtype=np.float64).reshape(-1),
            np.asarray(d["yTilde"], dtype=np.float64), np.asarray(d["YTilde"], dtype=np.float64).reshape(-1), float(d["theta"]))


@pytest.mark.parametrize("name", M808)
def test_the_weak_condition_on_the_m808_fixtures(bioen_amd, name):
    """tests/test_logw_dual_newton.py's test on the device: never status 0 above the golden; theta = 0 is refused; the
    context serves an evaluation afterwards"""
    from bioen_amd._lib import BioenHipError
    d = load_golden(name)
    g0, G, yT, YT, theta = golden_vectors(d)
    with bioen_amd.Context(yT, YT) as ctx:
        if theta > 0.0:
            res = ctx.opt_dual_newton_logw(g0, G, theta, PARAMS)
            print("%s: theta %g, status %d, fmin - golden = %.6g, %d iterations / %d evaluations"
                  % (name, theta, res["status"], res["fmin"] - float(d["lbfgs_conv_fmin"]), res["iterations"], res["evaluations"]))
            assert res["status"] != 0 or res["fmin"] <= float(d["lbfgs_conv_fmin"]) + 1e-6
        else:
            with pytest.raises(BioenHipError, match="theta > 0"):
                ctx.opt_dual_newton_logw(g0, G, theta, PARAMS)
        f, grad = ctx.logw_fdf(g0, G, theta)
        assert np.isfinite(f) and np.isfinite(grad).all()


def test_gamma_test_is_what_rejects_the_collapsed_point(bioen_amd):
    """potra part 1 (theta = 0.001) after ONE step: max|grad| <= gtol max w holds far above the golden, and the run has not
    stopped with status 0 -- k_logwn_stats's third maximum"""
    d = load_golden(M808[0])
    g0, G, yT, YT, theta = golden_vectors(d)
    with bioen_amd.Context(yT, YT) as ctx:
        one = ctx.opt_dual_newton_logw(g0, G, theta, dict(PARAMS, max_iterations=1))
    assert one["status"] == 1 and one["gmax"] <= 1e-6 * one["wmax"] and one["fmin"] > float(d["lbfgs_conv_fmin"]) + 1.0


def test_status_two_raises_through_find_optimum(bioen_amd):
    """potra part 1: the device run ends where the restatement does, at the rounding floor of f, and find_optimum raises
    instead of returning a false minimum"""
    d = load_golden(M808[0])
    host = log_weights.dual_newton_bioen_log_posterior_base(d["GInit"], *case_args(d), params=PARAMS)
    assert host["status"] == 2
    cfg = minimize.Parameters("dual_newton")
    cfg.update(verbose=False)
    with pytest.raises(RuntimeError, match="return code %d" % host["status"]):
        log_weights.find_optimum(np.asarray(d["GInit"], dtype=np.float64).reshape(-1, 1), d["G"], d["y"], d["yTilde"],
                                 d["YTilde"].reshape(1, -1), d["theta"], cfg)
    info = dict(c_bioen.last_opt_info)
    print("potra part 1: device status %d after %d iterations / %d evaluations; restatement status %d after %d / %d"
          % (info["status"], info["iterations"], info["evaluations"], host["status"], host["iterations"], host["evaluations"]))
    assert info["status"] == host["status"]

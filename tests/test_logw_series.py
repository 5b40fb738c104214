"""The log-weights theta series by dual Newton on a split-BF16 covariance, on the CPU: the numpy
statements that specify the device loop -- log_weights.dual_newton_covariance_bf16, dual_newton_bioen_log_posterior_base with
params["hessian"] and its switch, dual_newton_series_base -- and find_optimum_series with Parameters("dual_newton") on the
numpy objective.  tests/test_hip_logw_gram_bf16.py compares the device with the runs computed here."""
import numpy as np
import pytest

from conftest import load_golden

from bioen_amd.optimize import log_weights, minimize
from test_logw_dual_newton import GOOD, PARAMS, case_args, check_against_golden, host_dual_newton

BF16 = dict(PARAMS, hessian="gram_bf16")
THETAS = [1000.0, 316.0, 100.0, 31.6, 10.0, 3.16, 1.0, 0.316]
SERIES_CASES = ["synth_logw_M64xN2000", "recipe_300x9000"]

_RUNS, _SERIES = {}, {}


def counts(res):
    return res["iterations"], res["evaluations"], res["factorisations"]


def host_dual_newton_bf16(name):
    """the hessian=gram_bf16 restatement's run on a golden, computed once and shared"""
    if name not in _RUNS:
        d = load_golden(name)
        _RUNS[name] = (d, log_weights.dual_newton_bioen_log_posterior_base(
            np.asarray(d["GInit"], dtype=np.float64).reshape(-1), *case_args(d), params=BF16))
    return _RUNS[name]


def series_problem(case):
    """-> (yTilde, YTilde, G, g0): the golden's own start, or the 300 x 9000 recipe problem (tests/test_hip_strip_loops.py:
    data) from its prior"""
    if case == "recipe_300x9000":
        from test_hip_strip_loops import data
        yT, YT, G = data((300, 9000))[:3]
        return yT, YT, G, G.copy()
    d = load_golden(case + ".npz")
    return (np.asarray(d["yTilde"], dtype=np.float64), np.asarray(d["YTilde"], dtype=np.float64).reshape(-1),
            np.asarray(d["G"], dtype=np.float64).reshape(-1), np.asarray(d["GInit"], dtype=np.float64).reshape(-1))


def host_series(case, warm, params=PARAMS, thetas=THETAS):
    """dual_newton_series_base on a series problem, computed once and shared"""
    key = (case, warm, tuple(sorted(params.items())), tuple(thetas))
    if key not in _SERIES:
        yT, YT, G, g0 = series_problem(case)
        _SERIES[key] = log_weights.dual_newton_series_base(g0, G, yT, YT, thetas, params, warm=warm)
    return _SERIES[key]


def weights(g):
    return np.asarray(log_weights.getWeights(g)[0]).reshape(-1)


# ---- the covariance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synth_logw_M37xN500.npz", "synth_logw_M129xN257.npz"])
def test_covariance_from_split_operands(name):
    """symmetric bit for bit, not the FP64 covariance, and within 3 * 2^-16 sqrt(G'_ii G'_kk) of it: each operand keeps 16
    significant bits and lo lo is dropped (Cauchy-Schwarz on the summands)"""
    d = load_golden(name)
    G, yT, YT, theta = case_args(d)
    yT, YT = np.asarray(yT, dtype=np.float64), np.asarray(YT, dtype=np.float64).reshape(-1)
    g = np.asarray(d["GInit"], dtype=np.float64).reshape(-1) + 0.3 * np.random.default_rng(11).standard_normal(yT.shape[1])
    p = log_weights._dual_newton_point(g, np.asarray(G, dtype=np.float64).reshape(-1), yT, YT, theta, 0.0)
    C, Cb = log_weights.dual_newton_covariance(p, yT), log_weights.dual_newton_covariance_bf16(p, yT, YT)
    a = yT - YT[:, None]
    s = np.sqrt(np.einsum("ij,j,ij->i", a, p["w"], a))
    ratio = float((np.abs(Cb - C) / np.outer(s, s)).max())
    print("%s: max |C~ - C|_ik / sqrt(G'_ii G'_kk) = %.3g (bound %.3g)" % (name, ratio, 3 * 2.0 ** -16))
    assert np.array_equal(Cb, Cb.T)
    assert 0.0 < ratio <= 3 * 2.0 ** -16


# ---- the loop with the BF16 source ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOOD)
def test_bf16_loop_against_the_fp64_loop(name):
    """the gates un-widened, and the FP64 restatement's iterations and evaluations: only the step's quality depends on C"""
    d, res = host_dual_newton_bf16(name)
    _, _, ref = host_dual_newton(name)
    check_against_golden(d, res)
    assert counts(res) == counts(ref)
    assert res["bf16_passes"] == res["factorisations"] and res["switched"] is False
    assert ref["bf16_passes"] == 0 and ref["switched"] is False
    dw = np.abs(weights(res["g"]) - weights(ref["g"])).max() / weights(ref["g"]).max()
    print("%s: |dfmin| = %.3g, max |dw| = %.3g max w against the FP64 loop" % (name, abs(res["fmin"] - ref["fmin"]), dw))
    assert abs(res["fmin"] - ref["fmin"]) <= 1e-9 * abs(ref["fmin"]) and dw <= 1e-5


def test_default_source_keeps_its_bits():
    """no key and "gram": the same run, bit for bit"""
    name = "synth_logw_M37xN500.npz"
    d, g0, ref = host_dual_newton(name)
    res = log_weights.dual_newton_bioen_log_posterior_base(g0, *case_args(d), params=dict(PARAMS, hessian="gram"))
    assert np.array_equal(res["g"], ref["g"]) and res["fmin"] == ref["fmin"] and counts(res) == counts(ref)


def test_switch_when_the_source_is_wrong_at_the_floor():
    """The rule exercised by injection (forces.newton_bioen_log_posterior_base's hess= hook is the model): a "gram_bf16"
    source that is the FP64 covariance until the step's slope reaches the floor and 1e6 C from there on -- (1e6 C + theta I)
    z = -b leaves z ~ 0 in the range of C, the step loses its data term and max|grad| does not fall.  floor_ulps = 1e6 puts
    the floor where the run still has an iteration to go.  The run goes over to the FP64 source once, pays the rejected
    trial, the kept point again and one more factorisation, and ends with status 0 at the FP64 loop's optimum; with the
    FP64 source the same injection ends with status 2."""
    name = "synth_logw_M64xN2000.npz"
    d, g0, _ = host_dual_newton(name)
    G, yT, YT, theta = case_args(d)
    prm = dict(PARAMS, floor_ulps=1e6, hessian="gram_bf16")
    plain = log_weights.dual_newton_bioen_log_posterior_base(g0, G, yT, YT, theta, dict(prm, hessian="gram"))
    assert plain["status"] == 0
    calls = []

    def wrong_at_the_floor(p, yT_, centre):
        C = log_weights.dual_newton_covariance(p, yT_)
        u, _ = log_weights.dual_newton_step(p, yT_, theta, C=C)
        at_floor = abs(float(p["grad"].dot(u))) <= prm["floor_ulps"] * np.finfo(np.float64).eps * abs(p["f"])
        calls.append(bool(at_floor))
        return 1e6 * C if at_floor else C

    res = log_weights.dual_newton_bioen_log_posterior_base(g0, G, yT, YT, theta, prm, cov=dict(gram_bf16=wrong_at_the_floor))
    print("switch: status %d, %d / %d / %d, bf16 passes %d, source wrong at the floor %d time(s); plain %d / %d / %d"
          % ((res["status"],) + counts(res) + (res["bf16_passes"], sum(calls)) + counts(plain)))
    assert any(calls), "the injected source was never asked at the floor: the test does not exercise the rule"
    assert res["switched"] is True and res["status"] == 0
    assert sum(calls) == 1                                              # once: the FP64 source serves the rest
    assert res["bf16_passes"] == len(calls) and res["factorisations"] == plain["factorisations"] + 1
    assert res["iterations"] == plain["iterations"]
    assert res["evaluations"] == plain["evaluations"] + 2               # the rejected trial and the kept point again
    assert res["fmin"] == plain["fmin"] and np.array_equal(res["g"], plain["g"])      # the FP64 steps, bit for bit
    stuck = log_weights.dual_newton_bioen_log_posterior_base(g0, G, yT, YT, theta, dict(prm, hessian="gram"),
                                                             cov=dict(gram=wrong_at_the_floor))
    assert stuck["status"] == 2 and stuck["switched"] is False


# ---- the series ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SERIES_CASES)
def test_warm_and_cold_series_reach_the_same_optima(case):
    warm, cold = host_series(case, True), host_series(case, False)
    df = max(abs(a["fmin"] - b["fmin"]) for a, b in zip(warm, cold))
    dw = max(np.abs(weights(a["g"]) - weights(b["g"])).max() / weights(b["g"]).max() for a, b in zip(warm, cold))
    print("%s: warm iterations %s evaluations %s; cold iterations %s evaluations %s; max |dfmin| = %.3g, max |dw| = %.3g max w"
          % (case, [r["iterations"] for r in warm], [r["evaluations"] for r in warm], [r["iterations"] for r in cold],
             [r["evaluations"] for r in cold], df, dw))
    assert all(r["status"] == 0 for r in warm + cold)
    assert df <= 1e-6 and dw <= 1e-5
    assert sum(r["evaluations"] for r in warm) <= sum(r["evaluations"] for r in cold)


@pytest.mark.parametrize("case", SERIES_CASES)
def test_warm_series_equals_chained_single_runs(case):
    yT, YT, G, g = series_problem(case)
    for t, got in zip(THETAS, host_series(case, True)):
        one = log_weights.dual_newton_bioen_log_posterior_base(g, G, yT, YT, t, PARAMS)
        assert np.array_equal(got["g"], one["g"]) and got["fmin"] == one["fmin"] and counts(got) == counts(one)
        g = one["g"]


def test_cold_series_equals_single_runs():
    case = SERIES_CASES[0]
    yT, YT, G, g0 = series_problem(case)
    for t, got in zip(THETAS, host_series(case, False)):
        one = log_weights.dual_newton_bioen_log_posterior_base(g0, G, yT, YT, t, PARAMS)
        assert np.array_equal(got["g"], one["g"]) and got["fmin"] == one["fmin"] and counts(got) == counts(one)


def test_series_with_the_bf16_source():
    """the split-BF16 series takes the FP64 series' counts on these problems and reaches its optima"""
    case = SERIES_CASES[0]
    a, b = host_series(case, True, BF16), host_series(case, True)
    assert [counts(r) for r in a] == [counts(r) for r in b] and not any(r["switched"] for r in a)
    assert max(abs(x["fmin"] - y["fmin"]) for x, y in zip(a, b)) <= 1e-6


def test_a_failed_theta_does_not_stop_the_series():
    """max_iterations = 1: every theta ends with status 1 and every theta is run, the next from the kept point"""
    case = SERIES_CASES[0]
    yT, YT, G, g0 = series_problem(case)
    res = log_weights.dual_newton_series_base(g0, G, yT, YT, [10.0, 1.0, 0.1], dict(PARAMS, max_iterations=1))
    assert [r["status"] for r in res] == [1, 1, 1] and [r["iterations"] for r in res] == [1, 1, 1]
    again = log_weights.dual_newton_bioen_log_posterior_base(res[0]["g"], G, yT, YT, 1.0, dict(PARAMS, max_iterations=1))
    assert np.array_equal(again["g"], res[1]["g"])


@pytest.mark.parametrize("thetas", [[], [10.0, 0.0], [10.0, -1.0], [float("nan")], [float("inf")]])
def test_series_refuses_bad_thetas(thetas):
    yT, YT, G, g0 = series_problem(SERIES_CASES[0])
    with pytest.raises(RuntimeError, match="theta"):
        log_weights.dual_newton_series_base(g0, G, yT, YT, thetas, PARAMS)


# ---- parameters and find_optimum_series ------------------------------------------------------------------------------------
def _cfg(mod=""):
    cfg = minimize.Parameters("dual_newton", mod)
    cfg.update(verbose=False, use_c_functions=False)
    return cfg


def test_parameters():
    assert minimize.Parameters("dual_newton")["params"] == dict(gtol=1e-6, max_iterations=200)
    cfg = minimize.Parameters("dual_newton", "dual_newton:hessian=gram_bf16,dual_newton:series=cold")
    assert cfg["params"] == dict(gtol=1e-6, max_iterations=200, hessian="gram_bf16", series="cold")
    assert log_weights._dual_newton_source(cfg["params"]) == "gram_bf16"
    assert log_weights._dual_newton_series_mode(cfg["params"]) is False
    assert log_weights._dual_newton_source({}) == "gram" and log_weights._dual_newton_series_mode({}) is True


def _find_args(d):
    return d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1)


@pytest.mark.parametrize("use_c", [False, True])
def test_bad_parameters_are_refused_before_anything_runs(use_c):
    d = load_golden("synth_logw_M37xN500.npz")
    for mod, needle in (("dual_newton:hessian=fp32", "dual_newton:hessian=fp32 not recognized"),
                        ("dual_newton:series=hot", "dual_newton:series=hot not recognized")):
        cfg = _cfg(mod)
        cfg.update(use_c_functions=use_c)
        with pytest.raises(RuntimeError, match=needle):
            log_weights.find_optimum_series(*_find_args(d), [10.0, 1.0], cfg)
    cfg = _cfg("dual_newton:hessian=fp32")
    cfg.update(use_c_functions=use_c)
    with pytest.raises(RuntimeError, match="dual_newton:hessian=fp32 not recognized"):
        log_weights.find_optimum(*_find_args(d), 10.0, cfg)
    for thetas in ([], [10.0, 0.0]):
        with pytest.raises(RuntimeError, match="theta"):
            log_weights.find_optimum_series(*_find_args(d), thetas, _cfg())


def test_find_optimum_series_refuses_the_other_minimizers():
    d = load_golden("synth_logw_M37xN500.npz")
    for name in ("scipy", "gsl"):
        with pytest.raises(RuntimeError, match="find_optimum_series needs"):
            log_weights.find_optimum_series(*_find_args(d), [10.0, 1.0], minimize.Parameters(name))


@pytest.mark.parametrize("mod", ["", "dual_newton:series=cold", "dual_newton:hessian=gram_bf16"])
def test_find_optimum_series_on_the_numpy_objective(mod):
    """per theta the 5-tuple of find_optimum within the project's gates (cold with the FP64 source: bit for bit)"""
    d = load_golden("synth_logw_M37xN500.npz")
    thetas = [100.0, 10.0, 1.0]
    series = log_weights.find_optimum_series(*_find_args(d), thetas, _cfg(mod))
    assert len(series) == len(thetas)
    for t, got in zip(thetas, series):
        ref = log_weights.find_optimum(*_find_args(d), t, _cfg())
        assert len(got) == 5 and got[0].shape == ref[0].shape and np.shape(got[2]) == np.shape(ref[2])
        assert got[3] == ref[3]
        assert abs(got[4] - ref[4]) <= 1e-6
        assert np.abs(got[0] - ref[0]).max() <= 1e-5 * ref[0].max()
        assert np.abs(got[1] - ref[1]).max() <= 1e-5 * np.abs(ref[1]).max()
        if mod == "dual_newton:series=cold":
            assert got[4] == ref[4] and np.array_equal(got[2], ref[2])


def test_find_optimum_series_raises_for_the_theta_that_fails():
    d = load_golden("synth_logw_M37xN500.npz")
    with pytest.raises(RuntimeError, match=r"theta = 1\.0.*return code 1"):
        log_weights.find_optimum_series(*_find_args(d), [1.0, 0.1], _cfg("dual_newton:max_iterations=1"))


def test_find_optimum_with_the_bf16_source():
    name = "synth_logw_M37xN500.npz"
    d, res = host_dual_newton_bf16(name)
    out = log_weights.find_optimum(*_find_args(d), d["theta"], _cfg("dual_newton:hessian=gram_bf16"))
    assert out[4] == res["fmin"]                                 # the gram_bf16 restatement, bit for bit

"""Hessian-vector products of the log-weights objective on the CPU: the numpy restatement against finite differences of
the reference's own C gradient, and scipy's Newton-CG drivers on the numpy objective through find_optimum."""
import warnings

import numpy as np
import pytest

from conftest import load_golden, require_reference

from bioen_amd.optimize import forces, log_weights, minimize

FD_CASES = ["ref_data_16x15.npz", "synth_logw_M37xN500.npz", "synth_logw_M129xN257.npz"]
TRUST_CASES = FD_CASES + ["ref_data_potra_part_2_logw_M205xN10.npz"]
NEWTON_CASES = FD_CASES


def hessp_case(name):
    """(d, point, directions): GInit plus a seeded 0.3 sigma perturbation; three seeded directions and v = 1"""
    d = load_golden(name)
    n = d["GInit"].size
    rng = np.random.default_rng(4242)
    x = np.asarray(d["GInit"], dtype=np.float64).reshape(-1) + 0.3 * rng.standard_normal(n)
    vs = [rng.standard_normal(n) for _ in range(3)] + [np.ones(n)]
    return d, x, vs


def _hessp(d, x, v):
    return log_weights.hessp_bioen_log_posterior_base(x, v, d["GInit"].copy(), d["G"], d["yTilde"],
                                                      d["YTilde"].reshape(1, -1), d["theta"])


@pytest.mark.parametrize("name", FD_CASES)
def test_numpy_product_against_the_reference_gradient(name):
    """Richardson central difference (h = 1e-3 and h / 2) of the reference's C gradient; gate 1e-6 of the largest |Hv|
    entry of the case (a wrong term is O(1)).  Measured: 3e-13, 2e-11 and 6e-12 S on the three fixtures, more than 1e4 x inside the gate."""
    R = require_reference()
    d, x, vs = hessp_case(name)
    G, yT, YT, theta = d["G"], d["yTilde"], d["YTilde"], float(d["theta"])

    def grad(p):
        return np.asarray(R.logw_df(p, G, yT, YT, theta)).reshape(-1)

    def central(v, h):
        return (grad(x + h * v) - grad(x - h * v)) / (2.0 * h)

    hvs = [_hessp(d, x, v) for v in vs]
    S = max(np.abs(hv).max() for hv in hvs)
    h = 1e-3
    worst = 0.0
    for v, hv in zip(vs, hvs):
        fd = (4.0 * central(v, h / 2) - central(v, h)) / 3.0
        worst = max(worst, np.abs(hv - fd).max())
    print("%s: max |Hv - FD| = %.3g S (S = %.3g)" % (name, worst / S, S))
    assert worst <= 1e-6 * S
    assert worst <= 1e-8 * S                       # the room the gate is meant to have: at least 100 x
    assert np.abs(hvs[3]).max() <= 1e-12 * S       # H 1 = 0: the objective does not change along the constant
    for i in range(3):
        for j in range(i + 1, 3):
            a, b = vs[i].dot(hvs[j]), vs[j].dot(hvs[i])
            assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (a, b)


def test_numpy_product_twin_and_shapes():
    d, x, vs = hessp_case("ref_data_16x15.npz")
    a = _hessp(d, x, vs[0])
    b = log_weights.hessp_bioen_log_posterior(x, vs[0], d["GInit"].copy(), d["G"], d["yTilde"],
                                              d["YTilde"].reshape(1, -1), d["theta"], use_c=False)
    assert a.shape == (x.size,) and np.array_equal(a, b)


def run_driver(name, algorithm, mod, use_c):
    d = load_golden(name)
    cfg = minimize.Parameters("scipy", "scipy:algorithm=%s,%s" % (algorithm, mod))
    cfg.update(verbose=False, use_c_functions=use_c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1),
                                       d["theta"], cfg)
    return d, out


def check_optimum(d, out):
    wopt, yopt, gopt, f0, fmin = out
    n = d["GInit"].size
    assert wopt.shape == (n, 1) and yopt.shape == (d["yTilde"].shape[0],) and np.shape(gopt) == (n,)
    fref = float(d["lbfgs_conv_fmin"])
    wref = np.asarray(d["lbfgs_conv_wopt"]).reshape(-1)
    df, dw = abs(fmin - fref), np.abs(wopt.reshape(-1) - wref).max() / wref.max()
    print("|dfmin| = %.3g, max |dw| = %.3g max w" % (df, dw))
    assert df <= 1e-6
    assert dw <= 1e-5


_HOST_RUNS = {}


def host_run(name, algorithm):
    """the numpy-objective runs, computed once and shared (tests/test_hip_hessp.py compares the device runs with them)"""
    key = (name, algorithm)
    if key not in _HOST_RUNS:
        mod = "scipy:gtol=1e-9" if algorithm == "trust_ncg" else "scipy:xtol=1e-10"
        _HOST_RUNS[key] = run_driver(name, algorithm, mod, False)
    return _HOST_RUNS[key]


@pytest.mark.parametrize("name", TRUST_CASES)
def test_trust_ncg_on_the_numpy_objective(name):
    check_optimum(*host_run(name, "trust_ncg"))


@pytest.mark.parametrize("name", NEWTON_CASES)
def test_newton_cg_on_the_numpy_objective(name):
    check_optimum(*host_run(name, "newton_cg"))


@pytest.mark.parametrize("alias", ["fmin_ncg", "trust-ncg"])
def test_driver_aliases(alias):
    mod = "scipy:gtol=1e-9" if alias == "trust-ncg" else "scipy:xtol=1e-10"
    check_optimum(*run_driver("ref_data_16x15.npz", alias, mod, False))


# The two tests below are guards: they pin behaviour that must NOT change with the Newton drivers (the forces method's and
# the unknown-name errors, the on_device refusal), so unlike the rest of this file they pass without the feature too.
def test_forces_method_rejects_the_newton_names():
    d = load_golden("ref_data_forces_M64xN64.npz")
    for algorithm in ("newton_cg", "trust_ncg"):
        cfg = minimize.Parameters("scipy")
        cfg.update(verbose=False, use_c_functions=False, algorithm=algorithm)
        with pytest.raises(RuntimeError, match="not recognized for scipy/"):
            forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1),
                                d["theta"], cfg)


def test_unknown_name_is_still_rejected_and_on_device_has_no_newton_path():
    d = load_golden("ref_data_16x15.npz")
    args = (d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"])
    cfg = minimize.Parameters("scipy")
    cfg.update(verbose=False, use_c_functions=False, algorithm="newton")
    with pytest.raises(RuntimeError, match="not recognized for scipy/py"):
        log_weights.find_optimum(*args, cfg)
    cfg = minimize.Parameters("scipy", "scipy:algorithm=newton_cg,scipy:on_device=true")
    cfg.update(verbose=False)
    with pytest.raises(RuntimeError, match="has no device path"):
        log_weights.find_optimum(*args, cfg)

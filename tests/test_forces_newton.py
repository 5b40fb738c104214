"""The forces method's own Newton minimizer on the CPU: forces.newton_bioen_log_posterior_base, the numpy restatement that
specifies the device loop, on the driver cases of tests/test_forces_hessp.py from both Hessian
sources; the damping path on an indefinite Hessian; find_optimum with Parameters("newton") on the numpy objective; the
refusals."""
import numpy as np
import pytest

from conftest import load_golden
from test_forces_hessp import DRIVER_CASES, check_optimum

from bioen_amd.optimize import forces, log_weights, minimize

SOURCES = ("gram", "gram_bf16")
_RUNS = {}


def case_args(d):
    return d["w0"], np.asarray(d["yTilde"], dtype=np.float64), d["YTilde"].reshape(1, -1), float(d["theta"])


def host_newton(name, source, gtol=1e-6):
    """the restatement's runs, computed once and shared (tests/test_hip_forces_newton.py compares the device loop with them)"""
    key = (name, source, gtol)
    if key not in _RUNS:
        d = load_golden(name)
        res = forces.newton_bioen_log_posterior_base(d["forces_init"], *case_args(d),
                                                     params=dict(gtol=gtol, max_iterations=200, hessian=source))
        _RUNS[key] = (d, res)
    return _RUNS[key]


def as_tuple(d, res):
    """the restatement's result in find_optimum's shape, for check_optimum"""
    w0, yT, YT, theta = case_args(d)
    w = forces.get_weights_from_forces(w0, yT, res["forces"])
    return w, yT.dot(w).reshape(-1), res["forces"], None, res["fmin"], None, None


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", DRIVER_CASES)
def test_restatement_reaches_the_optimum_on_the_gradient(name, source):
    """status 0 with max|g| <= gtol and the project's gates on fmin and the weights, where the golden's L-BFGS run ended
    without a verdict on the gradient"""
    d, res = host_newton(name, source)
    print("%s %s: %d iterations, %d evaluations, %d Hessians, %d factorisations, lam %.3g, max|g| %.3g"
          % (name, source, res["iterations"], res["evaluations"], res["hessians"], res["factorisations"], res["lam"],
             res["gmax"]))
    assert res["status"] == 0 and res["gmax"] <= 1e-6
    assert res["hessians"] == res["iterations"] + (1 if res["switched"] else 0)
    assert res["factorisations"] >= res["hessians"] and res["iterations"] < res["evaluations"] <= res["factorisations"] + 1
    check_optimum(d, as_tuple(d, res))
    # the golden's converged L-BFGS run, the reference of those gates, ended in an exhausted line search, not on a gradient test
    assert int(d["lbfgs_conv_code"]) == -998


def test_tight_gtol():
    """gtol 1e-9: still status 0 (the rounding floor's rule carries the last steps)"""
    d, res = host_newton("synth_forces_M30xN1000.npz", "gram", 1e-9)
    assert res["status"] == 0 and res["gmax"] <= 1e-9
    check_optimum(d, as_tuple(d, res))


@pytest.mark.parametrize("use_source", SOURCES)
def test_find_optimum_on_the_numpy_objective(use_source):
    d = load_golden("ref_data_forces_M64xN64.npz")
    cfg = minimize.Parameters("newton", "newton:hessian=%s" % use_source)
    assert cfg["minimizer"] == "newton" and cfg["params"] == dict(gtol=1e-6, max_iterations=200, hessian=use_source)
    cfg.update(verbose=False, use_c_functions=False)
    out = forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)
    assert len(out) == 7
    check_optimum(d, out)
    assert out[4] == host_newton("ref_data_forces_M64xN64.npz", use_source)[1]["fmin"]


def test_parameters_defaults():
    cfg = minimize.Parameters("newton")
    assert cfg["params"] == dict(gtol=1e-6, max_iterations=200, hessian="gram")
    assert cfg["use_c_functions"] is True and cfg["algorithm"] == ""


def test_an_indefinite_hessian_takes_the_damping_path():
    """the first Hessian gets a negative diagonal entry: the factorisation reports it (info = index + 1), lambda grows until
    H + lambda I factorises, and the run converges all the same"""
    d = load_golden("synth_forces_M30xN1000.npz")
    calls = []

    def spoiled(x, *args):
        H = forces._hess_gram_base(x, *args).copy()
        if not calls:
            H[3, 3] = -abs(H[3, 3])
            assert forces._newton_cholesky(H, 0.0) == (None, 4)
        calls.append(1)
        return H

    res = forces.newton_bioen_log_posterior_base(d["forces_init"], *case_args(d),
                                                 params=dict(gtol=1e-6, max_iterations=200, hessian="gram"),
                                                 hess={"gram": spoiled})
    plain = host_newton("synth_forces_M30xN1000.npz", "gram")[1]
    print("factorisations %d for %d Hessians (undisturbed: %d for %d)"
          % (res["factorisations"], res["hessians"], plain["factorisations"], plain["hessians"]))
    assert res["status"] == 0 and res["gmax"] <= 1e-6
    assert res["factorisations"] > res["hessians"]
    check_optimum(d, as_tuple(d, res))


def test_cholesky_reports_lapack_info():
    A = np.diag([4.0, 9.0, 16.0])
    A[0, 2] = np.nan                                         # the upper triangle is not read
    L, info = forces._newton_cholesky(A, 0.0)
    assert info == 0 and np.array_equal(L, np.diag([2.0, 3.0, 4.0]))
    assert forces._newton_cholesky(np.diag([4.0, -1.0, 1.0]), 0.0) == (None, 2)
    assert forces._newton_cholesky(np.diag([4.0, -1.0, 1.0]), 1.0) == (None, 2)      # a zero pivot
    assert forces._newton_cholesky(np.diag([4.0, -1.0, 1.0]), 2.0)[1] == 0
    assert forces._newton_cholesky(np.diag([4.0, 1.0, np.nan]), 0.0) == (None, 3)


def test_bad_hessian_source_is_refused():
    d = load_golden("ref_data_forces_M64xN64.npz")
    for use_c in (False, True):                              # refused before anything touches a device
        cfg = minimize.Parameters("newton", "newton:hessian=products")
        cfg.update(verbose=False, use_c_functions=use_c)
        with pytest.raises(RuntimeError, match="newton:hessian=products not recognized .*'gram', 'gram_bf16'"):
            forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)


def test_log_weights_refuses_newton():
    d = load_golden("ref_data_16x15.npz")
    cfg = minimize.Parameters("newton")
    cfg.update(verbose=False, use_c_functions=False)
    with pytest.raises(RuntimeError, match="not recognized"):
        log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)


def test_max_iterations_raises_with_the_return_code():
    d = load_golden("ref_data_forces_M64xN64.npz")
    cfg = minimize.Parameters("newton", "newton:max_iterations=1")
    cfg.update(verbose=False, use_c_functions=False)
    with pytest.raises(RuntimeError, match="return code 1"):
        forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)

"""The dense Hessian and the covariance of the forces objective from two weighted Gram matrices, on the CPU: the numpy
restatement (forces.hessian_gram_bioen_log_posterior_base) against the Hessian built from products, the covariance against
finite differences of the averages, scipy's trust-exact fed by it through find_optimum, and the refusals of the scipy
parameter `hessian`."""
import numpy as np
import pytest

from conftest import FORCES_GOLDEN, load_golden
from test_forces_hessp import DRIVER_CASES, check_optimum, forces_case, run_driver

from bioen_amd.optimize import forces, minimize

SEEDED = [((48, 200), 10.0), ((80, 333), 0.5), ((16, 17), 100.0)]


def seeded_problem(shape, theta):
    """a point away from every optimum: x = yTilde^T f has standard deviation 1, the targets are off the prior's averages"""
    M, N = shape
    rng = np.random.default_rng(100 * M + N)
    yT = rng.normal(rng.normal(0.0, 2.0, (M, 1)), 1.0, (M, N))
    w0 = rng.uniform(0.5, 1.5, N)
    w0 /= w0.sum()
    YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
    f = rng.standard_normal(M)
    f /= yT.T.dot(f).std()
    return f, (w0.reshape(-1, 1), yT, YT.reshape(1, -1), theta)


def check_against_the_products(x, args, label):
    """gate 1e-10 max|H|: the project's gate for the rounding of a Hessian (forces_hessian's asymmetry check); measured
    <= 7e-15"""
    C, H = forces.hessian_gram_bioen_log_posterior_base(x, *args)
    ref = forces.hessian_bioen_log_posterior_base(x, *args)
    m = x.size
    assert C.shape == (m, m) and H.shape == (m, m)
    assert np.array_equal(C, C.T) and np.array_equal(H, H.T)
    S = np.abs(ref).max()
    err = np.abs(H - ref).max()
    print("%s: max |H_gram - H_products| = %.3g max|H|" % (label, err / S))
    assert err <= 1e-10 * S
    return C


@pytest.mark.parametrize("name", FORCES_GOLDEN)
def test_gram_hessian_is_the_hessian_of_the_products_on_the_goldens(name):
    d, args, x, _ = forces_case(name)
    check_against_the_products(x, args, name)


@pytest.mark.parametrize("shape,theta", SEEDED, ids=["%dx%d" % s for s, _ in SEEDED])
def test_gram_hessian_is_the_hessian_of_the_products_away_from_the_optimum(shape, theta):
    x, args = seeded_problem(shape, theta)
    C = check_against_the_products(x, args, "%dx%d theta %g" % (shape + (theta,)))
    assert np.linalg.eigvalsh(C).min() >= -1e-12 * np.abs(C).max()          # a covariance


@pytest.mark.parametrize("name", FORCES_GOLDEN)
def test_covariance_is_the_derivative_of_the_averages(name):
    """C v against a Richardson central difference (h = 1e-3 and h / 2) of ybar = yTilde w(forces) along v, at the points
    and directions of tests/test_forces_hessp.py (a step moves the log-weights by 1e-3) and its gate: 1e-6 of the largest
    |C v| entry of the case"""
    d, args, x, vs = forces_case(name)
    w0, yT, YT, theta = args

    def ybar(p):
        return yT.dot(forces.get_weights_from_forces(w0, yT, p)[:, 0])

    def central(v, h):
        return (ybar(x + h * v) - ybar(x - h * v)) / (2.0 * h)

    C, _ = forces.hessian_gram_bioen_log_posterior_base(x, *args)
    cvs = [C.dot(v) for v in vs]
    S = max(np.abs(cv).max() for cv in cvs)
    h = 1e-3
    worst = 0.0
    for v, cv in zip(vs, cvs):
        fd = (4.0 * central(v, h / 2) - central(v, h)) / 3.0
        worst = max(worst, np.abs(cv - fd).max())
    print("%s: max |C v - FD| = %.3g S (S = %.3g)" % (name, worst / S, S))
    assert worst <= 1e-6 * S


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_trust_exact_with_the_gram_hessian_on_the_numpy_objective(name):
    check_optimum(*run_driver(name, "trust_exact", False, mod="scipy:gtol=1e-6,scipy:hessian=gram"))


def test_the_default_is_the_products():
    cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact")
    assert forces._hessian_source(cfg) == "products"
    cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:hessian=gram")
    assert forces._hessian_source(cfg) == "gram"


@pytest.mark.parametrize("mod,needle", [("scipy:algorithm=fmin_bfgs,scipy:hessian=gram", "trust_exact"),
                                        ("scipy:algorithm=trust_exact,scipy:hessian=dense", "not recognized")],
                         ids=["wrong-algorithm", "unknown-value"])
@pytest.mark.parametrize("use_c", [False, True], ids=["numpy", "device"])
def test_refusals_come_before_anything_is_evaluated(monkeypatch, mod, needle, use_c):
    """RuntimeError before the device (or the numpy objective) is touched: the context cache is never asked"""
    from bioen_amd.optimize.ext import c_bioen

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(c_bioen, "hold", touched)
    monkeypatch.setattr(c_bioen, "_context_for", touched)
    monkeypatch.setattr(forces, "bioen_log_posterior_base", touched)
    d = load_golden("ref_data_forces_M64xN64.npz")
    cfg = minimize.Parameters("scipy", mod)
    cfg.update(verbose=False, use_c_functions=use_c)
    with pytest.raises(RuntimeError, match=needle):
        forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)

"""Second-order information of the forces objective on the CPU: the numpy restatement of the Hessian-vector product against
finite differences of the reference's own C gradient, the dense Hessian, and scipy's trust-exact on the numpy objective
through find_optimum."""
import warnings

import numpy as np
import pytest

from conftest import FORCES_GOLDEN, load_golden, require_reference

from bioen_amd.optimize import forces, log_weights, minimize

DRIVER_CASES = ["ref_data_forces_M64xN64.npz", "synth_forces_M30xN1000.npz", "synth_forces_M96xN3000.npz"]


def forces_case(name):
    """(d, args, point, directions): forces_init plus a seeded perturbation, three seeded directions and a unit vector.
    The point and the directions are scaled by the problem: the perturbation moves the log-weights by at most 0.3, a
    direction's dx = yTilde^T v has largest entry 1 -- so the finite-difference step h = 1e-3 moves the log-weights by
    1e-3 whatever M, N and the magnitude of yTilde, and the Richardson error, O(h^4) in that quantity, stays at 1e-12."""
    d = load_golden(name)
    yT = np.asarray(d["yTilde"], dtype=np.float64)
    m = yT.shape[0]
    args = (d["w0"], yT, d["YTilde"].reshape(1, -1), float(d["theta"]))
    rng = np.random.default_rng(4242)

    def unit_dx(v):
        return v / np.abs(yT.T.dot(v)).max()

    x = np.asarray(d["forces_init"], dtype=np.float64).reshape(-1) + 0.3 * unit_dx(rng.standard_normal(m))
    vs = [unit_dx(rng.standard_normal(m)) for _ in range(3)]
    e = np.zeros(m)
    e[m // 3] = 1.0
    vs.append(unit_dx(e))
    return d, args, x, vs


def test_the_four_forces_goldens_are_there():
    assert len(FORCES_GOLDEN) == 4 and set(DRIVER_CASES) <= set(FORCES_GOLDEN)


@pytest.mark.parametrize("name", FORCES_GOLDEN)
def test_numpy_product_against_the_reference_gradient(name):
    """Richardson central difference (h = 1e-3 and h / 2) of the reference's C gradient; gate 1e-6 of the largest |Hv|
    entry of the case (a wrong term is O(1)), as tests/test_hessp.py holds the log-weights restatement to."""
    R = require_reference()
    d, args, x, vs = forces_case(name)
    w0, yT, YT, theta = args

    def grad(p):
        return np.asarray(R.forces_df(p, w0, yT, YT, theta)).reshape(-1)

    def central(v, h):
        return (grad(x + h * v) - grad(x - h * v)) / (2.0 * h)

    hvs = [forces.hessp_bioen_log_posterior_base(x, v, *args) for v in vs]
    S = max(np.abs(hv).max() for hv in hvs)
    h = 1e-3
    worst = 0.0
    for v, hv in zip(vs, hvs):
        assert hv.shape == x.shape
        fd = (4.0 * central(v, h / 2) - central(v, h)) / 3.0
        worst = max(worst, np.abs(hv - fd).max())
    print("%s: max |Hv - FD| = %.3g S (S = %.3g)" % (name, worst / S, S))
    assert worst <= 1e-6 * S
    for i in range(4):                      # H is symmetric
        for j in range(i + 1, 4):
            a, b = vs[i].dot(hvs[j]), vs[j].dot(hvs[i])
            assert abs(a - b) <= 1e-10 * S * np.abs(vs[i]).sum(), (a, b)


@pytest.mark.parametrize("name", FORCES_GOLDEN)
def test_dense_hessian_is_the_stacked_products(name):
    """hessian_..._base against the products with the unit directions one by one (gemm against gemv: the order of the
    sums differs, 1e-13 of the largest entry covers it); symmetric to 1e-12 of the largest entry BEFORE it is symmetrised"""
    d, args, x, _ = forces_case(name)
    m = x.size
    H = forces.hessian_bioen_log_posterior_base(x, *args)
    assert H.shape == (m, m)
    S = np.abs(H).max()
    rows = range(m) if m <= 100 else range(0, m, 53)
    raw = np.array([forces.hessp_bioen_log_posterior_base(x, np.eye(m)[i], *args) for i in rows])
    assert np.abs(raw - H[list(rows)]).max() <= 1e-12 * S
    unsym = forces._hessp_base(x, np.eye(m), *args)
    print("%s: asymmetry of the stacked products %.3g max|H|" % (name, np.abs(unsym - unsym.T).max() / S))
    assert np.abs(unsym - unsym.T).max() <= 1e-12 * S
    assert np.array_equal(H, H.T)
    v = np.random.default_rng(5).standard_normal(m)
    hv = forces.hessp_bioen_log_posterior_base(x, v, *args)
    assert np.abs(H.dot(v) - hv).max() <= 1e-12 * S * np.abs(v).sum()


def test_numpy_twins_and_shapes():
    d, args, x, vs = forces_case("ref_data_forces_M64xN64.npz")
    w0, yT, YT, theta = args
    a = forces.hessp_bioen_log_posterior_base(x, vs[0], *args)
    b = forces.hessp_bioen_log_posterior(x, vs[0], w0, d["y"], yT, YT, theta, use_c=False)
    assert a.shape == (x.size,) and np.array_equal(a, b)
    b2 = forces.hessp_bioen_log_posterior(x.reshape(-1, 1), vs[0].reshape(-1, 1), w0, d["y"], yT, YT, theta, use_c=False)
    assert np.array_equal(a, b2)
    H = forces.hessian_bioen_log_posterior(x, w0, d["y"], yT, YT, theta, use_c=False)
    assert np.array_equal(H, forces.hessian_bioen_log_posterior_base(x, *args))


def run_driver(name, algorithm, use_c, mod="scipy:gtol=1e-6"):
    d = load_golden(name)
    cfg = minimize.Parameters("scipy", "scipy:algorithm=%s,%s" % (algorithm, mod))
    cfg.update(verbose=False, use_c_functions=use_c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1),
                                  d["theta"], cfg)
    return d, out


def check_optimum(d, out):
    wopt, yopt, fopt, f0, fmin, chi2, S = out
    m, n = d["yTilde"].shape
    assert wopt.shape == (n, 1) and yopt.shape == (m,) and np.shape(fopt) == (m,)
    fref = float(d["lbfgs_conv_fmin"])
    wref = np.asarray(d["lbfgs_conv_wopt"]).reshape(-1)
    df, dw = abs(fmin - fref), np.abs(wopt.reshape(-1) - wref).max() / wref.max()
    print("|dfmin| = %.3g, max |dw| = %.3g max w" % (df, dw))
    assert df <= 1e-6
    assert dw <= 1e-5


_HOST_RUNS = {}


def host_run(name):
    """the numpy-objective runs, computed once and shared (tests/test_hip_forces_hessp.py compares the device runs with them)"""
    if name not in _HOST_RUNS:
        _HOST_RUNS[name] = run_driver(name, "trust_exact", False)
    return _HOST_RUNS[name]


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_trust_exact_on_the_numpy_objective(name):
    check_optimum(*host_run(name))


def test_the_alias_works():
    check_optimum(*run_driver("ref_data_forces_M64xN64.npz", "trust-exact", False))


def test_log_weights_still_rejects_trust_exact():
    d = load_golden("ref_data_16x15.npz")
    for algorithm in ("trust_exact", "trust-exact"):
        cfg = minimize.Parameters("scipy")
        cfg.update(verbose=False, use_c_functions=False, algorithm=algorithm)
        with pytest.raises(RuntimeError, match="not recognized for scipy/py"):
            log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)


def test_on_device_stays_refused_for_forces():
    d = load_golden("ref_data_forces_M64xN64.npz")
    cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:on_device=true")
    cfg.update(verbose=False)
    with pytest.raises(RuntimeError, match="on_device"):
        forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)

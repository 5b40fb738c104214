"""CPU tests of bioen_amd.bfgs -- scipy's fmin_bfgs loop restated on scipy's own scalar line searches over a vector
backend: on NumpyBackend it must equal scipy.optimize.fmin_bfgs(full_output=True) bit for bit; the lazy rank-2 form
of the update the device uses must follow scipy's triple product; and the public opt-in refuses what it cannot serve."""
import warnings

import numpy as np
import pytest
import scipy.optimize as sopt

from conftest import load_golden


def _same(a, b):
    names = ("xopt", "fopt", "gopt", "Bopt", "func_calls", "grad_calls", "warnflag")
    for name, u, v in zip(names, a, b):
        u, v = np.asarray(u), np.asarray(v)
        assert u.shape == v.shape and np.array_equal(u, v), name


def _both(f, x0, fprime, args=(), **kw):
    from bioen_amd import bfgs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = sopt.fmin_bfgs(f, x0, fprime, args=args, full_output=True, disp=False, **kw)
        got = bfgs.fmin_bfgs_numpy(f, x0, fprime, args=args, **kw)
    return ref, got


def _seeded_logw(m=20, n=300, seed=3, theta=10.0):
    from bioen_amd.optimize import log_weights as lw
    rng = np.random.default_rng(seed)
    yT, YT = rng.normal(size=(m, n)), rng.normal(size=m)
    G = lw.getGs(np.full((n, 1), 1.0 / n))
    return np.asarray(G[:].T)[0], (G.copy(), G, yT, YT, theta)


@pytest.mark.parametrize("n", [2, 10, 50])
def test_rosenbrock_bit_for_bit(n):
    x0 = np.full(n, -1.2)
    x0[1::2] = 1.0
    ref, got = _both(sopt.rosen, x0, sopt.rosen_der)
    _same(ref, got)
    assert ref[6] == 0


@pytest.mark.parametrize("name", ["ref_data_deer_test_logw_M808xN10.npz", "synth_logw_M37xN500.npz"])
@pytest.mark.parametrize("gtol", [1e-3, 1e-8])
def test_logw_objective_bit_for_bit(name, gtol):
    from bioen_amd.optimize import log_weights as lw
    d = load_golden(name)
    x0 = np.asarray(d["GInit"], dtype=np.float64).reshape(-1)
    args = (d["GInit"].copy(), d["G"], d["yTilde"], d["YTilde"].reshape(1, -1), float(d["theta"]))
    ref, got = _both(lw.bioen_log_posterior_base, x0, lw.grad_bioen_log_posterior_base, args=args, gtol=gtol,
                     maxiter=5000)
    _same(ref, got)


def test_precision_loss_end_and_wolfe2_fallback(monkeypatch):
    """gtol 1e-12 on a seeded problem: one wolfe1 failure taken over by wolfe2, then warnflag 2; counts differ (f / g)"""
    import scipy.optimize._linesearch as ls
    from bioen_amd.optimize import log_weights as lw
    calls = []
    orig = ls.scalar_search_wolfe2

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    x0, args = _seeded_logw()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = sopt.fmin_bfgs(lw.bioen_log_posterior_base, x0, lw.grad_bioen_log_posterior_base,
                             args=(args[0].copy(),) + args[1:], gtol=1e-12, maxiter=5000, full_output=True, disp=False)
        monkeypatch.setattr(ls, "scalar_search_wolfe2", counted)
        from bioen_amd import bfgs
        got = bfgs.fmin_bfgs_numpy(lw.bioen_log_posterior_base, x0, lw.grad_bioen_log_posterior_base,
                                   args=(args[0].copy(),) + args[1:], gtol=1e-12, maxiter=5000)
    _same(ref, got)
    assert got[6] == 2
    assert len(calls) >= 1, "the wolfe2 fallback did not run"
    assert got[4] != got[5]


def test_maxiter_end():
    x0 = np.full(10, -1.2)
    ref, got = _both(sopt.rosen, x0, sopt.rosen_der, maxiter=7)
    _same(ref, got)
    assert got[6] == 1


def test_norm_two_bit_for_bit_and_bad_norm_refused():
    x0 = np.full(10, -1.2)
    ref, got = _both(sopt.rosen, x0, sopt.rosen_der, norm=2)
    _same(ref, got)
    from bioen_amd import bfgs
    with pytest.raises(ValueError):
        bfgs.fmin_bfgs_numpy(sopt.rosen, x0, sopt.rosen_der, norm=1)


def test_missing_scalar_searches_fail_at_call_time(monkeypatch):
    import builtins
    from bioen_amd import bfgs              # importing the package never needs them
    real = builtins.__import__

    def refuse(name, *a, **k):
        if name == "scipy.optimize._linesearch":
            raise ImportError("no scalar searches")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", refuse)
    with pytest.raises(RuntimeError, match="scalar line searches"):
        bfgs.fmin_bfgs_numpy(sopt.rosen, np.zeros(3), sopt.rosen_der)


def test_lazy_rank2_update_and_direction_identity_follow_the_triple_product():
    """The device's algebra in float64: H' = H - rho (s u^T + u s^T) + (rho^2 y.u + rho) s s^T with u = H y, and
    H' g = H g - rho s (u.g) - rho u (s.g) + c s (s.g), against scipy's triple product over 20 recorded steps."""
    from bioen_amd import bfgs
    from bioen_amd.optimize import log_weights as lw
    x0, args = _seeded_logw()
    b = bfgs.NumpyBackend(lw.bioen_log_posterior_base, lw.grad_bioen_log_posterior_base, x0, args)
    pairs = []
    orig_update = b.update

    def recording_update():
        pairs.append((b.sk.copy(), b.yk.copy(), b.gfk.copy()))
        return orig_update()
    b.update = recording_update
    bfgs.minimize(b, b.n, gtol=1e-8, maxiter=21)
    assert len(pairs) >= 20
    n = x0.size
    I = np.eye(n)
    Ht, Hl = I.copy(), I.copy()
    for s, y, g in pairs[:20]:
        ys = y.dot(s)
        rho = 1000.0 if ys == 0.0 else 1.0 / ys
        u = Hl.dot(y)
        c = rho * rho * y.dot(u) + rho
        hg = Hl.dot(g)
        direction = hg - rho * s * u.dot(g) - rho * u * s.dot(g) + c * s * s.dot(g)
        Hl = Hl - rho * (np.outer(s, u) + np.outer(u, s)) + c * np.outer(s, s)
        A1 = I - s[:, None] * y[None, :] * rho
        A2 = I - y[:, None] * s[None, :] * rho
        Ht = A1.dot(Ht.dot(A2)) + rho * s[:, None] * s[None, :]
        scale = np.abs(Ht).max()
        assert np.abs(Hl - Ht).max() <= 1e-12 * scale
        assert np.array_equal(Hl, Hl.T)
        ref = Ht.dot(g)
        assert np.abs(direction - ref).max() <= 1e-12 * scale * np.abs(g).sum()


# ---- the public opt-in (refusals raise before anything touches the device) -------------------------------------------
def _cfg(mod, **over):
    from bioen_amd.optimize import minimize
    cfg = minimize.Parameters("scipy", mod)
    cfg["verbose"] = False
    cfg.update(over)
    return cfg


def test_on_device_flag_reaches_the_parameters():
    assert _cfg("scipy:on_device=true")["params"]["on_device"] is True
    assert "on_device" not in _cfg("")["params"]


@pytest.mark.parametrize("algorithm", ["cg", "lbfgs", "fmin_cg", "fmin_l_bfgs_b"])
def test_on_device_refuses_other_scipy_algorithms(algorithm):
    from bioen_amd.optimize import log_weights
    d = load_golden("ref_data_16x15.npz")
    cfg = _cfg("scipy:on_device=true", algorithm=algorithm)
    with pytest.raises(RuntimeError, match="on_device"):
        log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)


def test_on_device_refuses_the_numpy_objective():
    from bioen_amd.optimize import log_weights
    d = load_golden("ref_data_16x15.npz")
    cfg = _cfg("scipy:on_device=true", use_c_functions=False)
    with pytest.raises(RuntimeError, match="use_c_functions"):
        log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)


def test_on_device_refuses_the_forces_method():
    from bioen_amd.optimize import forces
    d = load_golden("ref_data_deer_test_forces_M808xN10.npz")
    cfg = _cfg("scipy:on_device=true")
    with pytest.raises(RuntimeError, match="log-weights"):
        forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)

"""GPU tests of the dense inverse-Hessian BFGS (scipy's fmin_bfgs with H in HBM: bioen_amd/bfgs.py,
csrc/kernels_bfgs.hip, csrc/api_bfgs.cpp): H against a host recurrence on the device's own steps, the HBM regime,
parity with today's host fmin_bfgs on the device objective and with the reference's converged optimum, determinism,
footprint and limits, and the public API's opt-in."""
import warnings

import numpy as np
import pytest
import scipy.optimize as sopt

from conftest import LOGW_GOLDEN, load_golden

pytestmark = pytest.mark.gpu

REF_LOGW = [n for n in LOGW_GOLDEN if n.startswith("ref_") and "potra_part_1" not in n]   # as test_hip_api.py:67
SEEDED = ["synth_logw_M37xN500.npz", "synth_logw_M64xN2000.npz"]


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()


def _problem(m, n, seed):
    rng = np.random.default_rng(seed)
    yT = rng.normal(size=(m, n))
    YT = rng.normal(size=m)
    G = np.zeros(n)
    g0 = 0.1 * rng.standard_normal(n)
    return yT, YT, G, g0


class HostRecurrence(object):
    """H_k = I + sum_t [-rho_t (s_t u_t^T + u_t s_t^T) + c_t s_t s_t^T], u_t = H_t y_t, in float64 on the host -- kept
    as its factors, so that any block of rows can be formed without the N x N matrix."""

    def __init__(self, n):
        self.n = n
        self.terms = []

    def matvec(self, v):
        out = v.copy()
        for s, u, rho, c in self.terms:
            out += -rho * (s * u.dot(v) + u * s.dot(v)) + c * s * s.dot(v)
        return out

    def push(self, s, y):
        u = self.matvec(y)
        ys = y.dot(s)
        rho = 1000.0 if ys == 0.0 else 1.0 / ys
        self.terms.append((s, u, rho, rho * rho * y.dot(u) + rho))

    def rows(self, r0, r1):
        H = np.zeros((r1 - r0, self.n))
        H[np.arange(r1 - r0), np.arange(r0, r1)] = 1.0
        for s, u, rho, c in self.terms:
            H += -rho * (np.outer(s[r0:r1], u) + np.outer(u[r0:r1], s)) + c * np.outer(s[r0:r1], s)
        return H


def _steps(ctx, G, g0, theta, k, alpha=0.5):
    """k accepted steps of length alpha along the session's directions; -> the host recurrence on the device's s, y"""
    ctx.bfgs_begin(g0, G, theta, True)
    host = HostRecurrence(ctx.n)
    for _ in range(k):
        ctx.bfgs_trial(alpha, True)
        ctx.bfgs_accept(alpha, True)
        host.push(ctx.bfgs_read_vec("s"), ctx.bfgs_read_vec("y"))
        ctx.bfgs_update()
    return host


@pytest.mark.parametrize("n", [1000, 1537, 4096])
def test_inverse_hessian_matches_host_recurrence(bioen_amd, n):
    yT, YT, G, g0 = _problem(24, n, seed=n)
    with bioen_amd.Context(yT, YT) as ctx:
        for k in (1, 3, 5):
            host = _steps(ctx, G, g0, 2.0, k)
            Hd = ctx.bfgs_read_hinv()
            Hh = host.rows(0, n)
            scale = np.abs(Hh).max()
            assert np.abs(Hd - Hh).max() <= 1e-12 * scale, (k, np.abs(Hd - Hh).max(), scale)
            assert np.array_equal(Hd, Hd.T), "H must stay exactly symmetric"
            Hp = ctx.bfgs_read_hinv(padded=True)
            assert Hp.shape == ((n + 15) // 16 * 16,) * 2
            assert np.array_equal(Hp[:n, :n], Hd)
            assert not Hp[n:, :].any() and not Hp[:, n:].any(), "pad rows / columns must be zero"
            g, p = ctx.bfgs_read_vec("g"), ctx.bfgs_read_vec("p")
            ref = -Hh.dot(g)
            assert np.abs(p - ref).max() <= 1e-12 * np.abs(ref).max()
            ctx.bfgs_end()


def test_large_inverse_hessian_hbm_regime(bioen_amd):
    """N = 12000: H is 1.15 GB, past the 256 MiB Infinity Cache; read back in row blocks."""
    n = 12000
    yT, YT, G, g0 = _problem(64, n, seed=12000)
    with bioen_amd.Context(yT, YT) as ctx:
        host = _steps(ctx, G, g0, 2.0, 5)
        _, hb = ctx.footprint()
        blk = 1500
        H = np.empty((n, n))
        worst, scale = 0.0, 0.0
        for r0 in range(0, n, blk):
            H[r0:r0 + blk] = ctx.bfgs_read_hinv(r0, blk)
            Hh = host.rows(r0, r0 + blk)
            worst = max(worst, np.abs(H[r0:r0 + blk] - Hh).max())
            scale = max(scale, np.abs(Hh).max())
        ctx.bfgs_end()
    assert worst <= 1e-12 * scale, (worst, scale)
    for r0 in range(0, n, blk):
        assert np.array_equal(H[r0:r0 + blk], H[:, r0:r0 + blk].T), "H must stay exactly symmetric"


def _host_bfgs(ctx, x0, G, theta, gtol, maxiter=5000):
    """today's path: host scipy.optimize.fmin_bfgs on the device objective (log_weights._DeviceFdf's shape)"""
    cache = {}

    def ev(x):
        if cache.get("x") is None or not np.array_equal(cache["x"], x):
            cache["f"], cache["g"] = ctx.logw_fdf(x, G, theta)
            cache["x"] = x.copy()

    def f(x):
        ev(x)
        return cache["f"]

    def fp(x):
        ev(x)
        return cache["g"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return sopt.fmin_bfgs(f, x0, fp, gtol=gtol, maxiter=maxiter, full_output=True, disp=False)


@pytest.mark.parametrize("name", REF_LOGW + SEEDED)
def test_parity_with_host_fmin_bfgs(bioen_amd, name):
    d = load_golden(name)
    x0 = np.asarray(d["GInit"], dtype=np.float64).reshape(-1)
    G = np.asarray(d["G"], dtype=np.float64).reshape(-1)
    theta = float(d["theta"])
    with bioen_amd.Context(d["yTilde"], d["YTilde"]) as ctx:
        xh, fh, _, _, nfh, ngh, wfh = _host_bfgs(ctx, x0, G, theta, 1e-3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g, w, info = ctx.bfgs_logw(x0, G, theta, gtol=1e-3, maxiter=5000)
    print("%s yaml gtol: host %d/%d calls warnflag %d, device %d/%d calls warnflag %d, %d iterations"
          % (name, nfh, ngh, wfh, info.func_calls, info.grad_calls, info.warnflag, info.iterations))
    assert info.warnflag == wfh
    assert abs(info.fmin - fh) <= 1e-6 * abs(fh), (info.fmin, fh)
    assert info.fmin <= float(d["f_init"])
    if "ref_fmin_scipy_bfgs" in d:
        ref = float(d["ref_fmin_scipy_bfgs"])
        assert abs(info.fmin - ref) / abs(ref) < 1e-1
    assert abs(w.sum() - 1.0) < 1e-12


# scipy's BFGS itself (host, numpy objective) stops at gtol 1e-10 on a saturated point of the potra_part_2 fixtures (weights
# of 1e-23, where every gradient component w_k (...) is below gtol) rather than at the reference's converged optimum; on
# those the device path is held to host scipy's own converged result instead
SATURATING = {"ref_data_potra_part_2_logw_M205xN10.npz", "ref_data_potra_part_2_logw_M808xN10.npz"}


@pytest.mark.parametrize("name", REF_LOGW + SEEDED)
def test_converged_optimum_matches_reference(bioen_amd, name):
    d = load_golden(name)
    x0 = np.asarray(d["GInit"], dtype=np.float64).reshape(-1)
    G = np.asarray(d["G"], dtype=np.float64).reshape(-1)
    theta = float(d["theta"])
    with bioen_amd.Context(d["yTilde"], d["YTilde"]) as ctx:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g, w, info = ctx.bfgs_logw(x0, G, theta, gtol=1e-10, maxiter=200000)
        # host scipy's counts are recorded, not asserted; its O(N^3) update per iteration is only paid where it is cheap
        # (N <= 500) or where it is the yardstick (SATURATING)
        host = name in SATURATING or ctx.n <= 500
        if host:
            xh, fh, _, _, nfh, ngh, wfh = _host_bfgs(ctx, x0, G, theta, 1e-10, maxiter=200000)
    print("%s gtol 1e-10: device %d iterations %d/%d calls warnflag %d; %s"
          % (name, info.iterations, info.func_calls, info.grad_calls, info.warnflag,
             "host scipy %d/%d calls warnflag %d" % (nfh, ngh, wfh) if host else "host scipy not run (N > 500)"))
    assert info.warnflag in (0, 2)
    if name in SATURATING:
        assert info.warnflag == wfh
        assert abs(info.fmin - fh) <= 1e-6 * abs(fh), (info.fmin, fh)
        return
    fref = float(d["lbfgs_conv_fmin"])
    wref = np.asarray(d["lbfgs_conv_wopt"]).reshape(-1)
    assert abs(info.fmin - fref) <= 1e-6 * abs(fref), (info.fmin, fref)
    assert np.abs(w - wref).max() <= 1e-5 * wref.max()


def test_two_runs_are_bitwise_identical(bioen_amd):
    d = load_golden("synth_logw_M64xN2000.npz")
    x0 = np.asarray(d["GInit"], dtype=np.float64).reshape(-1)
    G = np.asarray(d["G"], dtype=np.float64).reshape(-1)
    with bioen_amd.Context(d["yTilde"], d["YTilde"]) as ctx:
        a = ctx.bfgs_logw(x0, G, float(d["theta"]), gtol=1e-6)
        b = ctx.bfgs_logw(x0, G, float(d["theta"]), gtol=1e-6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2].fmin == b[2].fmin
    assert (a[2].func_calls, a[2].grad_calls, a[2].iterations) == (b[2].func_calls, b[2].grad_calls, b[2].iterations)


def test_footprint_returns_after_run_and_error(bioen_amd):
    from bioen_amd._lib import BioenHipError
    yT, YT, G, g0 = _problem(16, 3000, seed=5)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.logw_fdf(g0, G, 1.0)                 # the matrix takes its evaluation form first
        start = ctx.footprint()
        ctx.bfgs_begin(g0, G, 1.0, True)
        forms, b = ctx.footprint()
        assert "bfgs_hinv" in forms and b == start[1] + 3008 * 3008 * 8
        ctx.bfgs_end()
        assert ctx.footprint() == start
        ctx.bfgs_logw(g0, G, 1.0, gtol=1e-4)
        assert ctx.footprint() == start
        ctx.bfgs_begin(g0, G, 1.0, True)
        with pytest.raises(BioenHipError):
            ctx.bfgs_accept(0.5)                 # no gradient at that step: an error ends the session
        assert ctx.footprint() == start


def test_too_large_inverse_hessian_is_refused_before_allocation(bioen_amd):
    from bioen_amd._lib import BioenHipError
    yT, YT, G, g0 = _problem(16, 200000, seed=7)
    with bioen_amd.Context(yT, YT) as ctx:
        start = ctx.footprint()
        with pytest.raises(BioenHipError) as e:
            ctx.bfgs_logw(g0, G, 1.0)
        assert "(-4)" in str(e.value) and "N x N" in str(e.value)
        assert ctx.footprint() == start
        f, _ = ctx.logw_fdf(g0, G, 1.0)          # the context is still usable
        assert np.isfinite(f)


def test_interrupted_session_returns_estate(bioen_amd):
    from bioen_amd._lib import BioenHipError
    yT, YT, G, g0 = _problem(16, 1000, seed=9)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.logw_fdf(g0, G, 1.0)                 # the matrix takes its evaluation form first
        start = ctx.footprint()
        ctx.bfgs_begin(g0, G, 1.0, True)
        ctx.bfgs_trial(0.5, True)
        ctx.logw_fdf(g0, G, 1.0)                 # another call on the context ends the session
        assert ctx.footprint() == start
        with pytest.raises(BioenHipError) as e:
            ctx.bfgs_trial(0.5, True)
        assert "(-6)" in str(e.value) and "ended by another call" in str(e.value)
        ctx.bfgs_logw(g0, G, 1.0, gtol=1e-4)     # a new session starts cleanly


def test_find_optimum_on_device_returns_host_shapes(bioen_amd):
    from bioen_amd import optimize
    d = load_golden("ref_data_deer_test_logw_M808xN10.npz")
    YT = d["YTilde"].reshape(1, -1)
    out = {}
    for mod in ("", "scipy:on_device=true"):
        params = optimize.minimize.Parameters("scipy", mod)
        params["verbose"] = False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[mod] = optimize.log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], YT, d["theta"], params)
    host, dev = out[""], out["scipy:on_device=true"]
    assert [np.shape(a) for a in host] == [np.shape(a) for a in dev]
    assert host[3] == dev[3]
    assert abs(dev[4] - host[4]) <= 1e-6 * abs(host[4])
    assert abs(dev[0].sum() - 1.0) < 1e-12

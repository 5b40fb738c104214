"""GPU tests of the forces method's device-resident Newton minimizer (csrc/kernels_forces_newton.hip,
csrc/api_forces_newton.cpp, Context.forces_newton_factor / forces_newton_solve / opt_newton_forces):
the Cholesky factorisation and the solves against LAPACK on caller matrices, pivot failures as ordinary results, the
bitwise invariants, the state rules and refusals, and the loop through find_optimum against its numpy restatement."""
import numpy as np
import pytest
import scipy.linalg

from conftest import load_golden
from test_forces_hessp import DRIVER_CASES, check_optimum, run_driver
from test_forces_newton import as_tuple, host_newton
from test_hip_forces_hessp import estate, problem
from test_hip_strip_loops import data as loop_data, enter_regime, on_thread_ranks

from bioen_amd.optimize import forces, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# |L L^T - A|_max <= GATE m eps |A|_max, |L - L_lapack|_max <= GATE m eps |A|_max cond(A), |A X - B|_max <= GATE m eps |A|_max
# |X|_max.  GATE is 8 x the worst ratio measured on the MI355X over FACTOR_M (the two orders of summation differ by rounding
# only; capped at 64) -- the ratios measured are in MEASURED below and in DESIGN 6h
GATE = 8 * 0.535
MEASURED = dict(LLt=(0.535, 0.145, 0.0383, 0.0628, 0.0195, 0.00625, 0.00564, 0.00362),      # by FACTOR_M; the worst: M = 1
                L_lapack=(0.0, 0.00965, 0.004, 0.00383, 0.00133, 0.000545, 0.000343, 0.000274),
                solve={65: 0.0335, 513: 0.00976, 1024: 0.00797})
# one element; under one tile; exactly one panel; one row past a panel; a ragged last panel; many panels; the padded shape
# of the offset golden; every tile full
FACTOR_M = (1, 7, 64, 65, 129, 513, 808, 1024)
N_SMALL = 40           # the contexts' N: M is what matters here


def spd(m, seed=None):
    """A = B B^T / m + I, cond <= 10"""
    B = np.random.default_rng(1000 + m if seed is None else seed).standard_normal((m, m))
    A = B.dot(B.T) / m + np.eye(m)
    return 0.5 * (A + A.T)


_CTX = {}


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()
    c_bioen.clear_cache()


def small_problem(m):
    rng = np.random.default_rng(m)
    return rng.standard_normal((m, N_SMALL)) + 3.0, rng.standard_normal(m) + 3.0


def context(bioen_amd, m):
    """one context per M for the tests on caller matrices (the matrix of the context plays no part in them)"""
    if m not in _CTX:
        yT, YT = small_problem(m)
        _CTX[m] = bioen_amd.Context(yT, YT)
    return _CTX[m]


@pytest.mark.parametrize("m", FACTOR_M)
def test_factorisation_against_lapack(bioen_amd, m):
    ctx = context(bioen_amd, m)
    A = spd(m)
    cond = np.linalg.cond(A)
    assert cond <= 10.0
    L, info = ctx.forces_newton_factor(A)
    assert info == 0 and L.shape == (m, m)
    assert not np.triu(L, 1).any()
    scale = m * EPS * np.abs(A).max()
    r1 = np.abs(L.dot(L.T) - A).max() / scale
    r2 = np.abs(L - np.linalg.cholesky(A)).max() / (scale * cond)
    print("M = %d: |L L^T - A| = %.3g m eps |A|, |L - L_lapack| = %.3g m eps |A| cond (cond %.2f)" % (m, r1, r2, cond))
    assert r1 <= GATE and r2 <= GATE
    L5, info = ctx.forces_newton_factor(A, lam=0.5)
    A5 = A + 0.5 * np.eye(m)
    assert info == 0 and np.abs(L5.dot(L5.T) - A5).max() <= GATE * m * EPS * np.abs(A5).max()
    assert np.abs(L5 - np.linalg.cholesky(A5)).max() <= GATE * m * EPS * np.abs(A5).max() * np.linalg.cond(A5)
    An = A.copy()                                            # the upper triangle is not read
    An[np.triu_indices(m, 1)] = np.nan
    Ln, info = ctx.forces_newton_factor(An)
    assert info == 0 and np.array_equal(Ln, L)
    again, _ = ctx.forces_newton_factor(A)                   # the same bits in, the same bits out
    assert np.array_equal(again, L)


@pytest.mark.parametrize("m", (129, 1024))
def test_a_pivot_that_is_not_positive_is_an_ordinary_result(bioen_amd, m):
    ctx = context(bioen_amd, m)
    A = spd(m)
    with bioen_amd.Context(*small_problem(m)) as fresh:
        L_fresh, info = fresh.forces_newton_factor(A)
        assert info == 0
    b = np.random.default_rng(m).standard_normal(m)
    for k, value in [(0, -1.0), (63, -1.0), (64, -1.0), (m - 1, -1.0), (64, np.nan), (m - 1, np.nan), (0, np.inf)]:
        bad = A.copy()
        bad[k, k] = value
        L, info = ctx.forces_newton_factor(bad)
        assert L is None and info == k + 1, (k, value, info)
        estate(lambda: ctx.forces_newton_solve(b), "bioen_hip_forces_newton_solve", "info = %d" % (k + 1))
        L, info = ctx.forces_newton_factor(A)                # the next valid one: a fresh context's bits
        assert info == 0 and np.array_equal(L, L_fresh)
        assert np.isfinite(ctx.forces_newton_solve(b)).all()
    zero = A.copy()                                          # a pivot that cancels to exactly zero
    zero[0, 0] = 0.0
    assert ctx.forces_newton_factor(zero) == (None, 1)
    ctx.forces_newton_factor(A, want_L=False)


@pytest.mark.parametrize("m", (65, 513, 1024))
def test_solve(bioen_amd, m):
    ctx = context(bioen_amd, m)
    A = spd(m)
    _, info = ctx.forces_newton_factor(A, want_L=False)
    assert info == 0
    B = np.random.default_rng(7 * m).standard_normal((8, m))
    X8 = ctx.forces_newton_solve(B)
    for k in (1, 3, 8):
        X = ctx.forces_newton_solve(B[:k] if k > 1 else B[0])
        assert X.shape == ((k, m) if k > 1 else (m,))
        assert np.array_equal(X, X8[:k] if k > 1 else X8[0])          # a column of a batch is the single solve, bit for bit
    bound = GATE * m * EPS * np.abs(A).max() * np.abs(X8).max()
    r = np.abs(X8.dot(A) - B).max()
    print("M = %d: |A X - B| = %.3g m eps |A| |X|" % (m, r / (bound / GATE)))
    assert r <= bound
    want = scipy.linalg.cho_solve((np.linalg.cholesky(A), True), B.T).T
    assert np.abs(X8 - want).max() <= GATE * m * EPS * np.linalg.cond(A) * np.abs(want).max()


def test_no_factor_no_solve(bioen_amd):
    with bioen_amd.Context(*small_problem(65)) as ctx:
        assert "forces_newton" not in ctx.footprint()[0]
        estate(lambda: ctx.forces_newton_solve(np.ones(65)), "bioen_hip_forces_newton_solve", "no factor")
        assert "forces_newton" not in ctx.footprint()[0]     # the buffer comes with the first factorisation
        before = ctx.footprint()[1]
        ctx.forces_newton_factor(spd(65), want_L=False)
        forms, after = ctx.footprint()
        assert "forces_newton" in forms and after - before >= 96 * 96 * 8
        ctx.forces_newton_factor(spd(65), want_L=False)
        assert ctx.footprint() == (forms, after)             # ... once
        with pytest.raises(ValueError):
            ctx.forces_newton_factor(np.eye(64))
        from bioen_amd import _lib
        info = _lib.C.c_int(0)
        A = spd(65)
        assert _lib.lib().bioen_hip_forces_newton_factor(ctx._h, _lib.ptr(A), 0, -1.0, None, _lib.C.byref(info)) == -1
        assert _lib.lib().bioen_hip_forces_newton_factor(ctx._h, _lib.ptr(A), 0, 0.0, None, None) == -1
        assert _lib.lib().bioen_hip_forces_newton_factor(ctx._h, None, 2, 0.0, None, _lib.C.byref(info)) == -1
        assert _lib.lib().bioen_hip_forces_newton_solve(ctx._h, 9, _lib.ptr(A), _lib.ptr(A)) == -1


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_the_kept_points_hessian_is_factorised_where_it_lies(bioen_amd, shape):
    """A=None factors exactly the H that forces_gram / forces_gram_bf16 download at the same point; the passes return their
    bits before, between and after: the L buffer and the sources' buffers do not alias; point and session are kept"""
    yT, YT, w0, f, pool = problem(shape)
    theta = 10.0
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=theta)
        C64, H64 = ctx.forces_gram()
        C16, H16 = ctx.forces_gram_bf16()
        for source, H in (("gram", H64), ("gram_bf16", H16)):
            # away from the optimum H need not be positive definite: lam lifts its smallest eigenvalue to 1e-2 max|H| or more
            m, low = shape[0], np.linalg.eigvalsh(H).min()
            lam = max(0.0, -low) + 1e-2 * np.abs(H).max()
            L, info = ctx.forces_newton_factor(None, source=source, lam=lam)
            assert info == 0
            again = ctx.forces_gram()
            assert np.array_equal(again[0], C64) and np.array_equal(again[1], H64)
            again = ctx.forces_gram_bf16()
            assert np.array_equal(again[0], C16) and np.array_equal(again[1], H16)
            L2, info = ctx.forces_newton_factor(H, lam=lam)  # the download, passed as a caller's matrix
            assert info == 0 and np.array_equal(L2, L)
            Hl = H + lam * np.eye(m)
            assert np.abs(L.dot(L.T) - Hl).max() <= GATE * m * EPS * np.abs(Hl).max()
            L3, info = ctx.forces_newton_factor(None, source=source, lam=2.0 * lam)
            L4, _ = ctx.forces_newton_factor(H, lam=2.0 * lam)
            assert info == 0 and np.array_equal(L3, L4) and not np.array_equal(L3, L)
            Hl = H + 2.0 * lam * np.eye(m)
            x = ctx.forces_newton_solve(pool[1])
            assert np.abs(Hl.dot(x) - pool[1]).max() <= GATE * m * EPS * np.abs(Hl).max() * np.abs(x).max() * np.linalg.cond(Hl)
            if low < 0.0:                                    # ... and without lam the failure is reported, from both ways in
                info0 = ctx.forces_newton_factor(None, source=source)[1]
                assert info0 > 0 and ctx.forces_newton_factor(H)[1] == info0
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)           # the point is still the products'


def test_state_rules(bioen_amd):
    from test_entry_effects import P
    yT, YT, w0, f, pool = problem((64, 2000))
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.forces_newton_factor(None), "bioen_hip_forces_newton_factor", "no point on this context")
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        ctx.forces_fdf(f, w0, 10.0)                          # drops the point
        estate(lambda: ctx.forces_newton_factor(None), "bioen_hip_forces_newton_factor", "is gone", "bioen_hip_forces_fdf")
        assert "forces_newton" not in ctx.footprint()[0]
        # the minimizer leaves its optimum as the kept point: the inputs of laplace_error_bars are served at once
        res = ctx.opt_newton_forces(np.zeros(64), w0, 10.0, dict(gtol=1e-8))
        assert res["status"] in (0, 2) and res["weights"].shape == (2000,) and abs(res["weights"].sum() - 1.0) <= 1e-12
        C, H = ctx.forces_gram()
        C2, H2, fv, grad = ctx.forces_gram(forces=res["forces"], w0=w0, theta=10.0)
        assert np.array_equal(C, C2) and np.array_equal(H, H2) and fv == res["fmin"]
        assert np.abs(grad).max() == res["gmax"]
        assert np.array_equal(ctx.forces_weights(res["forces"], w0), res["weights"])
        ctx.set_storage("fp32")
        for call, name in ((lambda: ctx.forces_newton_factor(spd(64)), "bioen_hip_forces_newton_factor"),
                           (lambda: ctx.forces_newton_solve(np.ones(64)), "bioen_hip_forces_newton_solve"),
                           (lambda: ctx.opt_newton_forces(np.zeros(64), w0, 10.0), "bioen_hip_opt_newton_forces")):
            estate(call, name, "reduced-storage")
        ctx.set_storage("f64")
    p = P.get()                                              # on a log-weights point
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        estate(lambda: ctx.forces_newton_factor(None), "log-weights point", "bioen_hip_forces_newton_factor")
        assert np.array_equal(ctx.logw_hessp(p.v), hl)
        ctx.bfgs_begin(p.x, p.G, p.theta)                    # the minimizer ends a BFGS session
        ctx.opt_newton_forces(np.zeros(p.m), p.w0, p.theta, dict(max_iterations=1))
        estate(lambda: ctx.bfgs_trial(1e-3, False), "ended by another call")
    yT, YT, w0, f, pool = problem((1100, 2000))              # row panels
    with bioen_amd.Context(yT, YT) as ctx:
        for call, name in ((lambda: ctx.forces_newton_factor(np.eye(1100)), "bioen_hip_forces_newton_factor"),
                           (lambda: ctx.forces_newton_solve(np.ones(1100)), "bioen_hip_forces_newton_solve"),
                           (lambda: ctx.opt_newton_forces(np.zeros(1100), w0, 10.0), "bioen_hip_opt_newton_forces")):
            estate(call, name, "M <= 1024")
        assert "forces_newton" not in ctx.footprint()[0]


def test_refused_without_the_strip_copies(bioen_amd, monkeypatch):
    yT, YT, w0, f, _ = problem((64, 2000))
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")
    with bioen_amd.Context(yT, YT) as ctx:
        f0, _ = ctx.forces_fdf(f, w0, 10.0)                  # the evaluation itself is served there
        assert np.isfinite(f0) and ctx.footprint()[0] == {"rowmajor"}
        estate(lambda: ctx.forces_newton_factor(spd(64)), "bioen_hip_forces_newton_factor", "strip copies")
        estate(lambda: ctx.opt_newton_forces(np.zeros(64), w0, 10.0), "bioen_hip_opt_newton_forces", "strip copies")
        assert "forces_newton" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 1000))

    def workload(ctx, local_segments):
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_newton_factor(None), "bioen_hip_forces_newton_factor", "structure-sharded")
        estate(lambda: ctx.forces_newton_factor(spd(129)), "bioen_hip_forces_newton_factor", "structure-sharded")
        estate(lambda: ctx.forces_newton_solve(np.ones(129)), "bioen_hip_forces_newton_solve", "structure-sharded")
        estate(lambda: ctx.opt_newton_forces(f, w0, 10.0), "bioen_hip_opt_newton_forces", "structure-sharded")
        return True

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))


# ---- the loop ---------------------------------------------------------------------------------------
def device_newton(d, source, mod=""):
    cfg = minimize.Parameters("newton", "newton:hessian=%s%s" % (source, mod))
    cfg.update(verbose=False)
    out = forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)
    return out, dict(c_bioen.last_opt_info)


@pytest.mark.parametrize("source", ("gram", "gram_bf16"))
@pytest.mark.parametrize("name", DRIVER_CASES)
def test_driver_through_find_optimum(bioen_amd, name, source):
    d, host = host_newton(name, source)
    out, info = device_newton(d, source)
    print("%s %s: device %d iterations, %d evaluations, %d Hessians, %d factorisations, status %d, max|g| %.3g, switched %s; "
          "restatement %d iterations, %d factorisations"
          % (name, source, info["iterations"], info["evaluations"], info["hessians"], info["factorisations"], info["status"],
             info["gmax"], info["switched"], host["iterations"], host["factorisations"]))
    check_optimum(d, out)
    assert info["status"] == 0 and info["gmax"] <= 1e-6
    ref = as_tuple(d, host)
    assert abs(out[4] - ref[4]) <= 1e-6
    assert np.abs(out[0].reshape(-1) - ref[0].reshape(-1)).max() <= 1e-5 * ref[0].max()
    assert abs(info["iterations"] - host["iterations"]) <= 2


def test_max_iterations_raises_with_the_return_code(bioen_amd):
    d = load_golden("ref_data_forces_M64xN64.npz")
    with pytest.raises(RuntimeError, match="return code 1"):
        device_newton(d, "gram", ",newton:max_iterations=1")


def loop_case(theta):
    shape = (300, 9000)
    yT, YT, G, w0, f, x = loop_data(shape)
    return dict(forces_init=np.zeros((shape[0], 1)), w0=w0.reshape(-1, 1), y=yT, yTilde=yT, YTilde=YT, theta=theta)


def test_where_a_set_runs_several_strips_of_its_segment(bioen_amd, monkeypatch):
    """300 x 9000 with ONE canonical segment (tests/test_hip_strip_loops.py's regime): several strips per set in the Gram
    pass; against scipy's trust-exact with hessian=gram on the same device objective"""
    enter_regime(monkeypatch, (300, 9000))
    c_bioen.clear_cache()
    gram_gmax = None
    for theta in (0.1, 10.0, 1000.0):
        d = loop_case(theta)
        cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:hessian=gram,scipy:gtol=1e-6")
        cfg.update(verbose=False)
        trust = forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), theta, cfg)
        out, info = device_newton(d, "gram")
        print("theta %g: newton fmin %.15g (trust-exact %.15g), status %d, %d iterations, %d factorisations, max|g| %.3g"
              % (theta, out[4], trust[4], info["status"], info["iterations"], info["factorisations"], info["gmax"]))
        assert info["status"] in (0, 2)
        assert out[4] <= trust[4] + 1e-9 * abs(trust[4])
        gram_gmax = info["gmax"]
    # theta = 1000 from the split-BF16 Hessian, where scipy's trust region ended with status 2 above gtol
    out16, info16 = device_newton(loop_case(1000.0), "gram_bf16")
    print("theta 1000, gram_bf16: status %d, %d iterations, max|g| %.3g (gram: %.3g), switched to gram: %s"
          % (info16["status"], info16["iterations"], info16["gmax"], gram_gmax, info16["switched"]))
    assert info16["status"] in (0, 2)
    assert info16["gmax"] <= 10.0 * gram_gmax
    c_bioen.clear_cache()


def test_a_singular_hessian_takes_the_damping_path(bioen_amd):
    """808 x 10: C has rank <= 10 and H is singular up to theta-independent terms -- lambda on the device"""
    yT, YT, w0, f, _ = problem((808, 10))
    with bioen_amd.Context(yT, YT) as ctx:
        res = ctx.opt_newton_forces(np.zeros(808), w0, 10.0, dict(gtol=1e-6), want_weights=False)
        print("808 x 10: status %d, %d iterations, %d Hessians, %d factorisations, lam %.3g, max|g| %.3g"
              % (res["status"], res["iterations"], res["hessians"], res["factorisations"], res["lam"], res["gmax"]))
        assert res["status"] in (0, 2)
        assert res["factorisations"] > res["hessians"]
        assert res["weights"] is None

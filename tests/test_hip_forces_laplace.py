"""GPU tests of the Laplace error bars formed on the device (csrc/kernels_forces_laplace.hip, csrc/api_forces_laplace.cpp,
Context.forces_inverse / forces_laplace, forces.laplace_error_bars(on_device=True)): the inverse from the
resident Cholesky factor against LAPACK on caller matrices, its bitwise invariants, pivot failures as ordinary results, the
whole entry against the host path at converged optima, the affine model, the kept-point rules, the refusals."""
import numpy as np
import pytest
import scipy.linalg

from test_hip_forces_hessp import estate, problem
from test_hip_forces_newton import small_problem, spd
from test_hip_strip_loops import on_thread_ranks

from bioen_amd.optimize import forces, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# one element; under a tile; a tile's edges; two full tiles; a ragged last tile at distance 1, 3 and 8; every tile full
INVERSE_M = (1, 7, 63, 64, 65, 128, 129, 200, 513, 808, 1024)
# |A Ainv - I|_max <= GATE m eps cond(A), |Ainv - inv_lapack|_max <= GATE m eps cond(A) |Ainv|_max, |logdet - slogdet| <=
# GATE_LOGDET m eps max(1, |logdet|).  A gate is 8 x the worst ratio measured on the MI355X over INVERSE_M (and the cond 1e6
# matrix) against LAPACK's dpotrf + dpotri and numpy's slogdet: the orders of summation differ, by rounding only.  The
# ratios measured, by INVERSE_M then the cond 1e6 matrix at M = 129:
MEASURED = dict(
    AAinv=(0.5, 0.0571, 0.0193, 0.0294, 0.0188, 0.0208, 0.0191, 0.0185, 0.00873, 0.00576, 0.00552, 0.00049),      # the worst: M = 1
    lapack=(0.0, 0.0414, 0.0155, 0.0207, 0.015, 0.0105, 0.0078, 0.0101, 0.00568, 0.0044, 0.00406, 0.000374),
    logdet=(0.5, 0.123, 0.0288, 0.0137, 0.0129, 0.00682, 0.00664, 0.00276, 0.00168, 0.0, 0.00084, 0.597),
)
GATE = 8 * max(max(MEASURED["AAinv"]), max(MEASURED["lapack"]))
GATE_LOGDET = 8 * max(MEASURED["logdet"])

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


def context(bioen_amd, m):
    """one context per M for the tests on caller matrices (the matrix of the context plays no part in them)"""
    if m not in _CTX:
        _CTX[m] = bioen_amd.Context(*small_problem(m))
    return _CTX[m]


def lapack_inverse(A):
    c, info = scipy.linalg.lapack.dpotrf(A, lower=1)
    assert info == 0
    inv, info = scipy.linalg.lapack.dpotri(c, lower=1)
    assert info == 0
    return np.tril(inv) + np.tril(inv, -1).T


def held_to_lapack(ctx, A, label):
    m = A.shape[0]
    cond = np.linalg.cond(A)
    Ainv, logdet, info = ctx.forces_inverse(A)
    assert info == 0 and Ainv.shape == (m, m)
    assert np.array_equal(Ainv, Ainv.T)                                  # bitwise symmetric
    want = lapack_inverse(A)
    sign, ld = np.linalg.slogdet(A)
    r1 = np.abs(A.dot(Ainv) - np.eye(m)).max() / (m * EPS * cond)
    r2 = np.abs(Ainv - want).max() / (m * EPS * cond * np.abs(want).max())
    r3 = abs(logdet - ld) / (m * EPS * max(1.0, abs(ld)))
    print("%s: |A Ainv - I| = %.3g m eps cond, |Ainv - lapack| = %.3g m eps cond |Ainv|, |logdet - slogdet| = %.3g m eps "
          "max(1, |logdet|) (cond %.3g)" % (label, r1, r2, r3, cond))
    assert sign == 1.0 and r1 <= GATE and r2 <= GATE and r3 <= GATE_LOGDET
    again = ctx.forces_inverse(A)                                        # the same bits in, the same bits out
    assert np.array_equal(again[0], Ainv) and again[1] == logdet
    return Ainv


@pytest.mark.parametrize("m", INVERSE_M)
def test_inverse_against_lapack(bioen_amd, m):
    ctx = context(bioen_amd, m)
    A = spd(m)
    assert np.linalg.cond(A) <= 10.0
    Ainv = held_to_lapack(ctx, A, "M = %d" % m)
    An = A.copy()                                                        # the upper triangle is not read
    An[np.triu_indices(m, 1)] = np.nan
    assert np.array_equal(ctx.forces_inverse(An)[0], Ainv)
    # the factor is the context's: the solve afterwards is Ainv b (the solve's error and the inverse's, each GATE m eps cond
    # on the scale |Ainv|_max |b|_1 that bounds |x|_max)
    b = np.random.default_rng(m).standard_normal(m)
    x = ctx.forces_newton_solve(b)
    assert np.abs(x - Ainv.dot(b)).max() <= 2 * GATE * m * EPS * np.linalg.cond(A) * np.abs(Ainv).max() * np.abs(b).sum()


def test_inverse_of_an_ill_conditioned_matrix(bioen_amd):
    m = 129
    Q, _ = np.linalg.qr(np.random.default_rng(6).standard_normal((m, m)))
    A = (Q * np.logspace(0.0, -6.0, m)).dot(Q.T)
    A = 0.5 * (A + A.T)
    assert 5e5 <= np.linalg.cond(A) <= 2e6
    held_to_lapack(context(bioen_amd, m), A, "M = 129, cond 1e6")


@pytest.mark.parametrize("m", (65, 200))
def test_a_poisoned_buffer_does_not_leak(bioen_amd, m):
    """a NaN-filled A: info = 1, nothing written; the next inverse on that context is a fresh context's, bit for bit -- what
    the failed call left in the padded buffers is never read"""
    A = spd(m)
    with bioen_amd.Context(*small_problem(m)) as fresh:
        want = fresh.forces_inverse(A)
        assert want[2] == 0
    with bioen_amd.Context(*small_problem(m)) as ctx:
        from bioen_amd import _lib
        bad = np.full((m, m), np.nan)
        out, logdet, info = np.full((m, m), 7.0), _lib.C.c_double(7.0), _lib.C.c_int(0)
        _lib.check(_lib.lib().bioen_laplace_forces_inverse(ctx._h, _lib.ptr(bad), _lib.ptr(out), _lib.C.byref(logdet),
                                                           _lib.C.byref(info)))
        assert info.value == 1 and (out == 7.0).all() and logdet.value == 7.0
        assert ctx.forces_inverse(bad)[::2] == (None, 1)
        estate(lambda: ctx.forces_newton_solve(np.ones(m)), "bioen_hip_forces_newton_solve", "info = 1")
        got = ctx.forces_inverse(A)
        assert got[2] == 0 and np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("m", (129, 1024))
def test_a_pivot_that_is_not_positive_is_reported_as_the_factorisation_reports_it(bioen_amd, m):
    ctx = context(bioen_amd, m)
    A = spd(m)
    want = ctx.forces_inverse(A)
    for k in (0, 63, 64, m - 1):                  # the first row, a panel's end, the next panel's start, the last row
        bad = A.copy()
        bad[k, k] = -1.0
        Ainv, logdet, info = ctx.forces_inverse(bad)
        assert Ainv is None and np.isnan(logdet) and info == k + 1 == ctx.forces_newton_factor(bad, want_L=False)[1]
    got = ctx.forces_inverse(A)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


# ---- the whole entry ----------------------------------------------------------------------------------
THETA = 10.0
ENTRY_SHAPES = [(65, 300), (129, 700), (513, 1537), (1024, 2500)]
_OPT = {}


def optimum(shape):
    """tests/test_hip_forces_colquad.py's generator (test_laplace_error_bars_on_the_device), seeded by the shape, and its
    converged optimum (the device Newton minimizer, gtol 1e-8), found once per shape"""
    if shape not in _OPT:
        M, N = shape
        rng = np.random.default_rng(M * N)
        yT = rng.normal(rng.normal(0.0, 2.0, (M, 1)), 1.0, (M, N))
        w0 = rng.uniform(0.5, 1.5, N)
        w0 /= w0.sum()
        YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
        cfg = minimize.Parameters("newton", "newton:gtol=1e-8")
        cfg.update(verbose=False, use_c_functions=True)
        out = forces.find_optimum(np.zeros((M, 1)), w0.reshape(-1, 1), yT, yT, YT.reshape(1, -1), THETA, cfg)
        _OPT[shape] = (yT, YT, w0, np.asarray(out[2]).reshape(-1))
    return _OPT[shape]


ARRAYS = ("w", "C", "H", "cov_forces", "std_forces", "cov_averages", "std_averages", "var_logw", "std_w")


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=["%dx%d" % s for s in ENTRY_SHAPES])
def test_error_bars_against_the_host_paths(bioen_amd, shape):
    """laplace_error_bars(on_device=True) against the path through the host (use_c=True) and against numpy (use_c=False):
    every array to 1e-8 of its largest entry -- the gate tests/test_hip_forces_colquad.py holds that function to --,
    logdet_H to 1e-12"""
    yT, YT, w0, fopt = optimum(shape)
    dev = forces.laplace_error_bars(fopt, w0, yT, yT, YT, THETA, use_c=True, on_device=True)
    lean = forces.laplace_error_bars(fopt, w0, yT, yT, YT, THETA, use_c=True, on_device=True, matrices=False)
    parent = forces.laplace_error_bars(fopt, w0, yT, yT, YT, THETA, use_c=True)
    host = forces.laplace_error_bars(fopt, w0, yT, yT, YT, THETA, use_c=False, on_device=True)
    assert set(dev) == set(lean) == set(host) == set(ARRAYS) | {"logdet_H"} and set(parent) == set(ARRAYS)
    for name, ref in (("host path", parent), ("numpy", host)):
        for k in ARRAYS:
            err = np.abs(dev[k] - ref[k]).max() / np.abs(ref[k]).max()
            print("%dx%d %s: max |on device - %s| = %.3g of its largest entry" % (shape + (k, name, err)))
            assert dev[k].shape == ref[k].shape and err <= 1e-8
    rel = abs(dev["logdet_H"] - host["logdet_H"]) / abs(host["logdet_H"])
    sld = np.linalg.slogdet(host["H"])
    print("%dx%d logdet_H: %.17g, numpy %.17g: relative difference %.3g" % (shape + (dev["logdet_H"], host["logdet_H"], rel)))
    assert rel <= 1e-12 and sld[0] == 1.0 and abs(dev["logdet_H"] - sld[1]) <= 1e-12 * abs(sld[1])
    for k in ("cov_forces", "cov_averages"):
        assert np.array_equal(dev[k], dev[k].T)
    for k in ("C", "H", "cov_forces", "cov_averages"):
        assert lean[k] is None
    for k in ("w", "std_forces", "std_averages", "var_logw", "std_w"):
        assert np.array_equal(lean[k], dev[k])
    assert lean["logdet_H"] == dev["logdet_H"]


def test_error_bars_with_an_affine_model(bioen_amd):
    """129 x 700 with row offsets and scales on the context: forces_laplace against forces_gram, the host's inverse and
    forces_colquad on the same context"""
    yT, YT, w0, fopt = optimum((129, 700))
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, 129), rng.uniform(0.5, 1.5, 129)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        res = ctx.opt_newton_forces(np.zeros(129), w0, THETA, dict(gtol=1e-8), want_weights=False)
        assert res["status"] in (0, 2)
        C, H, fv, grad = ctx.forces_gram(forces=res["forces"], w0=w0, theta=THETA)
        Hi = forces._laplace_inverse(H, THETA)
        ca = C.dot(Hi).dot(C)
        want = dict(cov_forces=Hi, std_forces=np.sqrt(np.diag(Hi)), cov_averages=0.5 * (ca + ca.T),
                    std_averages=np.sqrt(np.diag(ca)), var_logw=ctx.forces_colquad(Hi))
        got = ctx.forces_laplace(forces=res["forces"], w0=w0, theta=THETA)
        assert got["info"] == 0 and got["f"] == fv and np.array_equal(got["grad"], grad)
        for k in sorted(want):
            err = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
            print("affine 129x700 %s: max |on device - host path| = %.3g of its largest entry" % (k, err))
            assert err <= 1e-8
        assert got["min_pivot"] > 0.0 and abs(got["logdet_H"] - np.linalg.slogdet(H)[1]) <= 1e-12 * abs(np.linalg.slogdet(H)[1])


def test_the_kept_point_is_served_and_kept(bioen_amd):
    yT, YT, w0, fopt = optimum((65, 300))
    with bioen_amd.Context(yT, YT) as ctx:
        res = ctx.opt_newton_forces(np.zeros(65), w0, THETA, dict(gtol=1e-8), want_weights=False)
        C, H = ctx.forces_gram()
        kept = ctx.forces_laplace()                                      # the optimum, without forces
        assert kept["info"] == 0 and "f" not in kept
        again = ctx.forces_gram()
        assert np.array_equal(again[0], C) and np.array_equal(again[1], H)
        given = ctx.forces_laplace(forces=res["forces"], w0=w0, theta=THETA)
        assert given["f"] == res["fmin"]
        for k in ("std_forces", "std_averages", "var_logw", "cov_forces", "cov_averages"):
            assert np.array_equal(kept[k], given[k])
        assert kept["logdet_H"] == given["logdet_H"] and kept["min_pivot"] == given["min_pivot"]
        # the inverse of the kept point's Hessian stays resident; the factor serves the solve
        none, logdet, info = ctx.forces_inverse()
        assert none is None and info == 0 and logdet == kept["logdet_H"]
        b = np.random.default_rng(1).standard_normal(65)
        assert np.abs(ctx.forces_newton_solve(b) - kept["cov_forces"].dot(b)).max() <= (
            2 * GATE * 65 * EPS * np.linalg.cond(H) * np.abs(kept["cov_forces"]).max() * np.abs(b).sum())


def test_the_gram_pass_of_another_point_is_not_served(bioen_amd):
    """forces_laplace() takes C and H where forces_gram left them only while the point is the same: after a new point it
    computes them anew (a fresh context's bits)"""
    yT, YT, w0, fopt = optimum((65, 300))
    other = 0.5 * fopt
    with bioen_amd.Context(yT, YT) as fresh:
        want = fresh.forces_laplace(forces=fopt, w0=w0, theta=THETA)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.forces_gram(forces=other, w0=w0, theta=THETA)
        ctx.forces_hessp(None, forces=fopt, w0=w0, theta=THETA)           # a new point, no Gram pass at it
        got = ctx.forces_laplace()
        assert got["info"] == want["info"] == 0
        for k in ("std_forces", "std_averages", "var_logw", "cov_forces", "cov_averages"):
            assert np.array_equal(got[k], want[k]), k
        assert got["logdet_H"] == want["logdet_H"]


def test_refusals_footprint_and_failure_paths(bioen_amd, monkeypatch):
    from test_entry_effects import P
    yT, YT, w0, f, pool = problem((64, 2000))
    calls = ((lambda c: c.forces_inverse(spd(c.m)), "bioen_laplace_forces_inverse"),
             (lambda c: c.forces_laplace(forces=np.zeros(c.m), w0=np.full(c.n, 1.0 / c.n), theta=10.0), "bioen_laplace_forces"))
    with bioen_amd.Context(yT, YT) as ctx:
        assert "forces_laplace" not in ctx.footprint()[0]
        estate(lambda: ctx.forces_laplace(), "bioen_laplace_forces", "no point on this context")
        estate(lambda: ctx.forces_inverse(), "bioen_laplace_forces_inverse", "no point on this context")
        assert "forces_laplace" not in ctx.footprint()[0]                # the buffer comes with the first computing call
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        before = ctx.footprint()[1]
        ctx.forces_inverse(spd(64))
        forms, after = ctx.footprint()
        assert "forces_laplace" in forms and after - before >= 4 * 64 * 64 * 8
        ctx.forces_inverse(spd(64))
        assert ctx.footprint() == (forms, after)                         # ... once
        with pytest.raises(ValueError):
            ctx.forces_inverse(np.eye(63))
        ctx.set_storage("fp32")                                          # drops the point
        for call, name in calls:
            estate(lambda: call(ctx), name, "reduced-storage")
        ctx.set_storage("f64")
    with bioen_amd.Context(yT, YT) as ctx:                               # a new context starts without the buffer
        assert "forces_laplace" not in ctx.footprint()[0]
    p = P.get()                                                          # on a log-weights point
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        estate(lambda: ctx.forces_laplace(), "log-weights point")
        estate(lambda: ctx.forces_inverse(), "log-weights point", "bioen_laplace_forces_inverse")
        assert np.array_equal(ctx.logw_hessp(p.v), hl)
    yT, YT, w0, f, pool = problem((1100, 2000))                          # row panels
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        for call, name in calls:
            estate(lambda: call(ctx), name, "M <= 1024")
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv) and "forces_laplace" not in ctx.footprint()[0]
    yT, YT, w0, f, _ = problem((64, 2000))
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")
    with bioen_amd.Context(yT, YT) as ctx:
        f0, _ = ctx.forces_fdf(f, w0, 10.0)
        assert np.isfinite(f0) and ctx.footprint()[0] == {"rowmajor"}
        for call, name in calls:
            estate(lambda: call(ctx), name, "strip copies")
        assert "forces_laplace" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 1000))

    def workload(ctx, local_segments):
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_inverse(spd(129)), "bioen_laplace_forces_inverse", "structure-sharded")
        estate(lambda: ctx.forces_inverse(), "bioen_laplace_forces_inverse", "structure-sharded")
        estate(lambda: ctx.forces_laplace(), "bioen_laplace_forces", "structure-sharded")
        estate(lambda: ctx.forces_laplace(forces=f, w0=w0, theta=10.0), "bioen_laplace_forces", "structure-sharded")
        return np.array_equal(ctx.forces_hessp(pool[0]), hv)

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))


def test_a_singular_hessian_raises_the_host_paths_message(bioen_amd):
    """808 x 10 at its optimum (the damped Newton loop finds it): C has rank <= 10 and H is singular.  The device path judges
    it from the factorisation, downloads H and lets the host path's _laplace_inverse word the refusal: the same H bits, so
    the same message, character for character"""
    yT, YT, w0, f, _ = problem((808, 10))
    with bioen_amd.Context(yT, YT) as ctx:
        res = ctx.opt_newton_forces(np.zeros(808), w0, 10.0, dict(gtol=1e-6), want_weights=False)
        assert res["status"] in (0, 2)
    fopt = res["forces"]
    with pytest.raises(ValueError, match="the Hessian is singular") as parent:
        forces.laplace_error_bars(fopt, w0, yT, yT, YT, 10.0, use_c=True)
    for matrices in (True, False):
        with pytest.raises(ValueError, match="the Hessian is singular") as dev:
            forces.laplace_error_bars(fopt, w0, yT, yT, YT, 10.0, use_c=True, on_device=True, matrices=matrices)
        assert str(dev.value) == str(parent.value)

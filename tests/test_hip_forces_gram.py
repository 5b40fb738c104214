"""GPU tests of the dense Hessian and the covariance of the forces objective in one pass (csrc/kernels_forces_gram.hip,
csrc/api_forces_gram.cpp, Context.forces_gram): every entry against the Hessian the products build at the same kept point
(Context.forces_hessian, the device oracle) and against the formula in numpy.longdouble, the bitwise invariants, the
affine model, the state rules and refusals, and scipy's trust-exact fed by it through find_optimum."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_forces_hessp import DRIVER_CASES, check_optimum, run_driver
from test_hip_forces_hessp import estate, problem
from test_hip_strip_loops import data as loop_data, enter_regime, on_thread_ranks

pytestmark = pytest.mark.gpu

L = np.longdouble
THETAS = (0.1, 10.0, 1000.0)
GATE = 1e-10          # of max|H| (of max|C| for C): the project's gate for the rounding of a Hessian (forces_hessian)
# the smallest shapes at which the kernel can go wrong -- 7 x 37: rows padded to 16, redirected row blocks, a ragged last
# strip; 808 x 10: one strip, empty segments, 28 tiles; 129 x 257: a second tile of one row block; 64 x 2000: one full
# slice; 513 x 1537: nine slices, sets of several strips; 1024 x 528: every tile full
SHAPES = [(7, 37), (808, 10), (129, 257), (64, 2000), (513, 1537), (1024, 528)]


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()


def _gram_ld(A, u):
    """sum_j u_j a_j a_j^T in longdouble, row blocks on eight threads (numpy's longdouble products release the lock)"""
    Au = A * u[None, :]
    blocks = np.array_split(np.arange(A.shape[0]), 8)
    with ThreadPoolExecutor(8) as workers:
        parts = list(workers.map(lambda rows: Au[rows] @ A.T, [b for b in blocks if b.size]))
    return np.vstack(parts)


_LD = {}


def gram_longdouble(key, A, YT, w0, f):
    """forces.hessian_gram_bioen_log_posterior_base in numpy.longdouble, once per problem: the weights do not depend on
    theta and q = theta x + b is linear in it, so  H(theta) = theta C + C C + theta G[w (x - <x>)] + G[w (b - <b>)].
    -> theta -> (C, H) in float64"""
    if key not in _LD:
        x = f.astype(L) @ A
        e = w0.astype(L) * np.exp(x - x.max())
        w = e / e.sum()
        ybar = A @ w
        b = (ybar - YT.astype(L)) @ A
        a = A - ybar[:, None]
        _LD[key] = (_gram_ld(a, w), _gram_ld(a, w * (x - w @ x)), _gram_ld(a, w * (b - w @ b)))
    C, Gx, Gb = _LD[key]
    CC = None

    def at(theta):
        nonlocal CC
        if CC is None:
            CC = _gram_ld(C, np.ones(C.shape[0], dtype=L))          # C C^T = C C
        return C.astype(np.float64), (L(theta) * C + CC + L(theta) * Gx + Gb).astype(np.float64)
    return at


def held_to_both(ctx, C, H, ref, label):
    """C and H of forces_gram against the products' Hessian at the same kept point and against longdouble"""
    Cl, Hl = ref
    Hp = ctx.forces_hessian()
    S, SC = float(np.abs(Hl).max()), float(np.abs(Cl).max())
    dp, dl, dc = np.abs(H - Hp).max() / S, np.abs(H - Hl).max() / S, np.abs(C - Cl).max() / SC
    print("%s: max |H - H_products| = %.3g, |H - H_ld| = %.3g max|H|; |C - C_ld| = %.3g max|C|; |H_products - H_ld| = %.3g"
          % (label, dp, dl, dc, np.abs(Hp - Hl).max() / S))
    assert np.array_equal(H, H.T) and np.array_equal(C, C.T)
    assert dp <= GATE and dl <= GATE and dc <= GATE


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_gram_against_the_products_and_longdouble(bioen_amd, shape):
    """at the forces of tests/test_hip_forces_hessp.py's problem(): weights over decades, not an optimum; every theta"""
    yT, YT, w0, f, _ = problem(shape)
    ref = gram_longdouble(shape, yT.astype(L), YT, w0, f)
    with bioen_amd.Context(yT, YT) as ctx:
        for theta in THETAS:
            f0, g0 = ctx.forces_fdf(f, w0, theta)
            C, H, fv, grad = ctx.forces_gram(forces=f, w0=w0, theta=theta)
            assert fv == f0 and np.array_equal(grad, g0)                 # the point-setting call is forces_fdf's evaluation
            held_to_both(ctx, C, H, ref(theta), "%dx%d theta %g" % (shape + (theta,)))


def test_gram_where_a_set_runs_several_strips_of_its_segment(bioen_amd, monkeypatch):
    """300 x 9000 with ONE canonical segment (tests/test_hip_strip_loops.py's regime): 86 groups of 6 or 7 strips"""
    shape = (300, 9000)
    enter_regime(monkeypatch, shape)
    yT, YT, G, w0, f, x = loop_data(shape)
    f = f / 5.0                                                 # x with standard deviation 1
    ref = gram_longdouble("loop", yT.astype(L), YT, w0, f)
    with bioen_amd.Context(yT, YT) as ctx:
        assert ctx.strip_plan(1)["local_segments"] == 1
        for theta in THETAS:
            C, H, _, _ = ctx.forces_gram(forces=f, w0=w0, theta=theta)
            held_to_both(ctx, C, H, ref(theta), "300x9000, one segment, theta %g" % theta)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_bitwise_invariants(bioen_amd, shape):
    yT, YT, w0, f, pool = problem(shape)
    theta = 10.0
    with bioen_amd.Context(yT, YT) as ctx:
        C, H, fv, grad = ctx.forces_gram(forces=f, w0=w0, theta=theta)              # sets the point
        assert np.array_equal(H, H.T) and np.array_equal(C, C.T)
        for _ in range(2):                                                          # serves it: the same bits, call after call
            C2, H2 = ctx.forces_gram()
            assert np.array_equal(C2, C) and np.array_equal(H2, H)
        only_c, none = ctx.forces_gram(hess=False)
        assert none is None and np.array_equal(only_c, C)
        none, only_h = ctx.forces_gram(cov=False)
        assert none is None and np.array_equal(only_h, H)
        hv = ctx.forces_hessp(pool[:3])                                             # the products' point is this one
        ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)                        # ... and a point they set serves the pass
        C3, H3 = ctx.forces_gram()
        assert np.array_equal(C3, C) and np.array_equal(H3, H)
        assert np.array_equal(ctx.forces_hessp(pool[:3]), hv)
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))                       # (o, s) = (0, 1): the plain model's bits
        C4, H4, f4, g4 = ctx.forces_gram(forces=f, w0=w0, theta=theta)
        assert f4 == fv and np.array_equal(g4, grad)
        assert np.array_equal(C4, C) and np.array_equal(H4, H)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_gram_with_an_affine_model(bioen_amd, shape):
    """row offsets and scales set on the context; the test folds them into its own matrix"""
    yT, YT, w0, f, _ = problem(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    eff = off[:, None].astype(L) + sc[:, None].astype(L) * yT.astype(L)
    ref = gram_longdouble(("affine", shape), eff, YT, w0, f)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        C, H, _, _ = ctx.forces_gram(forces=f, w0=w0, theta=10.0)
        held_to_both(ctx, C, H, ref(10.0), "affine %dx%d" % shape)


def test_the_products_point_is_left_alone(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool, forces=f, w0=w0, theta=10.0)
        ctx.forces_gram()
        assert np.array_equal(ctx.forces_hessp(pool), hv)


def test_refusals_leave_the_point_alone(bioen_amd):
    from test_entry_effects import P
    yT, YT, w0, f, pool = problem((64, 2000))
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.forces_gram(), "no point on this context", "bioen_hip_forces_gram")
        C, H, _, _ = ctx.forces_gram(forces=f, w0=w0, theta=10.0)
        hv = ctx.forces_hessp(pool[0])
        ctx.forces_fdf(f, w0, 10.0)                                  # after an evaluation
        estate(lambda: ctx.forces_gram(), "is gone", "bioen_hip_forces_fdf")
        ctx.forces_gram(forces=f, w0=w0, theta=10.0, cov=False, hess=False)      # only sets the point
        # rejected for its arguments: the point stays
        from bioen_amd import _lib
        assert _lib.lib().bioen_hip_forces_gram(ctx._h, _lib.ptr(f), None, 10.0, None, None, None, None) == -1
        assert _lib.lib().bioen_hip_forces_gram(ctx._h, None, None, 0.0, None, None, None, None) == -1
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)
        ctx.set_storage("fp32")                                       # set_storage(2): the reduced-storage copies
        estate(lambda: ctx.forces_gram(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram", "reduced-storage")
        ctx.set_storage("f64")
        C2, H2, _, _ = ctx.forces_gram(forces=f, w0=w0, theta=10.0)
        assert np.array_equal(C2, C) and np.array_equal(H2, H)
    p = P.get()                                                      # on a log-weights point
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        estate(lambda: ctx.forces_gram(), "log-weights point", "bioen_hip_forces_gram")
        assert np.array_equal(ctx.logw_hessp(p.v), hl)
    yT, YT, w0, f, pool = problem((1100, 2000))                      # row panels
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_gram(), "bioen_hip_forces_gram", "M <= 1024")
        estate(lambda: ctx.forces_gram(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram", "M <= 1024")
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)
        assert "forces_gram" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 1000))

    def workload(ctx, local_segments):
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_gram(), "bioen_hip_forces_gram", "structure-sharded")
        estate(lambda: ctx.forces_gram(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram", "structure-sharded")
        return np.array_equal(ctx.forces_hessp(pool[0]), hv)

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))


def test_the_buffer_is_in_the_footprint_and_goes_with_the_context(bioen_amd):
    yT, YT, w0, f, _ = problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        forms, before = ctx.footprint()
        assert "forces_gram" not in forms                            # allocated at the first use, not before
        ctx.forces_gram()
        forms, with_buffer = ctx.footprint()
        assert "forces_gram" in forms and with_buffer - before >= 2 * 129 * 129 * 8
        ctx.forces_gram()
        assert ctx.footprint() == (forms, with_buffer)               # ... once
    with bioen_amd.Context(yT, YT) as ctx:                           # a new context starts without one
        assert "forces_gram" not in ctx.footprint()[0]


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_trust_exact_with_the_gram_hessian_on_the_device(bioen_amd, name):
    d, out = run_driver(name, "trust_exact", True, mod="scipy:gtol=1e-6,scipy:hessian=gram")
    check_optimum(d, out)
    _, products = run_driver(name, "trust_exact", True)
    assert abs(out[4] - products[4]) <= 1e-9 * abs(products[4])

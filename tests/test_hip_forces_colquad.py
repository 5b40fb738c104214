"""GPU tests of the per-structure quadratic forms a_j^T P a_j at a kept forces point (csrc/kernels_forces_colquad.hip,
csrc/api_forces_colquad.cpp, Context.forces_colquad) and of forces.laplace_error_bars on the device: every result against
the formula in numpy.longdouble for four kinds of P, the bitwise invariants, the affine model, the state rules and
refusals, the footprint, and the error bars at a converged optimum against the numpy restatements."""
import numpy as np
import pytest

from test_forces_colquad import GATE, centred_ld, colquad_ld, matrices
from test_hip_forces_hessp import estate, problem
from test_hip_strip_loops import data as loop_data, enter_regime, on_thread_ranks

pytestmark = pytest.mark.gpu

L = np.longdouble
# the six shapes of tests/test_hip_forces_gram.py for the strip format's edges -- 7 x 37: rows padded to 16, three of a
# slice's four row blocks redirected, a ragged last strip and a panel whose second strip is partly padding; 808 x 10: one
# strip, a panel without a second one, empty segments, a short last slice; 129 x 257: one row block in the third slice;
# 64 x 2000: one full slice; 513 x 1537: nine slices, the last with one row block; 1024 x 528: every slice full, sixteen
# blocks per wave -- and 16 x 8200: a panel is 32 columns and a launch has 256 blocks, so 257 panels (8193 columns and more)
# is the smallest size at which ONE block runs SEVERAL panels; 8200 = 256 x 32 + 8 makes its second panel a partial one
# (8 of 32 columns, its second strip beyond column n)
SHAPES = [(7, 37), (808, 10), (129, 257), (64, 2000), (513, 1537), (1024, 528), (16, 8200)]


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()


def held_to_longdouble(ctx, a, m, seed, label):
    """forces_colquad at the kept point for P = B + B^T, I, u u^T and 0 against longdouble; -> {name: v}"""
    mats, u = matrices(m, seed)
    out = {}
    for name, P in mats.items():
        v = ctx.forces_colquad(P)
        ref, scale = colquad_ld(a, P)
        err = np.abs(v - ref).max()
        print("%s, P = %s: max |v - v_ld| = %.3g of max_j |a|^T|P||a| = %.3g" % (label, name, err / scale if scale else 0.0, scale))
        assert v.shape == (a.shape[1],) and np.isfinite(v).all()
        assert err <= GATE * scale
        if name == "I":                 # the independent formulas
            assert np.abs(v - (a * a).sum(axis=0).astype(np.float64)).max() <= GATE * scale
        if name == "uu^T":
            assert np.abs(v - ((u.astype(L) @ a) ** 2).astype(np.float64)).max() <= GATE * scale
        if name == "0":
            assert not v.any()          # exact zeros
        out[name] = v
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_colquad_against_longdouble(bioen_amd, shape):
    """at the forces of tests/test_hip_forces_hessp.py's problem(): weights over decades"""
    yT, YT, w0, f, _ = problem(shape)
    a = centred_ld(yT.astype(L), w0, f)
    mats, _ = matrices(shape[0], 11 + shape[0])
    with bioen_amd.Context(yT, YT) as ctx:
        f0, g0 = ctx.forces_fdf(f, w0, 10.0)
        v, fv, grad = ctx.forces_colquad(mats["B+B^T"], forces=f, w0=w0, theta=10.0)
        assert fv == f0 and np.array_equal(grad, g0)                 # the point-setting call is forces_fdf's evaluation
        got = held_to_longdouble(ctx, a, shape[0], 11 + shape[0], "%dx%d" % shape)
        assert np.array_equal(got["B+B^T"], v)                       # ... and gives the bits of a call that serves the point


def test_colquad_in_the_one_segment_regime(bioen_amd, monkeypatch):
    """300 x 9000 with ONE canonical segment (tests/test_hip_strip_loops.py's regime): 282 panels on 256 blocks, the last
    panel 8 columns wide"""
    shape = (300, 9000)
    enter_regime(monkeypatch, shape)
    yT, YT, G, w0, f, x = loop_data(shape)
    f = f / 5.0                                                 # x with standard deviation 1
    a = centred_ld(yT.astype(L), w0, f)
    with bioen_amd.Context(yT, YT) as ctx:
        assert ctx.strip_plan(1)["local_segments"] == 1
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        held_to_longdouble(ctx, a, 300, 311, "300x9000, one segment")


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_bitwise_invariants(bioen_amd, shape):
    yT, YT, w0, f, pool = problem(shape)
    theta = 10.0
    P = matrices(shape[0], 5)[0]["B+B^T"]
    with bioen_amd.Context(yT, YT) as ctx:
        f0, g0 = ctx.forces_fdf(f, w0, theta)
        v, fv, grad = ctx.forces_colquad(P, forces=f, w0=w0, theta=theta)               # sets the point
        assert fv == f0 and np.array_equal(grad, g0)
        for _ in range(2):                                                              # serves it: the same bits, call after call
            assert np.array_equal(ctx.forces_colquad(P), v)
        hv = ctx.forces_hessp(pool[:3])                                                 # the products' point is this one
        ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)                            # a point the products set serves the pass
        assert np.array_equal(ctx.forces_colquad(P), v)
        ctx.forces_gram(forces=f, w0=w0, theta=theta)                                   # ... and one forces_gram set
        assert np.array_equal(ctx.forces_colquad(P), v)
        assert np.array_equal(ctx.forces_hessp(pool[:3]), hv)                           # the pass leaves the products' point alone
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))                           # (o, s) = (0, 1): the plain model's bits
        v4, f4, g4 = ctx.forces_colquad(P, forces=f, w0=w0, theta=theta)
        assert f4 == fv and np.array_equal(g4, grad) and np.array_equal(v4, v)


def test_the_products_point_is_left_alone(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool, forces=f, w0=w0, theta=10.0)
        ctx.forces_colquad(np.eye(129))
        assert np.array_equal(ctx.forces_hessp(pool), hv)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_colquad_with_an_affine_model(bioen_amd, shape):
    """row offsets and scales set on the context; the test folds them into its own matrix"""
    yT, YT, w0, f, _ = problem(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    eff = off[:, None].astype(L) + sc[:, None].astype(L) * yT.astype(L)
    a = centred_ld(eff, w0, f)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        held_to_longdouble(ctx, a, shape[0], 21 + shape[0], "affine %dx%d" % shape)


def test_refusals_leave_the_point_alone(bioen_amd, monkeypatch):
    from bioen_amd import _lib
    from test_entry_effects import P as LOGW
    yT, YT, w0, f, pool = problem((64, 2000))
    P = matrices(64, 9)[0]["B+B^T"]
    skew = P.copy()
    skew[3, 5] += 1.0
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.forces_colquad(P), "no point on this context", "bioen_hip_forces_colquad")
        v, _, _ = ctx.forces_colquad(P, forces=f, w0=w0, theta=10.0)
        hv = ctx.forces_hessp(pool[0])
        ctx.forces_fdf(f, w0, 10.0)                                  # after an evaluation
        estate(lambda: ctx.forces_colquad(P), "is gone", "bioen_hip_forces_fdf")
        fn, out = _lib.lib().bioen_hip_forces_colquad, np.empty(2000)
        assert fn(ctx._h, _lib.ptr(f), _lib.ptr(w0), 10.0, None, None, None, None) == 0      # P == NULL with forces: only sets the point
        # rejected for its arguments: the point stays
        assert fn(ctx._h, _lib.ptr(f), None, 10.0, _lib.ptr(P), _lib.ptr(out), None, None) == -1
        assert fn(ctx._h, None, None, 0.0, None, None, None, None) == -1                      # P == NULL without forces
        assert fn(ctx._h, None, None, 0.0, _lib.ptr(skew), _lib.ptr(out), None, None) == -1   # an unsymmetric P: EINVAL
        assert "P is not symmetric" in _lib.lib().bioen_hip_last_error().decode()
        with pytest.raises(ValueError, match="not symmetric"):
            ctx.forces_colquad(skew)
        with pytest.raises(ValueError):
            ctx.forces_colquad(np.eye(65))
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)
        assert np.array_equal(ctx.forces_colquad(P), v)
        ctx.set_storage("fp32")                                       # set_storage(2): the reduced-storage copies
        estate(lambda: ctx.forces_colquad(P, forces=f, w0=w0, theta=10.0), "bioen_hip_forces_colquad", "reduced-storage")
        ctx.set_storage("f64")
        v2, _, _ = ctx.forces_colquad(P, forces=f, w0=w0, theta=10.0)
        assert np.array_equal(v2, v)
    p = LOGW.get()                                                   # on a log-weights point
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        estate(lambda: ctx.forces_colquad(np.eye(p.m)), "log-weights point", "bioen_hip_forces_colquad")
        assert np.array_equal(ctx.logw_hessp(p.v), hl)
    yT, YT, w0, f, pool = problem((1040, 300))                       # row panels
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_colquad(np.eye(1040)), "bioen_hip_forces_colquad", "M <= 1024")
        estate(lambda: ctx.forces_colquad(np.eye(1040), forces=f, w0=w0, theta=10.0), "bioen_hip_forces_colquad", "M <= 1024")
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)
        assert "forces_colquad" not in ctx.footprint()[0]
    yT, YT, w0, f, pool = problem((64, 2000))                        # the streaming fallback: no strip copies
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")
    with bioen_amd.Context(yT, YT) as ctx:
        f0, _ = ctx.forces_fdf(f, w0, 10.0)                          # the evaluation itself is served there
        assert np.isfinite(f0) and ctx.footprint()[0] == {"rowmajor"}
        estate(lambda: ctx.forces_colquad(P, forces=f, w0=w0, theta=10.0), "bioen_hip_forces_colquad", "strip copies")
        assert "forces_colquad" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 1000))
    P = np.eye(129)

    def workload(ctx, local_segments):
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_colquad(P), "bioen_hip_forces_colquad", "structure-sharded")
        estate(lambda: ctx.forces_colquad(P, forces=f, w0=w0, theta=10.0), "bioen_hip_forces_colquad", "structure-sharded")
        return np.array_equal(ctx.forces_hessp(pool[0]), hv)

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))


def test_the_buffer_is_in_the_footprint_and_goes_with_the_context(bioen_amd):
    yT, YT, w0, f, _ = problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        forms, before = ctx.footprint()
        assert "forces_colquad" not in forms                         # allocated at the first use, not before
        ctx.forces_colquad(np.eye(129))
        forms, with_buffer = ctx.footprint()
        assert "forces_colquad" in forms and with_buffer - before >= (129 * 129 + 257) * 8
        ctx.forces_colquad(np.eye(129))
        assert ctx.footprint() == (forms, with_buffer)               # ... once
    with bioen_amd.Context(yT, YT) as ctx:                           # a new context starts without one
        assert "forces_colquad" not in ctx.footprint()[0]


def test_laplace_error_bars_on_the_device(bioen_amd):
    """forces.laplace_error_bars(use_c=True) against use_c=False at a converged optimum of a seeded 64 x 2000 problem
    (find_optimum with trust_exact on the Gram Hessian, gtol 1e-8): every returned array to 1e-8 of its largest entry.
    How far inputs that differ at rounding move inv(H) was measured as the issue asks: H perturbed by forces_gram's
    recorded 4e-14 max|H| (symmetric, seeded) in the numpy path moves cov_forces by 3.0e-14 and var_logw by 3.0e-14 of
    their largest entries (printed at the end of every run) -- the problem is well conditioned, 10 x the movement is
    3e-13, far inside 1e-8, so the issue's 1e-8 gate stands as it is.  Measured device against numpy: <= 1.1e-15."""
    from bioen_amd.optimize import forces, minimize
    M, N, theta = 64, 2000, 10.0
    rng = np.random.default_rng(64 * 2000)
    yT = rng.normal(rng.normal(0.0, 2.0, (M, 1)), 1.0, (M, N))
    w0 = rng.uniform(0.5, 1.5, N)
    w0 /= w0.sum()
    YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
    cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:hessian=gram,scipy:gtol=1e-8")
    cfg.update(verbose=False, use_c_functions=True)
    out = forces.find_optimum(np.zeros((M, 1)), w0.reshape(-1, 1), yT, yT, YT.reshape(1, -1), theta, cfg)
    fopt = np.asarray(out[2]).reshape(-1)
    dev = forces.laplace_error_bars(fopt, w0, yT, yT, YT, theta, use_c=True)
    host = forces.laplace_error_bars(fopt, w0, yT, yT, YT, theta, use_c=False)
    assert set(dev) == set(host) == {"w", "C", "H", "cov_forces", "std_forces", "cov_averages", "std_averages", "var_logw", "std_w"}
    for k in sorted(host):
        err = np.abs(dev[k] - host[k]).max() / np.abs(host[k]).max()
        print("%s: max |device - numpy| = %.3g of its largest entry" % (k, err))
        assert dev[k].shape == host[k].shape and err <= 1e-8
    # the measurement: what a perturbation of H at the size of forces_gram's rounding does in the numpy path
    E = np.random.default_rng(1).standard_normal((M, M))
    Hp = host["H"] + 4e-14 * np.abs(host["H"]).max() * 0.5 * (E + E.T) / np.abs(E).max()
    Hip = forces._laplace_inverse(Hp, theta)
    vp = forces.colquad_bioen_log_posterior_base(fopt, Hip, w0, yT, YT, theta)
    print("H moved by 4e-14 max|H|: cov_forces moves by %.3g, var_logw by %.3g of their largest entries"
          % (np.abs(Hip - host["cov_forces"]).max() / np.abs(host["cov_forces"]).max(),
             np.abs(vp - host["var_logw"]).max() / np.abs(host["var_logw"]).max()))

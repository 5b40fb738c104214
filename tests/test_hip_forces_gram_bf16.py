"""GPU tests of the forces Hessian from split-BF16 operands (csrc/kernels_forces_gram.hip: k_forces_gram_bf16,
csrc/api_forces_gram.cpp, Context.forces_gram_bf16): every entry against the FP64 pass at the same kept point
(Context.forces_gram) and against the numpy restatement with the same rounding points, the bitwise invariants, the affine
model, the state rules and refusals, the footprint, and scipy's trust-exact fed by it through find_optimum."""
import numpy as np
import pytest

from test_forces_hessp import DRIVER_CASES, check_optimum, run_driver
from test_hip_forces_hessp import estate, problem
from test_hip_strip_loops import data as loop_data, enter_regime, on_thread_ranks

from bioen_amd.optimize import forces

pytestmark = pytest.mark.gpu

THETAS = (0.1, 10.0, 1000.0)
CAP = 1e-3            # (i) against the FP64 pass, of max|H| (max|C|): what split-BF16 operands may cost (tests/test_forces_gram_bf16.py);
#                       measured 1.3e-6 ... 5.2e-6, and 1.6e-4 on 808 x 10, whose offset the rank corrections take off
REST = 2e-5           # (ii) against the restatement: f32 accumulation order and a few flipped last bits of lo are all that is left;
#                       measured <= 9.5e-8, and 1.1e-6 on 808 x 10
# tests/test_hip_forces_gram.py's shapes -- 7 x 37: rows padded to 16, redirected row blocks, a ragged last strip, three
# strips over eight segments; 808 x 10: one strip, empty segments, the offset golden's shape; 129 x 257: a second tile of one
# row block; 64 x 2000: one full slice; 513 x 1537: nine slices, sets of several strips; 1024 x 528: every tile full
SHAPES = [(7, 37), (808, 10), (129, 257), (64, 2000), (513, 1537), (1024, 528)]


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()


def held_to_both(ctx, Cb, Hb, restated, label):
    """C~ and H~ of forces_gram_bf16 against the FP64 pass at the same kept point (i) and against the restatement (ii)"""
    C, H = ctx.forces_gram()
    Cr, Hr = restated
    S, SC = float(np.abs(H).max()), float(np.abs(C).max())
    ih, ic = np.abs(Hb - H).max() / S, np.abs(Cb - C).max() / SC
    rh, rc = np.abs(Hb - Hr).max() / S, np.abs(Cb - Cr).max() / SC
    print("%s: (i) |H~ - H| = %.3g max|H|, |C~ - C| = %.3g max|C|; (ii) |H~ - H~_restated| = %.3g max|H|, |C~ - C~_restated| "
          "= %.3g max|C|" % (label, ih, ic, rh, rc))
    assert np.array_equal(Hb, Hb.T) and np.array_equal(Cb, Cb.T)
    assert ih <= CAP and ic <= CAP
    assert rh <= REST and rc <= REST
    assert ih > 0.0                                  # the split products, not the FP64 pass under another name


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_against_the_fp64_pass_and_the_restatement(bioen_amd, shape):
    """at the forces of tests/test_hip_forces_hessp.py's problem(): weights over decades, not an optimum; every theta"""
    yT, YT, w0, f, _ = problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        for theta in THETAS:
            f0, g0 = ctx.forces_fdf(f, w0, theta)
            Cb, Hb, fv, grad = ctx.forces_gram_bf16(forces=f, w0=w0, theta=theta)
            assert fv == f0 and np.array_equal(grad, g0)                 # the point-setting call is forces_fdf's evaluation
            restated = forces.hessian_gram_bf16_bioen_log_posterior_base(f, w0, yT, YT, theta)
            held_to_both(ctx, Cb, Hb, restated, "%dx%d theta %g" % (shape + (theta,)))


def test_where_a_set_runs_several_strips_of_its_segment(bioen_amd, monkeypatch):
    """300 x 9000 with ONE canonical segment (tests/test_hip_strip_loops.py's regime): 86 groups of 6 or 7 strips"""
    shape = (300, 9000)
    enter_regime(monkeypatch, shape)
    yT, YT, G, w0, f, x = loop_data(shape)
    f = f / 5.0                                                 # x with standard deviation 1
    with bioen_amd.Context(yT, YT) as ctx:
        assert ctx.strip_plan(1)["local_segments"] == 1
        for theta in THETAS:
            Cb, Hb, _, _ = ctx.forces_gram_bf16(forces=f, w0=w0, theta=theta)
            restated = forces.hessian_gram_bf16_bioen_log_posterior_base(f, w0, yT, YT, theta)
            held_to_both(ctx, Cb, Hb, restated, "300x9000, one segment, theta %g" % theta)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_bitwise_invariants(bioen_amd, shape):
    yT, YT, w0, f, pool = problem(shape)
    theta = 10.0
    with bioen_amd.Context(yT, YT) as ctx:
        C, H, fv, grad = ctx.forces_gram_bf16(forces=f, w0=w0, theta=theta)         # sets the point
        assert np.array_equal(H, H.T) and np.array_equal(C, C.T)
        for _ in range(2):                                                          # serves it: the same bits, call after call
            C2, H2 = ctx.forces_gram_bf16()
            assert np.array_equal(C2, C) and np.array_equal(H2, H)
        only_c, none = ctx.forces_gram_bf16(hess=False)
        assert none is None and np.array_equal(only_c, C)
        none, only_h = ctx.forces_gram_bf16(cov=False)
        assert none is None and np.array_equal(only_h, H)
        hv = ctx.forces_hessp(pool[:3])                                             # the products' point is this one
        ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)                        # ... and a point they set serves the pass
        C3, H3 = ctx.forces_gram_bf16()
        assert np.array_equal(C3, C) and np.array_equal(H3, H)
        assert np.array_equal(ctx.forces_hessp(pool[:3]), hv)
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))                       # (o, s) = (0, 1): the plain model's bits
        C4, H4, f4, g4 = ctx.forces_gram_bf16(forces=f, w0=w0, theta=theta)
        assert f4 == fv and np.array_equal(g4, grad)
        assert np.array_equal(C4, C) and np.array_equal(H4, H)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_with_an_affine_model(bioen_amd, shape):
    """row offsets and scales set on the context: held to (i) against forces_gram on the same model"""
    yT, YT, w0, f, _ = problem(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        Cb, Hb, _, _ = ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0)
        C, H = ctx.forces_gram()
        ih, ic = np.abs(Hb - H).max() / np.abs(H).max(), np.abs(Cb - C).max() / np.abs(C).max()
        print("affine %dx%d: (i) |H~ - H| = %.3g max|H|, |C~ - C| = %.3g max|C|" % (shape + (ih, ic)))
        assert np.array_equal(Hb, Hb.T) and np.array_equal(Cb, Cb.T)
        assert 0.0 < ih <= CAP and ic <= CAP


def test_the_fp64_pass_keeps_its_bits_beside_this_one(bioen_amd):
    yT, YT, w0, f, _ = problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        C, H, _, _ = ctx.forces_gram(forces=f, w0=w0, theta=10.0)                   # alone
    with bioen_amd.Context(yT, YT) as ctx:
        Cb, Hb, _, _ = ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0)
        C2, H2 = ctx.forces_gram()                                                  # after the BF16 pass, at its point
        assert np.array_equal(C2, C) and np.array_equal(H2, H)
        Cb2, Hb2 = ctx.forces_gram_bf16()                                           # ... and the other way round
        assert np.array_equal(Cb2, Cb) and np.array_equal(Hb2, Hb)


def test_refusals_leave_the_point_alone(bioen_amd):
    from test_entry_effects import P
    yT, YT, w0, f, pool = problem((64, 2000))
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.forces_gram_bf16(), "no point on this context", "bioen_hip_forces_gram_bf16")
        C, H, _, _ = ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0)
        hv = ctx.forces_hessp(pool[0])
        ctx.forces_fdf(f, w0, 10.0)                                  # after an evaluation
        estate(lambda: ctx.forces_gram_bf16(), "is gone", "bioen_hip_forces_fdf")
        ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0, cov=False, hess=False)      # only sets the point
        # rejected for its arguments: the point stays
        from bioen_amd import _lib
        assert _lib.lib().bioen_hip_forces_gram_bf16(ctx._h, _lib.ptr(f), None, 10.0, None, None, None, None) == -1
        assert _lib.lib().bioen_hip_forces_gram_bf16(ctx._h, None, None, 0.0, None, None, None, None) == -1
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)
        ctx.set_affine(np.zeros(64), np.ones(64))                     # drops the point
        estate(lambda: ctx.forces_gram_bf16(), "is gone", "bioen_hip_ctx_set_affine")
        ctx.set_storage("fp32")                                       # set_storage(2): the reduced-storage copies
        estate(lambda: ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram_bf16", "reduced-storage")
        ctx.set_storage("f64")
        C2, H2, _, _ = ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0)
        assert np.array_equal(C2, C) and np.array_equal(H2, H)
    p = P.get()                                                      # on a log-weights point
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        estate(lambda: ctx.forces_gram_bf16(), "log-weights point", "bioen_hip_forces_gram_bf16")
        assert np.array_equal(ctx.logw_hessp(p.v), hl)
    yT, YT, w0, f, pool = problem((1100, 2000))                      # row panels
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_gram_bf16(), "bioen_hip_forces_gram_bf16", "M <= 1024")
        estate(lambda: ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram_bf16", "M <= 1024")
        assert np.array_equal(ctx.forces_hessp(pool[0]), hv)
        assert "forces_gram_bf16" not in ctx.footprint()[0]


def test_refused_without_the_strip_copies(bioen_amd, monkeypatch):
    """the streaming fallback (the strip copies' allocation fails: tests/test_hip_forces_colquad.py's way there)"""
    yT, YT, w0, f, _ = problem((64, 2000))
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")
    with bioen_amd.Context(yT, YT) as ctx:
        f0, _ = ctx.forces_fdf(f, w0, 10.0)                          # the evaluation itself is served there
        assert np.isfinite(f0) and ctx.footprint()[0] == {"rowmajor"}
        estate(lambda: ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram_bf16", "strip copies")
        assert "forces_gram_bf16" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, w0, f, pool = problem((129, 1000))

    def workload(ctx, local_segments):
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        estate(lambda: ctx.forces_gram_bf16(), "bioen_hip_forces_gram_bf16", "structure-sharded")
        estate(lambda: ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0), "bioen_hip_forces_gram_bf16", "structure-sharded")
        return np.array_equal(ctx.forces_hessp(pool[0]), hv)

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))


def test_the_buffer_is_in_the_footprint_and_goes_with_the_context(bioen_amd):
    yT, YT, w0, f, _ = problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.forces_gram_bf16(forces=f, w0=w0, theta=10.0, cov=False, hess=False)    # sets the point, computes nothing
        forms, before = ctx.footprint()
        assert "forces_gram_bf16" not in forms                       # allocated at the first computing call, not before
        ctx.forces_gram_bf16()
        forms, with_buffer = ctx.footprint()
        assert "forces_gram_bf16" in forms and "forces_gram" not in forms
        assert with_buffer - before >= 2 * 129 * 129 * 8
        ctx.forces_gram_bf16()
        assert ctx.footprint() == (forms, with_buffer)               # ... once
    with bioen_amd.Context(yT, YT) as ctx:                           # a new context starts without one
        assert "forces_gram_bf16" not in ctx.footprint()[0]


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_trust_exact_with_the_bf16_hessian_on_the_device(bioen_amd, name):
    """the project's parity numbers against the hessian=gram run: fmin within 1e-6, the weights within 1e-5 max w"""
    d, out = run_driver(name, "trust_exact", True, mod="scipy:gtol=1e-6,scipy:hessian=gram_bf16")
    check_optimum(d, out)
    _, gram = run_driver(name, "trust_exact", True, mod="scipy:gtol=1e-6,scipy:hessian=gram")
    dw = np.abs(np.asarray(out[0]).reshape(-1) - np.asarray(gram[0]).reshape(-1)).max()
    print("%s: fmin - fmin_gram = %.3g, max |dw| = %.3g max w" % (name, out[4] - gram[4], dw / np.abs(gram[0]).max()))
    assert abs(out[4] - gram[4]) <= 1e-6
    assert dw <= 1e-5 * np.abs(gram[0]).max()

"""GPU tests of the log-weights method's dual Newton minimizer (csrc/kernels_logw_newton.hip, csrc/api_logw_newton.cpp,
Context.logw_cov / opt_dual_newton_logw): the covariance pass against the centred formula in
numpy.longdouble on the geometry list of tests/test_hip_forces_gram.py and against forces_gram's C for the same weights, its
bitwise invariants, canonical segments and the affine model; the loop through find_optimum against its numpy restatement;
the state rules, the refusals and the footprint."""
import numpy as np
import pytest

from conftest import LBFGS_DEFAULTS, load_golden
from test_hip_forces_gram import GATE, SHAPES as GRAM_SHAPES, _gram_ld
from test_hip_forces_hessp import estate, problem
from test_hip_strip_loops import data as loop_data, enter_regime, on_thread_ranks
from test_logw_dual_newton import GOOD, RANDOM_START, check_against_golden, host_dual_newton

from bioen_amd.optimize import log_weights, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

L = np.longdouble
# tests/test_hip_forces_gram.py's geometry list as it stands (it has M = 1024), and M = 1
SHAPES = GRAM_SHAPES + [(1, 37)]
THETA = 10.0


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    c_bioen.clear_cache()


def logw_problem(shape):
    """-> yTilde, YTilde, G (log prior), g: the point G + x, x = yTilde^T f with standard deviation 1 (weights over a few
    decades, not an optimum)"""
    if shape == (1, 37):
        rng = np.random.default_rng(137)
        yT, YT, w0 = rng.standard_normal((1, 37)) + 3.0, rng.standard_normal(1) + 3.0, rng.uniform(0.5, 1.5, 37)
        w0 /= w0.sum()
        f = np.array([1.0 / yT.std()])
    else:
        yT, YT, w0, f, _ = problem(shape)
    G = np.log(w0)
    return yT, YT, G, G + f @ yT


_LD = {}


def cov_longdouble(key, A, g):
    """C = sum_j w_j (a_j - abar)(a_j - abar)^T, w = softmax(g), in numpy.longdouble, once per problem"""
    if key not in _LD:
        gl = g.astype(L)
        e = np.exp(gl - gl.max())
        w = e / e.sum()
        a = A - (A @ w)[:, None]
        _LD[key] = _gram_ld(a, w).astype(np.float64)
    return _LD[key]


def held(C, ref, label):
    S = float(np.abs(ref).max())
    d = np.abs(C - ref).max() / S
    print("%s: |C - C_ld| = %.3g max|C|" % (label, d))
    assert np.array_equal(C, C.T)
    assert d <= GATE


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_cov_against_longdouble(bioen_amd, shape):
    yT, YT, G, g = logw_problem(shape)
    ref = cov_longdouble(shape, yT.astype(L), g)
    with bioen_amd.Context(yT, YT) as ctx:
        f0, g0 = ctx.logw_fdf(g, G, THETA)
        C, fv, grad = ctx.logw_cov(g=g, G=G, theta=THETA)
        assert fv == f0 and np.array_equal(grad, g0)                     # the point-setting call is logw_fdf's evaluation
        held(C, ref, "%dx%d" % shape)
        for _ in range(2):                                               # serves the kept point: the same bits, call after call
            assert np.array_equal(ctx.logw_cov(), C)
        hv = ctx.logw_hessp(np.ones(shape[1]))                           # the products' point is this one ...
        ctx.logw_hessp(None, g=g, G=G, theta=THETA)                      # ... and a point they set serves the pass
        assert np.array_equal(ctx.logw_cov(), C)
        assert np.array_equal(ctx.logw_hessp(np.ones(shape[1])), hv)
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))            # (o, s) = (0, 1): the plain model's bits
        assert np.array_equal(ctx.logw_cov(g=g, G=G, theta=THETA)[0], C)


@pytest.mark.parametrize("shape", [(7, 37), (129, 257), (513, 1537)], ids=["7x37", "129x257", "513x1537"])
def test_cov_equals_forces_grams_at_the_same_weights(bioen_amd, shape):
    """g = G against forces = 0 with w0 = softmax(G): the same weights, two kernels"""
    yT, YT, G, _ = logw_problem(shape)
    w0 = np.exp(G - G.max())
    w0 /= w0.sum()
    with bioen_amd.Context(yT, YT) as ctx:
        fg_before = ctx.forces_gram(forces=np.zeros(shape[0]), w0=w0, theta=THETA)
        C, _, _ = ctx.logw_cov(g=G, G=G, theta=THETA)
        d = np.abs(C - fg_before[0]).max() / np.abs(fg_before[0]).max()
        print("%dx%d: |C_logw - C_forces| = %.3g max|C|" % (shape + (d,)))
        assert d <= GATE
        fg_after = ctx.forces_gram(forces=np.zeros(shape[0]), w0=w0, theta=THETA)      # forces_gram's bits stay what they are
        assert all(np.array_equal(a, b) for a, b in zip(fg_before, fg_after))


@pytest.mark.parametrize("segments", (1, 8))
@pytest.mark.parametrize("shape", [(513, 1537), (300, 9000)], ids=["513x1537", "300x9000"])
def test_cov_with_one_canonical_segment_and_with_eight(bioen_amd, monkeypatch, shape, segments):
    """BIOEN_HIP_SEGMENTS is honoured; 300 x 9000 on one segment: sets of 6 or 7 strips (tests/test_hip_strip_loops.py)"""
    if shape == (300, 9000):
        yT, YT, G, w0, f, x = loop_data(shape)
        g = G + x / 5.0
    else:
        yT, YT, G, g = logw_problem(shape)
    ref = cov_longdouble(("seg", shape), yT.astype(L), g)
    if segments == 1:
        monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")
    with bioen_amd.Context(yT, YT) as ctx:
        assert ctx.strip_plan(0)["local_segments"] == segments
        C, _, _ = ctx.logw_cov(g=g, G=G, theta=THETA)
        held(C, ref, "%dx%d, %d segment(s)" % (shape + (segments,)))
        assert np.array_equal(ctx.logw_cov(), C)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537)], ids=["129x257", "513x1537"])
def test_cov_with_an_affine_model(bioen_amd, shape):
    """row offsets and scales set on the context; the test folds them into its own matrix"""
    yT, YT, G, g = logw_problem(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    eff = off[:, None].astype(L) + sc[:, None].astype(L) * yT.astype(L)
    ref = cov_longdouble(("affine", shape), eff, g)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        C, _, _ = ctx.logw_cov(g=g, G=G, theta=THETA)
        held(C, ref, "affine %dx%d" % shape)


# ---- the loop ---------------------------------------------------------------------------------------
def device_dual_newton(d, g0, mod=""):
    cfg = minimize.Parameters("dual_newton", mod)
    cfg.update(verbose=False)
    out = log_weights.find_optimum(np.asarray(g0, dtype=np.float64).reshape(-1, 1), d["G"], d["y"], d["yTilde"],
                                   d["YTilde"].reshape(1, -1), d["theta"], cfg)
    return out, dict(c_bioen.last_opt_info)


@pytest.mark.parametrize("name,random_start", [(n, False) for n in GOOD] + [(RANDOM_START, True)])
def test_driver_through_find_optimum(bioen_amd, name, random_start):
    d, g0, host = host_dual_newton(name, random_start)
    out, info = device_dual_newton(d, g0)
    print("%s: device %d iterations / %d evaluations / %d factorisations, status %d, gmax %.3g wmax; restatement %d / %d / %d; "
          "fmin device %.15g, restatement %.15g"
          % (name, info["iterations"], info["evaluations"], info["factorisations"], info["status"], info["gmax"] / info["wmax"],
             host["iterations"], host["evaluations"], host["factorisations"], out[4], host["fmin"]))
    assert (info["iterations"], info["evaluations"], info["factorisations"]) == \
        (host["iterations"], host["evaluations"], host["factorisations"])
    assert abs(out[4] - host["fmin"]) <= 1e-9 * abs(host["fmin"])
    check_against_golden(d, dict(info, g=out[2]))


def test_a_run_leaves_the_other_entries_bits_alone_and_its_optimum_as_the_point(bioen_amd):
    d, g0, host = host_dual_newton("synth_logw_M64xN2000.npz")
    yT, YT, G, theta = d["yTilde"], d["YTilde"].reshape(-1), d["G"].reshape(-1), float(d["theta"])
    w0 = np.exp(G - G.max())
    w0 /= w0.sum()
    f = 1e-3 * np.random.default_rng(3).standard_normal(yT.shape[0])
    v = np.random.default_rng(1).standard_normal(yT.shape[1])
    params = dict(LBFGS_DEFAULTS, max_iterations=20)
    with bioen_amd.Context(yT, YT) as fresh:
        lb_fresh = fresh.opt_lbfgs_logw(g0, G, theta, params)
    with bioen_amd.Context(yT, YT) as ctx:
        fdf = ctx.logw_fdf(g0, G, theta)
        fg = ctx.forces_gram(forces=f, w0=w0, theta=theta)
        res = ctx.opt_dual_newton_logw(g0, G, theta)
        assert res["status"] == 0 and res["iterations"] == host["iterations"]
        # the optimum is the kept point: the covariance and a product are served at once, with the bits of a call that sets it
        C, hv = ctx.logw_cov(), ctx.logw_hessp(v)
        C2, f2, grad2 = ctx.logw_cov(g=res["g"], G=G, theta=theta)
        assert np.array_equal(C, C2) and f2 == res["fmin"] and np.abs(grad2).max() == res["gmax"]
        assert np.array_equal(ctx.logw_hessp(v), hv)
        ctx.logw_fdf(g0, G, theta)                                       # an evaluation in between drops it
        estate(lambda: ctx.logw_cov(), "is gone", "bioen_hip_logw_fdf")
        estate(lambda: ctx.logw_hessp(v), "is gone", "bioen_hip_logw_fdf")
        fdf2 = ctx.logw_fdf(g0, G, theta)
        assert fdf2[0] == fdf[0] and np.array_equal(fdf2[1], fdf[1])
        fg2 = ctx.forces_gram(forces=f, w0=w0, theta=theta)
        assert all(np.array_equal(a, b) for a, b in zip(fg, fg2))
        lb = ctx.opt_lbfgs_logw(g0, G, theta, params)                    # the L-BFGS after it: its usual bits
        assert np.array_equal(lb[0], lb_fresh[0]) and np.array_equal(lb[1], lb_fresh[1]) and lb[2].fmin == lb_fresh[2].fmin


def test_max_iterations_raises_with_the_return_code(bioen_amd):
    d = load_golden("synth_logw_M37xN500.npz")
    with pytest.raises(RuntimeError, match="return code 1"):
        device_dual_newton(d, d["GInit"], "dual_newton:max_iterations=1")


def test_refusals(bioen_amd, monkeypatch):
    from bioen_amd._lib import BioenHipError
    yT, YT, G, g = logw_problem((64, 2000))
    calls = ((lambda c: c.logw_cov(g=g, G=G, theta=THETA), "bioen_logwn_cov"),
             (lambda c: c.opt_dual_newton_logw(g, G, THETA), "bioen_logwn_opt"))
    with bioen_amd.Context(yT, YT) as ctx:
        estate(lambda: ctx.logw_cov(), "no point on this context", "bioen_logwn_cov")
        for theta in (0.0, -1.0, float("nan")):                          # theta <= 0: the step divides by it
            with pytest.raises(BioenHipError, match="theta > 0"):
                ctx.opt_dual_newton_logw(g, G, theta)
        ctx.set_storage("fp32")                                          # the reduced-storage copies
        for call, name in calls:
            estate(lambda: call(ctx), name, "reduced-storage")
        ctx.set_storage("f64")
        assert "logw_gram" not in ctx.footprint()[0]
    t = problem((1100, 2000))                                            # row panels
    with bioen_amd.Context(t[0], t[1]) as ctx:
        Gt = np.log(t[2])
        for name, call in (("bioen_logwn_cov", lambda: ctx.logw_cov(g=Gt, G=Gt, theta=THETA)),
                           ("bioen_logwn_opt", lambda: ctx.opt_dual_newton_logw(Gt, Gt, THETA))):
            estate(call, name, "M <= 1024")
        assert "logw_gram" not in ctx.footprint()[0]
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")           # the streaming fallback: no strip copies
    with bioen_amd.Context(yT, YT) as ctx:
        f0, _ = ctx.logw_fdf(g, G, THETA)                                # the evaluation itself is served there
        assert np.isfinite(f0) and ctx.footprint()[0] == {"rowmajor"}
        for call, name in calls:
            estate(lambda: call(ctx), name, "strip copies")
        assert "logw_gram" not in ctx.footprint()[0]


def test_refused_on_a_sharded_context(bioen_amd):
    yT, YT, G, g = logw_problem((129, 1000))

    def workload(ctx, local_segments):
        estate(lambda: ctx.logw_cov(g=g, G=G, theta=THETA), "bioen_logwn_cov", "structure-sharded")
        estate(lambda: ctx.opt_dual_newton_logw(g, G, THETA), "bioen_logwn_opt", "structure-sharded")
        return True

    assert all(on_thread_ranks(bioen_amd, 2, yT, YT, workload))


def test_the_buffer_is_in_the_footprint_and_goes_with_the_context(bioen_amd):
    yT, YT, G, g = logw_problem((129, 257))
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.logw_cov(g=g, G=G, theta=THETA, cov=False)                   # only sets the point
        forms, before = ctx.footprint()
        assert "logw_gram" not in forms                                  # allocated at the first use, not before
        ctx.logw_cov()
        forms, with_buffer = ctx.footprint()
        assert "logw_gram" in forms and with_buffer - before >= 129 * 129 * 8
        ctx.logw_cov()
        assert ctx.footprint() == (forms, with_buffer)                   # ... once
    with bioen_amd.Context(yT, YT) as ctx:
        assert "logw_gram" not in ctx.footprint()[0]

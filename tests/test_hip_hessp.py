"""GPU tests of the Hessian-vector products of the log-weights objective (csrc/kernels_hessp.hip, csrc/api_hessp.cpp,
Context.logw_hessp) and of scipy's Newton-CG drivers on the device objective: the product against an independent
extended-precision evaluation of the formula on every pass family, the bitwise invariants, the point's state rule, the
launch counts behind "a product costs a gradient", eight thread-ranks, and the drivers through find_optimum."""
import numpy as np
import pytest

from conftest import load_golden, tall_forces_problem
from test_hessp import check_optimum, host_run, run_driver

pytestmark = pytest.mark.gpu

L = np.longdouble
THETAS = (0.1, 10.0, 1000.0)
WIDTHS = (1, 3, 5, 8)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()


def recipe(M, N, seed):
    """SURVEY 8(d)'s recipe, non-uniform prior"""
    rng = np.random.default_rng(seed)
    YTrue = rng.uniform(1, 10, M)
    sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
    YTilde = rng.normal(YTrue, sig_exp) / sig_exp
    yTilde = rng.normal(YTrue[:, None], sig_sim[:, None], (M, N)) / sig_exp[:, None]
    w0 = rng.uniform(0.5, 1.5, N)
    return yTilde, YTilde, np.log(w0 / w0.sum())


def problem(shape):
    M, N = shape
    if shape == (205, 10):
        d = load_golden("ref_data_potra_part_2_logw_M205xN10.npz")
        yT, YT, G = np.asarray(d["yTilde"], dtype=np.float64), d["YTilde"].reshape(-1), d["G"].reshape(-1)
    elif shape == (1100, 2000):
        t = tall_forces_problem()
        yT, YT, G = t["yTilde"], t["YTilde"], np.zeros(N)
    else:
        yT, YT, G = recipe(M, N, 1000 * M + N)
    assert yT.shape == shape
    rng = np.random.default_rng(77 + M)
    x = G + 0.3 * rng.standard_normal(N)
    pool = rng.standard_normal((8, N))
    pool[6] = 1.0                       # v = 1: H 1 = 0
    pool[7] = 0.0
    pool[7, N // 3] = 1.0               # a unit vector: one column of H
    return yT, YT, G, x, pool


def hessp_longdouble(yT, YT, G, x, theta, V):
    """the formula of DESIGN section 6b in numpy.longdouble, written out here on its own"""
    y = yT.astype(L)
    xl, Gl, Yl = x.astype(L), G.astype(L), YT.astype(L)
    e = np.exp(xl - xl.max())
    w = e / e.sum()
    ybar = y.dot(w)
    r = ybar - Yl
    adj = y.T.dot(r) - ybar.dot(r)
    dev = xl - Gl
    grad = w * (L(theta) * (dev - w.dot(dev)) + adj)
    out = []
    for v in V.astype(L):
        dv = v - w.dot(v)
        dr = y.dot(w * dv)
        c = y.T.dot(dr) - ybar.dot(dr)
        out.append(dv * grad + w * (L(theta) * dv + c - v.dot(grad)))
    return np.array(out), grad


def directions(pool, k):
    return pool[8 - k:]                 # k = 1: the unit vector; k >= 3: with v = 1 and normals


SHAPES = [(7, 37), (205, 10), (129, 257), (64, 2000), (513, 1537), (1100, 2000)]
CASES = [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES if s[0] <= 1024]


@pytest.mark.parametrize("shape,one_copy", CASES, ids=["%dx%d%s" % (s[0], s[1], "-onecopy" if o else "") for s, o in CASES])
def test_product_against_the_formula_in_longdouble(bioen_amd, shape, one_copy):
    """max |hv_dev - hv_ld| <= 1e-10 S, S = the largest |Hv| entry over the case's directions: the gate the gradient is
    held to.  Every theta, every batch width (widths above 4 take other strip forms), the context's default form and one
    strip copy."""
    yT, YT, G, x, pool = problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        if one_copy:
            ctx.set_one_copy(True)
        for theta in THETAS:
            ref, gref = hessp_longdouble(yT, YT, G, x, theta, pool)
            S = float(np.abs(ref).max())
            hv, f, grad = ctx.logw_hessp(pool, g=x, G=G, theta=theta)          # sets the point, k = 8
            assert np.abs(grad - gref).max() <= 1e-10 * float(np.abs(gref).max())
            worst = float(np.abs(hv - ref).max())
            for k in WIDTHS:
                got = ctx.logw_hessp(directions(pool, k) if k > 1 else pool[7])
                want = ref[8 - k:] if k > 1 else ref[7]
                assert got.shape == want.shape
                worst = max(worst, float(np.abs(got - want).max()))
            print("%s theta %g: max |hv - ld| = %.3g S (S = %.3g)" % (shape, theta, worst / S, S))
            assert worst <= 1e-10 * S


@pytest.mark.parametrize("one_copy", [False, True], ids=["twocopy", "onecopy"])
def test_product_with_an_affine_model(bioen_amd, one_copy):
    """row offsets and scales set on the context; the test folds them into its own matrix"""
    yT, YT, G, x, pool = problem((129, 257))
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, 129), rng.uniform(0.5, 1.5, 129)
    eff = off[:, None].astype(L) + sc[:, None].astype(L) * yT.astype(L)
    theta = 10.0
    with bioen_amd.Context(yT, YT) as ctx:
        if one_copy:
            ctx.set_one_copy(True)
        ctx.set_affine(off, sc)
        ref, _ = hessp_longdouble(eff, YT, G, x, theta, pool[5:])
        S = float(np.abs(ref).max())
        hv, _, _ = ctx.logw_hessp(pool[5:], g=x, G=G, theta=theta)
        print("affine: max |hv - ld| = %.3g S" % (float(np.abs(hv - ref).max()) / S))
        assert np.abs(hv - ref).max() <= 1e-10 * S


@pytest.mark.parametrize("shape", [(129, 257), (1100, 2000)], ids=["129x257", "1100x2000"])
def test_product_on_the_streaming_fallback(bioen_amd, monkeypatch, shape):
    """BIOEN_HIP_FWD_STREAM=1 (read when the context is created): the row-major streaming pair serves the evaluation and
    the product -- same gate, every theta and width, an affine model on top for the smaller shape"""
    monkeypatch.setenv("BIOEN_HIP_FWD_STREAM", "1")
    yT, YT, G, x, pool = problem(shape)
    rng = np.random.default_rng(8)
    affine = shape[0] <= 1024
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    eff = off[:, None].astype(L) + sc[:, None].astype(L) * yT.astype(L) if affine else yT
    with bioen_amd.Context(yT, YT) as ctx:
        if affine:
            ctx.set_affine(off, sc)
        ctx.kernel_stats_enable(True)
        for theta in THETAS:
            ref, gref = hessp_longdouble(eff, YT, G, x, theta, pool)
            S = float(np.abs(ref).max())
            hv, f, grad = ctx.logw_hessp(pool, g=x, G=G, theta=theta)
            assert np.abs(grad - gref).max() <= 1e-10 * float(np.abs(gref).max())
            worst = float(np.abs(hv - ref).max())
            for k in WIDTHS:
                got = ctx.logw_hessp(directions(pool, k))
                worst = max(worst, float(np.abs(got - ref[8 - k:]).max()))
                assert np.array_equal(got, hv[8 - k:])              # the batch invariant on this pass family too
            print("streaming %s theta %g: max |hv - ld| = %.3g S" % (shape, theta, worst / S))
            assert worst <= 1e-10 * S
        ctx.kernel_stats_reset()
        ctx.logw_hessp(pool[:3])
        st = ctx.kernel_stats()
        assert (st["forward"]["launches"], st["adjoint"]["launches"]) == (1, 1)     # one streaming launch each, no row panels


@pytest.mark.parametrize("which", ["M64xN2000", "tall"])
def test_bitwise_invariants(bioen_amd, which):
    if which == "tall":
        yT, YT, G, x, pool = problem((1100, 2000))
        theta = 100.0
    else:
        d = load_golden("synth_logw_M64xN2000.npz")
        yT, YT, G, theta = d["yTilde"], d["YTilde"].reshape(-1), d["G"].reshape(-1), float(d["theta"])
        rng = np.random.default_rng(11)
        x = d["GInit"].reshape(-1) + 0.2 * rng.standard_normal(G.size)
        pool = rng.standard_normal((8, G.size))
    with bioen_amd.Context(yT, YT) as ctx:
        f0, g0 = ctx.logw_fdf(x, G, theta)
        hv8, f, grad = ctx.logw_hessp(pool, g=x, G=G, theta=theta)
        assert f == f0 and np.array_equal(grad, g0)                 # the point-setting call is logw_fdf's evaluation
        again = ctx.logw_hessp(pool)                                # at the kept point
        assert np.array_equal(again, hv8)
        for a in range(8):                                          # eight single calls
            assert np.array_equal(ctx.logw_hessp(pool[a]), hv8[a]), a
        assert np.array_equal(ctx.logw_hessp(pool[2:5]), hv8[2:5])
        hv8b, fb, gradb = ctx.logw_hessp(pool, g=x, G=G, theta=theta)
        assert fb == f and np.array_equal(gradb, grad) and np.array_equal(hv8b, hv8)


def test_the_point_is_dropped_by_other_calls(bioen_amd):
    from bioen_amd._lib import BioenHipError
    d = load_golden("synth_logw_M64xN2000.npz")
    G, theta = d["G"].reshape(-1), float(d["theta"])
    x = d["GInit"].reshape(-1)
    n, m = G.size, d["yTilde"].shape[0]
    v = np.random.default_rng(1).standard_normal(n)
    w0 = np.full(n, 1.0 / n)
    with bioen_amd.Context(d["yTilde"], d["YTilde"]) as ctx:
        with pytest.raises(BioenHipError) as e:                     # no point yet
            ctx.logw_hessp(v)
        assert "(-6)" in str(e.value)
        others = [lambda: ctx.logw_fdf(x, G, theta), lambda: ctx.logw_weights(x),
                  lambda: ctx.set_target(d["YTilde"].reshape(-1)), lambda: ctx.forces_fdf(np.zeros(m), w0, theta)]
        for other in others:
            hv, _, _ = ctx.logw_hessp(v, g=x, G=G, theta=theta)
            assert np.array_equal(ctx.logw_hessp(v), hv)
            other()
            with pytest.raises(BioenHipError) as e:
                ctx.logw_hessp(v)
            assert "(-6)" in str(e.value) and "is gone" in str(e.value)
        hv2, _, _ = ctx.logw_hessp(v, g=x, G=G, theta=theta)       # with g it works again
        assert np.array_equal(hv2, hv)
        ctx.kernel_stats_enable(True)
        ctx.kernel_stats_reset()
        with pytest.raises((ValueError, BioenHipError)):
            ctx.logw_hessp(np.zeros((9, n)))
        with pytest.raises((ValueError, BioenHipError)):
            ctx.logw_hessp(np.zeros(n + 1))
        st = ctx.kernel_stats()
        assert all(st[key]["launches"] == 0 for key in st)          # rejected before the device is touched
        assert np.array_equal(ctx.logw_hessp(v), hv)                # ... and the point is still there


@pytest.mark.parametrize("shape,panels", [((64, 2000), 1), ((1100, 2000), 2)])
def test_a_product_costs_one_forward_and_one_adjoint_pass(bioen_amd, shape, panels):
    yT, YT, G, x, pool = problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.logw_hessp(pool[0], g=x, G=G, theta=10.0)               # the strip copies exist from here on
        ctx.kernel_stats_enable(True)

        def launches(call):
            ctx.kernel_stats_reset()
            call()
            st = ctx.kernel_stats()
            return st["forward"]["launches"], st["adjoint"]["launches"]

        for k in WIDTHS:
            assert launches(lambda: ctx.logw_hessp(pool[:k])) == (panels, panels), k
        assert launches(lambda: ctx.logw_hessp(pool[0], g=x, G=G, theta=10.0)) == (2 * panels, 2 * panels)
        assert launches(lambda: ctx.logw_fdf(x, G, 10.0)) == (panels, panels)       # the yardstick: a gradient


@pytest.mark.timeout(600)
def test_eight_thread_ranks_equal_the_single_context(bioen_amd):
    import threading
    from bioen_amd import sweep
    world = 8
    d = load_golden("synth_logw_M64xN2000.npz")
    G, theta = d["G"].reshape(-1), float(d["theta"])
    rng = np.random.default_rng(99)
    x = d["GInit"].reshape(-1) + 0.2 * rng.standard_normal(G.size)
    V = rng.standard_normal((3, G.size))

    def workload(ctx):
        hv1, f, grad = ctx.logw_hessp(V[0], g=x, G=G, theta=theta)
        return {"hv1": hv1, "f": f, "grad": grad, "hv3": ctx.logw_hessp(V)}

    with bioen_amd.Context(d["yTilde"], d["YTilde"]) as ctx:
        single = workload(ctx)
    comms = sweep.ThreadComm.create(world)
    results, errors = [None] * world, [None] * world

    def rank_main(r):
        try:
            ctx = bioen_amd.Context(d["yTilde"], d["YTilde"], device=0, rank=r, world=world)
            try:
                ctx.set_exchange(comms[r])
                results[r] = workload(ctx)
            finally:
                ctx.close()
        except BaseException as e:          # noqa: B902 -- reported below; the other ranks leave through the barrier's bound
            errors[r] = e
            try:
                comms[r]._s.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=500)
    assert not any(t.is_alive() for t in threads), "a rank did not finish"
    assert all(e is None for e in errors), errors
    for r in range(world):
        for key, val in single.items():
            assert np.array_equal(np.asarray(results[r][key]), np.asarray(val)), (r, key)


DRIVER_CASES = [("trust_ncg", n) for n in ("ref_data_16x15.npz", "synth_logw_M37xN500.npz", "synth_logw_M129xN257.npz",
                                           "ref_data_potra_part_2_logw_M205xN10.npz")] + \
               [("newton_cg", n) for n in ("ref_data_16x15.npz", "synth_logw_M37xN500.npz", "synth_logw_M129xN257.npz",
                                           "synth_logw_M64xN2000.npz")]


@pytest.mark.parametrize("algorithm,name", DRIVER_CASES)
def test_drivers_on_the_device_objective(bioen_amd, algorithm, name):
    """the pairs and gates of tests/test_hessp.py on the device objective, against the reference's converged optimum and
    against the numpy-objective run (not bitwise: the two sum in different orders)"""
    mod = "scipy:gtol=1e-9" if algorithm == "trust_ncg" else "scipy:xtol=1e-10"
    d, out = run_driver(name, algorithm, mod, True)
    check_optimum(d, out)
    _, host = host_run(name, algorithm)
    assert abs(out[4] - host[4]) <= 1e-6
    assert np.abs(out[0] - host[0]).max() <= 1e-5 * host[0].max()
    assert out[3] == pytest.approx(host[3], rel=1e-12)

"""GPU tests of the Hessian-vector products of the forces objective (csrc/kernels_forces_hessp.hip, the SM_TANGENT /
SM_PRODUCT forms of k_strip and k_strip2, csrc/api_forces_hessp.cpp, Context.forces_hessp / forces_hessian) and of scipy's
trust-exact on the device objective: the product against an independent extended-precision evaluation of the formula, the
strip loops with several strips per slot and segment, the affine model, the bitwise invariants, the one-point-per-context
state rules, the launch counts behind "a product costs a gradient", and the driver through find_optimum."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import load_golden, tall_forces_problem
from test_forces_hessp import DRIVER_CASES, check_optimum, host_run, run_driver
from test_hip_hessp import recipe
from test_hip_strip_loops import (assert_forces_regime, assert_ranks_equal_single, data as loop_data, enter_regime,
                                  on_thread_ranks)

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


def directions(M, seed):
    """eight directions: five normals, a zero vector, a normal, a unit vector (one column of H) -- pool[8 - k:] is a batch
    of width k: k = 1 the unit vector, k = 3 a normal, the zero vector and the unit vector, ..."""
    pool = np.random.default_rng(seed).standard_normal((8, M))
    pool[5] = 0.0
    pool[7] = 0.0
    pool[7, M // 3] = 1.0
    return pool


def problem(shape):
    """-> yTilde, YTilde, w0, forces (x = yTilde^T f has standard deviation 1: weights over a few decades), directions"""
    M, N = shape
    if shape == (808, 10):
        d = load_golden("ref_data_deer_test_forces_M808xN10.npz")
        yT, YT, w0 = np.asarray(d["yTilde"], dtype=np.float64), d["YTilde"].reshape(-1), d["w0"].reshape(-1)
    elif shape == (1100, 2000):
        t = tall_forces_problem()
        yT, YT, w0 = t["yTilde"], t["YTilde"], t["w0"]
    else:
        yT, YT, G = recipe(M, N, 1000 * M + N)
        w0 = np.exp(G)
    assert yT.shape == shape
    f = np.random.default_rng(5 + M).standard_normal(M)
    f /= (f @ yT).std()
    return yT, YT, w0, f, directions(M, 77 + M)


def hessp_longdouble(A, YT, w0, f, theta, V):
    """the formula of DESIGN section 6d in numpy.longdouble, written out here on its own (uncentred, as the text has it);
    A: the matrix of the model (longdouble).  -> (H V, L, grad)"""
    Yl, w0l, th = YT.astype(L), w0.astype(L), L(theta)
    x = f.astype(L) @ A
    e = w0l * np.exp(x - x.max())
    w = e / e.sum()
    ybar = A @ w
    r = ybar - Yl
    q = th * x + r @ A
    qbar = w @ q
    lw = np.log(w) - np.log(w0l)
    obj = th * (w * lw).sum() + L(0.5) * (r * r).sum()
    grad = A @ (w * q) - ybar * (w @ q)

    def one(v):
        dx = v @ A
        dxc = dx - w @ dx
        dy = A @ (w * dxc)
        s = w * (dxc * (q - qbar) + th * dx + dy @ A)
        return (A @ s - ybar * s.sum()).astype(np.float64)
    with ThreadPoolExecutor(8) as workers:                      # (numpy's longdouble products release the interpreter lock)
        hv = list(workers.map(one, V.astype(L)))
    return np.array(hv), float(obj), grad.astype(np.float64)


SHAPES = [(7, 37), (808, 10), (129, 257), (64, 2000), (513, 1537), (1100, 2000)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_product_against_the_formula_in_longdouble(bioen_amd, shape):
    """max |hv_dev - hv_ld| <= 1e-10 S, S = the largest |Hv| entry over the case's directions: the gate the log-weights
    product and the gradient are held to.  Every theta, every batch width (widths above 4 take other strip forms; 513 and
    808 rows: k_strip2; 808 x 10: fewer columns than segments; 1100 rows: the four passes over row panels); the
    point-setting call returns forces_fdf's bits."""
    yT, YT, w0, f, pool = problem(shape)
    A = yT.astype(L)
    with bioen_amd.Context(yT, YT) as ctx:
        for theta in THETAS:
            ref, fref, gref = hessp_longdouble(A, YT, w0, f, theta, pool)
            S = float(np.abs(ref).max())
            f0, g0 = ctx.forces_fdf(f, w0, theta)
            hv, fv, grad = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)          # sets the point, k = 8
            assert fv == f0 and np.array_equal(grad, g0)
            assert abs(fv - fref) <= 1e-12 * abs(fref)
            worst = float(np.abs(hv - ref).max())
            assert not hv[5].any()                                                       # H 0 = 0
            for k in WIDTHS:
                got = ctx.forces_hessp(pool[8 - k:] if k > 1 else pool[7])
                want = ref[8 - k:] if k > 1 else ref[7]
                assert got.shape == want.shape
                worst = max(worst, float(np.abs(got - want).max()))
            print("%s theta %g: max |hv - ld| = %.3g S (S = %.3g)" % (shape, theta, worst / S, S))
            assert worst <= 1e-10 * S


LOOP_CASES = [((64, 33000), "generated"), ((300, 9000), "generated"), ((300, 66000), "ascending"),
              ((600, 33700), "ascending"), ((64, 131500), "generated")]


@pytest.mark.parametrize("shape,order", LOOP_CASES, ids=["%dx%d-%s" % (s + (o,)) for s, o in LOOP_CASES])
def test_product_where_a_slot_runs_several_strips_per_segment(bioen_amd, monkeypatch, shape, order):
    """the regimes of tests/test_hip_strip_loops.py: the flush at segment ends and the deferred row-sum product under the
    new P2 forms; width 8 (DEPTH 3 in k_strip) and width 3 (two register sets); same gate"""
    enter_regime(monkeypatch, shape)
    yT, YT, G, w0, f, x = loop_data(shape)
    if order == "ascending":
        perm = np.argsort(x, kind="stable")
        yT, w0 = np.ascontiguousarray(yT[:, perm]), np.ascontiguousarray(w0[perm])
    f = f / 5.0                                                 # x with standard deviation 1
    pool = directions(shape[0], 3 + shape[0])
    theta = 10.0
    ref, fref, gref = hessp_longdouble(yT.astype(L), YT, w0, f, theta, pool)
    S = float(np.abs(ref).max())
    with bioen_amd.Context(yT, YT) as ctx:
        assert_forces_regime(ctx, shape)
        f0, g0 = ctx.forces_fdf(f, w0, theta)
        hv8, fv, grad = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)
        assert fv == f0 and np.array_equal(grad, g0)
        hv3 = ctx.forces_hessp(pool[5:])
        worst = max(float(np.abs(hv8 - ref).max()), float(np.abs(hv3 - ref[5:]).max()))
        print("%s %s: max |hv - ld| = %.3g S (S = %.3g)" % (shape, order, worst / S, S))
        assert worst <= 1e-10 * S
        assert np.array_equal(hv3, hv8[5:])


@pytest.mark.parametrize("shape", [(129, 257), (1100, 2000)], ids=["129x257", "1100x2000"])
def test_product_with_an_affine_model(bioen_amd, shape):
    """row offsets and scales set on the context; the test folds them into its own matrix"""
    yT, YT, w0, f, pool = problem(shape)
    rng = np.random.default_rng(3)
    off, sc = rng.normal(0.0, 0.5, shape[0]), rng.uniform(0.5, 1.5, shape[0])
    eff = off[:, None].astype(L) + sc[:, None].astype(L) * yT.astype(L)
    theta = 10.0
    ref, fref, gref = hessp_longdouble(eff, YT, w0, f, theta, pool)
    S = float(np.abs(ref).max())
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_affine(off, sc)
        f0, g0 = ctx.forces_fdf(f, w0, theta)
        hv, fv, grad = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)
        assert fv == f0 and np.array_equal(grad, g0)
        assert np.abs(grad - gref).max() <= 1e-10 * np.abs(gref).max()
        hv3 = ctx.forces_hessp(pool[5:])
        print("affine: max |hv - ld| = %.3g S" % (float(np.abs(hv - ref).max()) / S))
        assert np.abs(hv - ref).max() <= 1e-10 * S
        assert np.array_equal(hv3, hv[5:])
    with bioen_amd.Context(yT, YT) as ctx:                      # (o, s) = (0, 1) set explicitly: the plain model's bits
        plain, _, _ = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)
        ctx.set_affine(np.zeros(shape[0]), np.ones(shape[0]))
        same, _, _ = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)
        assert np.array_equal(plain, same)


@pytest.mark.parametrize("shape", [(129, 257), (513, 1537), (1100, 2000)], ids=["129x257", "513x1537", "1100x2000"])
def test_bitwise_invariants(bioen_amd, shape):
    yT, YT, w0, f, pool = problem(shape)
    theta = 10.0
    with bioen_amd.Context(yT, YT) as ctx:
        f0, g0 = ctx.forces_fdf(f, w0, theta)
        hv8, fv, grad = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)
        assert fv == f0 and np.array_equal(grad, g0)                # the point-setting call is forces_fdf's evaluation
        assert np.array_equal(ctx.forces_hessp(pool), hv8)          # at the kept point
        for a in range(8):                                          # eight single calls
            assert np.array_equal(ctx.forces_hessp(pool[a]), hv8[a]), a
        assert np.array_equal(ctx.forces_hessp(pool[2:5]), hv8[2:5])
        none, fb, gradb = ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)      # k = 0 only sets the point
        assert none is None and fb == fv and np.array_equal(gradb, grad)
        assert np.array_equal(ctx.forces_hessp(pool), hv8)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("shape", [(129, 1000), (1100, 2000)], ids=["129x1000", "1100x2000"])
def test_eight_thread_ranks_equal_the_single_context(bioen_amd, shape):
    """the scheme of tests/test_hip_hessp.py.  129 rows (k_strip, the fused passes) with 1000 columns, not the 257 of the
    other 129-row cases: a problem shards over eight ranks only if the last rank still owns a column, N > 7 x
    round_up(ceil(N / 8), 128) ("too few structures to shard" otherwise) -- 257 columns cannot be sharded
    over any number of ranks, 1000 can (segments of 128 columns, the last rank holds 104); 1100 x 2000: the row panels"""
    yT, YT, w0, f, pool = problem(shape)

    def workload(ctx, local_segments):
        hv1, fv, grad = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        return {"hv1": hv1, "f": fv, "grad": grad, "hv8": ctx.forces_hessp(pool), "hv3": ctx.forces_hessp(pool[5:])}

    with bioen_amd.Context(yT, YT) as ctx:
        single = workload(ctx, 8)
    assert_ranks_equal_single(on_thread_ranks(bioen_amd, 8, yT, YT, workload), single)


def estate(call, *needles):
    from bioen_amd._lib import BioenHipError
    with pytest.raises(BioenHipError) as e:
        call()
    assert "(-6)" in str(e.value) and all(s in str(e.value) for s in needles), str(e.value)


def test_one_point_per_context_and_what_drops_it(bioen_amd):
    """every rule of DESIGN 6c that drops the log-weights point drops a forces point (the rows of tests/test_entry_effects.py
    that evaluate or change the matrix state), the two methods' points replace each other, a rejected call leaves the point"""
    from bioen_amd._lib import BioenHipError
    from test_entry_effects import ENTRIES, P
    p = P.get()
    v = np.random.default_rng(2).standard_normal(p.m)
    f = 1e-3 * np.random.default_rng(3).standard_normal(p.m)
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        estate(lambda: ctx.forces_hessp(v), "no point on this context")
        hv, _, _ = ctx.forces_hessp(v, forces=f, w0=p.w0, theta=p.theta)
        n_drop = 0
        for name, r in sorted(ENTRIES.items()):
            for row in (r if isinstance(r, list) else (r,)):
                if row.how is None or row.session in ("needs", "starts") or name == "bioen_hip_logw_hessp":
                    continue
                hv2, _, _ = ctx.forces_hessp(v, forces=f, w0=p.w0, theta=p.theta)
                assert np.array_equal(hv2, hv), name
                if row.prepare:
                    row.prepare(ctx)
                row.how(ctx)
                if row.point == "drops":
                    n_drop += 1
                    estate(lambda: ctx.forces_hessp(v), "is gone", name)
                else:
                    assert row.point == "keeps"
                    assert np.array_equal(ctx.forces_hessp(v), hv), name
        assert n_drop >= 15
        # the BFGS session's calls drop it too
        ctx.forces_hessp(v, forces=f, w0=p.w0, theta=p.theta)
        ctx.bfgs_begin(p.x, p.G, p.theta)
        estate(lambda: ctx.forces_hessp(v), "is gone", "bioen_hip_bfgs_logw_begin")
        ctx.forces_hessp(None, forces=f, w0=p.w0, theta=p.theta)       # an evaluation: the session ends
        assert np.array_equal(ctx.forces_hessp(v), hv)
        estate(lambda: ctx.bfgs_trial(1e-3, False), "ended by another call")
        estate(lambda: ctx.forces_hessp(v), "is gone", "bioen_hip_bfgs_logw_trial")      # a session call drops the point, served or not
        ctx.forces_hessp(None, forces=f, w0=p.w0, theta=p.theta)
        # cross-method: one point, with a kind
        estate(lambda: ctx.logw_hessp(p.v), "forces point", "bioen_hip_forces_hessp")
        assert np.array_equal(ctx.forces_hessp(v), hv)                 # ... which the refused call has left alone
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        estate(lambda: ctx.forces_hessp(v), "log-weights point", "bioen_hip_logw_hessp")
        assert np.array_equal(ctx.logw_hessp(p.v), hl)
        # rejected for its arguments: nothing launched, the point stays
        ctx.forces_hessp(v, forces=f, w0=p.w0, theta=p.theta)
        ctx.kernel_stats_enable(True)
        ctx.kernel_stats_reset()
        with pytest.raises((ValueError, BioenHipError)):
            ctx.forces_hessp(np.zeros((9, p.m)))
        with pytest.raises((ValueError, BioenHipError)):
            ctx.forces_hessp(np.zeros(p.m + 1))
        from bioen_amd import _lib
        buf = np.zeros((9, p.m))
        assert _lib.lib().bioen_hip_forces_hessp(ctx._h, None, None, 0.0, 9, _lib.ptr(buf), _lib.ptr(buf), None, None) == -1
        assert _lib.lib().bioen_hip_forces_hessp(ctx._h, None, None, 0.0, 1, None, None, None, None) == -1
        assert _lib.lib().bioen_hip_forces_hessp(ctx._h, _lib.ptr(f), None, 0.0, 0, None, None, None, None) == -1
        st = ctx.kernel_stats()
        assert all(st[key]["launches"] == 0 for key in st)
        ctx.kernel_stats_enable(False)
        assert np.array_equal(ctx.forces_hessp(v), hv)


def test_refused_combinations(bioen_amd, monkeypatch):
    """BIOEN_HIP_ESTATE with a message of its own: the streaming fallback (BIOEN_HIP_PANELS=0 at M > 1024: no strip
    copies), the reduced-storage copies"""
    t = tall_forces_problem()
    v = np.ones(1100)
    monkeypatch.setenv("BIOEN_HIP_PANELS", "0")
    with bioen_amd.Context(t["yTilde"], t["YTilde"]) as ctx:
        estate(lambda: ctx.forces_hessp(v, forces=t["f0"], w0=t["w0"], theta=10.0), "bioen_hip_forces_hessp", "streaming")
        f0, g0 = ctx.forces_fdf(t["f0"], t["w0"], 10.0)              # the evaluation itself is served there
        assert np.isfinite(f0)
        estate(lambda: ctx.forces_hessp(v), "bioen_hip_forces_hessp", "streaming")
    monkeypatch.delenv("BIOEN_HIP_PANELS", raising=False)
    yT, YT, w0, f, pool = problem((64, 2000))
    with bioen_amd.Context(yT, YT) as ctx:
        hv, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        ctx.set_storage("split")
        estate(lambda: ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0), "reduced-storage")
        ctx.set_storage("f64")
        hv2, _, _ = ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        assert np.array_equal(hv, hv2)


def test_a_product_on_row_panels_costs_four_passes_per_panel(bioen_amd):
    """M > 1024: two column-sum and two row-sum launches per panel, for any k -- what a gradient costs there; setting the
    point costs no pass more than forces_fdf"""
    yT, YT, w0, f, pool = problem((1100, 2000))
    panels = 2
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)
        ctx.kernel_stats_enable(True)

        def launches(call):
            ctx.kernel_stats_reset()
            call()
            st = ctx.kernel_stats()
            return (st["forward"]["launches"], st["adjoint"]["launches"], st["forces_hessp_tangent"]["launches"],
                    st["forces_hessp_product"]["launches"])

        for k in WIDTHS:
            assert launches(lambda: ctx.forces_hessp(pool[:k])) == (2 * panels, 2 * panels, 0, 0), k
        evaluation = launches(lambda: ctx.forces_fdf(f, w0, 10.0))
        assert evaluation == (2 * panels, 2 * panels, 0, 0)
        assert launches(lambda: ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)) == evaluation


@pytest.mark.parametrize("shape", [(64, 2000), (513, 1537)], ids=["64x2000", "513x1537"])
def test_a_product_costs_two_fused_passes(bioen_amd, shape):
    """through kernel_stats: a product at the kept point, for any k, is one launch of each fused pass and no other matrix
    pass; setting the point is forces_fdf's two passes and ONE column-sum pass more"""
    yT, YT, w0, f, pool = problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.forces_hessp(pool[0], forces=f, w0=w0, theta=10.0)       # the strip copy exists from here on
        ctx.kernel_stats_enable(True)

        def launches(call):
            ctx.kernel_stats_reset()
            call()
            st = ctx.kernel_stats()
            return (st["forward"]["launches"], st["adjoint"]["launches"], st["forces_hessp_tangent"]["launches"],
                    st["forces_hessp_product"]["launches"])

        for k in WIDTHS:
            assert launches(lambda: ctx.forces_hessp(pool[:k])) == (0, 0, 1, 1), k
        evaluation = launches(lambda: ctx.forces_fdf(f, w0, 10.0))
        assert evaluation == (1, 1, 0, 0)                            # the yardstick: a gradient is two fused passes
        setting = launches(lambda: ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0))
        assert setting == (evaluation[0], evaluation[1] + 1, 0, 0)
        assert launches(lambda: ctx.forces_hessp(pool[:3], forces=f, w0=w0, theta=10.0)) == (1, 2, 1, 1)


@pytest.mark.parametrize("shape", [(64, 2000), (513, 1537)], ids=["64x2000", "513x1537"])
def test_dense_hessian_against_longdouble(bioen_amd, shape):
    yT, YT, w0, f, _ = problem(shape)
    M = shape[0]
    theta = 10.0
    ref, fref, gref = hessp_longdouble(yT.astype(L), YT, w0, f, theta, np.eye(M))
    S = float(np.abs(ref).max())
    with bioen_amd.Context(yT, YT) as ctx:
        H, fv, grad = ctx.forces_hessian(forces=f, w0=w0, theta=theta)
        f0, g0 = ctx.forces_fdf(f, w0, theta)
        assert fv == f0 and np.array_equal(grad, g0)
        assert H.shape == (M, M) and np.array_equal(H, H.T)
        print("%s: max |H - ld| = %.3g max|H|" % (shape, float(np.abs(H - ref).max()) / S))
        assert np.abs(H - ref).max() <= 1e-10 * S
        ctx.forces_hessp(None, forces=f, w0=w0, theta=theta)
        assert np.array_equal(ctx.forces_hessian(), H)               # at the kept point


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_trust_exact_on_the_device_objective(bioen_amd, name):
    """the cases and gates of tests/test_forces_hessp.py on the device objective, against the reference's converged optimum
    and against the numpy-objective run (not bitwise: the two sum in different orders)"""
    d, out = run_driver(name, "trust_exact", True)
    check_optimum(d, out)
    _, host = host_run(name)
    assert abs(out[4] - host[4]) <= 1e-6
    assert np.abs(out[0] - host[0]).max() <= 1e-5 * host[0].max()
    assert out[3] == pytest.approx(host[3], rel=1e-12)


def test_device_twins_of_the_numpy_functions(bioen_amd):
    from bioen_amd.optimize import forces
    d = load_golden("synth_forces_M30xN1000.npz")
    args = (d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"])
    x = np.asarray(d["forces_init"], dtype=np.float64).reshape(-1) + 1e-3
    v = np.random.default_rng(1).standard_normal(x.size)
    a = forces.hessp_bioen_log_posterior(x, v, *args, use_c=False)
    b = forces.hessp_bioen_log_posterior(x, v, *args, use_c=True)
    assert b.shape == a.shape and np.abs(a - b).max() <= 1e-10 * np.abs(a).max()
    Ha = forces.hessian_bioen_log_posterior(x, *args, use_c=False)
    Hb = forces.hessian_bioen_log_posterior(x, *args, use_c=True)
    assert np.abs(Ha - Hb).max() <= 1e-10 * np.abs(Ha).max()

"""GPU tests of the forces method on the affine observable model (Context.set_affine: yTilde_eff[i][j] = o_i + s_i Y_ij on
the resident matrix) and of nuisance.series_forces, the reference's `forces` refit loop on it.

The model reaches the evaluation on M-vectors only -- the operand of the first column-sum pass is f o s, the constant of
b_j gains sum_i o_i r_i, the gradient is multiplied by s_i on the device -- so the shapes are the smallest that reach each
pass family: M = 37 (k_strip), 520 (k_strip2), 1030 (row panels), and the streaming fallback at 37 (no strip copy) and at
1030 (BIOEN_HIP_PANELS=0).  Every test asserts its family from Context.footprint.

Yardstick of the evaluations: oracle_binding (the CPU restatement of the reference's C path) on the matrix REBUILT on the
host, which is what the reference's caller does for every refit.  Gates: test_hip_parity.py's as they stand.  Bit claims
are tested with ==."""
import threading

import numpy as np
import pytest

from conftest import LBFGS_DEFAULTS, LBFGS_CONV
from test_hip_api import _deer_problem

pytestmark = pytest.mark.gpu

SHAPES = [(37, 500), (520, 300), (1030, 200)]
AT_OPTIMUM = (0, 1, 2, -998, -1000, -1001)      # gradient test | rounding floor of the line search
CAPPED7 = dict(LBFGS_DEFAULTS, max_iterations=7)
CAPPED9 = dict(LBFGS_DEFAULTS, max_iterations=9)


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- data ------------------------------------------------------------------------------------------------------------
def synth(M, N, seed=0, with_off=True):
    """two row groups whose data were generated with the scales 0.7 / 1.6; uniform prior"""
    rng = np.random.default_rng(seed)
    Y = rng.normal(0.0, 1.0, (M, N)) + rng.normal(0.0, 2.0, (M, 1))
    groups = [np.arange(0, M // 2), np.arange(M // 2, M)]
    s_true = np.where(np.arange(M) < M // 2, 0.7, 1.6)
    o = rng.normal(0.0, 3.0, M) if with_off else None
    w_true = rng.dirichlet(np.full(N, 0.5))
    YT = (o if with_off else 0.0) + s_true * Y.dot(w_true) + rng.normal(0.0, 1.0, M)
    return dict(Y=Y, YT=YT, off=o, groups=groups, w0=np.full(N, 1.0 / N))


_EVAL = {}


def eval_problem(shape):
    """matrix, targets, a random model (o, s in U(0.5, 2)), a random prior, forces -- and the oracle's answers on the rebuilt
    matrix, once per shape"""
    if shape not in _EVAL:
        from oracle import oracle_binding as O
        M, N = shape
        if shape == (105, 400):       # the DEER problem: o = 1 / sigma, s = the modulation depths 0.15 / 0.4
            F, sigma, groups, Yexp, _ = _deer_problem()
            Y, YT, off = (F - 1.0) / sigma[:, None], Yexp / sigma, 1.0 / sigma
            sc = np.ones(M)
            sc[groups[0]], sc[groups[1]] = 0.15, 0.4
            rng = np.random.default_rng(1)
            forces = 1e-3 * rng.standard_normal(M)
        else:
            d = synth(M, N, seed=M + N)
            rng = np.random.default_rng(7 * M + N)
            Y, YT, off = d["Y"], d["YT"], rng.normal(0.0, 3.0, M)
            sc = rng.uniform(0.5, 2.0, M)
            forces = 0.01 * rng.standard_normal(M)
        w0 = rng.dirichlet(np.full(N, 2.0))
        eff = off[:, None] + sc[:, None] * Y
        p = dict(Y=Y, YT=YT, off=off, sc=sc, w0=w0, forces=forces, eff=eff, ref={})
        for theta in (100.0, 1.0):
            p["ref"][theta] = O.forces_fdf(forces, w0, eff, YT, theta)
        _EVAL[shape] = p
    return _EVAL[shape]


def enter_path(monkeypatch, shape, path):
    if path == "stream":
        if shape[0] > 1024:
            monkeypatch.setenv("BIOEN_HIP_PANELS", "0")
        else:
            monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")


def assert_path(ctx, path):
    forms = ctx.footprint()[0]
    assert forms == {"rowmajor"} if path == "stream" else "strips" in forms, (path, forms)


EVAL_CASES = [(s, "strip") for s in SHAPES + [(105, 400)]] + [((37, 500), "stream"), ((1030, 200), "stream")]


# ---- 1. evaluation against the oracle on the rebuilt matrix ------------------------------------------------------------
@pytest.mark.parametrize("shape,path", EVAL_CASES, ids=case_id)
def test_affine_evaluation_equals_the_oracle_on_the_rebuilt_matrix(bioen_amd, monkeypatch, shape, path):
    p = eval_problem(shape)
    enter_path(monkeypatch, shape, path)
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(p["off"], p["sc"])
        for theta in (100.0, 1.0):
            f_o, grad_o, w_o = p["ref"][theta]
            f, grad = ctx.forces_fdf(p["forces"], p["w0"], theta)
            w = ctx.forces_weights(p["forces"], p["w0"])
            floor = 1e-14 * np.abs(p["eff"]).max() * (abs(f_o) + 1)
            print("%s %s theta %g: rel f %.3g, grad %.3g of max|grad| (floor %.3g), w %.3g max w"
                  % (case_id(shape), path, theta, rel(f, f_o), np.abs(grad - grad_o).max() / np.abs(grad_o).max(),
                     floor / np.abs(grad_o).max(), np.abs(w - w_o).max() / w_o.max()))
            assert rel(f, f_o) < 1e-12, (theta, f, f_o)
            assert np.abs(grad - grad_o).max() <= 1e-10 * np.abs(grad_o).max() + floor, theta
            assert np.abs(w - w_o).max() <= 1e-13 * w_o.max(), theta
        assert_path(ctx, path)


# ---- 2. bits ---------------------------------------------------------------------------------------------------------
def plain_workload(ctx, p):
    th = [100.0, 1.0, 10.0, 0.3, 30.0]
    F = np.stack([s * p["forces"] for s in (1.0, -0.5, 2.0, 0.0, 0.25)])
    f1, g1 = ctx.forces_fdf(p["forces"], p["w0"], 10.0)
    fb, gb = ctx.forces_fdf_batch(F, p["w0"], th)
    res, w, info = ctx.opt_lbfgs_forces(p["forces"], p["w0"], 10.0, CAPPED7)
    return dict(f1=f1, g1=g1, fb=fb, gb=gb, res=res, w=w, stat=(info.lbfgs_code, info.iterations, info.evaluations, info.fmin))


def assert_same(got, want):
    for key, val in want.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(val)), key


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_the_plain_model_keeps_its_bits(bioen_amd, shape):
    """(o, s) = (0, 1) given explicitly, and a model set, used and removed again: both are the context that never had one"""
    p = eval_problem(shape)
    M = shape[0]
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        fresh = plain_workload(ctx, p)
        assert fresh["stat"][1] == 7
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(np.zeros(M), np.ones(M))
        assert_same(plain_workload(ctx, p), fresh)
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(p["off"], p["sc"])
        f_aff, _ = ctx.forces_fdf(p["forces"], p["w0"], 10.0)
        assert f_aff != fresh["f1"]
        ctx.set_affine(None, None)
        assert_same(plain_workload(ctx, p), fresh)


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_affine_batch_columns_equal_the_single_call(bioen_amd, shape):
    p = eval_problem(shape)
    th = [100.0, 1.0, 10.0, 0.3, 30.0, 3.0, 1000.0, 0.1]
    F = np.stack([s * p["forces"] for s in (1.0, -0.5, 2.0, 0.0, 0.25, -1.0, 0.5, -2.0)])
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(p["off"], p["sc"])
        single = [ctx.forces_fdf(F[a], p["w0"], th[a]) for a in range(8)]
        for K in range(1, 9):
            fb, gb = ctx.forces_fdf_batch(F[:K], p["w0"], th[:K])
            for a in range(K):
                assert fb[a] == single[a][0] and np.array_equal(gb[a], single[a][1]), (K, a)
        assert_path(ctx, "strip")


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_affine_capped_series_equals_its_capped_single_runs(bioen_amd, shape):
    p = eval_problem(shape)
    th = [100.0, 10.0, 1.0]
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(p["off"], p["sc"])
        res, w, infos = ctx.opt_lbfgs_forces_batch(th, p["forces"], p["w0"], CAPPED9)
        for a in range(3):
            f1, w1, i1 = ctx.opt_lbfgs_forces(p["forces"], p["w0"], th[a], CAPPED9)
            assert (infos[a].lbfgs_code, infos[a].iterations, infos[a].evaluations, infos[a].fmin) == \
                   (i1.lbfgs_code, i1.iterations, i1.evaluations, i1.fmin), a
            assert np.array_equal(res[a], f1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) == 9


def on_thread_ranks(bioen_amd, world, yT, YT, workload):
    """-> the workload's result on each of `world` ranks, threads of this process on device 0 (sweep.ThreadComm)"""
    from bioen_amd import sweep
    comms = sweep.ThreadComm.create(world)
    results, errors = [None] * world, [None] * world

    def rank_main(r):
        try:
            ctx = bioen_amd.Context(yT, YT, device=0, rank=r, world=world)
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
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a rank did not finish"
    assert all(e is None for e in errors), errors
    return results


@pytest.mark.parametrize("shape", [(37, 4000), (1030, 4000)], ids=case_id)
def test_affine_thread_ranks_equal_the_single_context(bioen_amd, shape):
    """2 and 8 ranks = the single context bit for bit: evaluation, batch, weights, a capped run and the averages it leaves"""
    p = eval_problem(shape)
    th = [100.0, 1.0, 10.0, 0.3, 30.0]
    F = np.stack([s * p["forces"] for s in (1.0, -0.5, 2.0, 0.0, 0.25)])

    def workload(ctx):
        ctx.set_affine(p["off"], p["sc"])
        out = {}
        out["f"], out["grad"] = ctx.forces_fdf(p["forces"], p["w0"], 10.0)
        out["fb"], out["gb"] = ctx.forces_fdf_batch(F, p["w0"], th)
        out["wf"] = ctx.forces_weights(p["forces"], p["w0"])
        out["res"], out["w"], info = ctx.opt_lbfgs_forces(p["forces"], p["w0"], 10.0, CAPPED9)
        out["stat"] = (info.lbfgs_code, info.iterations, info.evaluations, info.fmin)
        out["yraw"], out["yeff"] = ctx.last_average()
        return out

    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        single = workload(ctx)
        assert_path(ctx, "strip")
    assert rel(single["fb"][0], p["ref"][100.0][0]) < 1e-12      # (the single context itself is right: column 0 is theta = 100)
    for world in (2, 8):
        for r, res in enumerate(on_thread_ranks(bioen_amd, world, p["Y"], p["YT"], workload)):
            for key, val in single.items():
                assert np.array_equal(np.asarray(res[key]), np.asarray(val)), (world, r, key)


# ---- 3. averages -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,path", [(s, "strip") for s in SHAPES] + [((37, 500), "stream")], ids=case_id)
def test_last_average_after_an_affine_forces_call(bioen_amd, monkeypatch, shape, path):
    p = eval_problem(shape)
    enter_path(monkeypatch, shape, path)
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(p["off"], p["sc"])
        w = ctx.forces_weights(p["forces"], p["w0"])
        ctx.forces_fdf(p["forces"], p["w0"], 10.0)
        yraw, yeff = ctx.last_average()
        assert_path(ctx, path)
    raw = p["Y"].dot(w)
    eff = p["off"] + p["sc"] * raw
    assert np.abs(yraw - raw).max() <= 1e-12 * np.abs(raw).max()
    assert np.abs(yeff - eff).max() <= 1e-12 * np.abs(eff).max()


# ---- 4. the GSL minimizers --------------------------------------------------------------------------------------------
def test_opt_gsl_forces_on_an_affine_context(bioen_amd):
    from oracle import oracle_binding as O
    p = eval_problem((37, 500))
    params = dict(step_size=0.01, tol=1e-8, max_iterations=5000)
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_affine(p["off"], p["sc"])
        x, w, info = ctx.opt_gsl_forces(np.zeros(37), p["w0"], 10.0, "bfgs2", params)
    x_o, fmin_o, code_o, it_o, _ = O.opt_gsl_forces(np.zeros(37), p["w0"], p["eff"], p["YT"], 10.0, dict(params, algorithm="bfgs2"))
    print("gsl bfgs2: fmin %.15g (oracle %.15g), %d / %d iterations" % (info.fmin, fmin_o, info.iterations, it_o))
    assert rel(info.fmin, fmin_o) < 1e-6
    w_o = O.forces_weights(x, p["w0"], p["eff"])
    assert np.abs(w - w_o).max() <= 1e-12 * w_o.max()        # the weights handed out are those of the returned forces


# ---- 5. the loop against the reference's protocol done the slow way -------------------------------------------------------
def slow_forces_loop(Y, YT, off, groups, w0, thetas, scale0, iterations):
    """rebuild yTilde(s) on the host, optimise with the oracle from the previous optimum, refit -- per theta the last solve's
    (fmin, weights, scales it ran with) and the refitted scales"""
    from bioen_amd import nuisance
    from oracle import oracle_binding as O
    M = Y.shape[0]
    scales, forces, out = [scale0] * len(groups), np.zeros(M), []
    for theta in thetas:
        for _ in range(iterations):
            sc = np.ones(M)
            for s, ix in zip(scales, groups):
                sc[ix] = s
            explicit = (0.0 if off is None else off[:, None]) + sc[:, None] * Y
            forces, fmin, code, it, ev = O.opt_lbfgs_forces(forces, w0, explicit, YT, theta, LBFGS_CONV)
            assert code in AT_OPTIMUM
            w = O.forces_weights(forces, w0, explicit)
            used = sc
            scales = nuisance.refit_scales(Y.dot(w), YT, off, groups)
        out.append(dict(fmin=fmin, w=w, scales=list(scales), used=used))
    return out


@pytest.mark.parametrize("M,N,with_off", [(37, 500, True), (37, 500, False), (130, 700, True), (520, 300, True)])
def test_series_forces_matches_the_host_rebuild_loop(bioen_amd, M, N, with_off):
    """Both sides run to convergence (LBFGS_CONV; the rounding floor of the line search counts as the optimum) with four
    refits per theta, forces and scales carried from solve to solve.  Two converged runs of the reference (backtracking-Wolfe
    against More-Thuente) agree on these loops to 1.3e-12 in fmin, 2.4e-9 in the scales and 2.4e-7 max(w) in the weights;
    the device is held to north_star's 1e-6 / 1e-5 max(w) and to 1e-7 on the scales.  with_off = False: the scattering
    form, one scale for the whole data set."""
    from bioen_amd import nuisance
    d = synth(M, N, seed=1, with_off=with_off)
    groups = d["groups"] if with_off else [np.arange(M)]
    thetas = [100.0, 10.0]
    with bioen_amd.Context(d["Y"], d["YT"]) as ctx:
        res = nuisance.series_forces(ctx, thetas, d["w0"], np.zeros(M), LBFGS_CONV, d["YT"], groups=groups if with_off else None,
                                     row_offset=d["off"], scale0=1.0, iterations=4, accept_codes=AT_OPTIMUM)
        f_plain, _ = ctx.forces_fdf(np.zeros(M), d["w0"], 10.0)
        assert "strips" in ctx.footprint()[0]
    slow = slow_forces_loop(d["Y"], d["YT"], d["off"], groups, d["w0"], thetas, 1.0, 4)
    for k, theta in enumerate(thetas):
        dw = np.abs(res[k]["w"] - slow[k]["w"]).max() / slow[k]["w"].max()
        ds = np.abs(np.asarray(res[k]["scales"]) - np.asarray(slow[k]["scales"])).max()
        print("%dx%d off=%s theta %g: rel fmin %.3g, scales %.3g, weights %.3g max w, %d iterations on the device"
              % (M, N, with_off, theta, rel(res[k]["fmin"], slow[k]["fmin"]), ds, dw,
                 sum(t["iterations"] for t in res[k]["trace"])))
        assert rel(res[k]["fmin"], slow[k]["fmin"]) < 1e-6, theta
        assert ds <= 1e-7, (theta, res[k]["scales"], slow[k]["scales"])
        assert dw <= 1e-5, theta
    # the model is gone: the plain objective at f = 0 is 0.5 |Y w0 - YT|^2
    assert rel(f_plain, 0.5 * np.sum((d["Y"].dot(d["w0"]) - d["YT"]) ** 2)) < 1e-12


def test_series_forces_on_the_deer_problem(bioen_amd):
    """The DEER problem of test_hip_api (modulation depths as scales, o = 1 / sigma), theta = 100, four refits.  NO weight
    gate here: the problem is ill-conditioned in the forces parametrisation -- two converged runs of the reference
    (backtracking-Wolfe against More-Thuente) agree to 1.3e-9 in fmin and 8e-10 in the scales but differ by 3e-4 max(w) in
    the weights, more than north_star's 1e-5 allows, so a weight gate would test the reference's noise.  The averages the
    fit sees are gated instead: yeff to 1e-6 relative."""
    from bioen_amd import nuisance
    F, sigma, groups, Yexp, m_true = _deer_problem()
    Y, YT, off = (F - 1.0) / sigma[:, None], Yexp / sigma, 1.0 / sigma
    M, N = Y.shape
    w0 = np.full(N, 1.0 / N)
    with bioen_amd.Context(Y, YT) as ctx:
        res = nuisance.series_forces(ctx, [100.0], w0, np.zeros(M), LBFGS_CONV, YT, groups=groups, row_offset=off,
                                     scale0=0.15, iterations=4, accept_codes=AT_OPTIMUM)
    slow = slow_forces_loop(Y, YT, off, groups, w0, [100.0], 0.15, 4)
    used = np.ones(M)
    for s, ix in zip(res[0]["trace"][-1]["scales"], groups):
        used[ix] = s
    yeff = off + used * Y.dot(res[0]["w"])
    yeff_o = off + slow[0]["used"] * Y.dot(slow[0]["w"])
    ds = np.abs(np.asarray(res[0]["scales"]) - np.asarray(slow[0]["scales"])).max()
    print("deer: rel fmin %.3g, scales %.3g, yeff %.3g, weights %.3g max w (not gated), %d iterations on the device"
          % (rel(res[0]["fmin"], slow[0]["fmin"]), ds, np.abs(yeff - yeff_o).max() / np.abs(yeff_o).max(),
             np.abs(res[0]["w"] - slow[0]["w"]).max() / slow[0]["w"].max(), sum(t["iterations"] for t in res[0]["trace"])))
    assert rel(res[0]["fmin"], slow[0]["fmin"]) < 1e-6
    assert ds <= 1e-7, (res[0]["scales"], slow[0]["scales"])
    assert np.abs(yeff - yeff_o).max() <= 1e-6 * np.abs(yeff_o).max()


def test_logw_series_without_offset_matches_the_host_rebuild_loop(bioen_amd):
    """nuisance.series (log-weights) in the scattering form -- row_offset = None, one scale for the whole data set -- against
    the same loop done the slow way with oracle_binding.opt_lbfgs_logw: 1e-6 / 1e-5 max(w) / 1e-7."""
    from bioen_amd import nuisance
    from oracle import oracle_binding as O
    M, N = 37, 500
    d = synth(M, N, seed=1, with_off=False)
    G = np.log(d["w0"])
    thetas = [100.0, 10.0]
    with bioen_amd.Context(d["Y"], d["YT"]) as ctx:
        res = nuisance.series(ctx, thetas, G, G, LBFGS_CONV, d["YT"], scale0=1.0, iterations=4, accept_codes=AT_OPTIMUM)
    scale = [1.0]
    for k, theta in enumerate(thetas):
        for _ in range(4):
            g, fmin, code, it, ev = O.opt_lbfgs_logw(G, G, scale[0] * d["Y"], d["YT"], theta, LBFGS_CONV)
            assert code in AT_OPTIMUM
            w = O.logw_weights(g)[0]
            scale = nuisance.refit_scales(d["Y"].dot(w), d["YT"], None, [np.arange(M)])
        assert rel(res[k]["fmin"], fmin) < 1e-6, theta
        assert abs(res[k]["scales"][0] - scale[0]) <= 1e-7, (theta, res[k]["scales"], scale)
        assert np.abs(res[k]["w"] - w).max() <= 1e-5 * w.max(), theta


# ---- what is still refused ---------------------------------------------------------------------------------------------
def test_affine_on_the_reduced_storage_copies_is_refused_with_its_own_message(bioen_amd):
    p = eval_problem((37, 500))
    with bioen_amd.Context(p["Y"], p["YT"]) as ctx:
        ctx.set_storage("fp32")
        ctx.set_affine(p["off"], p["sc"])
        for call in (lambda: ctx.forces_fdf(p["forces"], p["w0"], 10.0), lambda: ctx.forces_weights(p["forces"], p["w0"]),
                     lambda: ctx.opt_lbfgs_forces(p["forces"], p["w0"], 10.0, CAPPED7)):
            with pytest.raises(bioen_amd.BioenHipError, match="reduced-storage"):
                call()
        ctx.set_storage("f64")
        f, _ = ctx.forces_fdf(p["forces"], p["w0"], 100.0)
        assert rel(f, p["ref"][100.0][0]) < 1e-12

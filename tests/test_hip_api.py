"""GPU tests at the drop-in boundary: the bioen.optimize-compatible API (find_optimum,
bioen_log_posterior, ...) driven the way the reference's own tests drive it
(test/optimize/test_find_opt_analytical_grad_{logw,forces}.py, test_func_gradient_*.py,
test_error_opt_*.py), with the reference's tolerances."""
import warnings

import numpy as np
import pytest

from conftest import LOGW_GOLDEN, FORCES_GOLDEN, load_golden

pytestmark = pytest.mark.gpu

tol = 5.e-14        # test_find_opt_analytical_grad_logw.py:9
tol_min = 1.e-1     # :10


@pytest.fixture(scope="module")
def optimize():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    from bioen_amd import optimize
    yield optimize
    optimize.ext.c_bioen.clear_cache() if hasattr(optimize, "ext") else None
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


REF_LOGW = [n for n in LOGW_GOLDEN if n.startswith("ref_")]
REF_FORCES = [n for n in FORCES_GOLDEN if n.startswith("ref_")]


@pytest.mark.parametrize("fast_openmp", [0, 1])
def test_func_gradient_logw_c_vs_python(optimize, fast_openmp):
    """test_func_gradient_logw.py:35-57: device value/gradient vs the numpy variants, 5e-14 / 5e-12."""
    optimize.minimize.set_fast_openmp_flag(fast_openmp)
    d = load_golden("ref_data_deer_test_logw_M808xN10.npz")
    YT = d["YTilde"].reshape(1, -1)
    g = d["GInit"].copy()
    gPrime = np.asarray(g[:].T)[0]
    f_c = optimize.log_weights.bioen_log_posterior(gPrime, g, d["G"], d["yTilde"], YT, d["theta"], use_c=True)
    g_c = optimize.log_weights.grad_bioen_log_posterior(gPrime, g, d["G"], d["yTilde"], YT, d["theta"], use_c=True)
    f_p = optimize.log_weights.bioen_log_posterior(gPrime, g, d["G"], d["yTilde"], YT, d["theta"], use_c=False)
    g_p = optimize.log_weights.grad_bioen_log_posterior(gPrime, g, d["G"], d["yTilde"], YT, d["theta"], use_c=False)
    assert optimize.util.compute_relative_difference_for_values(f_c, f_p) < 5e-14
    assert optimize.util.compute_relative_difference_for_arrays(g_c, g_p)[0] < 5e-12


def test_func_gradient_forces_c_vs_python(optimize):
    """test_func_gradient_forces.py:29-51: 5e-14 / 5e-8."""
    d = load_golden("ref_data_deer_test_forces_M808xN10.npz")
    YT = d["YTilde"].reshape(1, -1)
    args = (d["forces_init"], d["w0"], d["y"], d["yTilde"], YT, d["theta"])
    f_c = optimize.forces.bioen_log_posterior(*args, use_c=True)
    g_c = optimize.forces.grad_bioen_log_posterior(*args, use_c=True)
    f_p = optimize.forces.bioen_log_posterior(*args, use_c=False)
    g_p = optimize.forces.grad_bioen_log_posterior(*args, use_c=False)
    assert optimize.util.compute_relative_difference_for_values(f_c, f_p) < 5e-14
    assert optimize.util.compute_relative_difference_for_arrays(g_c, g_p)[0] < 5e-8


@pytest.mark.parametrize("name", REF_LOGW)
@pytest.mark.parametrize("minimizer,algorithm", [("lbfgs", "lbfgs"), ("scipy", "lbfgs"), ("scipy", "bfgs"), ("scipy", "cg")])
@pytest.mark.parametrize("as_matrix", [False, True])
def test_find_optimum_logw(optimize, name, minimizer, algorithm, as_matrix):
    """test_find_opt_analytical_grad_logw.py: fmin vs *.ref at 1e-1, fmin == L(gopt) at 5e-14."""
    if name == "ref_data_potra_part_1_logw_M808xN80.npz" and minimizer == "scipy":
        pytest.skip("listed by the reference as needing tuned scipy parameters (:21-27)")
    d = load_golden(name)
    conv = np.asmatrix if as_matrix else np.asarray
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        GInit, G, y, yTilde = conv(d["GInit"]), conv(d["G"]), conv(d["y"]), conv(d["yTilde"])
        YTilde = conv(d["YTilde"].reshape(1, -1))
        params = optimize.minimize.Parameters(minimizer)
        params["cache_ytilde_transposed"] = "False"         # the string the reference's test passes (:199)
        params["use_c_functions"] = True
        params["algorithm"] = algorithm
        params["verbose"] = False
        wopt, yopt, gopt, fmin_ini, fmin_fin = optimize.log_weights.find_optimum(GInit, G, y, yTilde, YTilde,
                                                                                d["theta"], params)
        assert wopt.shape == (G.shape[0], 1) and yopt.shape == (yTilde.shape[0],) and gopt.shape == (G.shape[0],)
        assert abs(wopt.sum() - 1.0) < 1e-12
        assert rel(fmin_ini, float(d["f_init"])) < 1e-12
        if "ref_fmin_scipy_bfgs" in d:
            assert optimize.util.compute_relative_difference_for_values(fmin_fin, float(d["ref_fmin_scipy_bfgs"])) < tol_min
        re_fmin = optimize.log_weights.bioen_log_posterior(gopt, GInit, G, yTilde, YTilde, d["theta"], use_c=True)
        assert optimize.util.compute_relative_difference_for_values(fmin_fin, re_fmin) < tol
        assert np.abs(yopt - np.asarray(y).dot(np.asarray(wopt))[:, 0]).max() < 1e-9 * max(1.0, np.abs(yopt).max())
    if minimizer == "lbfgs":
        assert rel(fmin_fin, float(d["lbfgs_def_fmin"])) < 2e-5


def test_find_optimum_uploads_the_matrix_at_most_once(optimize, monkeypatch):
    """One `find_optimum` makes three (forces: four) calls of the ctypes layer on the same matrix; a matrix the context
    cache refuses (> 256 MB: here the threshold is lowered to a kilobyte) used to be uploaded by every one of them.  r05:
    the matrix is HELD for the call -- ONE upload per find_optimum / find_optimum_series whatever the minimizer, NONE
    inside a caller's ``with optimize.resident(yTilde):`` around its theta loop (bioen/analyze/procedure.py:62-77's shape)
    -- and the results do not change by a bit.  (The reference pays one yTilde.T.copy() per call: c_bioen.pyx:463-473.)"""
    from bioen_amd.optimize.ext import c_bioen
    monkeypatch.setattr(c_bioen, "_FULL_CHECK_BYTES", 1024)
    c_bioen.clear_cache()
    d = load_golden("synth_logw_M37xN500.npz")
    YT = d["YTilde"].reshape(1, -1)

    def params(minimizer, algorithm):
        p = optimize.minimize.Parameters(minimizer)
        p.update(cache_ytilde_transposed="False", use_c_functions=True, algorithm=algorithm, verbose=False)
        return p

    def uploads(fn):
        before = c_bioen.uploads
        out = fn()
        return c_bioen.uploads - before, out

    lw = optimize.log_weights
    for minimizer, algorithm in (("lbfgs", "lbfgs"), ("scipy", "lbfgs"), ("gsl", "bfgs2")):
        n, out = uploads(lambda: lw.find_optimum(d["GInit"], d["G"], d["yTilde"], d["yTilde"], YT, d["theta"], params(minimizer, algorithm)))
        assert n == 1, (minimizer, n)
    thetas = [50.0, 5.0, 0.5]
    n, series = uploads(lambda: lw.find_optimum_series(d["GInit"], d["G"], d["yTilde"], d["yTilde"], YT, thetas, params("lbfgs", "lbfgs")))
    assert n == 1
    loose = [lw.find_optimum(d["GInit"], d["G"], d["yTilde"], d["yTilde"], YT, th, params("lbfgs", "lbfgs")) for th in thetas]

    def loop():
        with optimize.resident(d["yTilde"]):
            return [lw.find_optimum(d["GInit"], d["G"], d["yTilde"], d["yTilde"], YT, th, params("lbfgs", "lbfgs")) for th in thetas]
    n, held = uploads(loop)
    assert n == 1                                         # the theta loop of a caller: one upload for the block
    for a, b, c_ in zip(series, loose, held):
        for x, y, z in zip(a, b, c_):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    assert not c_bioen._HELD                              # nothing stays held behind the block

    fd = load_golden("synth_forces_M30xN1000.npz")
    FT = fd["YTilde"].reshape(1, -1)
    for minimizer, algorithm in (("lbfgs", "lbfgs"), ("scipy", "bfgs"), ("gsl", "bfgs2")):
        n, out = uploads(lambda: optimize.forces.find_optimum(fd["forces_init"], fd["w0"], fd["yTilde"], fd["yTilde"], FT,
                                                              fd["theta"], params(minimizer, algorithm)))
        assert n == 1, (minimizer, n)
    # a hold survives an exception inside the block and releases the copy
    with pytest.raises(ZeroDivisionError):
        with optimize.resident(d["yTilde"]):
            1 / 0
    assert not c_bioen._HELD


@pytest.mark.parametrize("name", REF_FORCES)
@pytest.mark.parametrize("minimizer,algorithm", [("lbfgs", "lbfgs"), ("scipy", "lbfgs"), ("scipy", "bfgs")])
def test_find_optimum_forces(optimize, name, minimizer, algorithm):
    d = load_golden(name)
    YT = d["YTilde"].reshape(1, -1)
    params = optimize.minimize.Parameters(minimizer)
    params.update(cache_ytilde_transposed="False", use_c_functions=True, algorithm=algorithm, verbose=False)
    out = optimize.forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], YT, d["theta"], params)
    wopt, yopt, forces_opt, fmin_ini, fmin_fin, chiSqr, S = out
    n, m = d["w0"].size, d["yTilde"].shape[0]
    assert wopt.shape == (n, 1) and yopt.shape == (m,) and np.asarray(forces_opt).size == m
    assert rel(fmin_ini, float(d["f_init"])) < 1e-12
    assert rel(fmin_fin, float(d["ref_fmin_scipy_bfgs"])) < tol_min
    re_fmin = optimize.forces.bioen_log_posterior(forces_opt, d["w0"], d["y"], d["yTilde"], YT, d["theta"], use_c=True)
    assert rel(fmin_fin, re_fmin) < 1e-12
    assert rel(d["theta"] * S + chiSqr, fmin_fin) < 1e-9 or d["theta"] == 0
    if minimizer == "lbfgs":
        assert rel(fmin_fin, float(d["lbfgs_def_fmin"])) < 2e-5


def test_error_opt_logw_and_forces(optimize):
    """test_error_opt_logw.py:65-83 / test_error_opt_forces.py:51-69: delta = -1 -> RuntimeError 'return code'."""
    d = load_golden("ref_data_potra_part_2_logw_M205xN10.npz")
    params = optimize.minimize.Parameters("lbfgs")
    params["verbose"] = False
    params["params"]["delta"] = -1.0
    with pytest.raises(RuntimeError) as exc:
        optimize.log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1),
                                          d["theta"], params)
    assert "return code" in str(exc.value) and "-1015" in str(exc.value)
    assert "liblbfgs" in str(exc.value) and "delta" in str(exc.value)
    f = load_golden("ref_data_forces_M64xN64.npz")
    with pytest.raises(RuntimeError) as exc:
        optimize.forces.find_optimum(f["forces_init"], f["w0"], f["y"], f["yTilde"], f["YTilde"].reshape(1, -1),
                                     f["theta"], params)
    assert "return code" in str(exc.value)
    # hitting max_iterations is an error in the reference too (-997 is not in {0,1,2})
    params = optimize.minimize.Parameters("lbfgs")
    params["verbose"] = False
    params["params"]["max_iterations"] = 2
    with pytest.raises(RuntimeError) as exc:
        optimize.log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1),
                                          d["theta"], params)
    assert "-997" in str(exc.value)
    g = optimize.minimize.Parameters("gsl")
    g["verbose"] = False
    g["algorithm"] = "TEST_INVALID"
    with pytest.raises(RuntimeError) as exc:
        optimize.log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1),
                                          d["theta"], g)
    assert "return code" in str(exc.value)


def test_theta_series_reuses_resident_matrix(optimize):
    """A theta series over the same yTilde object must not re-upload it (context cache)."""
    from bioen_amd.optimize.ext import c_bioen
    d = load_golden("synth_logw_M64xN2000.npz")
    c_bioen.clear_cache()
    params = optimize.minimize.Parameters("lbfgs")
    params["verbose"] = False
    YT = d["YTilde"].reshape(1, -1)
    fm = []
    for theta in (100.0, 10.0, 1.0):
        out = optimize.log_weights.find_optimum(d["GInit"], d["G"], d["yTilde"], d["yTilde"], YT, theta, params)
        fm.append(out[4])
        assert len(c_bioen._CACHE) == 1
    assert fm[0] > fm[1] > fm[2]
    info = c_bioen.last_opt_info
    assert info.iterations > 0 and info.seconds > 0
    # a different matrix at the same address is detected by the fingerprint
    y2 = d["yTilde"].copy()
    y2 *= 1.0001
    optimize.log_weights.bioen_log_posterior(d["GInit"].ravel(), d["GInit"], d["G"], y2, YT, 1.0)
    assert len(c_bioen._CACHE) == 2
    c_bioen.clear_cache()
    assert len(c_bioen._CACHE) == 0


def test_large_matrix_is_not_served_from_a_stale_device_copy(optimize, monkeypatch):
    """Above 256 MB the host matrix cannot be re-checked in full for less than the upload it would save, so such a matrix
    is uploaded afresh on every call -- the reference's behaviour (fresh pointers per call,
    /root/reference/bioen/optimize/ext/c_bioen.pyx:463-478): an in-place edit of ONE element between two calls is seen.
    Only BIOEN_HIP_CACHE_LARGE=1 (the caller's promise not to edit in place) caches such a matrix, on a sampled check."""
    from bioen_amd.optimize.ext import c_bioen
    c_bioen.clear_cache()
    M, N = 64, 525000                        # 268.8 MB
    rng = np.random.default_rng(11)
    y = rng.normal(5.0, 1.0, (M, N))
    assert y.nbytes > 256 << 20
    YT = rng.normal(5.0, 0.1, (1, M))
    g = np.zeros((N, 1))
    monkeypatch.delenv("BIOEN_HIP_CACHE_LARGE", raising=False)
    f0 = optimize.log_weights.bioen_log_posterior(g.ravel().copy(), g, g, y, YT, 2.0)
    assert len(c_bioen._CACHE) == 0          # not cached
    i, j = 17, 262147                        # off every stride a sampled check would visit ...
    stride = max(1, y.size // (1 << 22)) | 1
    assert (i * N + j) % stride != 0
    delta = 1.0e6
    y[i, j] += delta                         # ... one element, in place
    f1 = optimize.log_weights.bioen_log_posterior(g.ravel().copy(), g, g, y, YT, 2.0)
    # closed form of the change: ybar_i moves by delta / N, chi^2 / 2 by r_i d + d^2 / 2
    r_i = (y[i].sum() - delta) / N - YT[0, i]
    expect = r_i * (delta / N) + 0.5 * (delta / N) ** 2
    assert abs((f1 - f0) - expect) <= 1e-9 * abs(expect), (f0, f1, expect)
    # opt-in: cached on the sampled check (which, by construction, does not see this edit)
    monkeypatch.setenv("BIOEN_HIP_CACHE_LARGE", "1")
    f2 = optimize.log_weights.bioen_log_posterior(g.ravel().copy(), g, g, y, YT, 2.0)
    assert len(c_bioen._CACHE) == 1 and f2 == f1
    y[i, j] -= delta
    f3 = optimize.log_weights.bioen_log_posterior(g.ravel().copy(), g, g, y, YT, 2.0)
    assert f3 == f2                          # the documented price of the opt-in
    c_bioen.clear_cache()


def test_synthetic_generator_statistics_and_large_property_checks(optimize):
    """BASELINE config 2 size (N = 1e5 x M = 256), generated in HBM: the generator follows the
    recipe, the oracle agrees on the downloaded matrix, and size-independent properties hold."""
    import bioen_amd
    from oracle import oracle_binding as O
    M, N = 256, 100000
    rng = np.random.default_rng(12345)
    YTrue = rng.uniform(1, 10, M)
    sig_exp, sig_sim = 0.1 * YTrue, 0.5 * YTrue
    YTilde = rng.normal(YTrue, sig_exp) / sig_exp
    with bioen_amd.Context.synthetic(M, N, YTrue, sig_sim, sig_exp, YTilde, seed=12345) as ctx:
        y = ctx.read_ytilde()
        z = (y * sig_exp[:, None] - YTrue[:, None]) / sig_sim[:, None]
        assert abs(z.mean()) < 1e-3 and abs(z.std() - 1.0) < 1e-3
        assert abs(np.corrcoef(z[0], z[1])[0, 1]) < 0.02 and abs(np.corrcoef(z[0, :-1], z[0, 1:])[0, 1]) < 0.02
        G = np.zeros(N)
        g = 0.5 * rng.standard_normal(N)
        theta = 10.0
        f, grad = ctx.logw_fdf(g, G, theta)
        f_o, grad_o, w_o = O.logw_fdf(g, G, y, YTilde, theta)
        assert rel(f, f_o) < 1e-12 and np.abs(grad - grad_o).max() <= 1e-10 * np.abs(grad_o).max()
        # properties: weights sum to one; gradient is orthogonal to the gauge direction (L(g + c) = L(g) + 0
        # for the chi^2 term, and the prior is shift-invariant too) ; directional derivative
        w, _ = ctx.logw_weights(g)
        assert abs(w.sum() - 1.0) < 1e-12
        assert abs(grad.sum()) < 1e-9 * np.abs(grad).sum()
        dirn = rng.standard_normal(N)
        h = 1e-5
        fp, _ = ctx.logw_fdf(g + h * dirn, G, theta, need_grad=False)
        fm, _ = ctx.logw_fdf(g - h * dirn, G, theta, need_grad=False)
        assert abs((fp - fm) / (2 * h) - grad.dot(dirn)) < 1e-5 * max(1.0, abs(grad.dot(dirn)))
        # full L-BFGS run against the oracle (yaml defaults)
        gopt, wopt, info = ctx.opt_lbfgs_logw(G, G, theta, dict(linesearch=2, max_iterations=5000, delta=1e-6,
                                                                epsilon=1e-6, ftol=1e-5, gtol=0.9, wolfe=0.9,
                                                                past=10, max_linesearch=100))
        g_o, fmin_o, code_o, it_o, ev_o = O.opt_lbfgs_logw(G, G, y, YTilde, theta)
        assert info.lbfgs_code in (0, 1) and code_o in (0, 1)
        assert rel(info.fmin, fmin_o) < 5e-5      # width of the delta = 1e-6 stopping plateau
        assert abs(info.iterations - it_o) <= max(5, it_o // 4)


# ---------------------------------------------------------------------------------------
# affine observable model + nuisance refits (BASELINE config 4 in miniature: DEER modulation depth)
# ---------------------------------------------------------------------------------------
def _deer_problem(M1=60, M2=45, N=400, seed=3):
    """Two synthetic DEER traces F(d_j, t_i) in (0,1] with different modulation depths."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(2.0, 6.0, N)                      # nm
    def trace(t):
        return 0.5 * (1.0 + np.cos(2 * np.pi * 52.04 * t[:, None] / d[None, :] ** 3)) * np.exp(-0.2 * t[:, None])
    F = np.vstack([trace(np.linspace(0.0, 2.5, M1)), trace(np.linspace(0.0, 3.5, M2))])
    sigma = 0.01 * np.ones(M1 + M2)
    groups = [np.arange(M1), np.arange(M1, M1 + M2)]
    w_true = rng.dirichlet(np.ones(N) * 0.3)
    m_true = [0.22, 0.31]
    Y = np.empty(M1 + M2)
    for mt, ix in zip(m_true, groups):
        Y[ix] = 1 - mt + mt * F[ix].dot(w_true)
    Y += sigma * rng.standard_normal(M1 + M2)
    return F, sigma, groups, Y, m_true


def test_affine_model_equals_explicit_matrix(optimize):
    import bioen_amd
    from oracle import oracle_binding as O
    F, sigma, groups, Y, _ = _deer_problem()
    Ft = (F - 1.0) / sigma[:, None]
    YT = Y / sigma
    off = 1.0 / sigma
    sc = np.ones(F.shape[0])
    sc[groups[0]], sc[groups[1]] = 0.15, 0.4
    explicit = off[:, None] + sc[:, None] * Ft         # what the reference would rebuild on the host
    rng = np.random.default_rng(1)
    N = F.shape[1]
    G = np.zeros(N)
    g = 0.3 * rng.standard_normal(N)
    theta = 100.0
    f_o, grad_o, w_o = O.logw_fdf(g, G, explicit, YT, theta)
    with bioen_amd.Context(Ft, YT) as ctx:
        ctx.set_affine(off, sc)
        f, grad = ctx.logw_fdf(g, G, theta)
        chi2, yraw = ctx.chi_squared(w_o)
        gopt, w, info = ctx.opt_lbfgs_logw(G, G, theta, dict(linesearch=2, max_iterations=5000, delta=1e-11,
                                                             epsilon=1e-7, ftol=1e-5, gtol=0.9, wolfe=0.9, past=10,
                                                             max_linesearch=100))
        ctx.set_affine(None, None)
        f_plain, _ = ctx.logw_fdf(g, G, theta)
    assert rel(f, f_o) < 1e-12
    assert np.abs(grad - grad_o).max() <= 1e-10 * np.abs(grad_o).max()
    assert np.abs(yraw - Ft.dot(w_o)).max() <= 1e-12 * np.abs(Ft.dot(w_o)).max()
    assert rel(chi2, 0.5 * np.sum((explicit.dot(w_o) - YT) ** 2)) < 1e-12
    g2, fmin_o, code_o, it_o, ev_o = O.opt_lbfgs_logw(G, G, explicit, YT, theta, dict(epsilon=1e-7, delta=1e-11))
    assert info.lbfgs_code in (0, 1) and rel(info.fmin, fmin_o) < 1e-6
    f_plain_o, _, _ = O.logw_fdf(g, G, Ft, YT, theta)
    assert rel(f_plain, f_plain_o) < 1e-12             # switched back to the plain model


@pytest.mark.parametrize("linesearch", [0, 2])
def test_last_average_is_that_of_the_returned_point(optimize, linesearch):
    """bioen_hip_last_average after an optimisation = yTilde . w_opt, whichever column of the round's compact
    layout the final evaluation sat in (with trial steps speculated in idle slots the round is wider than 1)."""
    import bioen_amd
    rng = np.random.default_rng(5)
    M, N = 23, 1500
    Y = rng.standard_normal((M, N))
    YT = Y.dot(rng.dirichlet(np.ones(N))) + 0.05 * rng.standard_normal(M)
    G = np.zeros(N)
    for theta in (0.5, 50.0):
        with bioen_amd.Context(Y, YT) as ctx:
            g, w, info = ctx.opt_lbfgs_logw(G, G, theta, dict(linesearch=linesearch, max_iterations=5000, epsilon=1e-8, delta=0.0, past=0,
                                                             ftol=1e-5, gtol=0.9, wolfe=0.9, max_linesearch=100))
            yraw, yeff = ctx.last_average()
            assert info.lbfgs_code in (0, 1, 2, -998, -1001)
            ref = Y.dot(w)
            assert np.abs(yraw - ref).max() <= 1e-12 * np.abs(ref).max() + 1e-14
            assert np.array_equal(yraw, yeff)
            f, _ = ctx.logw_fdf(g, G, theta)
            assert np.abs(ctx.last_average()[0] - ref).max() <= 1e-12 * np.abs(ref).max() + 1e-14


@pytest.mark.parametrize("M,N", [(37, 1000), (205, 4099), (512, 3000), (600, 2000), (1100, 1500)])
def test_strip_copies_replace_the_rowmajor_matrix(optimize, M, N):
    """For M <= 1024 the strip copies hold the raw matrix and take the row-major one's place: 2 x the matrix for the
    log-weights method, 1 x for the forces method -- and read_ytilde still hands back the caller's numbers bit for bit,
    chi_squared still takes ANY w.  A call that needs the row-major form again (forces_weights' streaming kernels) gets
    it back from the strip copy."""
    import bioen_amd
    rng = np.random.default_rng(M + N)
    Y = rng.normal(3.0, 2.0, (M, N))
    YT = Y.dot(rng.dirichlet(np.ones(N))) + 0.1 * rng.standard_normal(M)
    G = np.zeros(N)
    w_any = rng.uniform(0.0, 2.0, N)                       # not normalised
    params = dict(linesearch=2, max_iterations=30, delta=1e-6, epsilon=1e-6, ftol=1e-5, gtol=0.9, wolfe=0.9, past=10,
                  max_linesearch=100)
    from bioen_amd._lib import column_segments
    unit = M * column_segments(N)[2] * 8                  # lower bound of one copy: 8 column segments, each padded to 128
    with bioen_amd.Context(Y, YT) as ctx:
        assert ctx.footprint()[0] == {"rowmajor"}
        assert np.array_equal(ctx.read_ytilde(), Y)
        chi2_before, yave_before = ctx.chi_squared(w_any)
        assert np.abs(yave_before - Y.dot(w_any)).max() <= 1e-12 * np.abs(Y.dot(w_any)).max()
        ctx.opt_lbfgs_logw(G, G, 10.0, params)
        forms, nbytes = ctx.footprint()
        if M <= 1024:
            assert forms == {"strips", "strips_colsum"} and nbytes < 2.2 * unit + (1 << 20)
        else:                                                  # row panels of <= 1024 rows, both orders: 2 x as well
            assert forms == {"strips", "strips_colsum"} and nbytes < 2.2 * unit + (1 << 20)
        assert np.array_equal(ctx.read_ytilde(), Y)                                   # the whole matrix, bit for bit
        assert np.array_equal(ctx.read_ytilde(M // 2, 1, N // 3, 5), Y[M // 2:M // 2 + 1, N // 3:N // 3 + 5])
        chi2, yave = ctx.chi_squared(w_any)
        assert np.abs(yave - Y.dot(w_any)).max() <= 1e-12 * np.abs(Y.dot(w_any)).max()
        assert rel(chi2, 0.5 * np.sum((Y.dot(w_any) - YT) ** 2)) < 1e-12
        f, g = ctx.forces_fdf(1e-3 * rng.standard_normal(M), np.full(N, 1.0 / N), 5.0)
        assert ctx.footprint()[0] == {"strips", "strips_colsum"}                      # the forces passes read the same copies
        assert np.array_equal(ctx.read_ytilde(), Y)
    with bioen_amd.Context(Y, YT) as ctx:                                             # a forces-only context
        ctx.forces_fdf(1e-3 * rng.standard_normal(M), np.full(N, 1.0 / N), 5.0)
        forms, nbytes = ctx.footprint()
        # M > 1024: both orders of the row panels (the forces method's four passes: column sums and row sums)
        assert forms == ({"strips"} if M <= 1024 else {"strips", "strips_colsum"})
        w = ctx.forces_weights(np.zeros(M), np.full(N, 1.0 / N))                      # streaming kernels: row-major again
        assert np.abs(w - 1.0 / N).max() < 1e-18 + 1e-12 / N
        assert np.array_equal(ctx.read_ytilde(), Y)


@pytest.mark.parametrize("M", [23, 600, 1100])
def test_last_average_after_forces_calls(optimize, M):
    """forces_fdf / opt_lbfgs_forces -> last_average hands out yTilde . w at the point the call ended on, on all three
    matrix-pass families (M <= 512 and 512 < M <= 1024: the two strip kernels on the raw copy, which keep ybar - centre on
    the device; beyond: streaming passes).  After a multi-problem call there is nothing to hand out."""
    import bioen_amd
    rng = np.random.default_rng(11)
    N = 900
    Y = rng.standard_normal((M, N)) + 3.0
    w0 = rng.dirichlet(np.ones(N) * 2.0)
    YT = Y.dot(rng.dirichlet(np.ones(N))) + 0.05 * rng.standard_normal(M)
    with bioen_amd.Context(Y, YT) as ctx:
        f = 1e-3 * rng.standard_normal(M)
        ctx.forces_fdf(f, w0, 5.0)
        w = ctx.forces_weights(f, w0)
        ctx.forces_fdf(f, w0, 5.0)
        yraw, yeff = ctx.last_average()
        ref = Y.dot(w)
        assert np.abs(yraw - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(yraw, yeff)
        fopt, wopt, info = ctx.opt_lbfgs_forces(np.zeros(M), w0, 50.0, dict(linesearch=2, max_iterations=200, delta=1e-8,
                                                                           epsilon=1e-6, ftol=1e-5, gtol=0.9, wolfe=0.9,
                                                                           past=10, max_linesearch=100))
        ref = Y.dot(wopt)
        assert np.abs(ctx.last_average()[0] - ref).max() <= 1e-12 * np.abs(ref).max()
        ctx.forces_fdf_batch(np.stack([f, 2 * f]), w0, [5.0, 1.0])
        with pytest.raises(bioen_amd.BioenHipError):
            ctx.last_average()
        ctx.chi_squared(w)                                     # a single-problem call makes it valid again
        assert np.abs(ctx.last_average()[0] - Y.dot(w)).max() <= 1e-12 * np.abs(ref).max()


def test_nuisance_series_matches_host_rebuild_loop(optimize):
    """The device loop (matrix resident, parameters through set_affine) against the reference's protocol done the slow
    way -- rebuild yTilde(m) on the host every iteration (observables.py:110-143), optimise with the oracle, refit m on
    chi^2 (observables.py:146-171, 205-210) -- with BOTH sides run to convergence (epsilon = 1e-9, no plateau test) and
    BOTH refits taken at the exact optimum of the parabola chi^2(m) (the reference's leastsq converges to it within
    its own tolerance, which is why it is not the yardstick here): north_star's tolerances as they stand, 1e-6 on the
    negative log-posterior, 1e-5 max(w) on the weights, and 1e-8 on the fitted modulation depths."""
    import bioen_amd
    from bioen_amd import nuisance
    from oracle import oracle_binding as O
    F, sigma, groups, Y, m_true = _deer_problem()
    Ft = (F - 1.0) / sigma[:, None]
    YT = Y / sigma
    off = 1.0 / sigma
    N = F.shape[1]
    G = np.zeros(N)
    conv = dict(linesearch=2, max_iterations=200000, delta=0.0, epsilon=1e-9, ftol=1e-5, gtol=0.9, wolfe=0.9,
                past=0, max_linesearch=100)
    at_optimum = (0, 1, 2, -998, -1000, -1001)     # gradient test | rounding floor of the line search
    thetas = [100.0, 10.0]
    with bioen_amd.Context(Ft, YT) as ctx:
        res = nuisance.series(ctx, thetas, G, G, conv, YT, groups=groups, row_offset=off, scale0=0.15,
                              iterations=6, accept_codes=at_optimum)
    m = [0.15, 0.15]
    for k, theta in enumerate(thetas):
        for _ in range(6):
            explicit = np.empty_like(Ft)
            for mv, ix in zip(m, groups):
                explicit[ix] = (1 - mv + mv * F[ix]) / sigma[ix, None]
            g, fmin, code, it, ev = O.opt_lbfgs_logw(G, G, explicit, YT, theta, conv)
            assert code in at_optimum
            w = O.logw_weights(g)[0]
            # chi^2(m) = 0.5 sum_i (1/sigma_i + m Ft_i.w - YT_i)^2 is a parabola: its minimiser in closed form, from the
            # host's own GEMV of the m-independent matrix
            m = nuisance.refit_scales(Ft.dot(w), YT, off, groups)
        assert rel(res[k]["fmin"], fmin) < 1e-6, (theta, res[k]["fmin"], fmin)
        assert np.abs(np.asarray(res[k]["scales"]) - np.asarray(m)).max() <= 1e-8, (theta, res[k]["scales"], m)
        assert np.abs(res[k]["w"] - w).max() <= 1e-5 * w.max(), (theta, np.abs(res[k]["w"] - w).max() / w.max())
    # the refits recover the modulation depths the data were generated with
    assert np.allclose(res[-1]["scales"], m_true, atol=0.03)


# ---------------------------------------------------------------------------------------
# yTilde assembled on the device from raw observables
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 1), (7, 33), (37, 1000), (130, 4099)])
def test_context_from_raw_observables_equals_host_division(M, N):
    import bioen_amd
    rng = np.random.default_rng(M * 7919 + N)
    sim = rng.normal(5.0, 2.0, (M, N))
    exp = rng.normal(5.0, 0.5, M)
    err = rng.uniform(0.05, 2.0, M)
    yTilde, YTilde = sim / err[:, None], exp / err
    g = 0.3 * rng.standard_normal(N)
    G = np.zeros(N)
    with bioen_amd.Context(yTilde, YTilde) as ref:
        f_ref, grad_ref = ref.logw_fdf(g, G, 3.0)
    for structure_major in (False, True):
        src = np.ascontiguousarray(sim.T) if structure_major else sim
        with bioen_amd.Context.from_raw(src, exp, err, structure_major=structure_major) as ctx:
            assert ctx.m == M and ctx.n == N
            assert np.array_equal(ctx.read_ytilde(), yTilde)          # true division on the device: same bits
            f, grad = ctx.logw_fdf(g, G, 3.0)
        assert f == f_ref and np.array_equal(grad, grad_ref)
    with pytest.raises(bioen_amd.BioenHipError):
        bioen_amd.Context.from_raw(sim, exp, np.zeros(M))
    with pytest.raises(ValueError):
        bioen_amd.Context.from_raw(sim, exp[:-1] if M > 1 else np.zeros(2), err)


def test_find_optimum_series_equals_find_optimum_per_theta(optimize):
    d = load_golden("synth_logw_M64xN2000.npz")
    YT = d["YTilde"].reshape(1, -1)
    params = optimize.minimize.Parameters("lbfgs")
    params["verbose"] = False
    thetas = [100.0, 10.0, 1.0]
    series = optimize.log_weights.find_optimum_series(d["GInit"], d["G"], d["y"], d["yTilde"], YT, thetas, params)
    for theta, got in zip(thetas, series):
        ref = optimize.log_weights.find_optimum(d["GInit"], d["G"], d["y"], d["yTilde"], YT, theta, params)
        assert got[4] == ref[4] and got[3] == ref[3]
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    with pytest.raises(RuntimeError):
        optimize.log_weights.find_optimum_series(d["GInit"], d["G"], d["y"], d["yTilde"], YT, thetas,
                                                 optimize.minimize.Parameters("scipy"))


def test_read_probe_streams_the_resident_matrix(optimize):
    """bench.py's measured read ceiling: a plain read-only pass over whichever form of the matrix is resident."""
    import bioen_amd
    rng = np.random.default_rng(3)
    M, N = 300, 40000
    Y = rng.standard_normal((M, N))
    with bioen_amd.Context(Y, Y.mean(axis=1)) as ctx:
        gbs, nbytes = ctx.read_probe(reps=3)
        assert nbytes == ctx.footprint()[1] and gbs > 50.0                  # row-major form
        ctx.logw_fdf(np.zeros(N), np.zeros(N), 1.0)                          # builds the strip copies, frees the row-major one
        gbs2, nbytes2 = ctx.read_probe(reps=3)
        from bioen_amd._lib import column_segments
        assert nbytes2 == column_segments(N)[2] * 304 * 8 and gbs2 > 50.0     # one strip copy: rows padded to 16, 8 column segments
        assert np.array_equal(ctx.read_ytilde(), Y)


def test_two_threads_two_contexts_equal_the_serial_runs():
    """SURVEY 8(b) threading: the reference is not re-entrant (globals in its C files); here all state is per context and
    ctypes releases the GIL: two threads driving two contexts at once -- both methods, batched -- return the bits of the
    runs done one after the other."""
    import threading
    import bioen_amd
    from conftest import LBFGS_DEFAULTS
    params = dict(LBFGS_DEFAULTS, max_iterations=60)

    def problem(M, N, seed):
        rng = np.random.default_rng(seed)
        YTrue = rng.uniform(1, 10, M)
        y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
        return y, rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)

    jobs = [problem(96, 30000, 1), problem(600, 9000, 2)]
    thetas = [100.0, 10.0, 1.0]

    def solve(ctx, M, N):
        G, w0 = np.zeros(N), np.full(N, 1.0 / N)
        a = ctx.opt_lbfgs_logw_batch(thetas, G, G, params)
        b = ctx.opt_lbfgs_forces_batch(thetas, np.zeros(M), w0, params)
        return [a[0].tobytes(), a[1].tobytes(), [i.fmin for i in a[2]], b[0].tobytes(), b[1].tobytes(), [i.fmin for i in b[2]]]

    ctxs = [bioen_amd.Context(y, YT) for y, YT in jobs]
    try:
        serial = [solve(c, *j[0].shape) for c, j in zip(ctxs, jobs)]
        out, errs = [None, None], []

        def work(k):
            try:
                for _ in range(3):
                    out[k] = solve(ctxs[k], *jobs[k][0].shape)
                    assert out[k] == serial[k]
            except Exception as e:          # surfaces in the main thread below
                errs.append(repr(e))
        ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert out == serial
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("engine", ["device", "host"])
def test_without_the_weights_the_optima_are_the_same(engine, monkeypatch):
    """w_opt = NULL in the C ABI (want_weights=False): nothing but the hand-out of the weights is skipped -- optimum,
    objective and counts of every problem keep their bits, both methods, batched and single, both engines."""
    import bioen_amd
    from conftest import LBFGS_DEFAULTS
    monkeypatch.setenv("BIOEN_HIP_DEVICE_LS", "1" if engine == "device" else "0")
    rng = np.random.default_rng(8)
    M, N = 80, 6000
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G, w0, f0 = np.zeros(N), np.full(N, 1.0 / N), np.zeros(M)
    params = dict(LBFGS_DEFAULTS, max_iterations=50)
    thetas = [100.0, 10.0, 1.0]

    def sig(infos):
        return [(i.fmin, i.iterations, i.evaluations, i.lbfgs_code, i.chi2, i.kl) for i in infos]

    with bioen_amd.Context(y, YT) as ctx:
        a = ctx.opt_lbfgs_logw_batch(thetas, G, G, params)
        b = ctx.opt_lbfgs_logw_batch(thetas, G, G, params, want_weights=False)
        assert b[1] is None and np.array_equal(a[0], b[0]) and sig(a[2]) == sig(b[2])
        c1 = ctx.opt_lbfgs_logw(G, G, 10.0, params, want_weights=False)
        assert c1[1] is None and np.array_equal(c1[0], a[0][1]) and sig([c1[2]]) == sig([a[2][1]])
        fa = ctx.opt_lbfgs_forces_batch(thetas, f0, w0, params)
        fb = ctx.opt_lbfgs_forces_batch(thetas, f0, w0, params, want_weights=False)
        assert fb[1] is None and np.array_equal(fa[0], fb[0]) and sig(fa[2]) == sig(fb[2])
        fc = ctx.opt_lbfgs_forces(f0, w0, 10.0, params, want_weights=False)
        assert fc[1] is None and np.array_equal(fc[0], fa[0][1]) and sig([fc[2]]) == sig([fa[2][1]])


def test_the_two_methods_leave_nothing_behind_for_each_other():
    """Both methods share the batch slots' N-vectors (weights, adjoint / x_j, direction / t): a forces series after a
    log-weights series on the same context -- and the other way round, and evaluations in between -- returns the bits it
    returns on a fresh context."""
    import bioen_amd
    from conftest import LBFGS_DEFAULTS
    rng = np.random.default_rng(9)
    M, N = 72, 5001                      # odd N: the last pair of every N-vector is half padding
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    w0 = rng.dirichlet(np.ones(N) * 2.0)
    f0 = np.zeros(M)
    params = dict(LBFGS_DEFAULTS, max_iterations=40)
    thetas = [30.0, 3.0, 0.3]

    def logw(ctx):
        r = ctx.opt_lbfgs_logw_batch(thetas, G, G, params)
        f, g = ctx.logw_fdf(G + 0.05, G, 2.0)
        return (r[0].tobytes(), r[1].tobytes(), [i.fmin for i in r[2]], f, g.tobytes(), ctx.logw_weights(G + 0.05)[0].tobytes())

    def forces(ctx):
        r = ctx.opt_lbfgs_forces_batch(thetas, f0, w0, params)
        f, g = ctx.forces_fdf(f0 + 1e-3, w0, 2.0)
        return (r[0].tobytes(), r[1].tobytes(), [i.fmin for i in r[2]], f, g.tobytes(), ctx.forces_weights(f0 + 1e-3, w0).tobytes())

    with bioen_amd.Context(y, YT) as ctx:
        fresh_l = logw(ctx)
    with bioen_amd.Context(y, YT) as ctx:
        fresh_f = forces(ctx)
    with bioen_amd.Context(y, YT) as ctx:
        assert logw(ctx) == fresh_l and forces(ctx) == fresh_f and logw(ctx) == fresh_l and forces(ctx) == fresh_f
    with bioen_amd.Context(y, YT) as ctx:
        assert forces(ctx) == fresh_f and logw(ctx) == fresh_l


def test_randomised_context_data_paths():
    """tools/fuzz_context.py as a test: 25 random shapes -- assembly from raw observables (row-major and structure-major),
    read-back of random blocks before and after the strip copies replace the matrix (bit for bit), the affine model against a
    rebuilt matrix, the plain model's bits back after it, a changed target against a fresh context."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "fuzz_context", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_context.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    bad = fuzz.run(0, 25)
    assert not bad, bad


def test_structures_reordered_in_place_are_not_served_from_the_cached_copy(optimize):
    """The context cache's content check is a hash of the host matrix's bytes: two structures swapped IN PLACE (sums over the
    buffer do not move -- the check of r01-r03 did not see it), or the smallest possible nudge of one number, upload afresh."""
    from bioen_amd.optimize.ext import c_bioen
    d = load_golden("synth_logw_M64xN2000.npz")
    c_bioen.clear_cache()
    y = d["yTilde"].copy()
    YT = d["YTilde"].reshape(1, -1)
    rng = np.random.default_rng(4)
    g = d["GInit"].ravel() + 0.3 * rng.standard_normal(y.shape[1])
    lp = optimize.log_weights.bioen_log_posterior
    f0 = lp(g, d["GInit"], d["G"], y, YT, 1.0)
    y[:, [10, 1500]] = y[:, [1500, 10]]                       # structures 10 and 1500 change places; g stays
    f1 = lp(g, d["GInit"], d["G"], y, YT, 1.0)
    fresh = lp(g, d["GInit"], d["G"], y.copy(), YT, 1.0)
    assert f1 == fresh and f1 != f0
    y[7, 123] = np.nextafter(y[7, 123], np.inf)               # one ulp in one number
    ctx_before = next(reversed(c_bioen._CACHE.values()))
    lp(g, d["GInit"], d["G"], y, YT, 1.0)
    assert c_bioen._CACHE[id(y)] is not ctx_before
    c_bioen.clear_cache()


@pytest.mark.parametrize("M,N", [(96, 4000), (600, 3000), (1100, 2500)])
@pytest.mark.parametrize("fail_at", [1, 2])
def test_a_strip_copy_that_cannot_be_allocated_falls_back_to_the_streaming_kernels(M, N, fail_at, monkeypatch):
    """An exhausted device while the strip copies are built (the k-th allocation fails: BIOEN_HIP_TEST_FAIL_STRIP_ALLOC) must
    leave a context that still answers correctly -- on the streaming kernels over the row-major matrix, for good; or, when
    only the SECOND copy of a matrix of at most 1024 rows is missing, on the one strip copy there is (r05: the adjoint
    through the forces kernels' LDS image) -- not one that mixes kernel families inside an evaluation or holds half a copy:
    objective, gradient and short runs of both methods against the restatement, the matrix still readable bit for bit, a
    second series the same as the first."""
    import bioen_amd
    from oracle import oracle_binding as O
    from conftest import LBFGS_DEFAULTS
    rng = np.random.default_rng(M + fail_at)
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    g = G + 0.2 * rng.standard_normal(N)
    w0 = rng.dirichlet(np.ones(N) * 2.0)
    f0 = 1e-3 * rng.standard_normal(M)
    params = dict(LBFGS_DEFAULTS, max_iterations=8)
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", str(fail_at))
    with bioen_amd.Context(y, YT) as ctx:
        f, grad = ctx.logw_fdf(g, G, 5.0)
        ff, fgrad = ctx.forces_fdf(f0, w0, 5.0)
        a = ctx.opt_lbfgs_logw_batch([50.0, 5.0], g, G, params)
        b = ctx.opt_lbfgs_forces_batch([50.0, 5.0], f0, w0, params)
        a2 = ctx.opt_lbfgs_logw_batch([50.0, 5.0], g, G, params)
        assert np.array_equal(a[0], a2[0]) and [i.fmin for i in a[2]] == [i.fmin for i in a2[2]]
        assert np.array_equal(ctx.read_ytilde(), y)
        forms, _ = ctx.footprint()
    f_o, grad_o, _ = O.logw_fdf(g, G, y, YT, 5.0)
    ff_o, fgrad_o, _ = O.forces_fdf(f0, w0, y, YT, 5.0)
    assert abs(f - f_o) <= 1e-12 * abs(f_o) and np.abs(grad - grad_o).max() <= 1e-10 * np.abs(grad_o).max()
    assert abs(ff - ff_o) <= 1e-12 * abs(ff_o) and np.abs(fgrad - fgrad_o).max() <= 1e-9 * np.abs(fgrad_o).max()
    for k, th in enumerate([50.0, 5.0]):
        _, fmin_o, code_o, it_o, ev_o = O.opt_lbfgs_logw(g, G, y, YT, th, params)
        assert (a[2][k].lbfgs_code, a[2][k].iterations) == (code_o, it_o) and abs(a[2][k].fmin - fmin_o) <= 1e-8 * abs(fmin_o)
        _, ffmin_o, fcode_o, fit_o, fev_o = O.opt_lbfgs_forces(f0, w0, y, YT, th, params)
        assert (b[2][k].lbfgs_code, b[2][k].iterations) == (fcode_o, fit_o) and abs(b[2][k].fmin - ffmin_o) <= 1e-8 * abs(ffmin_o)
    if fail_at == 2 and M <= 1024:
        assert forms == {"strips"}                  # one strip copy serves both matrix passes
    else:
        assert "rowmajor" in forms                  # what the streaming kernels read


@pytest.mark.parametrize("M,N", [(37, 1000), (205, 4099), (512, 3000), (600, 2000), (1024, 1500), (1100, 1500), (2100, 1000)])
def test_log_weights_on_one_strip_copy(M, N, monkeypatch):
    """BIOEN_HIP_ONE_COPY=1 (r05): the log-weights method with ONE strip copy of the matrix resident -- the forward pass as
    always, the adjoint on the same row-sum order copy through the forces kernels' LDS image (k_strip / k_strip2, ADJ form).
    Objective and gradient against the restatement at every batch width, capped series step for step, and against the
    two-copy default (another order of the sums over rows: last bits only).  Beyond 1024 rows: panel by panel, the column
    sums continued from panel to panel -- both methods on the one set of row panels."""
    import bioen_amd
    from oracle import oracle_binding as O
    from conftest import LBFGS_DEFAULTS
    rng = np.random.default_rng(3 * M + 1)
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    g = G + 0.2 * rng.standard_normal(N)
    thetas = [300.0, 100.0, 30.0, 10.0, 3.0, 1.0, 0.3, 0.1]
    params = dict(LBFGS_DEFAULTS, max_iterations=10)
    with bioen_amd.Context(y, YT) as ctx:
        two = ctx.opt_lbfgs_logw_batch(thetas, g, G, params)
        f2, grad2 = ctx.logw_fdf(g, G, 5.0)
        assert ctx.footprint()[0] == {"strips", "strips_colsum"}
        with pytest.raises(bioen_amd.BioenHipError):
            ctx.set_one_copy(True)                   # too late: the second copy exists
    with bioen_amd.Context(y, YT) as ctx:           # the switch on a live context, before its first gradient evaluation
        ctx.set_one_copy(True)
        fs, grads = ctx.logw_fdf(g, G, 5.0)
        assert ctx.footprint()[0] == {"strips"}
    monkeypatch.setenv("BIOEN_HIP_ONE_COPY", "1")
    with bioen_amd.Context(y, YT) as ctx:
        f, grad = ctx.logw_fdf(g, G, 5.0)
        assert f == fs and np.array_equal(grad, grads)
        one = ctx.opt_lbfgs_logw_batch(thetas, g, G, params)                     # K = 8: the two-quad form
        one3 = ctx.opt_lbfgs_logw_batch(thetas[:3], g, G, params)
        gg, wg, ig = ctx.opt_gsl_logw(g, G, 5.0, "bfgs2", dict(step_size=0.01, tol=1e-3, max_iterations=10))
        w0 = rng.dirichlet(np.ones(N) * 2.0)
        f0 = 1e-3 * rng.standard_normal(M)
        ff, fgrad = ctx.forces_fdf(f0, w0, 5.0)      # beyond 1024 rows: the forces method's four passes on the one set of panels
        assert ctx.footprint()[0] == {"strips"}
        assert np.array_equal(ctx.read_ytilde(), y)
    ff_o, fgrad_o, _ = O.forces_fdf(f0, w0, y, YT, 5.0)
    assert abs(ff - ff_o) <= 1e-12 * abs(ff_o) and np.abs(fgrad - fgrad_o).max() <= 1e-9 * np.abs(fgrad_o).max()
    f_o, grad_o, _ = O.logw_fdf(g, G, y, YT, 5.0)
    assert abs(f - f_o) <= 1e-12 * abs(f_o) and np.abs(grad - grad_o).max() <= 1e-10 * np.abs(grad_o).max()
    assert f == f2 and np.abs(grad - grad2).max() <= 1e-12 * np.abs(grad2).max()
    for k, th in enumerate(thetas):
        _, fmin_o, code_o, it_o, ev_o = O.opt_lbfgs_logw(g, G, y, YT, th, params)
        assert (one[2][k].lbfgs_code, one[2][k].iterations, one[2][k].evaluations) == (code_o, it_o, ev_o)
        assert abs(one[2][k].fmin - fmin_o) <= 1e-8 * abs(fmin_o)
        assert abs(one[2][k].fmin - two[2][k].fmin) <= 1e-9 * abs(two[2][k].fmin)
    for k in range(3):                               # a problem's bits do not depend on the width of its batch
        assert np.array_equal(one3[0][k], one[0][k]) and one3[2][k].fmin == one[2][k].fmin
    assert np.isfinite(ig.fmin) and abs(wg.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("M,N", [(37, 1000), (205, 20000), (512, 3000), (1024, 5000), (1100, 1500)])
def test_strip_layout_follows_the_method_and_changes_no_bit(M, N, monkeypatch):
    """r06: the row-sum order strip copy holds the local segments' strips INTERLEAVED for the log-weights passes (one
    contiguous window of the copy is read at any moment, csrc/strip.hpp: strip_phys) and in strip order for the forces
    passes; a context that changes method moves the copy.  Which layout served a call must not show in any bit: objective,
    gradient, capped batches of both methods, the matrix read back -- against a context that never interleaves
    (BIOEN_HIP_STRIP_INTERLEAVE=0, the r05 layout) and across the moves."""
    import bioen_amd
    from conftest import LBFGS_DEFAULTS
    rng = np.random.default_rng(5 * M + 3)
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    g = G + 0.2 * rng.standard_normal(N)
    w0 = rng.dirichlet(np.ones(N) * 2.0)
    f0 = 1e-3 * rng.standard_normal(M)
    thetas = [100.0, 10.0, 1.0, 0.3, 30.0, 3.0]
    params = dict(LBFGS_DEFAULTS, max_iterations=8)

    def run(ctx, order):
        out = {}
        for what in order:
            if what == "logw":
                out["logw"] = (ctx.logw_fdf(g, G, 5.0), ctx.opt_lbfgs_logw_batch(thetas, g, G, params))
                out["layout_logw"] = ctx.layout()
            else:
                out["forces"] = (ctx.forces_fdf(f0, w0, 5.0), ctx.opt_lbfgs_forces_batch(thetas, f0, w0, params))
                out["layout_forces"] = ctx.layout()
            assert np.array_equal(ctx.read_ytilde(), y)              # the caller's numbers, whichever layout holds them
        return out

    def same(a, b):
        (fa, ga), (xa, wa, ia) = a
        (fb, gb), (xb, wb, ib) = b
        assert fa == fb and np.array_equal(ga, gb)
        for k in range(len(thetas)):
            assert np.array_equal(xa[k], xb[k]) and np.array_equal(wa[k], wb[k])
            assert (ia[k].fmin, ia[k].iterations, ia[k].evaluations, ia[k].lbfgs_code) == \
                   (ib[k].fmin, ib[k].iterations, ib[k].evaluations, ib[k].lbfgs_code)

    with bioen_amd.Context(y, YT) as ctx:
        a = run(ctx, ["logw", "forces", "logw"])
        assert a["layout_logw"]["interleave"] == 8                  # one GPU holds the eight canonical segments
        if M <= 1024:                                                # (beyond: the forces method runs the log-weights kernels on row panels)
            assert a["layout_forces"]["interleave"] == 1 and a["layout_logw"]["relayouts"] == 2
    with bioen_amd.Context(y, YT) as ctx:
        b = run(ctx, ["forces", "logw"])
    monkeypatch.setenv("BIOEN_HIP_STRIP_INTERLEAVE", "0")
    with bioen_amd.Context(y, YT) as ctx:
        c = run(ctx, ["logw", "forces"])
        assert c["layout_logw"] == {"one_copy": 0, "interleave": 1, "relayouts": 0}
    for other in (b, c):
        same(a["logw"], other["logw"])
        same(a["forces"], other["forces"])


def test_a_strip_copy_that_cannot_be_moved_stays_and_serves(monkeypatch):
    """The move of the row-sum order copy into the other method's layout is best effort: when the buffer for it cannot be
    allocated (forced here: the context's third strip allocation fails) the copy stays as it is -- every kernel reads
    either layout -- and not a bit of the results changes."""
    import bioen_amd
    M, N = 300, 6000
    rng = np.random.default_rng(99)
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    g = G + 0.2 * rng.standard_normal(N)
    w0 = rng.dirichlet(np.ones(N) * 2.0)
    f0 = 1e-3 * rng.standard_normal(M)
    with bioen_amd.Context(y, YT) as ctx:
        ref_l = ctx.logw_fdf(g, G, 5.0)
        ref_f = ctx.forces_fdf(f0, w0, 5.0)
        assert ctx.layout() == {"one_copy": 0, "interleave": 1, "relayouts": 1}
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "3")          # 1, 2: the two strip copies; 3: the move's buffer
    with bioen_amd.Context(y, YT) as ctx:
        got_l = ctx.logw_fdf(g, G, 5.0)
        got_f = ctx.forces_fdf(f0, w0, 5.0)                              # wants strip order, cannot have it
        assert ctx.layout() == {"one_copy": 0, "interleave": 8, "relayouts": 0}
        again = ctx.forces_fdf(f0, w0, 5.0)                              # (tries again: this time the buffer is there)
        assert ctx.layout()["interleave"] == 1
        assert np.array_equal(ctx.read_ytilde(), y)
    assert got_l[0] == ref_l[0] and np.array_equal(got_l[1], ref_l[1])
    for r in (got_f, again):
        assert r[0] == ref_f[0] and np.array_equal(r[1], ref_f[1])


@pytest.mark.parametrize("M,N", [(37, 3000), (512, 20000), (1024, 6000), (1100, 3000)])
def test_single_segment_opt_out_on_one_gpu(M, N, monkeypatch):
    """BIOEN_HIP_SEGMENTS=1 (r06): an unsharded context with ONE column segment instead of the canonical eight -- every
    sum over structures one tree over the whole matrix (r04's shape: the forces passes write one partial set per block).
    The same mathematics in another summation order: objective and gradient of both methods against the restatement at the
    default context's tolerances, against the default context to rounding, batched = single bit for bit, and capped series
    step for step with the restatement."""
    import bioen_amd
    from oracle import oracle_binding as O
    from conftest import LBFGS_DEFAULTS
    rng = np.random.default_rng(11 * M + 5)
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    g = G + 0.2 * rng.standard_normal(N)
    w0 = rng.dirichlet(np.ones(N) * 2.0)
    f0 = 1e-3 * rng.standard_normal(M)
    thetas = [100.0, 10.0, 1.0, 30.0, 3.0]
    params = dict(LBFGS_DEFAULTS, max_iterations=8)
    with bioen_amd.Context(y, YT) as ctx:
        f8, g8 = ctx.logw_fdf(g, G, 5.0)
        ff8, fg8 = ctx.forces_fdf(f0, w0, 5.0)
    assert bioen_amd._lib.column_segments(N)[0] == 8
    monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")
    assert bioen_amd._lib.column_segments(N)[0] == 1
    with bioen_amd.Context(y, YT) as ctx:
        f1, g1 = ctx.logw_fdf(g, G, 5.0)
        ff1, fg1 = ctx.forces_fdf(f0, w0, 5.0)
        assert ctx.layout()["interleave"] == 1
        lw = ctx.opt_lbfgs_logw_batch(thetas, g, G, params)
        lf = ctx.opt_lbfgs_forces_batch(thetas, f0, w0, params)
        xs, ws, one = ctx.opt_lbfgs_logw(g, G, thetas[1], params)
        fs, wfs, onef = ctx.opt_lbfgs_forces(f0, w0, thetas[1], params)
        assert np.array_equal(ctx.read_ytilde(), y)
    assert np.array_equal(lw[0][1], xs) and lw[2][1].fmin == one.fmin            # a problem's bits do not depend on its batch
    assert np.array_equal(lf[0][1], fs) and lf[2][1].fmin == onef.fmin
    f_o, g_o, _ = O.logw_fdf(g, G, y, YT, 5.0)
    ff_o, fg_o, _ = O.forces_fdf(f0, w0, y, YT, 5.0)
    assert abs(f1 - f_o) <= 1e-12 * abs(f_o) and np.abs(g1 - g_o).max() <= 1e-10 * np.abs(g_o).max()
    assert abs(ff1 - ff_o) <= 1e-12 * abs(ff_o) and np.abs(fg1 - fg_o).max() <= 1e-9 * np.abs(fg_o).max()
    assert abs(f1 - f8) <= 1e-13 * abs(f8) and np.abs(g1 - g8).max() <= 1e-11 * np.abs(g8).max()      # another order of the same sums
    assert abs(ff1 - ff8) <= 1e-13 * abs(ff8) and np.abs(fg1 - fg8).max() <= 1e-10 * np.abs(fg8).max()
    for k, th in enumerate(thetas):
        _, fmin_o, code_o, it_o, ev_o = O.opt_lbfgs_logw(g, G, y, YT, th, params)
        assert (lw[2][k].lbfgs_code, lw[2][k].iterations, lw[2][k].evaluations) == (code_o, it_o, ev_o)
        assert abs(lw[2][k].fmin - fmin_o) <= 1e-8 * abs(fmin_o)
        _, ffmin_o, fcode_o, fit_o, fev_o = O.opt_lbfgs_forces(f0, w0, y, YT, th, params)
        assert (lf[2][k].lbfgs_code, lf[2][k].iterations) == (fcode_o, fit_o) and abs(lf[2][k].fmin - ffmin_o) <= 1e-8 * abs(ffmin_o)


@pytest.mark.parametrize("world", [1, 2])
def test_uploads_through_the_staging_buffer_change_nothing(world, monkeypatch):
    """api.hip: h2d_staged -- the path uploads of a caller's buffers take when the runtime refuses to pin them (ROCm 7.2: a
    pageable buffer on the address range of one it pinned before; tools/attic/onecopy_probe.py ran into it).  Forced here
    (BIOEN_HIP_TEST_STAGED_UPLOAD=1), in both directions: the matrix (row-major and assembled from raw observables in both
    layouts), N-vectors larger than one 8 MB chunk up and down (starts, priors; points, weights, read-back blocks), a column
    block of a sharded context -- the same bits as the direct copies."""
    import bioen_amd
    from conftest import LBFGS_DEFAULTS
    rng = np.random.default_rng(77)
    M, N = 40, 1200000                               # an N-vector of 9.6 MB: two chunks
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    G = np.log(rng.dirichlet(np.ones(N) * 2.0))
    g = G + 0.2 * rng.standard_normal(N)
    params = dict(LBFGS_DEFAULTS, max_iterations=5)

    def run():
        out = []
        kw = dict(device=0, rank=0, world=world) if world > 1 else {}
        with bioen_amd.Context(y, YT, **kw) as ctx:
            if world > 1:
                ctx.set_mirror_exchange(True)
            out.append(ctx.read_ytilde(0, M, 0, min(ctx.n_local, 5000)))
            f, grad = ctx.logw_fdf(g, G, 5.0)
            out += [np.float64(f), grad]
            r = ctx.opt_lbfgs_logw_batch([50.0, 5.0], g, G, params)
            out += [r[0], r[1], np.array([i.fmin for i in r[2]])]
            one = ctx.opt_lbfgs_logw(g, G, 5.0, params)             # the single-problem call: its own delivery of point and weights
            out += [one[0], one[1]]
            w0 = np.full(N, 1.0 / N)
            out.append(ctx.forces_weights(1e-3 * np.ones(M), w0))
            fr = ctx.opt_lbfgs_forces_batch([50.0, 5.0], np.zeros(M), w0, params)
            out += [fr[0], fr[1]]
        if world == 1:
            sim = y * (0.1 * YTrue[:, None])
            for major in (False, True):
                with bioen_amd.Context.from_raw(sim.T.copy() if major else sim, YT * 0.1 * YTrue, 0.1 * YTrue,
                                                structure_major=major) as ctx:
                    out.append(ctx.read_ytilde(0, M, 0, 4000))
        return out

    direct = run()
    monkeypatch.setenv("BIOEN_HIP_TEST_STAGED_UPLOAD", "1")
    staged = run()
    assert len(direct) == len(staged)
    for a, b in zip(direct, staged):
        assert np.array_equal(a, b)


def test_randomised_last_average_is_that_of_the_returned_weights():
    """tools/fuzz_last_average.py as a test: 50 random single-problem runs of both methods ending in every status (converged,
    plateau, budget, failed and refused searches that revert to the previous point), either engine, with and without an
    affine model -- the average left on the device for the nuisance refits equals yTilde . w of the returned weights."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "fuzz_la", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_last_average.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    bad, codes = fuzz.run(0, 50)
    assert not bad, bad
    assert len(codes) >= 4, codes


def test_randomised_calls_of_the_bioen_optimize_layer():
    """tools/fuzz_api.py as a test: 25 random find_optimum calls of both methods -- lbfgs, the five GSL algorithms, three scipy
    algorithms on the device or the numpy objective, ndarray or np.matrix inputs: tuple shapes as the reference documents
    them, weights normalised, fmin_final = f(returned point), yopt = y . wopt, fmin_final = theta S + chi^2 / 2, the lbfgs
    runs bit for bit the context-level call, statuses outside {0, 1, 2} raised as the reference raises them."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "fuzz_api", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_api.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    bad = fuzz.run(0, 25)
    assert not bad, bad

"""The dual Newton minimizer with the nuisance scales profiled out, its numpy statement in
bioen_amd/optimize/log_weights.py: the envelope gradient against central differences of the profile objective, the
projected covariance (bitwise symmetric, PSD, the step's z orthogonal to every vhat_k), and the optimum against the
alternation the reference's protocol runs -- a dual Newton optimisation on the explicit affine matrix, then
nuisance.refit_scales, until the scale stops moving."""
import numpy as np
import pytest

from bioen_amd import nuisance
from bioen_amd.optimize import log_weights as lw


def deer_problem(M1=60, M2=45, N=400, seed=3):
    """two synthetic DEER traces F(d_j, t_i) in (0, 1] with different modulation depths (tests/test_hip_api.py's
    construction) -> (Ft = (F - 1) / sigma, YT = Y / sigma, off = 1 / sigma, groups)"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(2.0, 6.0, N)

    def trace(t):
        return 0.5 * (1.0 + np.cos(2 * np.pi * 52.04 * t[:, None] / d[None, :] ** 3)) * np.exp(-0.2 * t[:, None])
    F = np.vstack([trace(np.linspace(0.0, 2.5, M1)), trace(np.linspace(0.0, 3.5, M2))])
    sigma = 0.01 * np.ones(M1 + M2)
    groups = [np.arange(M1), np.arange(M1, M1 + M2)]
    w_true = rng.dirichlet(np.ones(N) * 0.3)
    Y = np.empty(M1 + M2)
    for mt, ix in zip([0.22, 0.31], groups):
        Y[ix] = 1 - mt + mt * F[ix].dot(w_true)
    Y += sigma * rng.standard_normal(M1 + M2)
    return (F - 1.0) / sigma[:, None], Y / sigma, 1.0 / sigma, groups


def scattering_problem(M=40, N=300, seed=5):
    """intensities I_ij > 0 / sigma, the target 1.7 x a mixture's average plus noise: one scale, no offset"""
    rng = np.random.default_rng(seed)
    q = np.linspace(0.05, 1.0, M)
    rg = rng.uniform(1.0, 3.0, N)
    I = np.exp(-(q[:, None] * rg[None, :]) ** 2 / 3.0)
    sigma = 0.02
    Y = 1.7 * I.dot(rng.dirichlet(np.ones(N))) + sigma * rng.standard_normal(M)
    return I / sigma, Y / sigma, None, None


def _point(g, G, Y, YT, theta, groups, off):
    gr = lw._profile_groups(groups, Y.shape[0])
    o = np.zeros(Y.shape[0]) if off is None else off
    return lw._dual_newton_profile_point(g, G, Y, YT, theta, lw._log_sum_exp(G), gr, o), gr


@pytest.mark.parametrize("problem", [deer_problem, scattering_problem], ids=["deer", "scattering"])
def test_envelope_gradient_equals_central_differences(problem):
    Y, YT, off, groups = problem()
    n = Y.shape[1]
    rng = np.random.default_rng(11)
    G = np.log(rng.dirichlet(np.ones(n) * 5.0))
    g = G + 0.3 * rng.standard_normal(n)
    theta = 3.0
    p, _ = _point(g, G, Y, YT, theta, groups, off)
    scale = np.abs(p["grad"]).max()
    h = 1e-5
    for j in rng.choice(n, 12, replace=False):
        e = np.zeros(n)
        e[j] = h
        fd = (_point(g + e, G, Y, YT, theta, groups, off)[0]["f"] - _point(g - e, G, Y, YT, theta, groups, off)[0]["f"]) / (2 * h)
        # central differences of an f of size |f|: error ~ eps |f| / h + h^2 |f'''|
        assert abs(fd - p["grad"][j]) <= 1e-6 * scale + 4 * np.finfo(float).eps * abs(p["f"]) / h, (j, fd, p["grad"][j])
    # the profiled scales are refit_scales' at the raw averages
    assert np.allclose(p["scales"], nuisance.refit_scales(p["ybar"], YT, off, _point(g, G, Y, YT, theta, groups, off)[1]),
                       rtol=1e-14, atol=0)


@pytest.mark.parametrize("problem", [deer_problem, scattering_problem], ids=["deer", "scattering"])
def test_projected_covariance_and_step(problem):
    Y, YT, off, groups = problem()
    n = Y.shape[1]
    rng = np.random.default_rng(12)
    G = np.zeros(n)
    g = 0.5 * rng.standard_normal(n)
    theta = 2.0
    p, gr = _point(g, G, Y, YT, theta, groups, off)
    CP, bP, V = lw.dual_newton_profile_covariance(p, Y, gr)
    assert np.array_equal(CP, CP.T)
    ev = np.linalg.eigvalsh(CP)
    assert ev.min() >= -1e-12 * ev.max()
    assert np.abs(V.T.dot(bP)).max() <= 1e-12 * np.abs(bP).max()
    u, z = lw.dual_newton_profile_step(p, Y, theta, gr)
    assert np.abs(V.T.dot(z)).max() <= 1e-12 * np.abs(z).max()
    assert abs(p["w"].dot(u)) <= 1e-10 * np.abs(u).max()              # the step keeps the gauge
    assert p["grad"].dot(u) < 0.0                                     # and descends


def deer_fixture(N=3000, seed=7, sigma=0.01):
    """bench.deer_inputs's problem at N structures: the measured trace exp-370-292, seeded distances"""
    from bench import deer_inputs
    return deer_inputs(N, seed, sigma)


def alternation(G, Y, YT, off, theta, params, scale0=0.15, rounds=30, tol=1e-10):
    """the reference's protocol with the dual Newton as the inner solver, until the scale moves by < tol"""
    s, total = scale0, 0
    for k in range(rounds):
        explicit = off[:, None] + s * Y
        res = lw.dual_newton_bioen_log_posterior_base(G, G, explicit, YT, theta, params)
        assert res["status"] == 0
        total += res["iterations"]
        w = np.exp(res["g"] - res["g"].max())
        w /= w.sum()
        new = nuisance.refit_scales(Y.dot(w), YT, off, [np.arange(Y.shape[0])])[0]
        moved, s = abs(new - s), new
        if moved < tol:
            # f at the refitted scale: the alternation's objective at its fixed point
            return dict(res, w=w, scale=s, newton_iterations=total, rounds=k + 1)
    raise AssertionError("the alternation did not converge in %d rounds" % rounds)


@pytest.fixture(scope="module")
def deer3000():
    return deer_fixture()


@pytest.mark.parametrize("theta", [100.0, 10.0])
def test_optimum_equals_the_alternations(deer3000, theta):
    Y, YT, off = deer3000
    n = Y.shape[1]
    G = np.zeros(n)
    params = dict(gtol=1e-9, max_iterations=200)
    res = lw.dual_newton_profile_base(G, G, Y, YT, theta, params, None, row_offset=off)
    assert res["status"] == 0
    alt = alternation(G, Y, YT, off, theta, params)
    w = np.exp(res["g"] - res["g"].max())
    w /= w.sum()
    print("theta %g: profiled %d iterations, alternation %d in %d rounds; f %.17g / %.17g, scale %.17g / %.17g"
          % (theta, res["iterations"], alt["newton_iterations"], alt["rounds"], res["fmin"], alt["fmin"],
             res["scales"][0], alt["scale"]))
    assert abs(res["fmin"] - alt["fmin"]) <= 1e-6 * abs(alt["fmin"])
    assert np.abs(w - alt["w"]).max() <= 1e-5 * alt["w"].max()
    assert abs(res["scales"][0] - alt["scale"]) <= 1e-6 * abs(alt["scale"])
    assert res["iterations"] < alt["newton_iterations"]


def test_series_warm_and_cold(deer3000):
    Y, YT, off = deer3000
    G = np.zeros(Y.shape[1])
    params = dict(gtol=1e-8)
    warm = lw.dual_newton_profile_series_base(G, G, Y, YT, [100.0, 10.0], params, None, off, warm=True)
    cold = lw.dual_newton_profile_series_base(G, G, Y, YT, [100.0, 10.0], params, None, off, warm=False)
    assert [r["status"] for r in warm + cold] == [0] * 4
    assert np.array_equal(warm[0]["g"], cold[0]["g"])
    assert warm[1]["iterations"] <= cold[1]["iterations"]
    assert abs(warm[1]["fmin"] - cold[1]["fmin"]) <= 1e-9 * abs(cold[1]["fmin"])
    single = lw.dual_newton_profile_base(G, G, Y, YT, 10.0, params, None, off)
    assert np.array_equal(single["g"], cold[1]["g"]) and single["scales"] == cold[1]["scales"]


def test_refusals_and_the_degenerate_denominator():
    Y, YT, off, groups = deer_problem()
    G = np.zeros(Y.shape[1])
    with pytest.raises(RuntimeError, match="theta > 0"):
        lw.dual_newton_profile_base(G, G, Y, YT, 0.0, {}, groups, off)
    with pytest.raises(RuntimeError, match="empty"):
        lw.dual_newton_profile_base(G, G, Y, YT, 1.0, {}, [np.arange(5), np.array([], dtype=int)], off)
    with pytest.raises(RuntimeError, match="disjoint"):
        lw.dual_newton_profile_base(G, G, Y, YT, 1.0, {}, [np.arange(5), np.arange(4, 9)], off)
    Z = Y.copy()
    Z[groups[1]] = 0.0                                               # sum ybar^2 = 0 in group 1: f is not finite
    res = lw.dual_newton_profile_base(G, G, Z, YT, 1.0, {}, groups, off)
    assert res["status"] == 3 and not np.isfinite(res["fmin"]) and res["iterations"] == 0

"""Per-structure quadratic forms a_j^T P a_j and the Laplace error bars built on them, on the CPU: the numpy restatement
(forces.colquad_bioen_log_posterior_base) against the formula in numpy.longdouble, and forces.laplace_error_bars
(use_c=False) against central-difference Jacobians of ln w(f) and ybar(f) at a converged optimum, with its refusals."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import FORCES_GOLDEN
from test_forces_hessp import forces_case
from test_hip_forces_hessp import problem

from bioen_amd.optimize import forces

L = np.longdouble
GATE = 1e-10          # the project's gate for the rounding of second-order quantities, here of max_j |a_j|^T |P| |a_j|


def centred_ld(A, w0, f):
    """a = A - ybar at the weights of f, in longdouble"""
    x = f.astype(L) @ A
    e = w0.astype(L) * np.exp(x - x.max())
    w = e / e.sum()
    return A - (A @ w)[:, None]


def colquad_ld(a, P):
    """((P a) o a).sum(0) in longdouble and the scale of its rounding, max_j |a_j|^T |P| |a_j| (a bound: float64 serves).
    The product P a runs in row blocks on eight threads (numpy's longdouble products release the interpreter lock); for
    P = I and P = 0 it is a and 0 in any arithmetic, bit for bit, and is not multiplied out."""
    m = P.shape[0]
    if not P.any():
        Pa = np.zeros_like(a)
    elif np.array_equal(P, np.eye(m)):
        Pa = a
    else:
        Pl = P.astype(L)
        blocks = [b for b in np.array_split(np.arange(m), 8) if b.size]
        with ThreadPoolExecutor(8) as workers:
            Pa = np.vstack(list(workers.map(lambda rows: Pl[rows] @ a, blocks)))
    ref = (Pa * a).sum(axis=0)
    a64 = np.abs(a.astype(np.float64))
    scale = ((np.abs(P) @ a64) * a64).sum(axis=0).max()
    return ref.astype(np.float64), float(scale)


def matrices(m, seed):
    """P1 = B + B^T (indefinite), P2 = I (-> |a_j|^2), P3 = u u^T (-> (u . a_j)^2), P = 0"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m, m))
    u = rng.standard_normal(m)
    return {"B+B^T": B + B.T, "I": np.eye(m), "uu^T": np.outer(u, u), "0": np.zeros((m, m))}, u


def check_restatement(yT, YT, w0, f, thetas, label):
    """(the weights, hence v, do not depend on theta: the longdouble reference is formed once per matrix)"""
    a = centred_ld(yT.astype(L), w0.reshape(-1), f)
    mats, u = matrices(yT.shape[0], 11 + yT.shape[0])
    for name, P in mats.items():
        ref, scale = colquad_ld(a, P)
        for theta in thetas:
            v = forces.colquad_bioen_log_posterior_base(f, P, w0, yT, YT, theta)
            assert v.shape == (yT.shape[1],)
            err = np.abs(v - ref).max()
            print("%s theta %g, P = %s: max |v - v_ld| = %.3g of max_j |a|^T|P||a| = %.3g"
                  % (label, theta, name, err / scale if scale else 0.0, scale))
            assert err <= GATE * scale
        if name == "I":         # the independent formulas
            assert np.abs(v - (a * a).sum(axis=0).astype(np.float64)).max() <= GATE * scale
        if name == "uu^T":
            assert np.abs(v - ((u.astype(L) @ a) ** 2).astype(np.float64)).max() <= GATE * scale
        if name == "0":
            assert not v.any()


@pytest.mark.parametrize("name", FORCES_GOLDEN)
def test_restatement_against_longdouble_on_the_goldens(name):
    d, args, x, _ = forces_case(name)
    w0, yT, YT, theta = args
    check_restatement(yT, YT, np.asarray(w0, dtype=np.float64), x, (theta,), name)


@pytest.mark.parametrize("shape", [(7, 37), (129, 257), (513, 1537)], ids=["7x37", "129x257", "513x1537"])
def test_restatement_against_longdouble_on_the_seeded_problems(shape):
    yT, YT, w0, f, _ = problem(shape)
    check_restatement(yT, YT, w0, f, (0.1, 10.0, 1000.0), "%dx%d" % shape)


def test_restatement_refuses_a_wrong_shape():
    yT, YT, w0, f, _ = problem((7, 37))
    with pytest.raises(ValueError):
        forces.colquad_bioen_log_posterior_base(f, np.eye(8), w0, yT, YT, 10.0)


# ---- laplace_error_bars ----------------------------------------------------------------------------------
def converged(shape=(6, 40), theta=5.0, seed=12, duplicate_row=False):
    """a small seeded problem with N > M and its optimum: Newton steps on the numpy objective until the gradient is at
    rounding.  duplicate_row: the last observable repeats the first -- C is singular, the optimum a line of forces, and the
    steps are least-squares ones"""
    M, N = shape
    rng = np.random.default_rng(seed)
    yT = rng.normal(rng.normal(0.0, 2.0, (M, 1)), 1.0, (M, N))
    w0 = rng.uniform(0.5, 1.5, N)
    w0 /= w0.sum()
    YT = yT.dot(w0) + rng.normal(0.0, 0.3, M)
    if duplicate_row:
        yT[-1], YT[-1] = yT[0], YT[0]
    args = (w0, yT, YT, theta)
    f = np.zeros(M)
    for _ in range(50):
        g = forces.grad_bioen_log_posterior_base(f, *args)
        if np.abs(g).max() <= 1e-13:
            break
        H = forces.hessian_gram_bioen_log_posterior_base(f, *args)[1]
        step = np.linalg.lstsq(H, g, rcond=1e-12)[0]
        t, L0 = 1.0, forces.bioen_log_posterior_base(f, *args)
        while forces.bioen_log_posterior_base(f - t * step, *args) > L0 and t > 1e-6:
            t *= 0.5
        f = f - t * step
    assert np.abs(forces.grad_bioen_log_posterior_base(f, *args)).max() <= 1e-10
    return f, args


def jacobian(fun, f, h=1e-4):
    """Richardson central difference (h and h / 2) of fun along every unit direction: columns d fun / d f_i"""
    cols = []
    for i in range(f.size):
        e = np.zeros(f.size)
        e[i] = 1.0

        def central(s):
            return (fun(f + s * e) - fun(f - s * e)) / (2.0 * s)
        cols.append((4.0 * central(h / 2) - central(h)) / 3.0)
    return np.array(cols).T


def test_error_bars_against_finite_difference_jacobians():
    """var_logw = diag(J H^-1 J^T), J the Jacobian of ln w(f); cov_averages = J_y H^-1 J_y^T, J_y the Jacobian of ybar(f);
    both to 1e-6 of the largest entry (DESIGN 6e's gate for its Richardson check of C)"""
    f, args = converged()
    w0, yT, YT, theta = args

    def weights(p):
        return forces.get_weights_from_forces(w0, yT, p)[:, 0]
    eb = forces.laplace_error_bars(f, w0, yT, yT, YT, theta, use_c=False)
    m, n = yT.shape
    assert eb["w"].shape == (n,) and eb["var_logw"].shape == (n,) and eb["std_w"].shape == (n,)
    for k in ("C", "H", "cov_forces", "cov_averages"):
        assert eb[k].shape == (m, m) and np.array_equal(eb[k], eb[k].T)
    assert eb["std_forces"].shape == (m,) and eb["std_averages"].shape == (m,)
    Hi = np.linalg.inv(forces.hessian_bioen_log_posterior_base(f, *args))
    J = jacobian(lambda p: np.log(weights(p)), f)
    Jy = jacobian(lambda p: yT.dot(weights(p)), f)
    var_fd = np.einsum("ji,ik,jk->j", J, Hi, J)
    cov_fd = Jy.dot(Hi).dot(Jy.T)
    ev, ec = np.abs(eb["var_logw"] - var_fd).max() / np.abs(var_fd).max(), np.abs(eb["cov_averages"] - cov_fd).max() / np.abs(cov_fd).max()
    print("max |var_logw - FD| = %.3g of its largest entry, |cov_averages - FD| = %.3g" % (ev, ec))
    assert ev <= 1e-6 and ec <= 1e-6
    assert np.allclose(eb["cov_forces"], Hi, rtol=0, atol=1e-9 * np.abs(Hi).max())
    assert np.array_equal(eb["std_forces"], np.sqrt(np.diag(eb["cov_forces"])))
    assert np.array_equal(eb["std_w"], eb["w"] * np.sqrt(eb["var_logw"]))
    assert np.array_equal(eb["w"], weights(f))


def test_error_bars_refuse_a_point_that_is_no_minimum():
    """problem()'s point: H is indefinite there (smallest eigenvalue -77 ... -8.6e3 over the shapes)"""
    yT, YT, w0, f, _ = problem((7, 37))
    with pytest.raises(ValueError, match="indefinite"):
        forces.laplace_error_bars(f, w0, yT, yT, YT, 10.0, use_c=False)


def test_error_bars_refuse_808x10():
    """808 x 10: N <= M, the covariance has rank < N, H is singular (and at problem()'s point indefinite as well)"""
    yT, YT, w0, f, _ = problem((808, 10))
    with pytest.raises(ValueError, match="singular|indefinite"):
        forces.laplace_error_bars(f, w0, yT, yT, YT, 10.0, use_c=False)


def test_error_bars_name_a_singular_covariance_at_a_minimum():
    """a converged optimum whose covariance is singular (an observable entered twice): the message says so"""
    f, args = converged(duplicate_row=True)
    w0, yT, YT, theta = args
    with pytest.raises(ValueError, match="singular"):
        forces.laplace_error_bars(f, w0, yT, yT, YT, theta, use_c=False)

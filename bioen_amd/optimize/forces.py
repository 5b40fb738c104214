"""Forces method: public API of ``bioen/optimize/forces.py`` on MI355X.

M generalised forces f parametrise the weights, w = w0 * exp(f^T yTilde) / Z:

  L(f)      = theta * sum_j w_j log(w_j / w0_j) + 0.5 |yTilde w - YTilde|^2
  dL/df_i   = sum_j (yTilde_ij - ybar_i) w_j [ theta (1 + log(w_j/w0_j)) + (yTilde^T r)_j ]

`use_c=True` paths evaluate on the device (ext.c_bioen); the ``*_base`` functions are
the reference's explicit numpy variants.
"""
from __future__ import print_function

import time

import numpy as np
import scipy.optimize as sopt

from . import common
from .ext import c_bioen
from .log_weights import _run_scipy


# ------------------------------------------------------------------ synthetic data
def gen_synthetic_data(M, N, YTrue, sig_exp):
    """Observed values ~ N(YTrue, sig_exp) and their scaled form (forces.py:19-41)."""
    YObs = np.array(np.random.normal(YTrue, sig_exp))
    return YObs, YObs / sig_exp


def gen_sythetic_ensemble(M, N, YTrue, sig_exp, sig_sim):
    """Ensemble observables ~ N(YTrue, sig_sim) per structure, and yTilde = y / sig_exp
    (forces.py:44-68).  Returns (y, yTilde), both (M, N)."""
    YTrue = np.asarray(YTrue, dtype=np.float64)
    y = np.array(np.random.normal(np.repeat(YTrue[:, None], N, axis=1), sig_sim))
    yTilde = y / np.asarray(sig_exp, dtype=np.float64).reshape(-1, 1)
    return y, yTilde


def init_forces(M, val=0):
    forces = np.zeros((M, 1))
    forces[:, 0] = val
    return forces


# ------------------------------------------------------------------ numpy helpers
def get_weights_from_forces(w0, y, forces):
    """w (n,1) from forces (1,m) or (m,) (forces.py:91-111); host numpy."""
    f = np.asarray(forces, dtype=np.float64)
    if f.ndim == 1:
        f = f[None, :]
    x = f.dot(np.asarray(y, dtype=np.float64))
    e = np.exp(x - np.max(x))
    w = np.asarray(w0, dtype=np.float64).reshape(-1, 1) * e.T
    return w / w.sum()


def _kl(w, w0):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    w0 = np.asarray(w0, dtype=np.float64).reshape(-1)
    ind = w > 0                      # lim w->0 of w log w is 0
    return float(np.log(w[ind] / w0[ind]).dot(w[ind]))


def bioen_chi2_s_forces(forces, w0, yTilde, YTilde):
    """(S, chiSqr) at `forces` (m,1)/(m,): relative entropy sum w log(w/w0) and
    0.5 chi^2 (forces.py:116-136)."""
    w = get_weights_from_forces(w0, yTilde, np.asarray(forces).T)
    return _kl(w, w0), common.chiSqrTerm(w, yTilde, YTilde)


def check_params_forces(forcesInit, w0, y, yTilde, YTilde):
    """Shape contract: forcesInit (m,1); w0 (n,1); y,yTilde (m,n); YTilde (1,m) (forces.py:139-182)."""
    m, n = yTilde.shape
    expected = (("forcesInit", forcesInit, (m, 1)), ("w0", w0, (n, 1)), ("y", y, (m, n)),
                ("YTilde", YTilde, (1, m)))
    bad = False
    for name, arr, shape in expected:
        if arr.shape != shape:
            print("Unexpected shape for variable: {name}\nExpected: {expected}\nCurrent:  {current}".format(
                name=name, expected=shape, current=arr.shape))
            bad = True
    if bad:
        raise ValueError("arguments dimensionality for the 'forces' method are wrong")


# ------------------------------------------------------------------ objective / gradient
def bioen_log_posterior(forces, w0, y, yTilde, YTilde, theta, use_c=True, caching=False):
    """Negative log-posterior in the forces parametrisation (forces.py:187-212); `y` unused."""
    if use_c:
        return c_bioen.bioen_log_posterior_forces(forces, w0, yTilde, YTilde, theta)
    return bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta)


def grad_bioen_log_posterior(forces, w0, y, yTilde, YTilde, theta, use_c=True, caching=False):
    """Gradient w.r.t. the m forces (forces.py:216-244); `y` unused."""
    if use_c:
        return c_bioen.grad_bioen_log_posterior_forces(forces, w0, yTilde, YTilde, theta)
    return grad_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta)


def bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta, use_c=True):
    """Pure-numpy objective (forces.py:248-289)."""
    w = get_weights_from_forces(w0, yTilde, np.asarray(forces).T)
    return theta * _kl(w, w0) + common.chiSqrTerm(w, yTilde, YTilde)


def grad_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta, use_c=True):
    """Pure-numpy gradient (forces.py:293-333)."""
    yT = np.asarray(yTilde, dtype=np.float64)
    w = get_weights_from_forces(w0, yT, np.asarray(forces).T)[:, 0]
    w0v = np.asarray(w0, dtype=np.float64).reshape(-1)
    ybar = yT.dot(w)
    b = yT.T.dot(ybar - np.asarray(YTilde, dtype=np.float64).reshape(-1))
    ratio = np.where(w > 0, w / w0v, 1.0)
    t = ((np.log(ratio) + 1.0) * theta + b) * w
    return (yT - ybar[:, None]).dot(t)        # centred, as forces.py:329-332 (no cancellation)


# ------------------------------------------------------------------ second order
def _hessp_base(forces, V, w0, yTilde, YTilde, theta):
    """H V for the columns of V (m, k), centred throughout:

      x = A^T f,  w ~ w0 e^x,  ybar = A w,  r = ybar - YTilde,  q = theta x + A^T r
      dx  = A^T v - <A^T v>                        (<.> the average under w)
      dy  = A (w dx)
      s   = w [ dx (q - <q>) + theta dx + (A^T dy - <A^T dy>) ]
      H v = (A - ybar) s

    Constants added to x, q, dx or the bracket of s cancel in the centred last line: each is taken off where it arises,
    so every sum stays at the scale of the data's spread, as in grad_bioen_log_posterior_base."""
    yT = np.asarray(yTilde, dtype=np.float64)
    f = np.asarray(forces, dtype=np.float64).reshape(-1)
    w = get_weights_from_forces(w0, yT, f)[:, 0]
    ybar = yT.dot(w)
    r = ybar - np.asarray(YTilde, dtype=np.float64).reshape(-1)
    x = yT.T.dot(f)
    q = theta * (x - w.dot(x)) + yT.T.dot(r)
    q -= w.dot(q)
    dx = yT.T.dot(V)
    dx -= w.dot(dx)[None, :]
    c = yT.T.dot(yT.dot(w[:, None] * dx))
    c -= w.dot(c)[None, :]
    s = w[:, None] * (dx * (q[:, None] + theta) + c)
    return yT.dot(s) - ybar[:, None] * s.sum(axis=0)[None, :]


def hessp_bioen_log_posterior_base(forces, p, w0, yTilde, YTilde, theta, use_c=True):
    """Pure-numpy Hessian-vector product H(forces) p of the negative log-posterior, p (m,) -> (m,).  Not in the
    reference, which has no second-order information; checked against finite differences of its C gradient
    (tests/test_forces_hessp.py).  H is the exact Hessian: symmetric, not positive definite away from the optimum."""
    pv = np.asarray(p, dtype=np.float64).reshape(-1, 1)
    return _hessp_base(forces, pv, w0, yTilde, YTilde, theta)[:, 0]


def hessian_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta, use_c=True):
    """Pure-numpy dense Hessian (m, m): the products with the m unit directions, symmetrised as (H + H^T) / 2 (the
    products are symmetric to rounding: the asymmetry removed is below 1e-12 of the largest entry)."""
    m = np.asarray(yTilde).shape[0]
    H = _hessp_base(forces, np.eye(m), w0, yTilde, YTilde, theta)
    return 0.5 * (H + H.T)


def hessian_gram_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta, use_c=True):
    """(C, H), both (m, m): the covariance of the observables under the weights, C = d ybar / d forces, and the dense
    Hessian, from two weighted, centred Gram matrices instead of m products.  With a_j = A_:j - ybar,
    q_j = theta x_j + b_j and G[u] = sum_j u_j a_j a_j^T:

      C = G[w],    H = theta C + C C + G[w (q - <q>)]

    Centred like hessian_bioen_log_posterior_base, which it agrees with to rounding (tests/test_forces_gram.py); both
    results are symmetric bit for bit."""
    yT = np.asarray(yTilde, dtype=np.float64)
    f = np.asarray(forces, dtype=np.float64).reshape(-1)
    w = get_weights_from_forces(w0, yT, f)[:, 0]
    ybar = yT.dot(w)
    r = ybar - np.asarray(YTilde, dtype=np.float64).reshape(-1)
    x = yT.T.dot(f)
    q = theta * (x - w.dot(x)) + yT.T.dot(r)
    q -= w.dot(q)
    a = yT - ybar[:, None]
    C = (a * w[None, :]).dot(a.T)
    G2 = (a * (w * q)[None, :]).dot(a.T)
    C = 0.5 * (C + C.T)
    H = theta * C + C.dot(C) + G2
    return C, 0.5 * (H + H.T)


def _bf16_round(v):
    """float32 array -> the nearest bfloat16 (ties to even) as float32, by integer arithmetic on the bit pattern"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def _bf16_split(v):
    """FP64 array -> (hi, lo) as FP64 arrays holding bfloat16 numbers: hi = bf((float)v), lo = bf((float)v - hi) -- the
    subtraction is exact in float32"""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    hi = _bf16_round(f)
    lo = _bf16_round(f - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def hessian_gram_bf16_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta, use_c=True):
    """(C~, H~), both (m, m): the numpy restatement of Context.forces_gram_bf16 -- the covariance and the dense
    Hessian of hessian_gram_bioen_log_posterior_base with the two M x M x N products formed from split-BF16 operands, as
    a Newton minimizer's Hessian (good to about 1e-5 ... 1e-4 of max|H|).  With Y' = yTilde - YTilde (the device's centre),
    u1 = w, u2 = w (q - <q>) and bf(v) = round-to-nearest-even of (float)v to bfloat16:

      a = Y'_ij (FP64)         a_hi = bf(a),  a_lo = bf((float)a - a_hi)
      t = a u_j (FP64)         t_hi = bf(t),  t_lo = bf((float)t - t_hi)
      G'[u] = sum_j (a_hi t_hi + a_hi t_lo + a_lo t_hi)         each product exact in FP64, summed in FP64
      g = sum_j u2_j Y'_j,  ybar' = ybar - YTilde               FP64
      C~ = G'[u1] - ybar' ybar'^T,   G2 = G'[u2] - g ybar'^T - ybar' g^T,   H~ = theta C~ + G2 + C~ C~

    The lower triangle is computed and mirrored: both results are symmetric bit for bit."""
    yT = np.asarray(yTilde, dtype=np.float64)
    f = np.asarray(forces, dtype=np.float64).reshape(-1)
    w = get_weights_from_forces(w0, yT, f)[:, 0]
    centre = np.asarray(YTilde, dtype=np.float64).reshape(-1)
    ybar = yT.dot(w)
    x = yT.T.dot(f)
    q = theta * (x - w.dot(x)) + yT.T.dot(ybar - centre)
    q -= w.dot(q)
    a = yT - centre[:, None]
    a_hi, a_lo = _bf16_split(a)

    def gram(u):
        t_hi, t_lo = _bf16_split(a * u[None, :])
        return a_hi.dot(t_hi.T) + a_hi.dot(t_lo.T) + a_lo.dot(t_hi.T)

    u2 = w * q
    yc = a.dot(w)                        # ybar' = ybar - centre, formed from the centred operand
    g = a.dot(u2)
    C = gram(w) - np.outer(yc, yc)
    G2 = gram(u2) - np.outer(g, yc) - np.outer(yc, g)
    T = theta * C + G2
    C = np.tril(C) + np.tril(C, -1).T
    T = np.tril(T) + np.tril(T, -1).T
    S = C.dot(C)
    H = T + (np.tril(S) + np.tril(S, -1).T)
    return C, H


def hessp_bioen_log_posterior(forces, p, w0, y, yTilde, YTilde, theta, use_c=True, caching=False):
    """Hessian-vector product w.r.t. the m forces; `y` unused."""
    if use_c:
        return c_bioen.hessp_bioen_log_posterior_forces(forces, p, w0, yTilde, YTilde, theta)
    return hessp_bioen_log_posterior_base(forces, p, w0, yTilde, YTilde, theta)


def hessian_bioen_log_posterior(forces, w0, y, yTilde, YTilde, theta, use_c=True, caching=False):
    """Dense Hessian (m, m) w.r.t. the m forces; `y` unused."""
    if use_c:
        return c_bioen.hessian_bioen_log_posterior_forces(forces, w0, yTilde, YTilde, theta)
    return hessian_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta)


# ------------------------------------------------------------------ Laplace error bars
def colquad_bioen_log_posterior_base(forces, P, w0, yTilde, YTilde, theta, use_c=True):
    """Pure-numpy v (n,): v_j = a_j^T P a_j with a_j = A_:j - ybar at the weights of `forces` and P (m, m) symmetric -- the
    restatement of Context.forces_colquad.  d ln w_j / d forces = a_j, so with P = inv(H) this is the Laplace
    variance of ln w_j.  The operand is centred first; the quadratic is not expanded."""
    yT = np.asarray(yTilde, dtype=np.float64)
    f = np.asarray(forces, dtype=np.float64).reshape(-1)
    Pm = np.asarray(P, dtype=np.float64)
    if Pm.shape != (yT.shape[0], yT.shape[0]):
        raise ValueError("P must be (M, M) with M = %d, got %s" % (yT.shape[0], (Pm.shape,)))
    w = get_weights_from_forces(w0, yT, f)[:, 0]
    a = yT - yT.dot(w)[:, None]
    return (Pm.dot(a) * a).sum(axis=0)


def _laplace_inverse(H, theta):
    """inv(H) through a Cholesky factorisation; ValueError, saying which of the two it found, if H is not positive
    definite: indefinite (away from a minimum) or singular to rounding (C singular, always so for N <= M)"""
    scale = float(np.abs(H).max())
    try:
        L = np.linalg.cholesky(H)
        definite = float(np.diag(L).min()) ** 2 > 1e-13 * scale          # (a pivot at rounding: the factorisation got through by luck)
    except np.linalg.LinAlgError:
        definite = False
    if not definite:
        lo = float(np.linalg.eigvalsh(H)[0])
        # H = theta C + C C + G2: at a minimum its smallest eigenvalue is >= theta x that of C, so one within rounding of
        # zero on the scale of theta and of H says C is singular; a clearly negative one says this is no minimum
        if lo < -1e-8 * max(abs(theta), scale):
            raise ValueError("laplace_error_bars: the Hessian is indefinite (smallest eigenvalue %.3g): the forces are not "
                             "at a minimum of the objective" % lo)
        raise ValueError("laplace_error_bars: the Hessian is singular (smallest eigenvalue %.3g against theta = %.3g): the "
                         "covariance of the observables is singular, as it always is for N <= M" % (lo, theta))
    Li = np.linalg.solve(L, np.eye(H.shape[0]))
    Hi = Li.T.dot(Li)
    return 0.5 * (Hi + Hi.T)


def laplace_error_bars(forces, w0, y, yTilde, YTilde, theta, use_c=True, caching=False, on_device=False, matrices=True):
    """Laplace error bars at an optimum `forces` of the forces objective, the negative log-posterior L = theta KL + chi^2 / 2:
    the forces are Gaussian around it with covariance inv(H), and d ybar / d forces = C, d ln w_j / d forces = a_j.  -> dict:

      w (n,), C (m, m), H (m, m)
      cov_forces = inv(H), std_forces                  (m, m), (m,)
      cov_averages = C inv(H) C, std_averages          (m, m), (m,)   of ybar in the units of yTilde
      var_logw (n,): a_j^T inv(H) a_j,  std_w = w sqrt(var_logw)

    use_c: C and H from Context.forces_gram and var_logw from Context.forces_colquad at one kept point of a resident
    context (M <= 1024); else the numpy restatements.  ValueError if H is not positive definite.  `y` unused.

    on_device=True: the dict gains logdet_H = ln det H.  With use_c it comes from one Context.forces_laplace
    call, plus the weights (and with matrices the forces_gram call that sets the point and hands out C and H): H is factorised and inverted where forces_gram leaves it, and the inverse
    is handed to forces_colquad's pass on the device; with matrices=False the four (m, m) arrays C, H, cov_forces and
    cov_averages are None and nothing of size m^2 is downloaded.  Without use_c it is the numpy path, with logdet_H = 2 sum
    ln diag(cholesky(H)): the restatement the device is checked against.  H is judged as _laplace_inverse judges it: on
    info != 0 or min L_ii^2 <= 1e-13 max|H| the Hessian is downloaded and _laplace_inverse raises its ValueError.
    (matrices=False knows max|H| only from below -- the larger of max_i 1 / var_forces_i and det(H)^(1/m), both <= max_i
    H_ii --, so a pivot within a few digits of the threshold may pass there.)"""
    f = np.asarray(forces, dtype=np.float64).reshape(-1)
    w0v = np.asarray(w0, dtype=np.float64).reshape(-1)
    if on_device:
        return _laplace_error_bars_on_device(f, w0v, yTilde, YTilde, theta, use_c, matrices)
    if use_c:
        ctx, cached = c_bioen._context_for(yTilde, YTilde)
        try:
            C, H, _, _ = ctx.forces_gram(forces=f, w0=w0v, theta=theta)
            Hi = _laplace_inverse(H, theta)
            var_logw = ctx.forces_colquad(Hi)
            w = np.asarray(ctx.forces_weights(f, w0v), dtype=np.float64).reshape(-1)      # (an evaluation: the point goes)
        finally:
            c_bioen._release(ctx, cached)
    else:
        C, H = hessian_gram_bioen_log_posterior_base(f, w0v, yTilde, YTilde, theta)
        Hi = _laplace_inverse(H, theta)
        var_logw = colquad_bioen_log_posterior_base(f, Hi, w0v, yTilde, YTilde, theta)
        w = get_weights_from_forces(w0v, np.asarray(yTilde, dtype=np.float64), f)[:, 0]
    cov_av = C.dot(Hi).dot(C)
    cov_av = 0.5 * (cov_av + cov_av.T)
    var_logw = np.maximum(var_logw, 0.0)
    return {"w": w, "C": C, "H": H,
            "cov_forces": Hi, "std_forces": np.sqrt(np.diag(Hi)),
            "cov_averages": cov_av, "std_averages": np.sqrt(np.maximum(np.diag(cov_av), 0.0)),
            "var_logw": var_logw, "std_w": w * np.sqrt(var_logw)}


def _laplace_error_bars_on_device(f, w0v, yTilde, YTilde, theta, use_c, matrices):
    """laplace_error_bars(on_device=True): see there"""
    if not use_c:
        C, H = hessian_gram_bioen_log_posterior_base(f, w0v, yTilde, YTilde, theta)
        Hi = _laplace_inverse(H, theta)
        logdet = 2.0 * float(np.log(np.diag(np.linalg.cholesky(H))).sum())
        var_logw = np.maximum(colquad_bioen_log_posterior_base(f, Hi, w0v, yTilde, YTilde, theta), 0.0)
        w = get_weights_from_forces(w0v, np.asarray(yTilde, dtype=np.float64), f)[:, 0]
        cov_av = C.dot(Hi).dot(C)
        cov_av = 0.5 * (cov_av + cov_av.T)
        out = {"w": w, "C": C, "H": H,
               "cov_forces": Hi, "std_forces": np.sqrt(np.diag(Hi)),
               "cov_averages": cov_av, "std_averages": np.sqrt(np.maximum(np.diag(cov_av), 0.0)),
               "var_logw": var_logw, "std_w": w * np.sqrt(var_logw), "logdet_H": logdet}
        if not matrices:
            out.update(C=None, H=None, cov_forces=None, cov_averages=None)
        return out
    ctx, cached = c_bioen._context_for(yTilde, YTilde)
    try:
        C = H = None
        if matrices:
            C, H, _, _ = ctx.forces_gram(forces=f, w0=w0v, theta=theta)
            r = ctx.forces_laplace()                 # at the kept point: the pass's C and H serve where they stand
            scale = float(np.abs(H).max())
        else:
            r = ctx.forces_laplace(forces=f, w0=w0v, theta=theta, matrices=False)
            if r["info"] == 0:
                scale = max(float((1.0 / r["std_forces"] ** 2).max()), float(np.exp(r["logdet_H"] / f.size)))
        if r["info"] != 0 or not r["min_pivot"] > 1e-13 * scale:
            _laplace_inverse(H if H is not None else ctx.forces_gram(cov=False)[1], theta)      # raises: indefinite or singular, in its words
            if r["info"] != 0:
                raise ValueError("laplace_error_bars: the Hessian is singular (the device factorisation ended at pivot %d)"
                                 % r["info"])
        w = np.asarray(ctx.forces_weights(f, w0v), dtype=np.float64).reshape(-1)      # (an evaluation: the point goes)
    finally:
        c_bioen._release(ctx, cached)
    var_logw = np.maximum(r["var_logw"], 0.0)
    return {"w": w, "C": C, "H": H,
            "cov_forces": r["cov_forces"], "std_forces": r["std_forces"],
            "cov_averages": r["cov_averages"], "std_averages": r["std_averages"],
            "var_logw": var_logw, "std_w": w * np.sqrt(var_logw), "logdet_H": r["logdet_H"]}


# The driver that fits M unknowns with a dense Hessian.  (trust-krylov is not offered: scipy 1.15.3's failed to converge
# on a 5-variable quartic.  newton_cg / trust_ncg stay the log-weights method's: tests/test_hessp.py pins the refusal.)
_SCIPY_DENSE = {"trust_exact": "trust-region Newton, exact subproblem", "trust-exact": "trust-region Newton, exact subproblem"}


# scipy:hessian -- where trust-exact's dense Hessian comes from: "products" (the default: ceil(m / 8) batched products at
# the kept point, Context.forces_hessian), "gram" (one compute-bound pass on the FP64 matrix cores, Context.forces_gram;
# M <= 1024) or "gram_bf16" (the same pass from split-BF16 operands, Context.forces_gram_bf16: a minimizer's Hessian, good
# to 1e-5 ... 1e-4 of max|H|; the gradient stays FP64, so the minimum is the same, but the last steps converge linearly, not
# quadratically: with a large theta or a tight gtol scipy may end with status 2 just above gtol -- DESIGN 6g)
_HESSIAN_SOURCES = ("products", "gram", "gram_bf16")


def _hessian_source(cfg):
    """the scipy parameter `hessian`, checked: -> "products" | "gram" | "gram_bf16" """
    source = str(cfg["params"].get("hessian", "products")).lower()
    if source not in _HESSIAN_SOURCES:
        raise RuntimeError("scipy:hessian=" + source + " not recognized (valid values = 'products', 'gram', 'gram_bf16')")
    if source != "products" and str(cfg["algorithm"]).lower() not in _SCIPY_DENSE:
        raise RuntimeError("scipy:hessian=" + source + " serves scipy:algorithm=trust_exact only (the other drivers take no dense "
                           "Hessian); got algorithm " + str(cfg["algorithm"]))
    return source


def _hess_gram_base(forces, w0, yTilde, YTilde, theta):
    return hessian_gram_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta)[1]


def _hess_gram_bf16_base(forces, w0, yTilde, YTilde, theta):
    return hessian_gram_bf16_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta)[1]


def _run_scipy_trust_exact(cfg, f, fprime, hess, x0, args):
    """scipy's trust-exact on f, f' and the dense Hessian; -> (xopt, fopt)"""
    p = cfg["params"]
    verbose = cfg["verbose"]
    common.print_highlighted('method ' + _SCIPY_DENSE[cfg["algorithm"].lower()], verbose)
    res = sopt.minimize(f, np.asarray(x0, dtype=np.float64).reshape(-1), args=args, method="trust-exact", jac=fprime,
                        hess=hess, options={"gtol": p["gtol"], "maxiter": p["max_iterations"], "disp": bool(verbose)})
    return res.x, res.fun


# ------------------------------------------------------------------ the forces method's own Newton minimizer
# newton:hessian -- where the Newton minimizer's Hessian comes from: "gram" (Context.forces_gram's FP64 pass) or "gram_bf16"
# (Context.forces_gram_bf16's; the loop goes over to "gram" by itself where the approximate Hessian stops helping)
_NEWTON_SOURCES = ("gram", "gram_bf16")
# the damping constants of the loop; the device loop's defaults (bioen_amd._lib.NEWTON_DEFAULTS) are the same
_NEWTON_CONSTANTS = dict(armijo=1e-4, rho_good=0.75, lambda_factor=4.0, lambda_first=1e-10, lambda_max=1e10,
                         lambda_zero=1e-12, floor_ulps=8.0)
NEWTON_STATUS = {0: "max|g| <= gtol", 1: "max_iterations reached", 2: "at the minimum to the rounding of f",
                 3: "the damping left its range"}


def _newton_source(params):
    """the newton parameter `hessian`, checked: -> "gram" | "gram_bf16" """
    source = str(params.get("hessian", "gram")).lower()
    if source not in _NEWTON_SOURCES:
        raise RuntimeError("newton:hessian=" + source + " not recognized (valid values = 'gram', 'gram_bf16')")
    return source


def _newton_cholesky(H, lam):
    """(L, info) of H + lam I as the device factorisation reports it: info = 0, or k + 1 where pivot k was <= 0 or not
    finite (LAPACK dpotrf's convention; only the lower triangle is read)"""
    import scipy.linalg.lapack as lapack
    A = np.tril(np.asarray(H, dtype=np.float64))
    A[np.diag_indices_from(A)] += lam
    if not np.all(np.isfinite(np.diag(A))):
        return None, int(np.flatnonzero(~np.isfinite(np.diag(A)))[0]) + 1
    L, info = lapack.dpotrf(A, lower=1, clean=1)
    return (L if info == 0 else None), int(info)


def newton_bioen_log_posterior_base(forces0, w0, yTilde, YTilde, theta, params, hess=None):
    """The numpy restatement of Context.opt_newton_forces, the specification of the device loop: regularised
    Newton on bioen_log_posterior_base with the dense Hessian of `params["hessian"]` ("gram": _hess_gram_base, "gram_bf16":
    _hess_gram_bf16_base; `hess`, a dict source -> function, replaces them) and a Cholesky factorisation of H + lam I.

      1. max|g| <= gtol -> status 0.           2. H at x from `source`, d = max|diag H|.
      3. factorise H + lam I; info != 0: lam <- max(4 lam, 1e-10 d), again, no evaluation; lam > 1e10 d -> status 3.
      4. p = -(L L^T)^-1 g, pred = (-g.p + lam p.p) / 2.        5. f+, g+ at x + p.
      6. accept if f+ is finite and f+ - f <= -1e-4 pred; at the rounding floor (pred <= 8 eps |f|: f cannot judge the
         step) if max|g+| < max|g| instead.
      7. accepted: x <- x + p; (f - f+) / pred > 0.75, or a step at the floor: lam <- lam / 4, 0 below 1e-12 d; to 1.
      8. rejected at the floor: "gram_bf16" goes over to "gram" (once), H again; "gram" -> status 2: at the minimum to
         the rounding of f.
      9. any other rejection: lam <- max(4 lam, 1e-10 d), to 3: no new Hessian.     10. max_iterations accepted steps -> status 1.

    -> dict(forces, status, fmin, gmax, lam, iterations, evaluations, hessians, factorisations, switched)"""
    import scipy.linalg
    p_ = dict(_NEWTON_CONSTANTS, **{k: v for k, v in dict(params).items() if k in _NEWTON_CONSTANTS})
    gtol, maxit = float(params.get("gtol", 1e-6)), int(params.get("max_iterations", 200))
    source = _newton_source(params)
    sources = dict({"gram": _hess_gram_base, "gram_bf16": _hess_gram_bf16_base}, **(hess or {}))
    args = (w0, yTilde, YTilde, theta)
    eps = np.finfo(np.float64).eps

    def fdf(x):
        return (float(bioen_log_posterior_base(x, *args)),
                np.asarray(grad_bioen_log_posterior_base(x, *args), dtype=np.float64).reshape(-1))

    x = np.asarray(forces0, dtype=np.float64).reshape(-1).copy()
    f, g = fdf(x)
    lam, d, H, L = 0.0, 1.0, None, None
    count = dict(iterations=0, evaluations=1, hessians=0, factorisations=0)
    switched, need_h, status = False, True, None

    def grow(lam):
        lam = max(p_["lambda_factor"] * lam, p_["lambda_first"] * d)
        return lam, lam > p_["lambda_max"] * d

    while status is None:
        gmax = float(np.abs(g).max())
        if gmax <= gtol:
            status = 0
            break
        if count["iterations"] >= maxit:
            status = 1
            break
        if need_h:
            H = np.asarray(sources[source](x, *args), dtype=np.float64)
            count["hessians"] += 1
            dm = float(np.abs(np.diag(H)).max())
            d = dm if dm > 0.0 and np.isfinite(dm) else 1.0
            need_h = False
        while True:
            L, info = _newton_cholesky(H, lam)
            count["factorisations"] += 1
            if info == 0:
                break
            lam, out = grow(lam)
            if out:
                status = 3
                break
        if status == 3:
            break
        p = -scipy.linalg.cho_solve((L, True), g)
        pred = 0.5 * (-float(g.dot(p))) + 0.5 * lam * float(p.dot(p))
        ft, gt = fdf(x + p)
        count["evaluations"] += 1
        gtmax = float(np.abs(gt).max())
        floor = pred <= p_["floor_ulps"] * eps * abs(f)
        accept = bool(np.isfinite(ft)) and (gtmax < gmax if floor else ft - f <= -p_["armijo"] * pred)
        if accept:
            if floor or (f - ft) / pred > p_["rho_good"]:
                lam /= p_["lambda_factor"]
                if lam < p_["lambda_zero"] * d:
                    lam = 0.0
            x, f, g = x + p, ft, gt
            need_h = True
            count["iterations"] += 1
            continue
        if floor:
            if source == "gram_bf16":
                source, switched, need_h = "gram", True, True
                continue
            status = 2
            break
        lam, out = grow(lam)
        if out:
            status = 3
    return dict(count, forces=x, status=status, fmin=f, gmax=float(np.abs(g).max()), lam=lam, switched=switched)


def _newton_finish(who, res):
    """status 0 and 2 return; 1 and 3 raise as the other device minimizers do"""
    if res["status"] not in (0, 2):
        raise RuntimeError("%s: return code %d (%s) after %d iterations, max|g| = %.3g"
                           % (who, res["status"], NEWTON_STATUS.get(res["status"], "?"), res["iterations"], res["gmax"]))
    return res["forces"], res["fmin"]


# ------------------------------------------------------------------ optimizer
class _DeviceFdf(object):
    """One fused device evaluation per point for scipy's separate f / f' callbacks."""

    def __init__(self, w0, yTilde, YTilde, theta, keep_point=False, hessian="products"):
        self.ctx, self._cached = c_bioen._context_for(yTilde, YTilde)
        self._keep_point = keep_point       # trust-exact: every evaluation leaves the point for the products at it
        self._hessian = hessian             # "gram" / "gram_bf16": the dense Hessian from Context.forces_gram / forces_gram_bf16
        self.w0 = np.asarray(w0, dtype=np.float64).reshape(-1)
        self.theta = theta
        self._x = None
        self._point = False       # the context keeps self._x as the point of forces_hessp

    def _eval(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if self._x is None or not np.array_equal(x, self._x):
            if self._keep_point:      # the same evaluation, same bits, and the point stays for the products at this x
                _, self._f, self._g = self.ctx.forces_hessp(None, forces=x, w0=self.w0, theta=self.theta)
            else:
                self._f, self._g = self.ctx.forces_fdf(x, self.w0, self.theta)
            self._x = x.copy()
            self._point = self._keep_point

    def _set_point(self, x):
        """the context's point is x afterwards; an x already evaluated with keep_point is not evaluated again"""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if not (self._x is not None and self._point and np.array_equal(x, self._x)):
            _, self._f, self._g = self.ctx.forces_hessp(None, forces=x, w0=self.w0, theta=self.theta)
            self._x = x.copy()
            self._point = True

    def hessp(self, x, p, *unused):
        """H(x) p: at the cached x the product refers to the point the context keeps (two matrix passes, like a gradient)"""
        self._set_point(x)
        return self.ctx.forces_hessp(np.asarray(p, dtype=np.float64).reshape(-1))

    def hess(self, x, *unused):
        """the dense Hessian at x: ceil(m / 8) batched products at the kept point, or (scipy:hessian=gram, gram_bf16) one
        Gram pass"""
        self._set_point(x)
        if self._hessian == "gram":
            return self.ctx.forces_gram(cov=False)[1]
        if self._hessian == "gram_bf16":
            return self.ctx.forces_gram_bf16(cov=False)[1]
        return self.ctx.forces_hessian()

    def f(self, x, *unused):
        self._eval(x)
        return self._f

    def fprime(self, x, *unused):
        self._eval(x)
        return self._g

    def close(self):
        c_bioen._release(self.ctx, self._cached)


def find_optimum(forcesInit, w0, y, yTilde, YTilde, theta, cfg):
    """Minimise over the m generalised forces (forces.py:336-548): see `_find_optimum`.  The matrix is HELD for the
    duration of the call (ext/c_bioen.py: hold): the initial objective, the optimisation, chi^2 / S and the averages of the
    optimum are served by one device copy -- at most ONE upload per call whatever the size of the matrix."""
    check_params_forces(forcesInit, w0, y, yTilde, YTilde)
    if str(cfg["minimizer"]).upper() not in ('LIBLBFGS', 'LBFGS', 'GSL', 'SCIPY', 'NEWTON'):      # rejected before anything touches the device
        raise RuntimeError("Library " + cfg["minimizer"] +
                           " not recognized (valid values =  'LIBLBFGS', 'GSL', 'scipy', 'scipy', 'newton' ) ")
    if str(cfg["minimizer"]).upper() == 'NEWTON':
        _newton_source(cfg["params"])
    if str(cfg["minimizer"]).upper() == 'SCIPY' and cfg["params"].get("on_device"):
        raise RuntimeError("scipy:on_device (scipy's BFGS with the inverse Hessian on the device) serves the "
                           "log-weights method only (optimize.log_weights.find_optimum); the forces method has none")
    if str(cfg["minimizer"]).upper() == 'SCIPY':
        _hessian_source(cfg)
    if not (str(cfg["minimizer"]).upper() in ('SCIPY', 'NEWTON') and not bool(cfg["use_c_functions"])):
        with c_bioen.hold(yTilde, YTilde):
            return _find_optimum(forcesInit, w0, y, yTilde, YTilde, theta, cfg)
    return _find_optimum(forcesInit, w0, y, yTilde, YTilde, theta, cfg)


def _find_optimum(forcesInit, w0, y, yTilde, YTilde, theta, cfg):
    """Minimise over the m generalised forces (forces.py:336-548).

    Returns (wopt (n,1), yopt (m,), forces_opt (m,), fmin_initial, fmin_final,
    chiSqr (= 0.5 chi^2), S (= sum w log(w/w0)))."""

    caching = cfg["cache_ytilde_transposed"]
    if caching == "auto":
        caching = common.set_caching_heuristics(yTilde.shape[0], yTilde.shape[1])
    cfg["cache_ytilde_transposed"] = caching

    minimizer = cfg["minimizer"].upper()
    if minimizer not in ('LIBLBFGS', 'LBFGS', 'GSL', 'SCIPY', 'NEWTON'):
        raise RuntimeError("Library " + cfg["minimizer"] +
                           " not recognized (valid values =  'LIBLBFGS', 'GSL', 'scipy', 'scipy', 'newton' ) ")
    use_c = bool(cfg["use_c_functions"])
    use_device = not (minimizer in ('SCIPY', 'NEWTON') and not use_c)

    if use_device:
        fmin_initial = c_bioen.bioen_log_posterior_forces(forcesInit, w0, yTilde, YTilde, theta)
    else:
        fmin_initial = bioen_log_posterior_base(forcesInit, w0, yTilde, YTilde, theta)
    if cfg["verbose"]:
        print("fmin_initial", fmin_initial)

    forces = np.asarray(forcesInit, dtype=np.float64).copy().T    # (1, m)
    dense = minimizer == 'SCIPY' and str(cfg["algorithm"]).lower() in _SCIPY_DENSE
    hessian = _hessian_source(cfg) if minimizer == 'SCIPY' else "products"

    start = time.time()
    if minimizer in ('LIBLBFGS', 'LBFGS'):
        common.print_highlighted("FORCES -- Library L-BFGS/HIP", cfg["verbose"])
        res = c_bioen.bioen_opt_lbfgs_forces(forces, w0, yTilde, YTilde, theta, cfg)
    elif minimizer == 'GSL':
        common.print_highlighted("FORCES -- Library GSL/C", cfg["verbose"])
        res = c_bioen.bioen_opt_bfgs_forces(forces, w0, yTilde, YTilde, theta, cfg)
    elif minimizer == 'NEWTON' and use_c:
        common.print_highlighted("FORCES -- Library Newton/HIP", cfg["verbose"])
        res = c_bioen.bioen_opt_newton_forces(forces, w0, yTilde, YTilde, theta, cfg)
    elif minimizer == 'NEWTON':
        common.print_highlighted("FORCES -- Library Newton/PY", cfg["verbose"])
        res = _newton_finish("newton_bioen_log_posterior_base",
                             newton_bioen_log_posterior_base(forces, w0, yTilde, YTilde, theta, cfg["params"]))
    elif minimizer == 'SCIPY' and use_c:
        common.print_highlighted("FORCES -- Library scipy/HIP", cfg["verbose"])
        dev = _DeviceFdf(w0, yTilde, YTilde, theta, keep_point=dense, hessian=hessian)
        try:
            if dense:
                res = _run_scipy_trust_exact(cfg, dev.f, dev.fprime, dev.hess, forces, ())
            else:
                res = _run_scipy(cfg, dev.f, dev.fprime, forces, (), "c", True)
        finally:
            dev.close()
    else:
        common.print_highlighted("FORCES -- Library scipy/PY", cfg["verbose"])
        if dense:
            res = _run_scipy_trust_exact(cfg, bioen_log_posterior_base, grad_bioen_log_posterior_base,
                                         {"gram": _hess_gram_base, "gram_bf16": _hess_gram_bf16_base}.get(
                                             hessian, hessian_bioen_log_posterior_base),
                                         forces, (w0, yTilde, YTilde, theta))
        else:
            res = _run_scipy(cfg, bioen_log_posterior_base, grad_bioen_log_posterior_base, forces,
                             (w0, yTilde, YTilde, theta), "py", False)
    end = time.time()
    if cfg["verbose"]:
        print('time elapsed ', (end - start))

    # the reference's c_bioen / scipy drivers hand back a 1-D (m,) vector whose `.T` is itself (forces.py:532-535),
    # and bioen/analyze/procedure.py:77 relies on it: np.matrix(out_min[2]).T must be the (m, 1) start of the next theta
    forces_opt = np.asarray(res[0], dtype=np.float64).reshape(-1)
    fmin_final = res[1]

    if use_device:
        w, chiSqr = c_bioen.chi2_and_kl_forces(forces_opt, w0, yTilde, YTilde)
        wopt = w.reshape(-1, 1)
        S = _kl(wopt, w0)
        yopt = c_bioen.get_ave(wopt, yTilde, YTilde) if y is yTilde else common.getAve(wopt, y)
    else:
        wopt = get_weights_from_forces(w0, yTilde, forces_opt)
        yopt = common.getAve(wopt, y)
        S, chiSqr = bioen_chi2_s_forces(forces_opt, w0, yTilde, YTilde)

    if cfg["verbose"]:
        print("========================")
        print("fmin_initial           =", fmin_initial)
        print("fmin_final             =", fmin_final)
        print("========================")
    return wopt, yopt, forces_opt, fmin_initial, fmin_final, chiSqr, S

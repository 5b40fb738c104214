"""Log-weights method: public API of ``bioen/optimize/log_weights.py`` on MI355X.

Signatures, argument shapes, return tuples and exception types follow the
reference (file:line cited per function); the numerics of every `use_c=True`
path run in the HIP kernels behind ``ext.c_bioen``.  The ``*_base`` functions are
the reference's explicit pure-numpy variants (``use_c=False`` /
``use_c_functions: false``), kept because callers can ask for them by name.

  L(g)      = theta * ( sum_j w_j (g_j - G_j) - log sum e^g + log sum e^G ) + 0.5 |yTilde w - YTilde|^2
  dL/dg_k   = theta w_k [(g_k - G_k) - sum_j w_j (g_j - G_j)] + w_k [(yTilde^T r)_k - ybar . r]
"""
from __future__ import print_function

import time

import numpy as np
import scipy.optimize as sopt

from . import common
from .ext import c_bioen


def _col(x):
    """(n,1) float64 ndarray view of a vector-like (np.matrix, (n,), (n,1), (1,n))."""
    return np.asarray(x, dtype=np.float64).reshape(-1, 1)


# ------------------------------------------------------------------ legacy helpers
def getWeights(g):
    """w = exp(g) / s, s = sum exp(g)  (log_weights.py:93-110). Returns (w, s)."""
    ga = np.asarray(g, dtype=np.float64)
    shift = ga.max()
    e = np.exp(ga - shift)
    se = e.sum()
    return np.array(e / se), float(se * np.exp(shift))


def getGs(w):
    """log-weights relative to the last structure (log_weights.py:113-127); w is (n,1)."""
    g = np.log(w)
    g -= g[-1, 0]
    return g


def init_log_weights(w0):
    """(gPrime, g, G, GInit) from reference weights (log_weights.py:71-90)."""
    G = getGs(w0)
    GInit = getGs(np.array(w0))
    g = GInit.copy()
    gPrime = np.asarray(g[:-1].T)[0]
    return gPrime, g, G, GInit


def getWOpt(G, gPrimeOpt):
    """Optimal weights as an (n,1) array from optimal log-weights (log_weights.py:130-160)."""
    w, _ = getWeights(_col(gPrimeOpt))
    return w


def bioen_log_prior(w, s, g, G, theta):
    """theta * ( g.w - G.w - log s + log s0 )  (log_weights.py:18-68)."""
    _, s0 = getWeights(G)
    w, g, G = _col(w), _col(g), _col(G)
    return float(theta * ((g.T.dot(w)).item() - (G.T.dot(w)).item() - np.log(s) + np.log(s0)))


def grad_chiSqrTerm(gPrime, g, G, yTilde, YTilde, theta):
    """Gradient of the chi^2 term w.r.t. the first n-1 log-weights, the last one pinned
    to zero (legacy parametrisation, log_weights.py:164-188)."""
    np.asarray(g)[:-1, 0] = np.asarray(gPrime).reshape(-1)
    np.asarray(g)[-1, 0] = 0
    w, _ = getWeights(g)
    w = _col(w)
    yT = np.asarray(yTilde, dtype=np.float64)
    ybar = yT.dot(w)
    r = ybar - _col(YTilde)
    tmp = w[:, 0] * (yT.T.dot(r)[:, 0] - ybar.T.dot(r).item())
    return tmp[:-1]


def check_params_logweights(GInit, G, y, yTilde, YTilde):
    """Shape contract: GInit,G (n,1); y,yTilde (m,n); YTilde (1,m) (log_weights.py:191-233)."""
    m, n = yTilde.shape
    expected = (("GInit", GInit, (n, 1)), ("G", G, (n, 1)), ("y", y, (m, n)), ("YTilde", YTilde, (1, m)))
    bad = False
    for name, arr, shape in expected:
        if arr.shape != shape:
            print("Unexpected shape for variable: {name}\nExpected: {expected}\nCurrent:  {current}".format(
                name=name, expected=shape, current=arr.shape))
            bad = True
    if bad:
        raise ValueError("arguments dimensionality for the 'log_weights' method are wrong")


# ------------------------------------------------------------------ objective / gradient
def bioen_log_posterior(gPrime, g, G, yTilde, YTilde, theta, use_c=True, caching=False):
    """Negative log-posterior (log_weights.py:237-260). use_c=True -> HIP kernels."""
    if use_c:
        return c_bioen.bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, theta, caching=caching)
    return bioen_log_posterior_base(gPrime, g, G, yTilde, YTilde, theta)


def grad_bioen_log_posterior(gPrime, g, G, yTilde, YTilde, theta, use_c=True, caching=False):
    """Gradient w.r.t. the n log-weights (log_weights.py:263-286). use_c=True -> HIP kernels."""
    if use_c:
        return c_bioen.grad_bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, theta, caching=caching)
    return grad_bioen_log_posterior_base(gPrime, g, G, yTilde, YTilde, theta)


def hessp_bioen_log_posterior(gPrime, p, g, G, yTilde, YTilde, theta, use_c=True, caching=False):
    """Hessian-vector product H(gPrime) p w.r.t. the n log-weights (no reference counterpart; the twin of
    grad_bioen_log_posterior). use_c=True -> HIP kernels."""
    if use_c:
        return c_bioen.hessp_bioen_log_posterior_logw(gPrime, p, g, G, yTilde, YTilde, theta, caching=caching)
    return hessp_bioen_log_posterior_base(gPrime, p, g, G, yTilde, YTilde, theta)


def bioen_log_posterior_base(gPrime, g, G, yTilde, YTilde, theta):
    """Pure-numpy objective (log_weights.py:289-328).  Like the reference it writes the
    current point into `g` in place."""
    np.asarray(g)[:, 0] = np.asarray(gPrime, dtype=np.float64).reshape(-1)   # view: works for np.matrix too
    w, s = getWeights(g)
    return bioen_log_prior(w, s, g, G, theta) + common.chiSqrTerm(w, yTilde, YTilde)


def grad_bioen_log_posterior_base(gPrime, g, G, yTilde, YTilde, theta):
    """Pure-numpy gradient (log_weights.py:332-406) in closed form.

    The reference's Python version has a sign slip in the <G> term
    (`op2 = G + G.T w`, log_weights.py:370,389); its C kernel
    (c_bioen_kernels_logw.c:216) and the mathematics have `- G + <G>`, which is what
    this function implements.  The two agree whenever G == 0 or theta == 0 -- the only
    cases the reference's tests exercise."""
    gp = _col(gPrime)
    Gc = _col(G)
    w, _ = getWeights(gp)
    yT = np.asarray(yTilde, dtype=np.float64)
    ybar = yT.dot(w)
    r = ybar - _col(YTilde)
    t = w * (yT.T.dot(r) - ybar.T.dot(r).item())
    dev = gp - Gc
    grad = theta * w * (dev - w.T.dot(dev).item()) + t
    return grad[:, 0]


def hessp_bioen_log_posterior_base(gPrime, p, g, G, yTilde, YTilde, theta):
    """Pure-numpy Hessian-vector product H(gPrime) p in closed form (exact, not Gauss-Newton; H is indefinite away from
    the optimum).  With w = softmax(g), pbar = w . p and grad the gradient above:

      dw   = w (p - pbar)
      c    = yTilde^T dr - ybar . dr,   dr = yTilde dw
      H p  = (p - pbar) grad + w [ theta (p - pbar) + c - p . grad ]
    """
    gp = _col(gPrime)
    Gc = _col(G)
    pc = _col(p)
    w, _ = getWeights(gp)
    yT = np.asarray(yTilde, dtype=np.float64)
    ybar = yT.dot(w)
    r = ybar - _col(YTilde)
    dev = gp - Gc
    grad = theta * w * (dev - w.T.dot(dev).item()) + w * (yT.T.dot(r) - ybar.T.dot(r).item())
    dp = pc - w.T.dot(pc).item()
    dr = yT.dot(w * dp)
    c = yT.T.dot(dr) - ybar.T.dot(dr).item()
    hp = dp * grad + w * (theta * dp + c - grad.T.dot(pc).item())
    return hp[:, 0]


# ------------------------------------------------------------------ the dual Newton minimizer
#  N unknowns through an M x M system: with the gradient-proportional terms of the Hessian dropped,
#   H~ = theta S + W Yc^T Yc W   (S = W - w w^T, Yc = yTilde - ybar 1^T; = H at the optimum),
# the step H~ u = -grad, w . u = 0, is  (C + theta I) z = -Yc grad,  C = Yc W Yc^T,
#   u = -[(dev - P) + (1 / theta) Yc^T (r + z)]      (dev = g - G, P = w . dev, r = ybar - YTilde)
_DUAL_NEWTON_CONSTANTS = dict(armijo=1e-4, floor_ulps=8.0, max_halvings=60)
DUAL_NEWTON_STATUS = {0: "max|grad| <= gtol max w", 1: "max_iterations reached",
                      2: "step exhausted at the rounding floor of f", 3: "step exhausted"}


def _dual_newton_point(g, G, yT, YT, theta, logs0):
    """everything the loop keeps of a point: f, grad = w gamma, and the pieces of the step"""
    shift = g.max()
    e = np.exp(g - shift)
    s = e.sum()
    w = e / s
    ybar = yT.dot(w)
    r = ybar - YT
    dev = g - G
    P = float(w.dot(dev))
    f = float(theta * (P - (np.log(s) + shift) + logs0) + 0.5 * r.dot(r))
    gamma = theta * (dev - P) + (yT.T.dot(r) - float(ybar.dot(r)))
    return dict(g=g, f=f, w=w, ybar=ybar, r=r, dev=dev, P=P, gamma=gamma, grad=w * gamma)


def dual_newton_covariance(p, yT):
    """C = Yc W Yc^T of a point of _dual_newton_point: the covariance of the observables under its weights"""
    Yc = yT - p["ybar"][:, None]
    return (Yc * p["w"]).dot(Yc.T)


def dual_newton_covariance_bf16(p, yT, centre):
    """The numpy restatement of Context.logw_cov_bf16: dual_newton_covariance with the M x M x N product from
    split-BF16 operands, as the covariance of a Newton step.  With Y' = yT - centre (the device's centre: YTilde), w the
    point's weights and bf(v) = round-to-nearest-even of (float)v to bfloat16 (forces._bf16_split):

      a = Y'_ij (FP64)         a_hi = bf(a),  a_lo = bf((float)a - a_hi)
      t = a w_j (FP64)         t_hi = bf(t),  t_lo = bf((float)t - t_hi)
      G' = sum_j (a_hi t_hi + a_hi t_lo + a_lo t_hi)            each product exact in FP64, summed in FP64
      C~ = G' - ybar' ybar'^T,  ybar' = ybar - centre           FP64

    The lower triangle is computed and mirrored: symmetric bit for bit."""
    from .forces import _bf16_split
    a = yT - np.asarray(centre, dtype=np.float64).reshape(-1)[:, None]
    a_hi, a_lo = _bf16_split(a)
    t_hi, t_lo = _bf16_split(a * p["w"][None, :])
    yc = p["ybar"] - np.asarray(centre, dtype=np.float64).reshape(-1)
    C = a_hi.dot(t_hi.T) + a_hi.dot(t_lo.T) + a_lo.dot(t_hi.T) - np.outer(yc, yc)
    return np.tril(C) + np.tril(C, -1).T


def dual_newton_step(p, yT, theta, C=None):
    """(u, z) at a point of _dual_newton_point: one covariance (C: from another source than dual_newton_covariance; only
    the step's quality depends on it), one Cholesky factorisation of C + theta I (SPD for every theta > 0), one centred
    forward pass on grad, one centred adjoint pass on r + z"""
    import scipy.linalg
    Yc = yT - p["ybar"][:, None]
    if C is None:
        C = (Yc * p["w"]).dot(Yc.T)
    b = Yc.dot(p["grad"])
    L = np.linalg.cholesky(C + theta * np.eye(C.shape[0]))
    z = -scipy.linalg.cho_solve((L, True), b)
    u = -((p["dev"] - p["P"]) + Yc.T.dot(p["r"] + z) / theta)
    return u, z


# ------------------------------------------------------------------ Laplace error bars
def laplace_error_bars(gPrime, G, y, yTilde, YTilde, theta, observables=None, use_c=True, matrices=True):
    """Laplace error bars at log-weights `gPrime` (n,) -- an optimum of the log-weights objective -- from the Hessian
    H~ = theta (W - w w^T) + W Yc^T Yc W of the dual Newton step, which is the exact Hessian at an optimum.  H~ 1 = 0 is
    the gauge of the log-weights, so only gauge-invariant quantities have a posterior covariance; through Woodbury on the
    M x M system the dual Newton solves, with w = softmax(gPrime), a_j = y_j - ybar, C = sum_j w_j a_j a_j^T and
    P = inv(C + theta I):  -> dict

      w (n,), C (m, m), logdet = ln det (C + theta I)
      leverage (n,): w_j a_j^T P a_j, in [0, 1 - w_j) -- the share of structure j's prior log-weight variance the data removed
      var_logw (n,): (1 - w_j - leverage_j) / (theta w_j) = (e_j - w)^T pinv(H~) (e_j - w), the variance of ln w_j
      std_w (n,):    sqrt(w_j (1 - w_j - leverage_j) / theta)
      cov_averages = C P = I - theta P, std_averages    (m, m), (m,)   of ybar in the units of yTilde
      with `observables`, (n,) or (k, n) -- per-structure quantities o that were NOT fitted (a held-out data set, a radius
      of gyration): obs_averages (k,) = sum_j w_j o_j, and std_observables (k,), the roots of
      var(obar) = (Var_w(o) - c^T P c) / theta,  c = sum_j w_j (o_j - obar) a_j,  Var_w(o) = sum_j w_j (o_j - obar)^2

    An individual weight is poorly determined whenever theta w_j << 1 (std_w_j / w_j ~ 1 / sqrt(theta w_j)): the
    information is in the averages and the held-out averages.  cov_averages coincides with forces.laplace_error_bars' at the
    shared optimum (H = theta C + C C there).

    use_c: one Context.logw_laplace call on a resident context (M <= 1024), plus logw_cov at the kept point
    for C; with matrices=False C and cov_averages are None and nothing of size m^2 is downloaded.  Else the numpy
    restatement, the specification: the closed forms above with np.linalg.cholesky.  ValueError if theta <= 0 or the
    factorisation fails (a point that is not finite).  `G` enters only the device's evaluation of the point; `y` unused."""
    g = np.asarray(gPrime, dtype=np.float64).reshape(-1)
    theta = float(theta)
    if not (theta > 0.0 and np.isfinite(theta)):
        raise ValueError("laplace_error_bars needs theta > 0 (the error bars divide by theta), got %r" % theta)
    obs = None
    if observables is not None:
        obs = np.asarray(observables, dtype=np.float64)
        obs = obs.reshape(1, -1) if obs.ndim == 1 else obs
        if obs.ndim != 2 or obs.shape[1] != g.size or obs.shape[0] < 1:
            raise ValueError("observables must be (n,) or (k, n) with n = %d, got %s" % (g.size, (np.shape(observables),)))
    if use_c:
        r, C = c_bioen.laplace_logw(g, G, yTilde, YTilde, theta, obs, matrices)
        if r["info"] != 0:
            raise ValueError("laplace_error_bars: C + theta I did not factorise (the device factorisation ended at pivot "
                             "%d): the point is not finite" % r["info"])
        out = {"w": r["w"], "C": C, "cov_averages": r["cov_averages"], "std_averages": r["std_averages"],
               "leverage": r["leverage"], "var_logw": r["var_logw"], "std_w": r["std_w"], "logdet": r["logdet"]}
        if obs is not None:
            out.update(obs_averages=r["obs_averages"], std_observables=np.sqrt(np.maximum(r["var_observables"], 0.0)))
        return out
    import scipy.linalg
    yT = np.asarray(yTilde, dtype=np.float64)
    if not np.isfinite(g).all():
        raise ValueError("laplace_error_bars: the point is not finite")
    e = np.exp(g - g.max())
    w = e / e.sum()
    A = yT - yT.dot(w)[:, None]
    C = (A * w).dot(A.T)
    C = np.tril(C) + np.tril(C, -1).T
    m = C.shape[0]
    try:
        L = np.linalg.cholesky(C + theta * np.eye(m))
    except np.linalg.LinAlgError:
        raise ValueError("laplace_error_bars: C + theta I did not factorise: the point is not finite")
    P = scipy.linalg.cho_solve((L, True), np.eye(m))
    P = 0.5 * (P + P.T)
    leverage = w * np.einsum("ij,ij->j", A, P.dot(A))
    rest = (1.0 - w) - leverage
    cov_av = np.eye(m) - theta * P
    out = {"w": w, "C": C, "cov_averages": cov_av, "std_averages": np.sqrt(np.maximum(np.diag(cov_av), 0.0)),
           "leverage": leverage, "var_logw": rest / (theta * w), "std_w": np.sqrt(np.maximum(w * rest, 0.0) / theta),
           "logdet": 2.0 * float(np.log(np.diag(L)).sum())}
    if obs is not None:
        obar = obs.dot(w)
        d = obs - obar[:, None]
        var_w = (d * d).dot(w)
        c = (d * w).dot(A.T)                                   # (k, m)
        var = (var_w - np.einsum("ki,ki->k", c, scipy.linalg.cho_solve((L, True), c.T).T)) / theta
        out.update(obs_averages=obar, std_observables=np.sqrt(np.maximum(var, 0.0)))
    if not matrices:
        out.update(C=None, cov_averages=None)
    return out


_DUAL_NEWTON_SOURCES = ("gram", "gram_bf16")


def _dual_newton_source(params):
    """the dual_newton parameter `hessian`, checked: -> "gram" | "gram_bf16" """
    source = str(dict(params).get("hessian", "gram")).lower()
    if source not in _DUAL_NEWTON_SOURCES:
        raise RuntimeError("dual_newton:hessian=" + source + " not recognized (valid values = 'gram', 'gram_bf16')")
    return source


def _dual_newton_series_mode(params):
    """the dual_newton parameter `series`, checked: -> warm (True) | cold (False)"""
    mode = str(dict(params).get("series", "warm")).lower()
    if mode not in ("warm", "cold"):
        raise RuntimeError("dual_newton:series=" + mode + " not recognized (valid values = 'warm', 'cold')")
    return mode == "warm"


def dual_newton_bioen_log_posterior_base(gInit, G, yTilde, YTilde, theta, params, cov=None):
    """The numpy statement of the dual Newton minimizer of the log-weights objective, the specification
    of the device loop.  The covariance of the step comes from `params["hessian"]`: "gram" (dual_newton_covariance, the
    default) or "gram_bf16" (dual_newton_covariance_bf16); `cov`, a dict source -> function(p, yT, centre), replaces them.

      1. stop: max|grad| <= gtol max w (the weight gate is relative to max w, so the test is) AND max|gamma| <= theta,
         grad = w gamma -> status 0.  The second half is the globalisation: where a step of size ~ 1 / theta has
         collapsed the softmax onto a few structures, every w_k gamma_k is tiny although gamma is not; gamma_k / theta is
         the change of log-weight k the mirror step still asks for, and at a minimum it is far below 1 for EVERY k (the
         step sets the negligible structures' log-weights to exactly that).  A point that fails it is iterated on.
      2. max_iterations accepted steps -> status 1.
      3. u from dual_newton_step (one factorisation), slope = grad . u.
      4. alpha = 1, 1/2, ...: f+ at g + alpha u; accept if f+ is finite and f+ - f <= 1e-4 alpha slope; at the rounding
         floor (|alpha slope| <= 8 eps |f|: f cannot judge the step) accept on max|grad+| < max|grad| instead, and a
         rejection there ends the run: status 2.  max_halvings rejections elsewhere: status 3.
      5. rejected at the floor with "gram_bf16": the run goes over to "gram" (once, for the rest of this theta): the kept
         point is evaluated again (one evaluation), then to 1 -- C anew, a new step.  Gradient, stop test and Armijo test
         are FP64 whatever the source: only the step's quality depends on C, the optimum does not move.

    -> dict(g, fmin, status, iterations, evaluations, factorisations, gmax, wmax, bf16_passes, switched).  theta <= 0 is
    refused: the step divides by theta."""
    theta = _dual_newton_theta(theta)
    source = _dual_newton_source(params)
    sources = dict(dict(gram=lambda p, yT, centre: dual_newton_covariance(p, yT), gram_bf16=dual_newton_covariance_bf16),
                   **(cov or {}))
    yT = np.asarray(yTilde, dtype=np.float64)
    YT = np.asarray(YTilde, dtype=np.float64).reshape(-1)
    Gv = np.asarray(G, dtype=np.float64).reshape(-1)
    logs0 = _log_sum_exp(Gv)
    return _dual_newton_loop(lambda g: _dual_newton_point(g, Gv, yT, YT, theta, logs0),
                             lambda p, src: dual_newton_step(p, yT, theta, C=sources[src](p, yT, YT))[0],
                             gInit, theta, params, source)[0]


def _dual_newton_theta(theta):
    theta = float(theta)
    if not theta > 0.0:
        raise RuntimeError("dual_newton needs theta > 0 (the step divides by theta), got %r" % theta)
    return theta


def _log_sum_exp(Gv):
    return float(np.log(np.exp(Gv - Gv.max()).sum()) + Gv.max())


def _dual_newton_loop(point, step, gInit, theta, params, source):
    """The decisions 1 .. 5 of dual_newton_bioen_log_posterior_base on a point function g -> dict(g, f, w, gamma, grad, ...)
    and a step function (p, source) -> u: what the plain and the profiled minimizer share"""
    c_ = dict(_DUAL_NEWTON_CONSTANTS, **{k: v for k, v in dict(params).items() if k in _DUAL_NEWTON_CONSTANTS})
    gtol, maxit = float(params.get("gtol", 1e-6)), int(params.get("max_iterations", 200))
    eps = np.finfo(np.float64).eps
    p = point(np.asarray(gInit, dtype=np.float64).reshape(-1).copy())
    count = dict(iterations=0, evaluations=1, factorisations=0, bf16_passes=0)
    status, switched = None, False
    while status is None:
        gmax, wmax = float(np.abs(p["grad"]).max()), float(p["w"].max())
        if np.isfinite(p["f"]) and gmax <= gtol * wmax and float(np.abs(p["gamma"]).max()) <= theta:
            status = 0
            break
        if count["iterations"] >= maxit:
            status = 1
            break
        if not np.isfinite(p["f"]):                 # C + theta I of a point that is not finite does not factorise
            count["factorisations"] += 1
            count["bf16_passes"] += source == "gram_bf16"
            status = 3
            break
        u = step(p, source)
        count["factorisations"] += 1
        count["bf16_passes"] += source == "gram_bf16"
        slope = float(p["grad"].dot(u))
        alpha, trial, go_over = 1.0, None, False
        for _ in range(int(c_["max_halvings"])):
            q = point(p["g"] + alpha * u)
            count["evaluations"] += 1
            floor = abs(alpha * slope) <= c_["floor_ulps"] * eps * abs(p["f"])
            if floor:
                if np.isfinite(q["f"]) and float(np.abs(q["grad"]).max()) < gmax:
                    trial = q
                elif source == "gram_bf16":
                    go_over = True
                else:
                    status = 2
                break
            if np.isfinite(q["f"]) and q["f"] - p["f"] <= c_["armijo"] * alpha * slope:
                trial = q
                break
            alpha *= 0.5
        if go_over:
            source, switched = "gram", True
            count["evaluations"] += 1               # the device evaluates the kept point again: the slot held the trial
            continue
        if trial is None:
            status = status or 3
            break
        p = trial
        count["iterations"] += 1
    return dict(count, g=p["g"], fmin=p["f"], status=status, gmax=float(np.abs(p["grad"]).max()),
                wmax=float(p["w"].max()), switched=switched), p


def dual_newton_series_base(gInit, G, yTilde, YTilde, thetas, params, warm=True):
    """The numpy statement of Context.opt_dual_newton_logw_series: dual_newton_bioen_log_posterior_base for
    the thetas in the order given; warm: theta k starts at the g theta k - 1 returned -- whatever its status --, else every
    theta at gInit.  -> the list of its dicts; a status != 0 does not stop the series."""
    thetas = [float(t) for t in thetas]
    if not thetas or not all(t > 0.0 and np.isfinite(t) for t in thetas):
        raise RuntimeError("dual_newton needs at least one theta, every theta > 0 and finite, got %r" % (thetas,))
    g = np.asarray(gInit, dtype=np.float64).reshape(-1)
    out = []
    for t in thetas:
        out.append(dual_newton_bioen_log_posterior_base(g, G, yTilde, YTilde, t, params))
        if warm:
            g = out[-1]["g"]
    return out


# ------------------------------------------------------------------ nuisance scales profiled out
# The affine model r = off + sigma o (Y w) - YTilde with one least-squares scale s_k per group of rows, sigma_i = s_group(i):
# the scales are a function of the point (nuisance.refit_scales's closed form at ybar = Y w), the profile objective
#   phi(g) = theta KL(w || w0) + 1/2 r^T r     has the gradient of the affine objective at row_scale = sigma (envelope:
# d/ds_k 1/2 r^T r = sum_{i in k} r_i ybar_i = 0 at s_k), and its Gauss-Newton Hessian is theta S_w + W Yc^T S Pi S Yc W,
# Pi = I - sum_k vhat_k vhat_k^T, vhat_k = ybar restricted to group k, normalised (Kaufman's variable projection).
def _profile_groups(groups, m):
    """groups (None: one group of all rows) -> a list of sorted int64 index arrays, checked: disjoint, inside 0 .. m - 1,
    none empty"""
    if groups is None:
        groups = [np.arange(m)]
    out = [np.unique(np.asarray(ix, dtype=np.int64).reshape(-1)) for ix in groups]
    seen = np.zeros(m, dtype=np.int64)
    for ix in out:
        if ix.size == 0 or ix.min() < 0 or ix.max() >= m:
            raise RuntimeError("dual_newton profile: a group is empty or holds a row outside 0 .. %d" % (m - 1))
        seen[ix] += 1
    if not out or seen.max() > 1:
        raise RuntimeError("dual_newton profile: the groups must be disjoint, and at least one")
    return out


def _dual_newton_profile_point(g, G, Y, YT, theta, logs0, groups, off):
    """_dual_newton_point on the profiled model: the scales are formed from the raw averages between the forward pass
    and the residual; ybar stays the RAW average Y w"""
    shift = g.max()
    e = np.exp(g - shift)
    s = e.sum()
    w = e / s
    ybar = Y.dot(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        scales = np.array([ybar[ix].dot(YT[ix] - off[ix]) / ybar[ix].dot(ybar[ix]) for ix in groups])
    sigma = np.ones(Y.shape[0])
    for sk, ix in zip(scales, groups):
        sigma[ix] = sk
    r = off + sigma * ybar - YT
    sr = sigma * r
    dev = g - G
    P = float(w.dot(dev))
    f = float(theta * (P - (np.log(s) + shift) + logs0) + 0.5 * r.dot(r))
    gamma = theta * (dev - P) + (Y.T.dot(sr) - float(ybar.dot(sr)))
    return dict(g=g, f=f, w=w, ybar=ybar, r=r, dev=dev, P=P, gamma=gamma, grad=w * gamma, scales=scales, sigma=sigma)


def dual_newton_profile_covariance(p, Y, groups, C=None):
    """(C_Pi, b_Pi, V) at a point of _dual_newton_profile_point: C_A = S C S and b_A = S Yc grad projected by
    Pi = I - V V^T, V's columns the vhat_k.  C: the raw covariance from another source than dual_newton_covariance.
    C_Pi is formed on the lower triangle from T = V^T C_A and q = T V and mirrored: symmetric bit for bit."""
    Yc = Y - p["ybar"][:, None]
    if C is None:
        C = (Yc * p["w"]).dot(Yc.T)
    sg = p["sigma"]
    CA = (sg[:, None] * C) * sg[None, :]
    b = sg * Yc.dot(p["grad"])
    m = Y.shape[0]
    V = np.zeros((m, len(groups)))
    for k, ix in enumerate(groups):
        V[ix, k] = p["ybar"][ix] / np.sqrt(p["ybar"][ix].dot(p["ybar"][ix]))
    T = V.T.dot(CA)
    q = T.dot(V)
    CP = CA - V.dot(T) - T.T.dot(V.T) + V.dot(q).dot(V.T)
    CP = np.tril(CP) + np.tril(CP, -1).T
    return CP, b - V.dot(V.T.dot(b)), V


def dual_newton_profile_step(p, Y, theta, groups, C=None):
    """(u, z) of the profiled minimizer: (C_Pi + theta I) z = -b_Pi (SPD for every theta > 0; z in the range of Pi),
    u = -[(dev - P) + (1 / theta) Yc^T (sigma o (r + z))]"""
    import scipy.linalg
    CP, bP, _ = dual_newton_profile_covariance(p, Y, groups, C)
    L = np.linalg.cholesky(CP + theta * np.eye(CP.shape[0]))
    z = -scipy.linalg.cho_solve((L, True), bP)
    Yc = Y - p["ybar"][:, None]
    u = -((p["dev"] - p["P"]) + Yc.T.dot(p["sigma"] * (p["r"] + z)) / theta)
    return u, z


def dual_newton_profile_base(gInit, G, Y, YTilde, theta, params, groups, row_offset=None):
    """The numpy statement of the dual Newton minimizer with the nuisance scales profiled out, the
    specification of bioen_logwn_profile_series's loop: dual_newton_bioen_log_posterior_base decision for decision, on
    _dual_newton_profile_point and dual_newton_profile_step.  Y: the parameter-independent matrix; groups: a list of row
    index arrays (None: one group of all rows), rows in no group keep the scale 1.  -> its dict plus scales (one per
    group, at the returned point)."""
    theta = _dual_newton_theta(theta)
    source = _dual_newton_source(params)
    Ym = np.asarray(Y, dtype=np.float64)
    YT = np.asarray(YTilde, dtype=np.float64).reshape(-1)
    off = np.zeros_like(YT) if row_offset is None else np.asarray(row_offset, dtype=np.float64).reshape(-1)
    Gv = np.asarray(G, dtype=np.float64).reshape(-1)
    gr = _profile_groups(groups, Ym.shape[0])
    logs0 = _log_sum_exp(Gv)
    raw = dict(gram=lambda p: None, gram_bf16=lambda p: dual_newton_covariance_bf16(p, Ym, YT))
    res, p = _dual_newton_loop(lambda g: _dual_newton_profile_point(g, Gv, Ym, YT, theta, logs0, gr, off),
                               lambda p, src: dual_newton_profile_step(p, Ym, theta, gr, C=raw[src](p))[0],
                               gInit, theta, params, source)
    return dict(res, scales=[float(s) for s in p["scales"]])


def dual_newton_profile_series_base(gInit, G, Y, YTilde, thetas, params, groups, row_offset=None, warm=True):
    """dual_newton_series_base for the profiled minimizer: the numpy statement of
    Context.opt_dual_newton_logw_profile_series"""
    thetas = [float(t) for t in thetas]
    if not thetas or not all(t > 0.0 and np.isfinite(t) for t in thetas):
        raise RuntimeError("dual_newton needs at least one theta, every theta > 0 and finite, got %r" % (thetas,))
    g = np.asarray(gInit, dtype=np.float64).reshape(-1)
    out = []
    for t in thetas:
        out.append(dual_newton_profile_base(g, G, Y, YTilde, t, params, groups, row_offset))
        if warm:
            g = out[-1]["g"]
    return out


def _dual_newton_finish(who, res):
    """status 0 returns; every other status raises with the return code, as the forces Newton does"""
    if res["status"] != 0:
        raise RuntimeError("%s: return code %d (%s) after %d iterations, max|grad| = %.3g, max w = %.3g"
                           % (who, res["status"], DUAL_NEWTON_STATUS.get(res["status"], "?"), res["iterations"],
                              res["gmax"], res["wmax"]))
    return res["g"], res["fmin"]


# ------------------------------------------------------------------ optimizer
class _DeviceFdf(object):
    """scipy asks for f(x) and f'(x) in separate calls at the same x; one fused device
    evaluation (two matrix passes) serves both."""

    def __init__(self, G, yTilde, YTilde, theta, keep_point=False):
        self.ctx, self._cached = c_bioen._context_for(yTilde, YTilde)
        self._keep_point = keep_point       # the Newton drivers: every evaluation leaves the point for the products at it
        self.G = np.asarray(G, dtype=np.float64).reshape(-1)
        self.theta = theta
        self._x = None
        self._f = None
        self._g = None
        self._point = False       # the context keeps self._x as the point of logw_hessp

    def _eval(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if self._x is None or not np.array_equal(x, self._x):
            if self._keep_point:      # the same evaluation, same bits, and the point stays for hessp at this x
                _, self._f, self._g = self.ctx.logw_hessp(None, g=x, G=self.G, theta=self.theta)
            else:
                self._f, self._g = self.ctx.logw_fdf(x, self.G, self.theta)
            self._x = x.copy()
            self._point = self._keep_point

    def f(self, x, *unused):
        self._eval(x)
        return self._f

    def fprime(self, x, *unused):
        self._eval(x)
        return self._g

    def hessp(self, x, p, *unused):
        """H(x) p: at an x not seen yet ONE device call sets the point and serves f, f' and the product; at the cached x
        the product refers to the point the context keeps (two matrix passes, like a gradient)"""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if self._x is not None and self._point and np.array_equal(x, self._x):
            return self.ctx.logw_hessp(p)
        hv, self._f, self._g = self.ctx.logw_hessp(p, g=x, G=self.G, theta=self.theta)
        self._x = x.copy()
        self._point = True
        return hv

    def close(self):
        c_bioen._release(self.ctx, self._cached)


_SCIPY_ALGORITHMS = {
    # name -> (scipy driver, name of its gradient tolerance, label)
    "lbfgs": (sopt.fmin_l_bfgs_b, "pgtol", "L-BFGS"),
    "fmin_l_bfgs_b": (sopt.fmin_l_bfgs_b, "pgtol", "L-BFGS"),
    "bfgs": (sopt.fmin_bfgs, "gtol", "BFGS"),
    "fmin_bfgs": (sopt.fmin_bfgs, "gtol", "BFGS"),
    "cg": (sopt.fmin_cg, "gtol", "CG"),
    "fmin_cg": (sopt.fmin_cg, "gtol", "CG"),
}


# Second-order drivers: they need Hessian-vector products, which only the log-weights method has (`hessp` of _run_scipy)
_SCIPY_NEWTON = {
    "newton_cg": "Newton-CG", "fmin_ncg": "Newton-CG",
    "trust_ncg": "trust-region Newton-CG", "trust-ncg": "trust-region Newton-CG",
}


def _run_scipy_newton(cfg, f, fprime, hessp, x0, args):
    """scipy's Newton-CG (line search) and trust-region Newton-CG on f, f' and H p; -> (xopt, fopt)"""
    key = cfg["algorithm"].lower()
    p = cfg["params"]
    verbose = cfg["verbose"]
    common.print_highlighted('method ' + _SCIPY_NEWTON[key], verbose)
    if key in ("newton_cg", "fmin_ncg"):
        res = sopt.fmin_ncg(f, x0, fprime, fhess_p=hessp, args=args, avextol=p.get("xtol", 1e-5),
                            maxiter=p["max_iterations"], full_output=True, disp=bool(verbose))
        return res[0], res[1]
    res = sopt.minimize(f, x0, args=args, method="trust-ncg", jac=fprime, hessp=hessp,
                        options={"gtol": p["gtol"], "maxiter": p["max_iterations"], "disp": bool(verbose)})
    return res.x, res.fun


def _run_scipy(cfg, f, fprime, x0, args, flavour, show_caching, hessp=None):
    """The three scipy drivers of log_weights.py:464-598 / forces.py:389-518 as one table; with `hessp` (the log-weights
    method) also the Newton drivers of _SCIPY_NEWTON."""
    key = cfg["algorithm"].lower()
    if hessp is not None and key in _SCIPY_NEWTON:
        return _run_scipy_newton(cfg, f, fprime, hessp, x0, args)
    if key not in _SCIPY_ALGORITHMS:
        raise RuntimeError("Method '" + cfg["algorithm"] + "' not recognized for scipy/" + flavour +
                           " library (valid values =  'lbfgs', 'bfgs', 'cg' ) ")
    driver, tolname, label = _SCIPY_ALGORITHMS[key]
    p = cfg["params"]
    verbose = cfg["verbose"]
    common.print_highlighted('method ' + label, verbose)
    if verbose:
        print("\t", "=" * 25)
        if show_caching:
            print("\t", "caching_yTilde_transposed :     ", cfg["cache_ytilde_transposed"])
        print("\t", "epsilon                   :     ", p["epsilon"])
        print("\t", "%-26s:     " % tolname, p[tolname])
        print("\t", "maxiter                   :     ", p["max_iterations"])
        print("\t", "=" * 25)
    kw = {"args": args, "fprime": fprime, "epsilon": p["epsilon"], tolname: p[tolname],
          "maxiter": p["max_iterations"]}
    if driver is sopt.fmin_l_bfgs_b:
        if verbose:
            kw["disp"] = 1
    else:
        kw["disp"] = bool(verbose)
        kw["full_output"] = True
    return driver(f, x0, **kw)


def _uses_device(cfg):
    return not (str(cfg["minimizer"]).upper() in ('SCIPY', 'DUAL_NEWTON') and not bool(cfg["use_c_functions"]))


def _bfgs_on_device(cfg):
    """scipy's BFGS with the inverse Hessian in HBM (bioen_amd.bfgs): opt-in through the scipy parameter `on_device`
    (``Parameters("scipy", "scipy:on_device=true")``, or the CLI's ``--optimization_parameters scipy:on_device=true``).
    Combinations it cannot serve raise instead of falling back."""
    if str(cfg["minimizer"]).upper() != 'SCIPY' or not cfg["params"].get("on_device"):
        return False
    if str(cfg["algorithm"]).lower() not in ("bfgs", "fmin_bfgs"):
        raise RuntimeError("scipy:on_device runs scipy's BFGS on the device; algorithm '" + str(cfg["algorithm"]) +
                           "' has no device path (use 'bfgs' / 'fmin_bfgs', or drop on_device)")
    if not bool(cfg["use_c_functions"]):
        raise RuntimeError("scipy:on_device needs use_c_functions: true (the device objective); "
                           "use_c_functions: false asks for the numpy objective on the host")
    return True


def _run_device_bfgs(cfg, gPrime, G, yTilde, YTilde, theta):
    """fmin_bfgs's parameters (gtol, max_iterations, disp = verbose) on the device session; -> (gopt, fmin)"""
    p = cfg["params"]
    ctx, cached = c_bioen._context_for(yTilde, YTilde)
    try:
        gopt, _, info = ctx.bfgs_logw(np.asarray(gPrime, dtype=np.float64), np.asarray(G, dtype=np.float64).reshape(-1),
                                      theta, gtol=p["gtol"], maxiter=p["max_iterations"], disp=bool(cfg["verbose"]))
    finally:
        c_bioen._release(ctx, cached)
    return gopt, info.fmin


def find_optimum(GInit, G, y, yTilde, YTilde, theta, cfg):
    """Minimise the BioEn negative log-posterior over the n log-weights (log_weights.py:409-621): see `_find_optimum`.
    The matrix is HELD for the duration of the call (ext/c_bioen.py: hold): the initial objective, the optimisation and
    the averages of the optimum are served by one device copy -- at most ONE upload per call whatever the size of the
    matrix (none inside a caller's ``with optimize.resident(yTilde):``), as the reference's one ``yTilde.T.copy()`` per
    call (c_bioen.pyx:463-473)."""
    check_params_logweights(GInit, G, y, yTilde, YTilde)
    if str(cfg["minimizer"]).upper() not in ('LIBLBFGS', 'LBFGS', 'GSL', 'SCIPY', 'DUAL_NEWTON'):      # rejected before anything touches the device
        raise RuntimeError("Library " + cfg["minimizer"] +
                           " not recognized (valid values =  'LIBLBFGS', 'GSL', 'scipy', 'scipy', 'dual_newton' ) ")
    if str(cfg["minimizer"]).upper() == 'DUAL_NEWTON':
        if not float(theta) > 0.0:
            raise RuntimeError("dual_newton needs theta > 0 (the step divides by theta), got %r" % float(theta))
        _dual_newton_source(cfg["params"])
    _bfgs_on_device(cfg)                               # refused combinations raise here, before the device is touched
    if _uses_device(cfg):
        with c_bioen.hold(yTilde, YTilde):
            return _find_optimum(GInit, G, y, yTilde, YTilde, theta, cfg)
    return _find_optimum(GInit, G, y, yTilde, YTilde, theta, cfg)


def _find_optimum(GInit, G, y, yTilde, YTilde, theta, cfg):
    """Minimise the BioEn negative log-posterior over the n log-weights
    (log_weights.py:409-621).

    Returns (wopt (n,1), yopt (m,), gopt (n,), fmin_initial, fmin_final).
    cfg comes from ``minimize.Parameters``; minimizer "lbfgs"/"liblbfgs" runs the
    device-resident L-BFGS, "scipy" drives the device (or, with
    use_c_functions False, the numpy) objective from the host; "gsl": the library's GSL-style minimizers with all vectors in HBM."""

    caching = cfg["cache_ytilde_transposed"]
    if caching == "auto":
        caching = common.set_caching_heuristics(yTilde.shape[0], yTilde.shape[1])
    cfg["cache_ytilde_transposed"] = caching      # the reference writes this back, :440

    minimizer = cfg["minimizer"].upper()
    if minimizer not in ('LIBLBFGS', 'LBFGS', 'GSL', 'SCIPY', 'DUAL_NEWTON'):
        raise RuntimeError("Library " + cfg["minimizer"] +
                           " not recognized (valid values =  'LIBLBFGS', 'GSL', 'scipy', 'scipy', 'dual_newton' ) ")
    use_c = bool(cfg["use_c_functions"])
    use_device = _uses_device(cfg)

    g = GInit.copy()
    gPrime = np.asarray(g[:].T)[0]

    if use_device:
        fmin_initial = c_bioen.bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, theta)
    else:
        fmin_initial = bioen_log_posterior_base(gPrime, g, G, yTilde, YTilde, theta)
    if cfg["verbose"]:
        print("fmin_initial", fmin_initial)

    start = time.time()
    if minimizer in ('LIBLBFGS', 'LBFGS'):
        common.print_highlighted("LOGW -- Library L-BFGS/HIP", cfg["verbose"])
        res = c_bioen.bioen_opt_lbfgs_logw(gPrime, G, yTilde, YTilde, theta, cfg)
    elif minimizer == 'GSL':
        common.print_highlighted("LOGW -- Library GSL/C", cfg["verbose"])
        res = c_bioen.bioen_opt_bfgs_logw(gPrime, G, yTilde, YTilde, theta, cfg)
    elif minimizer == 'DUAL_NEWTON' and use_c:
        common.print_highlighted("LOGW -- Library dual Newton/HIP", cfg["verbose"])
        res = c_bioen.bioen_opt_dual_newton_logw(gPrime, G, yTilde, YTilde, theta, cfg)
    elif minimizer == 'DUAL_NEWTON':
        common.print_highlighted("LOGW -- Library dual Newton/PY", cfg["verbose"])
        res = _dual_newton_finish("dual_newton_bioen_log_posterior_base",
                                  dual_newton_bioen_log_posterior_base(gPrime, G, yTilde, YTilde, theta, cfg["params"]))
    elif minimizer == 'SCIPY' and use_c and _bfgs_on_device(cfg):
        common.print_highlighted("LOGW -- Library scipy-BFGS/HIP, inverse Hessian in HBM", cfg["verbose"])
        res = _run_device_bfgs(cfg, gPrime, G, yTilde, YTilde, theta)
    elif minimizer == 'SCIPY' and use_c:
        common.print_highlighted("LOGW -- Library scipy/HIP", cfg["verbose"])
        dev = _DeviceFdf(G, yTilde, YTilde, theta, keep_point=str(cfg["algorithm"]).lower() in _SCIPY_NEWTON)
        try:
            res = _run_scipy(cfg, dev.f, dev.fprime, gPrime, (), "c", True, hessp=dev.hessp)
        finally:
            dev.close()
    else:
        common.print_highlighted("LOGW -- Library scipy/PY", cfg["verbose"])
        res = _run_scipy(cfg, bioen_log_posterior_base, grad_bioen_log_posterior_base, gPrime,
                         (g, G, yTilde, YTilde, theta), "py", False, hessp=hessp_bioen_log_posterior_base)
    end = time.time()
    if cfg["verbose"]:
        print('time elapsed ', (end - start))

    gopt = res[0]
    fmin_final = res[1]
    wopt = getWOpt(G, gopt)
    if use_device and y is yTilde:
        yopt = c_bioen.get_ave(wopt, yTilde, YTilde)   # yTilde . wopt from the resident matrix
    else:
        yopt = common.getAve(wopt, y)

    if cfg["verbose"]:
        print("========================")
        print("fmin_initial  = ", fmin_initial)
        print("fmin_final    = ", fmin_final)
        print("========================")
    return wopt, yopt, gopt, fmin_initial, fmin_final


def _find_optimum_series_dual_newton(GInit, G, y, yTilde, YTilde, thetas, cfg):
    """find_optimum_series with the dual_newton minimizer: on the device one call for the series (the matrix held once),
    with use_c_functions false dual_newton_series_base on the numpy objective"""
    thetas = [float(t) for t in thetas]
    if not thetas or not all(t > 0.0 and np.isfinite(t) for t in thetas):       # refused before anything touches the device
        raise RuntimeError("dual_newton needs at least one theta, every theta > 0 (the step divides by theta), got %r" % (thetas,))
    _dual_newton_source(cfg["params"])
    warm = _dual_newton_series_mode(cfg["params"])
    g = GInit.copy()
    gPrime = np.asarray(g[:].T)[0]

    def finish(f0, gopts, fmins, ave):
        out = []
        for k in range(len(thetas)):
            wopt = getWOpt(G, gopts[k])
            out.append((wopt, ave(wopt), gopts[k], f0[k], fmins[k]))
        return out

    if not _uses_device(cfg):
        f0 = [bioen_log_posterior_base(gPrime, g, G, yTilde, YTilde, t) for t in thetas]
        res = dual_newton_series_base(gPrime, G, yTilde, YTilde, thetas, cfg["params"], warm=warm)
        for t, r in zip(thetas, res):
            _dual_newton_finish("dual_newton_series_base: theta = %r" % t, r)
        return finish(f0, [r["g"] for r in res], [r["fmin"] for r in res], lambda w: common.getAve(w, y))
    with c_bioen.hold(yTilde, YTilde):                 # one device copy for the whole series: at most one upload
        f0 = [c_bioen.bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, t) for t in thetas]
        gopts, fmins = c_bioen.bioen_opt_dual_newton_logw_series(gPrime, G, yTilde, YTilde, thetas, cfg)
        return finish(f0, gopts, fmins,
                      lambda w: c_bioen.get_ave(w, yTilde, YTilde) if y is yTilde else common.getAve(w, y))


def find_optimum_series(GInit, G, y, yTilde, YTilde, thetas, cfg):
    """Not in the reference: ``find_optimum`` for a whole theta series in one device call
    (what bioen/analyze/procedure.py:62-67 does one theta at a time).  Minimizer "lbfgs"/"liblbfgs": cold-started,
    the optimisation itself bit for bit the single runs, since a batched run equals them.  Minimizer "dual_newton"
    (DESIGN 6k): the thetas in the order given, theta k warm-started at theta k - 1's optimum -- or every theta from GInit
    with ``dual_newton:series=cold`` --, the covariance of the steps from ``dual_newton:hessian``; a theta whose status is
    not 0 raises, as ``find_optimum`` does.  Every entry of the returned list is the 5-tuple ``find_optimum`` returns
    for that theta."""
    check_params_logweights(GInit, G, y, yTilde, YTilde)
    if cfg["minimizer"].upper() == 'DUAL_NEWTON':
        return _find_optimum_series_dual_newton(GInit, G, y, yTilde, YTilde, thetas, cfg)
    if cfg["minimizer"].upper() not in ('LIBLBFGS', 'LBFGS'):
        raise RuntimeError("find_optimum_series needs the lbfgs or the dual_newton minimizer, got " + str(cfg["minimizer"]))
    g = GInit.copy()
    gPrime = np.asarray(g[:].T)[0]
    with c_bioen.hold(yTilde, YTilde):                 # one device copy for the whole series: at most one upload
        fmin_initial = [c_bioen.bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, float(t)) for t in thetas]
        gopts, fmins = c_bioen.bioen_opt_lbfgs_logw_series(gPrime, G, yTilde, YTilde, [float(t) for t in thetas], cfg)
        out = []
        for k in range(len(fmins)):
            wopt = getWOpt(G, gopts[k])
            yopt = c_bioen.get_ave(wopt, yTilde, YTilde) if y is yTilde else common.getAve(wopt, y)
            out.append((wopt, yopt, gopts[k], fmin_initial[k], fmins[k]))
    return out

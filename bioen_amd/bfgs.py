"""scipy's BFGS on a vector backend: the loop of ``scipy.optimize._optimize._minimize_bfgs`` (scipy 1.15) and its
``_line_search_wolfe12`` glue, restated on top of scipy's OWN scalar line searches (``scalar_search_wolfe1`` /
``scalar_search_wolfe2``), with every vector operation behind a small backend:

  begin(norm)            -> (f0, |g0| in `norm`, |g0|_2, g0.p0)        p0 = -g0
  trial(alpha, need_grad)-> (f or None, phi'(alpha) or None, nf, ng)   nf / ng: evaluations ScalarFunction would count
  accept(alpha, norm)    -> (|g| in `norm`, |p|_2, |x|_2)              x += alpha p, the pair (s, y), g = g(alpha)
  update()               -> (g.p, rho_fallback)                        the inverse-Hessian update, p = -H g
  finish()               -> (x, g, H or None)

``NumpyBackend`` does what scipy does, with numpy, in scipy's order: the driver on it reproduces
``scipy.optimize.fmin_bfgs(..., full_output=True)`` bit for bit (the CPU oracle of the driver logic).
``DeviceBackend`` runs on a log-weights ``Context``: the point, the gradient and the N x N inverse Hessian stay in HBM
(include/bioen_hip.h: bioen_hip_bfgs_logw_*); only scalars cross PCIe per trial.  The scalar decisions are scipy's.
"""
from __future__ import print_function

import warnings

import numpy as np

STATUS_MESSAGES = {
    0: "Optimization terminated successfully.",
    1: "Maximum number of iterations has been exceeded.",
    2: "Desired error not necessarily achieved due to precision loss.",
    3: "NaN result encountered.",
}


class BfgsResult(object):
    """What the driver decided: fmin, iterations, func_calls, grad_calls, warnflag, message."""

    def __init__(self, fmin, iterations, func_calls, grad_calls, warnflag):
        self.fmin = fmin
        self.iterations = iterations
        self.func_calls = func_calls
        self.grad_calls = grad_calls
        self.warnflag = warnflag
        self.message = STATUS_MESSAGES[warnflag]

    def __repr__(self):
        return ("BfgsResult(fmin=%r, iterations=%d, func_calls=%d, grad_calls=%d, warnflag=%d)"
                % (self.fmin, self.iterations, self.func_calls, self.grad_calls, self.warnflag))


class _LineSearchError(RuntimeError):
    pass


def _scalar_searches():
    """scipy's scalar line searches, imported when a run starts (not at package import)."""
    try:
        from scipy.optimize._linesearch import scalar_search_wolfe1, scalar_search_wolfe2, LineSearchWarning
        from scipy.optimize import OptimizeWarning
    except ImportError as e:
        raise RuntimeError("bioen_amd.bfgs needs scipy's scalar line searches "
                           "(scipy.optimize._linesearch.scalar_search_wolfe1 / _wolfe2): %s" % e)
    return scalar_search_wolfe1, scalar_search_wolfe2, LineSearchWarning, OptimizeWarning


class _Counted(object):
    """phi / derphi of the current direction, and the evaluation counts of scipy's ScalarFunction."""

    def __init__(self, backend):
        self.b = backend
        self.nfev = 1          # ScalarFunction evaluates f and g at x0 when it is built
        self.ngev = 1
        self.last_grad_alpha = None

    def phi(self, alpha):
        f, _, nf, ng = self.b.trial(alpha, False)
        self.nfev += nf
        self.ngev += ng
        return f

    def derphi(self, alpha):
        _, d, nf, ng = self.b.trial(alpha, True)
        self.nfev += nf
        self.ngev += ng
        self.last_grad_alpha = alpha
        return d


def _line_search_wolfe12(ev, derphi0, old_fval, old_old_fval, c1, c2, searches):
    """_line_search_wolfe12 (scipy/optimize/_optimize.py) for fmin_bfgs: wolfe1 with amin = 1e-100, amax = 1e100,
    then wolfe2 with only c1, c2 and amax.  -> (alpha, f(alpha), f(x), whether g(alpha) was evaluated last)."""
    wolfe1, wolfe2, LineSearchWarning, _ = searches
    ev.last_grad_alpha = None
    stp, fval, old = wolfe1(ev.phi, ev.derphi, old_fval, old_old_fval, derphi0,
                            c1=c1, c2=c2, amax=1e100, amin=1e-100, xtol=1e-14)
    if stp is not None:
        return stp, fval, old, True
    ev.last_grad_alpha = None
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', LineSearchWarning)
        alpha, phi_star, old, derphi_star = wolfe2(ev.phi, ev.derphi, old_fval, old_old_fval, derphi0,
                                                   c1, c2, 1e100, None, maxiter=10)
    if alpha is None:
        raise _LineSearchError()
    return alpha, phi_star, old, derphi_star is not None


def minimize(backend, n, gtol=1e-5, norm=np.inf, maxiter=None, c1=1e-4, c2=0.9, xrtol=0, disp=False):
    """scipy's BFGS loop on `backend` (n variables).  -> BfgsResult.  Stopping order as scipy: the gtol test, the xrtol
    test, a non-finite f, and only after those the update."""
    searches = _scalar_searches()
    if not (norm == np.inf or norm == 2):
        raise ValueError("norm must be numpy.inf or 2, got %r" % (norm,))
    if maxiter is None:
        maxiter = n * 200
    f0, gnorm, gnorm2, derphi0 = backend.begin(norm)
    ev = _Counted(backend)
    old_fval = f0
    old_old_fval = old_fval + gnorm2 / 2          # sets the initial step guess to dx ~ 1
    k = 0
    warnflag = 0
    xnorm = 0.0
    while (gnorm > gtol) and (k < maxiter):
        try:
            alpha_k, fval, old, have_grad = _line_search_wolfe12(ev, derphi0, old_fval, old_old_fval, c1, c2, searches)
        except _LineSearchError:
            warnflag = 2
            break
        if not have_grad:                          # scipy: gfkp1 = myfprime(xkp1)
            ev.derphi(alpha_k)
        old_fval, old_old_fval = fval, old
        gnorm, pnorm, xnorm = backend.accept(alpha_k, norm)
        k += 1
        if gnorm <= gtol:
            break
        if alpha_k * pnorm <= xrtol * (xrtol + xnorm):
            break
        if not np.isfinite(old_fval):
            warnflag = 2
            break
        derphi0, fallback = backend.update()
        if fallback and disp:
            warnings.warn("Divide-by-zero encountered: rhok assumed large", searches[3], stacklevel=2)
    fval = old_fval
    if warnflag == 2:
        pass
    elif k >= maxiter:
        warnflag = 1
    elif np.isnan(gnorm) or np.isnan(fval) or backend.x_has_nan():
        warnflag = 3
    res = BfgsResult(fval, k, ev.nfev, ev.ngev, warnflag)
    if disp:
        if warnflag == 0:
            print(res.message)
        else:
            warnings.warn(res.message, searches[3], stacklevel=2)
        print("         Current function value: %f" % fval)
        print("         Iterations: %d" % k)
        print("         Function evaluations: %d" % res.func_calls)
        print("         Gradient evaluations: %d" % res.grad_calls)
    return res


def _vecnorm(x, ord=2):
    if ord == np.inf:
        return np.amax(np.abs(x))
    return np.sum(np.abs(x) ** ord, axis=0) ** (1.0 / ord)


class NumpyBackend(object):
    """scipy's vector work with numpy, in scipy's order (the dense triple-product update included): the CPU oracle of
    the driver.  `fun(x, *args)` -> f, `grad(x, *args)` -> gradient, called on copies of x as ScalarFunction does."""

    def __init__(self, fun, grad, x0, args=()):
        x0 = np.asarray(x0).flatten()
        if x0.ndim == 0:
            x0.shape = (1,)
        if not np.issubdtype(x0.dtype, np.floating):
            x0 = x0.astype(np.float64)
        self.fun, self.grad, self.args = fun, grad, tuple(args)
        self.xk = x0
        self.n = x0.size

    def _f(self, x):
        fx = self.fun(np.copy(x), *self.args)
        if not np.isscalar(fx):
            fx = np.asarray(fx).item()
        return fx

    def _g(self, x):
        return np.atleast_1d(self.grad(np.copy(x), *self.args))

    def _point(self, x):            # ScalarFunction's one-deep memo
        if not np.array_equal(x, self._mx):
            self._mx = x.astype(np.float64)
            self._fup = self._gup = False

    def begin(self, norm):
        self._mx = self.xk.astype(np.float64)
        self._fval = self._f(self._mx)
        self._gval = self._g(self._mx)
        self._fup = self._gup = True
        self.gfk = self._gval
        self.I = np.eye(self.n, dtype=int)
        self.Hk = self.I
        self.pk = -np.dot(self.Hk, self.gfk)
        return self._fval, _vecnorm(self.gfk, ord=norm), np.linalg.norm(self.gfk), np.dot(self.gfk, self.pk)

    def trial(self, alpha, need_grad):
        self._point(self.xk + alpha * self.pk)
        nf = ng = 0
        if need_grad:
            if not self._gup:
                self._gval = self._g(self._mx)
                self._gup = True
                ng = 1
            self._glast = self._gval          # line_search_wolfe1/2: gval[0]
            return None, np.dot(self._glast, self.pk), nf, ng
        if not self._fup:
            self._fval = self._f(self._mx)
            self._fup = True
            nf = 1
        return self._fval, None, nf, ng

    def accept(self, alpha, norm):
        self.sk = alpha * self.pk
        self.xk = self.xk + self.sk
        self.yk = self._glast - self.gfk
        self.gfk = self._glast
        return _vecnorm(self.gfk, ord=norm), _vecnorm(self.pk), _vecnorm(self.xk)

    def update(self):
        sk, yk, I = self.sk, self.yk, self.I
        rhok_inv = np.dot(yk, sk)
        fallback = rhok_inv == 0.
        rhok = 1000.0 if fallback else 1. / rhok_inv
        A1 = I - sk[:, np.newaxis] * yk[np.newaxis, :] * rhok
        A2 = I - yk[:, np.newaxis] * sk[np.newaxis, :] * rhok
        self.Hk = np.dot(A1, np.dot(self.Hk, A2)) + (rhok * sk[:, np.newaxis] * sk[np.newaxis, :])
        self.pk = -np.dot(self.Hk, self.gfk)
        return np.dot(self.gfk, self.pk), fallback

    def x_has_nan(self):
        return bool(np.isnan(self.xk).any())

    def finish(self):
        return self.xk, self.gfk, self.Hk


def fmin_bfgs_numpy(f, x0, fprime, args=(), gtol=1e-5, norm=np.inf, maxiter=None, disp=False, xrtol=0, c1=1e-4,
                    c2=0.9):
    """The driver on NumpyBackend, returned as scipy.optimize.fmin_bfgs(..., full_output=True) does:
    (xopt, fopt, gopt, Bopt, func_calls, grad_calls, warnflag)."""
    b = NumpyBackend(f, fprime, x0, args)
    r = minimize(b, b.n, gtol=gtol, norm=norm, maxiter=maxiter, c1=c1, c2=c2, xrtol=xrtol, disp=disp)
    x, g, H = b.finish()
    return x, r.fmin, g, H, r.func_calls, r.grad_calls, r.warnflag


class DeviceBackend(object):
    """The session of include/bioen_hip.h (bioen_hip_bfgs_logw_*) on a log-weights Context: the point, the gradient,
    the direction, the step pairs and H in HBM.  trial() counts as ScalarFunction would on the same sequence of calls
    (its memo is the last trial step of the current direction)."""

    def __init__(self, ctx, g0, G, theta):
        self.ctx = ctx
        self.g0, self.G, self.theta = g0, G, float(theta)
        self._alpha = None

    def begin(self, norm):
        self._norm_inf = norm == np.inf
        self._alpha = None
        return self.ctx.bfgs_begin(self.g0, self.G, self.theta, self._norm_inf)

    def trial(self, alpha, need_grad):
        alpha = float(alpha)
        if alpha != self._alpha:
            self._alpha, self._fcount, self._gcount = alpha, False, False
        f, d = self.ctx.bfgs_trial(alpha, need_grad)
        nf = ng = 0
        if need_grad:
            ng = 0 if self._gcount else 1
            self._gcount = True
            return None, d, nf, ng
        nf = 0 if self._fcount else 1
        self._fcount = True
        return f, None, nf, ng

    def accept(self, alpha, norm):
        r = self.ctx.bfgs_accept(float(alpha), self._norm_inf)
        self._xnorm = r[2]
        self._alpha = None
        return r

    def update(self):
        self._alpha = None
        return self.ctx.bfgs_update()

    def x_has_nan(self):
        return bool(np.isnan(getattr(self, "_xnorm", 0.0)))

    def finish(self):
        return self.ctx.bfgs_end()

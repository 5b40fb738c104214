"""Drop-in replacement for the reference's Cython module ``bioen.optimize.ext.c_bioen``
(``bioen/optimize/ext/c_bioen.pyx``): same 14 Python-callable names, same
arguments, same return values and the same exception texts -- but every
numerical call goes through ``libbioen_hip.so`` (hand-written gfx950 kernels)
via ctypes.  There is no CPU path in here; a missing library or GPU raises.

Differences from the reference, on purpose:
* ``yTilde`` is uploaded once and kept resident in HBM.  Calls that pass the same
  matrix again (scipy's separate f / f' callbacks, a theta series) reuse the
  device copy instead of re-uploading -- see ``_context_for`` -- as long as the WHOLE host
  buffer can be re-checked for in-place edits (up to 256 MB); larger matrices are uploaded
  afresh by every call of THIS module that is not inside a hold (the reference hands a pointer over and
  pays no upload: c_bioen.pyx:463-478), unless ``BIOEN_HIP_CACHE_LARGE=1`` opts into a sampled check.
  ``hold`` (= ``bioen_amd.optimize.resident``) pins one device copy for a block of calls: the library's
  ``find_optimum*`` hold the matrix for the duration of a call (ONE upload per call at any size), a caller
  looping over theta wraps its loop.
* ``caching`` / ``cache_ytilde_transposed`` are accepted and ignored: both matrix passes stream
  strip-major copies of the matrix built on the device (``csrc/kernels_strip_copy.hip``, ``csrc/strip.hpp``); no host-side
  transposed copy exists.
* ``bioen_log_posterior_logw`` uses its ``G`` argument.  The reference passes the
  *initial* log-weights ``g`` in the ``G`` slot (c_bioen.pyx:279), which is
  invisible in its tests because every fixture has ``GInit == G``.
* GSL is not linked.  ``bioen_opt_bfgs_logw`` / ``bioen_opt_bfgs_forces`` run the library's own
  restatement of the five GSL 2.5 multimin algorithms the reference selects from
  (``bioen_amd/csrc/multimin.hpp``) on the device objective, so ``library_gsl()`` is True and
  ``minimizer: gsl`` configurations keep working; iterates agree with a GSL build to rounding,
  not bit for bit.
"""
import os
import weakref
from collections import OrderedDict

import numpy as np

from ... import _lib

# --- GSL / liblbfgs status conventions of the reference (c_bioen.pyx:104-120) ---
gsl_continue = -2
gsl_enoprog = 27
gsl_success = [gsl_continue, gsl_enoprog, 0]
lbfgs_success = [0, 1, 2]

gsl_continue_msg = "Note: GSL might require more iterations, please check the parameters of the minimizer."


# ------------------------------------------------------------------------------------
# device-context cache
# ------------------------------------------------------------------------------------
_CACHE = OrderedDict()
_CACHE_MAX = int(os.environ.get("BIOEN_HIP_CACHE", "2"))


_FULL_CHECK_BYTES = int(os.environ.get("BIOEN_HIP_CACHE_FULLCHECK_MB", "256")) << 20


def _cache_large():
    return os.environ.get("BIOEN_HIP_CACHE_LARGE", "0") == "1"


try:                                   # byte-exact and 7 GB/s here; the fallback (zlib) is byte-exact too, at 1-3 GB/s
    import xxhash as _xxhash
except ImportError:                    # pragma: no cover - the image has it
    _xxhash = None
import zlib as _zlib


def _digest(buf):
    mv = memoryview(buf).cast("B")
    if _xxhash is not None:
        return _xxhash.xxh3_64_intdigest(mv)
    return (_zlib.adler32(mv), _zlib.crc32(mv))


def _fingerprint(a):
    """Content check of the host matrix: a hash of its BYTES.  Up to BIOEN_HIP_CACHE_FULLCHECK_MB (default 256 MB)
    every byte enters (xxh3-64: 37 ms per 256 MB here, against the upload and the two strip copies it saves) -- any
    in-place edit is seen, however small (a finite-difference perturbation below the rounding of a sum over the
    buffer) and however symmetric (two structures swapped: sums over the buffer do not move; until r04 the check WAS
    such sums).  Beyond that size a complete check costs more than the upload it would save (8 GB: ~1.2 s against
    0.15-0.26 s), so such matrices are NOT cached at all (`_context_for`) -- unless the caller opts in with
    BIOEN_HIP_CACHE_LARGE=1 and thereby promises not to edit the matrix in place: then a strided sample of ~4 M
    elements spread over all rows and columns is all that is hashed."""
    flat = a.reshape(-1)
    if flat.nbytes > _FULL_CHECK_BYTES:
        stride = max(1, flat.size // (1 << 22)) | 1          # odd: walks through every column residue
        flat = np.ascontiguousarray(flat[::stride])
    return (a.shape, _digest(flat))


# Holds (r05).  One `find_optimum` makes three or four calls of this module on the same matrix (the initial objective, the
# optimisation, the averages of the optimum), and a caller like bioen/analyze/procedure.py:62-77 repeats that for every
# theta.  A HELD matrix is served from one device context for as long as the hold lasts -- no upload, and no hashing of
# the host buffer either (the holder vouches for it: the library's own `find_optimum*` hold the matrix for the duration
# of the call, in which nobody else can edit it; a caller's `with optimize.resident(yTilde):` around its theta loop
# promises not to edit the matrix in place inside the block).  Matrices of any size, including those above the 256 MB
# the cache refuses.
_HELD = {}                             # id(host object) -> [object, context, cached, depth]
uploads = 0                            # device contexts created by this module so far (= uploads of a matrix): tests, bench.py


def _new_context(yT, YT):
    global uploads
    uploads += 1
    return _lib.Context(yT, YT)


class hold(object):
    """``with hold(yTilde, YTilde):`` -- every call of this module on THIS matrix object inside the block is served by one
    resident device copy: at most one upload, no per-call hashing.  Nestable; the targets YTilde may change from call to
    call (they are re-sent, M doubles).  Exported as ``bioen_amd.optimize.resident``."""

    def __init__(self, yTilde, YTilde=None):
        self.obj, self.YT = yTilde, YTilde

    def __enter__(self):
        e = _HELD.get(id(self.obj))
        if e is not None and e[0] is self.obj:
            e[3] += 1
            return self
        YT = self.YT if self.YT is not None else np.zeros(np.shape(self.obj)[0])
        ctx, cached = _context_for(self.obj, YT)
        if not hasattr(ctx, "_YT_host"):
            ctx._YT_host = _lib.as_f64(YT).ravel().copy()
        if cached:
            # the hold OWNS the context while it lasts (r06): out of the LRU cache, so that calls on other matrices
            # inside the block -- or clear_cache() -- cannot evict and close the copy the block is served from
            _CACHE.pop(id(self.obj), None)
        _HELD[id(self.obj)] = [self.obj, ctx, cached, 1]
        return self

    def __exit__(self, *exc):
        e = _HELD.get(id(self.obj))
        if e is None or e[0] is not self.obj:
            return False
        e[3] -= 1
        if e[3] == 0:
            del _HELD[id(self.obj)]
            if e[2] and _CACHE_MAX > 0 and getattr(e[1], "_h", None):
                _cache_insert(id(self.obj), e[1])        # back under the cache's rules (checked again on its next use)
            else:
                e[1].close()
        return False


def _cache_insert(key, ctx):
    stale = _CACHE.pop(key, None)
    if stale is not None and stale is not ctx:
        stale.close()
    _CACHE[key] = ctx
    while len(_CACHE) > _CACHE_MAX:
        _, old = _CACHE.popitem(last=False)
        old.close()


def _context_for(yTilde, YTilde):
    """Return a device context holding yTilde, creating/uploading it if needed.

    A cached context is reused only for the VERY SAME live host object (identity through a weak
    reference -- a new array that happens to land on a freed address never matches) whose content check
    still agrees (`_fingerprint`: a hash of every byte, so in-place edits -- finite-difference perturbations,
    reordered structures -- are seen).  Anything else is a miss and uploads afresh, which is what the reference does on every call
    (c_bioen.pyx:463-478).  Matrices above 256 MB (BIOEN_HIP_CACHE_FULLCHECK_MB) are never cached -- a
    complete check would cost more than the upload -- unless BIOEN_HIP_CACHE_LARGE=1 opts into a sampled
    check.  BIOEN_HIP_CACHE=0 switches the cache off."""
    held = _HELD.get(id(yTilde))
    if held is not None and held[0] is yTilde:             # held (above): the resident copy, unchecked
        ctx = held[1]
        YT = _lib.as_f64(YTilde).ravel()
        if not np.array_equal(ctx._YT_host, YT):
            ctx.set_target(YT)
            ctx._YT_host = YT.copy()
        return ctx, True
    yT = _lib.as_f64(yTilde)
    if yT.ndim != 2:
        raise ValueError("yTilde must be a 2-D (M x N) array")
    YT = _lib.as_f64(YTilde).ravel()
    weakable = isinstance(yTilde, np.ndarray)              # np.matrix included; lists etc. are never cached
    if _CACHE_MAX <= 0 or not weakable or (yT.nbytes > _FULL_CHECK_BYTES and not _cache_large()):
        return _new_context(yT, YT), False
    key = id(yTilde)
    fp = _fingerprint(yT)
    ctx = _CACHE.get(key)
    if ctx is not None:
        if ctx._host_ref() is yTilde and ctx._fingerprint == fp:
            _CACHE.move_to_end(key)
            if not np.array_equal(ctx._YT_host, YT):
                ctx.set_target(YT)
                ctx._YT_host = YT.copy()
            return ctx, True
        _CACHE.pop(key).close()                            # same id, other object or other content: stale
    ctx = _new_context(yT, YT)
    ctx._YT_host = YT.copy()
    ctx._fingerprint = fp
    ctx._host_ref = weakref.ref(yTilde)
    _cache_insert(key, ctx)
    return ctx, True


def clear_cache():
    """Free every cached device context (and the HBM copies of yTilde they hold)."""
    while _CACHE:
        _, ctx = _CACHE.popitem()
        ctx.close()


def _release(ctx, cached):
    if not cached:
        ctx.close()


# ------------------------------------------------------------------------------------
# flags / capabilities  (c_bioen.pyx:176-243)
# ------------------------------------------------------------------------------------
def set_fast_openmp_flag(flag):
    _lib.lib().bioen_hip_set_fast_openmp_flag(int(flag))


def get_fast_openmp_flag():
    return _lib.lib().bioen_hip_get_fast_openmp_flag()


def omp_set_num_threads(i):
    """Kept for API compatibility; the device grid is not an OpenMP team."""
    return None


def get_gsl_method(algorithm):
    names = {"conjugate_fr": 0, "gsl_multimin_fdfminimizer_conjugate_fr": 0,
             "conjugate_pr": 1, "gsl_multimin_fdfminimizer_conjugate_pr": 1,
             "bfgs2": 2, "gsl_multimin_fdfminimizer_vector_bfgs2": 2,
             "bfgs": 3, "gsl_multimin_fdfminimizer_vector_bfgs": 3,
             "steepest_descent": 4, "gsl_multimin_fdfminimizer_steepest_descent": 4}
    if algorithm in names:
        return names[algorithm]
    raise RuntimeError("{}, GSL return code: {}:{}".format(
        "get_gsl_method", -1, ' The algorithm ' + str(algorithm) + ' is not available.'))


def library_gsl():
    """True: the five GSL minimizers are part of the device library (restated, GSL itself is not linked)."""
    return True


def library_lbfgs():
    return True


# ------------------------------------------------------------------------------------
# log-weights  (c_bioen.pyx:246-520)
# ------------------------------------------------------------------------------------
def bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, theta, caching=False):
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        f, _ = ctx.logw_fdf(gPrime, G, theta, need_grad=False)
    finally:
        _release(ctx, cached)
    return f


def grad_bioen_log_posterior_logw(gPrime, g, G, yTilde, YTilde, theta, caching=False, print_timing=False):
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        _, grad = ctx.logw_fdf(gPrime, G, theta, need_f=False)
    finally:
        _release(ctx, cached)
    return grad


def hessp_bioen_log_posterior_logw(gPrime, p, g, G, yTilde, YTilde, theta, caching=False):
    """H(gPrime) p of the log-weights objective on the device (Context.logw_hessp: the point is set by this call)"""
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        hv, _, _ = ctx.logw_hessp(np.asarray(p, dtype=np.float64).reshape(-1), g=gPrime, G=G, theta=theta)
    finally:
        _release(ctx, cached)
    return hv


def _gsl_finish(func, info):
    """c_bioen.pyx:432-438: {0, GSL_CONTINUE, GSL_ENOPROG} count as success"""
    if info.lbfgs_code in gsl_success:
        if info.lbfgs_code == gsl_continue:
            print(gsl_continue_msg)
        return
    msg = _lib.lib().bioen_hip_gsl_strerror(int(info.lbfgs_code)).decode()
    raise RuntimeError("{}, GSL return code: {}:{}".format(func, info.lbfgs_code, msg))


def bioen_opt_bfgs_logw(g, G, yTilde, YTilde, theta, params):
    """-> (gopt[n], fmin) with params["algorithm"] in {conjugate_fr, conjugate_pr, bfgs2, bfgs,
    steepest_descent} and params["params"] = {step_size, tol, max_iterations} (c_bioen.pyx:341-438)."""
    global last_opt_info
    alg = get_gsl_method(params["algorithm"])      # same "unknown algorithm" error as the reference
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        res, w, info = ctx.opt_gsl_logw(g, G, theta, alg, params["params"], verbose=params.get("verbose", False),
                                        debug=params.get("debug", False), want_weights=False)
    finally:
        _release(ctx, cached)
    last_opt_info = info
    _gsl_finish("bioen_opt_bfgs_logw", info)
    return res, info.fmin


def _raise_lbfgs(func, code):
    msg = _lib.lib().bioen_hip_lbfgs_strerror(int(code)).decode()
    raise RuntimeError("{}, liblbfgs return code: {}:{}".format(func, code, msg))


last_opt_info = None   # OptResult of the most recent L-BFGS run (iterations, evaluations, seconds, ...)


def bioen_opt_lbfgs_logw(g, G, yTilde, YTilde, theta, params):
    """-> (gopt[n], fmin).  Raises RuntimeError('..., liblbfgs return code: n:msg')
    unless the status is 0, 1 or 2 (c_bioen.pyx:516-520)."""
    global last_opt_info
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        res, w, info = ctx.opt_lbfgs_logw(g, G, theta, params["params"], verbose=params.get("verbose", False),
                                          debug=params.get("debug", False), want_weights=False)
    finally:
        _release(ctx, cached)
    last_opt_info = info
    if info.lbfgs_code not in lbfgs_success:
        _raise_lbfgs("bioen_opt_lbfgs_logw", info.lbfgs_code)
    return res, info.fmin


def bioen_opt_lbfgs_logw_series(g, G, yTilde, YTilde, thetas, params):
    """Not in the reference: a cold-started theta series (the loop of bioen/analyze/procedure.py:62-67)
    as ONE call -- up to 8 thetas share every pass over the resident matrix, each result bitwise what
    bioen_opt_lbfgs_logw returns for that theta.  -> ([gopt[n]] * ntheta, [fmin] * ntheta)"""
    global last_opt_info
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        res, w, infos = ctx.opt_lbfgs_logw_batch(thetas, g, G, params["params"], verbose=params.get("verbose", False),
                                                 debug=params.get("debug", False), want_weights=False)
    finally:
        _release(ctx, cached)
    last_opt_info = infos
    for info in infos:
        if info.lbfgs_code not in lbfgs_success:
            _raise_lbfgs("bioen_opt_lbfgs_logw_series", info.lbfgs_code)
    return [res[k] for k in range(len(infos))], [info.fmin for info in infos]


# ------------------------------------------------------------------------------------
# forces  (c_bioen.pyx:523-792)
# ------------------------------------------------------------------------------------
def bioen_log_posterior_forces(forces, w0, yTilde, YTilde, theta, caching=False):
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        f, _ = ctx.forces_fdf(forces, w0, theta, need_grad=False)
    finally:
        _release(ctx, cached)
    return f


def grad_bioen_log_posterior_forces(forces, w0, yTilde, YTilde, theta, caching=False):
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        _, grad = ctx.forces_fdf(forces, w0, theta, need_f=False)
    finally:
        _release(ctx, cached)
    return grad


def hessp_bioen_log_posterior_forces(forces, p, w0, yTilde, YTilde, theta, caching=False):
    """H(forces) p on the device (not in the reference: c_bioen.pyx has first-order entries only); p (m,) or (k <= 8, m)"""
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        hv, _, _ = ctx.forces_hessp(p, forces=forces, w0=w0, theta=theta)
    finally:
        _release(ctx, cached)
    return hv


def hessian_bioen_log_posterior_forces(forces, w0, yTilde, YTilde, theta, caching=False):
    """the dense Hessian (m, m) on the device: ceil(m / 8) batched products at one kept point"""
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        H, _, _ = ctx.forces_hessian(forces=forces, w0=w0, theta=theta)
    finally:
        _release(ctx, cached)
    return H


def bioen_opt_bfgs_forces(forces, w0, yTilde, YTilde, theta, params):
    """-> (forces_opt[m], fmin); c_bioen.pyx:620-716"""
    global last_opt_info
    alg = get_gsl_method(params["algorithm"])
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        res, w, info = ctx.opt_gsl_forces(forces, w0, theta, alg, params["params"],
                                          verbose=params.get("verbose", False), debug=params.get("debug", False),
                                          want_weights=False)
    finally:
        _release(ctx, cached)
    last_opt_info = info
    _gsl_finish("bioen_opt_bfgs_forces", info)
    return res, info.fmin


def bioen_opt_lbfgs_forces(forces, w0, yTilde, YTilde, theta, params):
    """-> (forces_opt[m], fmin); same error convention as bioen_opt_lbfgs_logw."""
    global last_opt_info
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        res, w, info = ctx.opt_lbfgs_forces(forces, w0, theta, params["params"],
                                            verbose=params.get("verbose", False),
                                            debug=params.get("debug", False), want_weights=False)
    finally:
        _release(ctx, cached)
    last_opt_info = info
    if info.lbfgs_code not in lbfgs_success:
        _raise_lbfgs("bioen_opt_lbfgs_forces", info.lbfgs_code)
    return res, info.fmin


class _dense_panels(object):
    """``with _dense_panels(ctx):`` -- the dual Newton calls of this module beyond 1024 observables: the context's switch
    (Context.set_dense_panels) is on inside the block and back as it was afterwards, so a context a caller holds
    (``optimize.resident``) is left as the caller set it.  M <= 1024 needs no switch and none is touched."""

    def __init__(self, ctx):
        self.ctx, self.was = ctx, None

    def __enter__(self):
        if self.ctx.m > 1024 and not self.ctx.dense_panels:
            self.was = False
            self.ctx.set_dense_panels(True)
        return self.ctx

    def __exit__(self, *exc):
        if self.was is not None and getattr(self.ctx, "_h", None):
            self.ctx.set_dense_panels(self.was)
        return False


def bioen_opt_dual_newton_logw(g, G, yTilde, YTilde, theta, params):
    """-> (gopt[n], fmin): the device-resident dual Newton minimizer of the log-weights method
    (Context.opt_dual_newton_logw).  Status 0 returns; every other status raises RuntimeError with the return code, as
    the other device minimizers do.  last_opt_info: the result dict."""
    global last_opt_info
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        with _dense_panels(ctx):
            res = ctx.opt_dual_newton_logw(np.asarray(g, dtype=np.float64).reshape(-1),
                                           np.asarray(G, dtype=np.float64).reshape(-1), theta, params["params"])
    finally:
        _release(ctx, cached)
    last_opt_info = res
    if res["status"] != 0:
        raise RuntimeError("bioen_opt_dual_newton_logw: return code %d after %d iterations, max|grad| = %.3g, max w = %.3g"
                           % (res["status"], res["iterations"], res["gmax"], res["wmax"]))
    return res["g"], res["fmin"]


def bioen_opt_dual_newton_logw_series(g, G, yTilde, YTilde, thetas, params):
    """-> ([gopt[n]] * ntheta, [fmin] * ntheta): the dual Newton minimizer for a theta series in one device call
    (Context.opt_dual_newton_logw_series), in the order given; warm-started unless params["params"]["series"] is "cold".
    Every theta runs; then the first status != 0 raises RuntimeError naming its theta, as bioen_opt_dual_newton_logw does.
    last_opt_info: the list of result dicts."""
    global last_opt_info
    p = dict(params["params"])
    mode = str(p.pop("series", "warm")).lower()
    if mode not in ("warm", "cold"):
        raise RuntimeError("dual_newton:series=" + mode + " not recognized (valid values = 'warm', 'cold')")
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        with _dense_panels(ctx):
            res = ctx.opt_dual_newton_logw_series([float(t) for t in thetas], np.asarray(g, dtype=np.float64).reshape(-1),
                                                  np.asarray(G, dtype=np.float64).reshape(-1), p, warm=(mode == "warm"))
    finally:
        _release(ctx, cached)
    last_opt_info = res
    for t, r in zip(thetas, res):
        if r["status"] != 0:
            raise RuntimeError("bioen_opt_dual_newton_logw_series: theta = %r: return code %d after %d iterations, "
                               "max|grad| = %.3g, max w = %.3g" % (float(t), r["status"], r["iterations"], r["gmax"], r["wmax"]))
    return [r["g"] for r in res], [r["fmin"] for r in res]


def laplace_logw(g, G, yTilde, YTilde, theta, observables=None, matrices=True):
    """-> (Context.logw_laplace's dict at the point (g, G, theta), C or None): the Laplace error bars of the log-weights
    method formed on the device; with `matrices` the covariance of the observables comes from logw_cov at the
    point the call has kept.  info != 0 is the caller's to judge (log_weights.laplace_error_bars raises ValueError)."""
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        r = ctx.logw_laplace(g=np.asarray(g, dtype=np.float64).reshape(-1), G=np.asarray(G, dtype=np.float64).reshape(-1),
                             theta=theta, observables=observables, matrices=matrices)
        C = ctx.logw_cov() if matrices and r["info"] == 0 else None
    finally:
        _release(ctx, cached)
    return r, C


def bioen_opt_newton_forces(forces, w0, yTilde, YTilde, theta, params):
    """-> (forces_opt[m], fmin): the device-resident Newton minimizer (Context.opt_newton_forces).  Status 0 (max|g| <=
    gtol) and 2 (at the minimum to the rounding of f) return; 1 (max_iterations) and 3 (the damping left its range) raise
    RuntimeError with the return code, as the other device minimizers do.  last_opt_info: the result dict."""
    global last_opt_info
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        res = ctx.opt_newton_forces(forces, w0, theta, params["params"], want_weights=False)
    finally:
        _release(ctx, cached)
    last_opt_info = res
    if res["status"] not in (0, 2):
        raise RuntimeError("bioen_opt_newton_forces: return code %d (%s) after %d iterations, max|g| = %.3g"
                           % (res["status"], {1: "max_iterations reached", 3: "the damping left its range"}.get(
                               res["status"], "?"), res["iterations"], res["gmax"]))
    return res["forces"], res["fmin"]


# helpers the Python layer uses to keep post-processing on the device ------------------
def get_weights_logw(g, yTilde, YTilde):
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        w, _ = ctx.logw_weights(g)
    finally:
        _release(ctx, cached)
    return w


def get_ave(w, yTilde, YTilde):
    """yTilde . w as an (M,) array, from the device-resident matrix (_getAve,
    c_bioen_kernels_forces.c:93-109)."""
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        _, yave = ctx.chi_squared(w)
    finally:
        _release(ctx, cached)
    return yave


def chi2_and_kl_forces(forces, w0, yTilde, YTilde):
    """(w, chi2 = 0.5|yTilde w - YTilde|^2, KL(w||w0)) at `forces`, one device evaluation."""
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        w = ctx.forces_weights(forces, w0)
        chi2, _ = ctx.chi_squared(w)
    finally:
        _release(ctx, cached)
    return w, chi2


def get_weights_forces(forces, w0, yTilde, YTilde):
    ctx, cached = _context_for(yTilde, YTilde)
    try:
        w = ctx.forces_weights(forces, w0)
    finally:
        _release(ctx, cached)
    return w

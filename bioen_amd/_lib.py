"""ctypes loader for ``libbioen_hip.so`` (C ABI: ``include/bioen_hip.h``).

There is deliberately NO CPU fallback: if the HIP library is missing, or no
MI355X is visible, every compute entry point raises.  No torch, no numpy
compute -- this module only moves pointers.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BIOEN_HIP_LIBRARY: another build of the same library (diagnostic / A-B builds of tools/); never a fallback
LIB_PATH = os.environ.get("BIOEN_HIP_LIBRARY") or os.path.join(_HERE, "libbioen_hip.so")

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
ctx_p = C.c_void_p


class LbfgsConfig(C.Structure):
    # field order = reference lbfgs_config_params (c_bioen_common.h:69-79)
    _fields_ = [("linesearch", C.c_int), ("max_iterations", C.c_int),
                ("delta", C.c_double), ("epsilon", C.c_double),
                ("ftol", C.c_double), ("gtol", C.c_double),
                ("wolfe", C.c_double), ("past", C.c_int),
                ("max_linesearch", C.c_int)]


class GslConfig(C.Structure):
    # field order = reference gsl_config_params (c_bioen_common.h:62-67)
    _fields_ = [("step_size", C.c_double), ("tol", C.c_double), ("max_iterations", C.c_int),
                ("algorithm", C.c_int)]


class VisualParams(C.Structure):
    # reference visual_params (c_bioen_common.h:89-92)
    _fields_ = [("debug", C.c_size_t), ("verbose", C.c_size_t)]


class OptResult(C.Structure):
    _fields_ = [("fmin", C.c_double), ("chi2", C.c_double), ("kl", C.c_double),
                ("seconds", C.c_double), ("lbfgs_code", C.c_int), ("iterations", C.c_int),
                ("evaluations", C.c_int), ("reserved", C.c_int)]


class NewtonConfig(C.Structure):
    # bioen_newton_config (include/bioen_hip.h)
    _fields_ = [("gtol", C.c_double), ("armijo", C.c_double), ("rho_good", C.c_double), ("lambda_factor", C.c_double),
                ("lambda_first", C.c_double), ("lambda_max", C.c_double), ("lambda_zero", C.c_double),
                ("floor_ulps", C.c_double), ("max_iterations", C.c_int), ("hessian", C.c_int)]


class NewtonResult(C.Structure):
    # bioen_newton_result (include/bioen_hip.h)
    _fields_ = [("fmin", C.c_double), ("gmax", C.c_double), ("lam", C.c_double), ("status", C.c_int),
                ("iterations", C.c_int), ("evaluations", C.c_int), ("hessians", C.c_int), ("factorisations", C.c_int),
                ("switched", C.c_int)]


class LogwNewtonConfig(C.Structure):
    # bioen_logwn_config (include/bioen_hip.h)
    _fields_ = [("gtol", C.c_double), ("armijo", C.c_double), ("floor_ulps", C.c_double), ("max_iterations", C.c_int),
                ("max_halvings", C.c_int)]


class LogwNewtonResult(C.Structure):
    # bioen_logwn_result (include/bioen_hip.h)
    _fields_ = [("fmin", C.c_double), ("gmax", C.c_double), ("wmax", C.c_double), ("status", C.c_int),
                ("iterations", C.c_int), ("evaluations", C.c_int), ("factorisations", C.c_int)]


class LogwNewtonSeriesResult(C.Structure):
    # bioen_logwn_series_result (include/bioen_hip.h)
    _fields_ = [("fmin", C.c_double), ("gmax", C.c_double), ("wmax", C.c_double), ("status", C.c_int),
                ("iterations", C.c_int), ("evaluations", C.c_int), ("factorisations", C.c_int), ("bf16_passes", C.c_int),
                ("switched", C.c_int)]


# the dual Newton minimizer's constants (log_weights.dual_newton_bioen_log_posterior_base uses the same)
LOGW_NEWTON_DEFAULTS = dict(gtol=1e-6, max_iterations=200, armijo=1e-4, floor_ulps=8.0, max_halvings=60)
LOGW_NEWTON_SOURCES = ("gram", "gram_bf16")      # the covariance of the step: the FP64 pass | the split-BF16 one


# the Newton minimizer's damping constants (forces.newton_bioen_log_posterior_base uses the same)
NEWTON_DEFAULTS = dict(gtol=1e-6, max_iterations=200, hessian="gram", armijo=1e-4, rho_good=0.75, lambda_factor=4.0,
                       lambda_first=1e-10, lambda_max=1e10, lambda_zero=1e-12, floor_ulps=8.0)
NEWTON_SOURCES = ("gram", "gram_bf16")


class BioenHipError(RuntimeError):
    """Failure inside libbioen_hip (HIP runtime, allocation, bad argument)."""


# every symbol include/bioen_hip.h declares: name -> (restype, argtypes)
_SIGNATURES = {
    "bioen_hip_version": (C.c_char_p, []),
    "bioen_hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "bioen_hip_strerror": (C.c_char_p, [C.c_int]),
    "bioen_hip_last_error": (C.c_char_p, []),
    "bioen_hip_lbfgs_strerror": (C.c_char_p, [C.c_int]),
    "bioen_hip_set_fast_openmp_flag": (None, [C.c_int]),
    "bioen_hip_get_fast_openmp_flag": (C.c_int, []),
    "bioen_hip_ctx_create": (C.c_int, [C.c_int, C.c_int, dp, dp, C.c_int, C.POINTER(ctx_p)]),
    "bioen_hip_ctx_create_synthetic": (C.c_int, [C.c_int, C.c_int, dp, dp, dp, dp, C.c_ulonglong, C.c_int,
                                                 C.POINTER(ctx_p)]),
    "bioen_hip_ctx_create_sharded": (C.c_int, [C.c_int, C.c_longlong, dp, dp, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(ctx_p)]),
    "bioen_hip_ctx_create_synthetic_sharded": (C.c_int, [C.c_int, C.c_longlong, dp, dp, dp, dp, C.c_ulonglong,
                                                         C.c_int, C.c_int, C.c_int, C.POINTER(ctx_p)]),
    "bioen_hip_ctx_set_exchange_callback": (C.c_int, [ctx_p, C.c_void_p, C.c_void_p]),
    "bioen_hip_ctx_shard": (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong),
                                      C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "bioen_hip_ctx_set_force_exchange": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_ctx_set_mirror_exchange": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_exchange_counts": (C.c_int, [ctx_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "bioen_hip_ctx_destroy": (C.c_int, [ctx_p]),
    "bioen_hip_ctx_shape": (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bioen_hip_ctx_read_ytilde": (C.c_int, [ctx_p, C.c_int, C.c_int, C.c_int, C.c_int, dp]),
    "bioen_hip_ctx_footprint": (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "bioen_hip_ctx_set_ytilde_target": (C.c_int, [ctx_p, dp]),
    "bioen_hip_ctx_set_affine": (C.c_int, [ctx_p, dp, dp]),
    "bioen_hip_ctx_set_direction_mode": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_ctx_set_storage": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_ctx_set_dense_panels": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_ctx_set_one_copy": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_synchronize": (C.c_int, [ctx_p]),
    "bioen_hip_logw_weights": (C.c_int, [ctx_p, dp, dp, dp]),
    "bioen_hip_logw_fdf": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp]),
    "bioen_hip_logw_hessp": (C.c_int, [ctx_p, dp, dp, C.c_double, C.c_int, dp, dp, dp, dp]),
    "bioen_hip_opt_lbfgs_logw": (C.c_int, [ctx_p, dp, dp, C.c_double, C.POINTER(LbfgsConfig),
                                           C.POINTER(VisualParams), dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_opt_lbfgs_logw_batch": (C.c_int, [ctx_p, C.c_int, dp, dp, C.c_size_t, dp, C.POINTER(LbfgsConfig),
                                                 C.POINTER(VisualParams), C.c_int, dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_forces_weights": (C.c_int, [ctx_p, dp, dp, dp]),
    "bioen_hip_forces_fdf": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp]),
    "bioen_hip_forces_fdf_batch": (C.c_int, [ctx_p, C.c_int, dp, dp, dp, dp, dp]),
    "bioen_hip_opt_lbfgs_forces": (C.c_int, [ctx_p, dp, dp, C.c_double, C.POINTER(LbfgsConfig),
                                             C.POINTER(VisualParams), dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_opt_lbfgs_forces_batch": (C.c_int, [ctx_p, C.c_int, dp, dp, C.c_size_t, dp, C.POINTER(LbfgsConfig),
                                                   C.POINTER(VisualParams), C.c_int, dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_chi_squared": (C.c_int, [ctx_p, dp, dp, dp]),
    "bioen_hip_last_average": (C.c_int, [ctx_p, dp, dp]),
    "bioen_hip_kernel_stats": (C.c_int, [ctx_p, C.c_int, dp, C.POINTER(C.c_longlong)]),
    "bioen_hip_kernel_stats_ex": (C.c_int, [ctx_p, C.c_int, dp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "bioen_hip_kernel_stats_reset": (C.c_int, [ctx_p]),
    "bioen_hip_kernel_stats_enable": (C.c_int, [ctx_p, C.c_int]),
    "bioen_hip_speculation_stats": (C.c_int, [ctx_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "bioen_hip_debug_strip_stamps": (C.c_int, [ctx_p, C.c_int, C.POINTER(C.c_longlong), C.c_int]),
    "bioen_hip_ctx_layout": (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bioen_hip_ctx_strip_plan": (C.c_int, [ctx_p, C.c_int] + [C.POINTER(C.c_int)] * 6),
    "bioen_hip_debug_pass_probe": (C.c_int, [ctx_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bioen_hip_ctx_create_raw": (C.c_int, [C.c_int, C.c_longlong, C.c_int, dp, dp, dp, C.c_int, C.POINTER(ctx_p)]),
    "bioen_hip_gsl_strerror": (C.c_char_p, [C.c_int]),
    "bioen_hip_opt_gsl_logw": (C.c_int, [ctx_p, dp, dp, C.c_double, C.POINTER(GslConfig), C.POINTER(VisualParams),
                                         dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_opt_gsl_forces": (C.c_int, [ctx_p, dp, dp, C.c_double, C.POINTER(GslConfig), C.POINTER(VisualParams),
                                           dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_selftest_multimin": (C.c_int, [C.c_int, C.c_int, dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_multimin_host": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, dp, C.POINTER(GslConfig), dp,
                                          C.POINTER(OptResult)]),
    "bioen_hip_selftest_lbfgs": (C.c_int, [C.c_int, C.c_int, dp, C.POINTER(LbfgsConfig), dp, C.POINTER(OptResult)]),
    "bioen_hip_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "bioen_hip_comm_init": (C.c_int, [ctx_p, C.POINTER(C.c_ubyte), C.c_int, C.c_int]),
    "bioen_hip_comm_allgather": (C.c_int, [ctx_p, dp, C.c_size_t, dp]),
    "bioen_hip_comm_init_abandoned": (C.c_int, []),
    "bioen_hip_exchange_probe": (C.c_int, [ctx_p, C.c_size_t, C.c_int, dp]),
    "bioen_hip_read_probe": (C.c_int, [ctx_p, C.c_int, C.c_int, dp, C.POINTER(C.c_longlong)]),
    "bioen_hip_comm_destroy": (C.c_int, [ctx_p]),
    "bioen_hip_p2p_export": (C.c_int, [ctx_p, C.POINTER(C.c_ubyte)]),
    "bioen_hip_p2p_attach": (C.c_int, [ctx_p, C.POINTER(C.c_ubyte)]),
    "bioen_hip_p2p_detach": (C.c_int, [ctx_p]),
    "bioen_hip_exchange_transport": (C.c_int, [ctx_p]),
    "bioen_hip_exchange_selftest": (C.c_int, [ctx_p, C.c_int, C.POINTER(C.c_longlong)]),
    "bioen_hip_exchange_counts3": (C.c_int, [ctx_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                             C.POINTER(C.c_longlong)]),
    "bioen_hip_ctx_set_wait_timeout": (C.c_int, [ctx_p, C.c_double]),
    "bioen_hip_bfgs_logw_begin": (C.c_int, [ctx_p, dp, dp, C.c_double, C.c_int, dp, dp, dp, dp]),
    "bioen_hip_bfgs_logw_trial": (C.c_int, [ctx_p, C.c_double, C.c_int, dp, dp]),
    "bioen_hip_bfgs_logw_accept": (C.c_int, [ctx_p, C.c_double, C.c_int, dp, dp, dp]),
    "bioen_hip_bfgs_logw_update": (C.c_int, [ctx_p, dp, C.POINTER(C.c_int)]),
    "bioen_hip_bfgs_logw_end": (C.c_int, [ctx_p, dp, dp, C.POINTER(OptResult)]),
    "bioen_hip_bfgs_logw_read_hinv": (C.c_int, [ctx_p, C.c_int, C.c_int, C.c_int, dp]),
    "bioen_hip_bfgs_logw_read_vec": (C.c_int, [ctx_p, C.c_int, dp]),
    # forces method: Hessian-vector products
    "bioen_hip_forces_hessp": (C.c_int, [ctx_p, dp, dp, C.c_double, C.c_int, dp, dp, dp, dp]),
    # forces method: the dense Hessian and the covariance in one pass
    "bioen_hip_forces_gram": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp, dp, dp]),
    # forces method: one quadratic form per structure at a kept forces point
    "bioen_hip_forces_colquad": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp, dp, dp]),
    # forces method: the Hessian for a Newton minimizer from split-BF16 operands
    "bioen_hip_forces_gram_bf16": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp, dp, dp]),
    # forces method: the device-resident Newton minimizer, its Cholesky factorisation and solves
    "bioen_hip_forces_newton_factor": (C.c_int, [ctx_p, dp, C.c_int, C.c_double, dp, C.POINTER(C.c_int)]),
    "bioen_hip_forces_newton_solve": (C.c_int, [ctx_p, C.c_int, dp, dp]),
    "bioen_hip_opt_newton_forces": (C.c_int, [ctx_p, dp, dp, C.c_double, C.POINTER(NewtonConfig), dp, dp,
                                              C.POINTER(NewtonResult)]),
    # forces method: the Laplace error bars without leaving the device
    "bioen_laplace_forces_inverse": (C.c_int, [ctx_p, dp, dp, dp, ip]),
    "bioen_laplace_forces": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp, dp, dp, dp, dp, dp, ip, dp, dp]),
    # log-weights method: the dual Newton minimizer and the covariance it is built on
    "bioen_logwn_cov": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp, dp]),
    "bioen_logwn_opt": (C.c_int, [ctx_p, dp, dp, C.c_double, C.POINTER(LogwNewtonConfig), dp, C.POINTER(LogwNewtonResult)]),
    "bioen_logwn_cov_bf16": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, dp, dp]),
    "bioen_logwn_series": (C.c_int, [ctx_p, dp, dp, dp, C.c_int, C.POINTER(LogwNewtonConfig), C.c_int, C.c_int, dp,
                                     C.POINTER(LogwNewtonSeriesResult)]),
    "bioen_logwn_profile_series": (C.c_int, [ctx_p, dp, dp, dp, C.c_int, C.POINTER(LogwNewtonConfig), C.c_int, C.c_int, dp, ip,
                                             C.c_int, dp, dp, dp, dp, C.POINTER(LogwNewtonSeriesResult)]),
    "bioen_logwn_laplace": (C.c_int, [ctx_p, dp, dp, C.c_double, dp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, dp, dp]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGNATURES)


def lib():
    """Load libbioen_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise BioenHipError(
                "bioen_amd: %s not found -- build it with `make -C bioen_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as e; e.build()'`). "
                "There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        L = lib()
        raise BioenHipError("libbioen_hip: %s (%d): %s" % (L.bioen_hip_strerror(rc).decode(), rc,
                                                          L.bioen_hip_last_error().decode()))


def leave_process(status=0):
    """End the process the safe way for a rank whose RCCL initialisation was abandoned at its time bound: a helper thread
    is then still blocked inside ncclCommInitRank, and normal interpreter teardown would run librccl's / HIP's static
    destructors under it (hang or crash at exit).  Flushes stdio and leaves through os._exit in that case; a plain
    sys.exit otherwise.  Never re-executes anything."""
    import sys
    abandoned = False
    try:
        abandoned = bool(_lib is not None and _lib.bioen_hip_comm_init_abandoned())
    except Exception:
        abandoned = False
    if abandoned:
        try:
            sys.stdout.flush()
            sys.stderr.flush()
        finally:
            os._exit(int(status))
    sys.exit(int(status))


def column_segments(n, world=1):
    """The canonical column segments of an n-structure problem on `world` ranks (csrc/ctx.hpp: XStage; api.hip:
    segment_geometry): -> (nseg, segcols, columns per rank).  nseg = 8 whenever world divides 8 -- every sum over
    structures then has ONE shape on 1, 2, 4 and 8 GPUs, and their results are bit-identical --, else world;
    segcols = ceil(n / nseg) rounded up to 128; a rank holds nseg / world consecutive segments."""
    nseg = 8 if (world <= 8 and 8 % world == 0) else world
    if world == 1 and os.environ.get("BIOEN_HIP_SEGMENTS") == "1":      # the single-GPU opt-out (api.hip: segment_geometry)
        nseg = 1
    segcols = (-(-n // nseg) + 127) // 128 * 128
    return nseg, segcols, segcols * (nseg // world)


def device_count():
    n = C.c_int(0)
    check(lib().bioen_hip_device_count(C.byref(n)))
    return n.value


def as_f64(x, shape=None):
    """float64, C-contiguous, np.matrix-safe view/copy of x (the reference's pyx reads
    `.data` unchecked, c_bioen.pyx:274-290; we normalise instead)."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a


def ptr(a):
    return a.ctypes.data_as(dp)


def newton_source(value):
    """the Newton minimizer's Hessian source, checked: "gram" | "gram_bf16" -> 0 | 1"""
    v = str(value).lower()
    if v not in NEWTON_SOURCES:
        raise RuntimeError("newton:hessian=" + v + " not recognized (valid values = 'gram', 'gram_bf16')")
    return NEWTON_SOURCES.index(v)


def logw_newton_source(value):
    """the dual Newton minimizer's covariance source, checked: "gram" | "gram_bf16" -> 0 | 1"""
    v = str(value).lower()
    if v not in LOGW_NEWTON_SOURCES:
        raise RuntimeError("dual_newton:hessian=" + v + " not recognized (valid values = 'gram', 'gram_bf16')")
    return LOGW_NEWTON_SOURCES.index(v)


def logw_newton_config(params):
    """params (a dict; missing keys take LOGW_NEWTON_DEFAULTS; "hessian" and "series" are not the struct's) -> LogwNewtonConfig"""
    p = dict(LOGW_NEWTON_DEFAULTS, **(params or {}))
    return LogwNewtonConfig(float(p["gtol"]), float(p["armijo"]), float(p["floor_ulps"]), int(p["max_iterations"]),
                            int(p["max_halvings"]))


def newton_config(params):
    """params (a dict; missing keys take NEWTON_DEFAULTS) -> NewtonConfig"""
    p = dict(NEWTON_DEFAULTS, **(params or {}))
    return NewtonConfig(float(p["gtol"]), float(p["armijo"]), float(p["rho_good"]), float(p["lambda_factor"]),
                        float(p["lambda_first"]), float(p["lambda_max"]), float(p["lambda_zero"]), float(p["floor_ulps"]),
                        int(p["max_iterations"]), newton_source(p["hessian"]))


def lbfgs_config(params):
    c = LbfgsConfig()
    for k in ("linesearch", "max_iterations", "past", "max_linesearch"):
        setattr(c, k, int(params[k]))
    for k in ("delta", "epsilon", "ftol", "gtol", "wolfe"):
        setattr(c, k, float(params[k]))
    return c


def selftest_lbfgs(kind, x0, params):
    """Run the library's L-BFGS driver on a built-in host objective (no GPU). -> (x, OptResult)"""
    x0 = as_f64(x0).ravel()
    cfg = lbfgs_config(params)
    out = np.empty_like(x0)
    info = OptResult()
    check(lib().bioen_hip_selftest_lbfgs(int(kind), x0.size, ptr(x0), C.byref(cfg), ptr(out), C.byref(info)))
    return out, info


GSL_ALGORITHMS = {"conjugate_fr": 0, "conjugate_pr": 1, "bfgs2": 2, "bfgs": 3, "steepest_descent": 4}


def gsl_config(algorithm, params):
    """algorithm: id 0..4 or one of GSL_ALGORITHMS; params: step_size, tol, max_iterations"""
    c = GslConfig()
    c.step_size, c.tol = float(params["step_size"]), float(params["tol"])
    c.max_iterations = int(params["max_iterations"])
    c.algorithm = GSL_ALGORITHMS[algorithm] if isinstance(algorithm, str) else int(algorithm)
    return c


def selftest_multimin(algorithm, kind, x0):
    """GSL's multimin test programme on the library's minimizers (host vectors, no GPU).
    -> (x, OptResult); OptResult.lbfgs_code = GSL status, .reserved = gradient evaluations"""
    x0 = as_f64(x0).ravel()
    out = np.empty_like(x0)
    info = OptResult()
    alg = GSL_ALGORITHMS[algorithm] if isinstance(algorithm, str) else int(algorithm)
    check(lib().bioen_hip_selftest_multimin(alg, int(kind), ptr(x0), ptr(out), C.byref(info)))
    return out, info


HOST_OBJECTIVE = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, dp, dp)


def multimin_host(objective, user, x0, algorithm, params):
    """The library's GSL-style minimizers on a host objective (no GPU).  `objective`: address of a C
    function ``int(void* user, const double* x, double* f, double* grad_or_NULL)`` (an int / c_void_p /
    ctypes function pointer) or a Python callable ``(x ndarray) -> f`` / ``(x, grad_out) -> f``
    wrapped here.  -> (x, OptResult); .lbfgs_code = GSL status, .reserved = gradient evaluations"""
    x0 = as_f64(x0).ravel()
    n = x0.size
    keep = None
    if callable(objective) and not isinstance(objective, C._CFuncPtr):
        pyfn = objective

        def _cb(_user, xp, fp, gp):
            try:
                x = np.ctypeslib.as_array(xp, shape=(n,))
                g = np.ctypeslib.as_array(gp, shape=(n,)) if gp else None
                fp[0] = float(pyfn(x, g))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        keep = HOST_OBJECTIVE(_cb)
        fn_addr = C.cast(keep, C.c_void_p)
    else:
        fn_addr = C.cast(objective, C.c_void_p) if not isinstance(objective, int) else C.c_void_p(objective)
    out = np.empty_like(x0)
    info = OptResult()
    cfg = gsl_config(algorithm, params)
    check(lib().bioen_hip_multimin_host(n, fn_addr, user, ptr(x0), C.byref(cfg), ptr(out), C.byref(info)))
    return out, info


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_size_t)


class Context(object):
    """Device-resident problem: yTilde (M x N) lives in HBM until close().

    rank/world > 1: the structures (columns) are sharded over `world` GPUs, one process each;
    this process keeps block `rank`.  N-vector arguments stay GLOBAL on every rank.  Before the
    first evaluation give the context a communicator: ``comm_init`` (RCCL) or ``set_exchange``
    (host-staged through any object with ``allgather_array``)."""

    def __init__(self, yTilde=None, YTilde=None, device=0, rank=0, world=1, _handle=None, _shape=None):
        L = lib()
        self._h = None
        self._exchange_keepalive = None
        self.rank, self.world = int(rank), int(world)
        if _handle is not None:
            self._h = _handle
            self.m, self.n = _shape
            self._query_shard()
            return
        yT = as_f64(yTilde)
        if yT.ndim != 2:
            raise ValueError("yTilde must be a 2-D (M x N) array")
        self.m, self.n = yT.shape
        YT = as_f64(YTilde).ravel()
        if YT.size != self.m:
            raise ValueError("YTilde must have M = %d entries" % self.m)
        h = ctx_p()
        check(L.bioen_hip_ctx_create_sharded(self.m, self.n, ptr(yT), ptr(YT), int(device), self.rank, self.world,
                                             C.byref(h)))
        self._h = h
        self._query_shard()

    def _query_shard(self):
        r, w, nl = C.c_int(0), C.c_int(1), C.c_int(0)
        ng, c0 = C.c_longlong(0), C.c_longlong(0)
        check(lib().bioen_hip_ctx_shard(self._h, C.byref(r), C.byref(w), C.byref(ng), C.byref(c0), C.byref(nl)))
        self.rank, self.world, self.col0, self.n_local = r.value, w.value, c0.value, nl.value

    @classmethod
    def synthetic(cls, m, n, YTrue, sig_sim, sig_exp, YTilde, seed=12345, device=0, rank=0, world=1):
        L = lib()
        a = [as_f64(v).ravel() for v in (YTrue, sig_sim, sig_exp, YTilde)]
        for v in a:
            if v.size != m:
                raise ValueError("synthetic(): every per-observable vector needs M entries")
        h = ctx_p()
        check(L.bioen_hip_ctx_create_synthetic_sharded(int(m), int(n), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]),
                                                       C.c_ulonglong(seed), int(device), int(rank), int(world),
                                                       C.byref(h)))
        return cls(rank=rank, world=world, _handle=h, _shape=(int(m), int(n)))

    @classmethod
    def from_raw(cls, sim, exp, exp_err, structure_major=False, device=0):
        """Context from RAW observables: yTilde = sim / exp_err and YTilde = exp / exp_err are formed on
        the device.  sim: (M, N), or (N, M) with structure_major=True (one structure's observables
        contiguous -- uploaded in chunks and transposed on the device)."""
        sim = as_f64(sim)
        if sim.ndim != 2:
            raise ValueError("sim must be 2-D")
        n, m = sim.shape if structure_major else sim.shape[::-1]
        exp, err = as_f64(exp).ravel(), as_f64(exp_err).ravel()
        if exp.size != m or err.size != m:
            raise ValueError("exp / exp_err need one entry per observable")
        h = ctx_p()
        check(lib().bioen_hip_ctx_create_raw(int(m), int(n), 1 if structure_major else 0, ptr(sim), ptr(exp), ptr(err),
                                             int(device), C.byref(h)))
        return cls(_handle=h, _shape=(int(m), int(n)))

    def set_exchange(self, comm):
        """Complete cross-rank reductions through `comm.allgather_array` (host-staged; for ranks
        that cannot share an RCCL communicator).  `comm` = None removes the hook."""
        if comm is None:
            self._exchange_keepalive = None
            check(lib().bioen_hip_ctx_set_exchange_callback(self._h, None, None))
            return
        world, rank = self.world, self.rank

        def _cb(user, buf, count):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(world * count,)).reshape(world, count)
                arr[:] = comm.allgather_array(arr[rank].copy())
                return 0
            except Exception:            # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        fn = EXCHANGE_FN(_cb)
        self._exchange_keepalive = fn
        check(lib().bioen_hip_ctx_set_exchange_callback(self._h, C.cast(fn, C.c_void_p), None))

    # -- lifetime ---------------------------------------------------------------
    def close(self):
        if self._h is not None:
            lib().bioen_hip_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _nvec(self, x, name):
        a = as_f64(x).ravel()
        if a.size != self.n:
            raise ValueError("%s must have N = %d entries, got %d" % (name, self.n, a.size))
        return a

    def _mvec(self, x, name):
        a = as_f64(x).ravel()
        if a.size != self.m:
            raise ValueError("%s must have M = %d entries, got %d" % (name, self.m, a.size))
        return a

    # -- data ---------------------------------------------------------------------
    def read_ytilde(self, row0=0, rows=None, col0=0, cols=None):
        """Block of the resident matrix; on a sharded context columns are relative to this rank's block."""
        rows = self.m - row0 if rows is None else rows
        cols = self.n_local - col0 if cols is None else cols
        out = np.empty((rows, cols))
        check(lib().bioen_hip_ctx_read_ytilde(self._h, row0, rows, col0, cols, ptr(out)))
        return out

    def footprint(self):
        """(forms, bytes) of the resident copies of the matrix: forms is a set out of {"rowmajor", "strips", "strips_colsum"};
        plus "bfgs_hinv" and its N x N bytes while a BFGS session (bfgs_logw) is live, and "forces_gram", the device buffer
        of forces_gram, "forces_colquad", the one of forces_colquad, "forces_gram_bf16", the one of forces_gram_bf16, and
        "forces_newton", the factor L and the work buffers of forces_newton_factor / opt_newton_forces, and "forces_laplace",
        the inverse factor and the covariances of forces_inverse / forces_laplace, and "logw_gram", the device buffer of logw_cov /
        opt_dual_newton_logw, each from its first call on"""
        f, b = C.c_int(0), C.c_longlong(0)
        check(lib().bioen_hip_ctx_footprint(self._h, C.byref(f), C.byref(b)))
        names = {1: "rowmajor", 2: "strips", 4: "strips_colsum", 8: "reduced", 16: "bfgs_hinv", 32: "forces_gram",
                 64: "forces_colquad", 128: "forces_gram_bf16", 256: "forces_newton", 512: "forces_laplace", 1024: "logw_gram",
                 2048: "logw_profile"}
        return {names[k] for k in names if f.value & k}, b.value

    def layout(self):
        """How the strip copies are held: {"one_copy": 0 | 1, "interleave": segments interleaved in the row-sum order copy,
        "relayouts": times that copy was moved to the other method's layout} (bioen_hip_ctx_layout)"""
        a, b, c_ = C.c_int(0), C.c_int(1), C.c_int(0)
        check(lib().bioen_hip_ctx_layout(self._h, C.byref(a), C.byref(b), C.byref(c_)))
        return {"one_copy": a.value, "interleave": b.value, "relayouts": c_.value}

    def strip_plan(self, which):
        """The regime of the strip passes' launch plan (bioen_hip_ctx_strip_plan; no device call).  which: 0 = the
        log-weights forward pass, 1 = the forces passes.  -> {"sps": strips per segment, "gs": groups per segment (0: the
        strip passes do not apply), "tc": strips per chunk (forces: the most strips a group runs per segment), "nch": chunks
        per group, "fold": a slot runs a whole group, "local_segments"}
        which = 2: the streaming pair on the row-major matrix (what serves a context without strip copies; answered whether
        or not the context is on it -- pair it with footprint() == {"rowmajor"} after the first evaluation): "sps": 128-column
        steps per segment, "gs": column tiles per segment, "tc": steps per tile, "nch": rows a wave of the adjoint kernel
        walks, "fold": 1 = non-temporal matrix loads, "local_segments".
        which = 3: the forces method's dense Gram passes (forces_gram, forces_gram_bf16): "gs": sets per segment, "tc": the
        longest chain of strips a set adds up, "nch": sets in all, "fold": tile pairs.  which = 4: forces_colquad's pass:
        "sps": panels of 32 columns, "gs": blocks of the launch, "tc": the most panels a block runs, "nch": 64-row slices of
        a strip (the kernel's NB), "fold": the strips' padded rows."""
        o = [C.c_int(0) for _ in range(6)]
        check(lib().bioen_hip_ctx_strip_plan(self._h, int(which), *[C.byref(v) for v in o]))
        return dict(zip(("sps", "gs", "tc", "nch", "fold", "local_segments"), (v.value for v in o)))

    def set_target(self, YTilde):
        check(lib().bioen_hip_ctx_set_ytilde_target(self._h, ptr(self._mvec(YTilde, "YTilde"))))

    def set_affine(self, row_offset=None, row_scale=None):
        """Optimise against row_offset[i] + row_scale[i] * yTilde[i][j] without touching the resident
        matrix (DEER modulation depths, SAXS scaling factor).  None -> 0 resp. 1; a scalar
        row_scale applies to every row.  Both methods honour it: the log-weights evaluations, products and
        optimizers, and every forces call (forces_weights, forces_fdf(_batch), opt_lbfgs_forces(_batch),
        opt_gsl_forces; sharded contexts too).  (0, 1) -- or None, None -- is the plain model, bit for bit.  The
        forces calls raise BioenHipError (invalid state) while a model AND a reduced storage format are set."""
        off = None if row_offset is None else self._mvec(row_offset, "row_offset")
        if row_scale is not None and np.ndim(row_scale) == 0:
            row_scale = np.full(self.m, float(row_scale))
        sc = None if row_scale is None else self._mvec(row_scale, "row_scale")
        check(lib().bioen_hip_ctx_set_affine(self._h, ptr(off) if off is not None else None,
                                             ptr(sc) if sc is not None else None))

    def set_direction_mode(self, mode):
        """'auto' (= 'gram'), 'twoloop' (liblbfgs' literal order of operations on the vectors) or
        'gram' (see include/bioen_hip.h: bioen_hip_ctx_set_direction_mode)."""
        code = {"auto": 0, "twoloop": 1, "gram": 2}[mode]
        check(lib().bioen_hip_ctx_set_direction_mode(self._h, code))

    STORAGE_FORMATS = {"f64": 0, "split": 1, "fp32": 2}

    def set_storage(self, fmt):
        """EXPERIMENT (opt-in, never the default): the log-weights matrix passes stream the centred matrix as
        'split' (fp32 + bf16 residual, 6 bytes per element, 2^-33 relative) or 'fp32' (4 bytes) instead of 'f64';
        reassembled to FP64 in registers, all sums FP64.  M <= 1024; served: the log-weights passes and the forces method's
        fused strip passes (forces_fdf(_batch), the forces optimizers); everything else of the forces method (forces_weights)
        raises BioenHipError (invalid state) while a reduced format is selected (the contract as implemented)."""
        check(lib().bioen_hip_ctx_set_storage(self._h, self.STORAGE_FORMATS[fmt]))

    def set_one_copy(self, on=True):
        """The log-weights method with ONE strip copy of the matrix resident (M <= 1024; 1 x instead of 2 x the matrix): the
        adjoint runs on the row-sum order copy, 1-3 % slower per launch; same minima, last bits differ from the two-copy
        default.  Call before the context's first gradient evaluation.  (Also: BIOEN_HIP_ONE_COPY=1 at creation; and a context
        takes this form by itself when the second copy does not fit.)"""
        check(lib().bioen_hip_ctx_set_one_copy(self._h, int(bool(on))))

    dense_panels = False        # what set_dense_panels left (the default of a context: off)

    def set_dense_panels(self, on=True):
        """The log-weights dual Newton beyond 1024 observables (bioen_hip_ctx_set_dense_panels): with it logw_cov,
        logw_cov_bf16, opt_dual_newton_logw and opt_dual_newton_logw_series serve 1024 < M <= 4096 over the row panels of the
        matrix (their strip copies must be resident); beyond 4096 rows they raise BioenHipError (invalid state) naming 4096.
        Off by default; logw_laplace, the profiled series, every forces dense entry, sharded contexts and the
        reduced-storage copies refuse M > 1024 as before.  Keeps the point and a session.  The Gram buffer grows with M^2:
        (sets + 1) x 68 MB at 4096 rows (sets: 8 unless BIOEN_HIP_SEGMENTS says otherwise) plus C, the factor's 2 M^2
        doubles (footprint(): "logw_gram", "forces_newton").  `dense_panels` holds what was set."""
        check(lib().bioen_hip_ctx_set_dense_panels(self._h, int(bool(on))))
        self.dense_panels = bool(on)

    def synchronize(self):
        check(lib().bioen_hip_synchronize(self._h))

    # -- log-weights --------------------------------------------------------------
    def logw_weights(self, g):
        g = self._nvec(g, "g")
        w = np.empty(self.n)
        logs = C.c_double(0.0)
        check(lib().bioen_hip_logw_weights(self._h, ptr(g), ptr(w), C.byref(logs)))
        return w, logs.value

    def logw_fdf(self, g, G, theta, need_f=True, need_grad=True):
        g, G = self._nvec(g, "g"), self._nvec(G, "G")
        f = C.c_double(0.0)
        grad = np.empty(self.n) if need_grad else None
        check(lib().bioen_hip_logw_fdf(self._h, ptr(g), ptr(G), float(theta), C.byref(f),
                                       ptr(grad) if need_grad else None))
        return (f.value if need_f else None), grad

    def logw_hessp(self, v, g=None, G=None, theta=None):
        """Hessian-vector products H(g) v of the log-weights objective for up to 8 directions in one call: `v` is (n,) or
        (k, n), the result has its shape.  With `g` (and G, theta) the point is evaluated first, as by logw_fdf, and kept on
        the context: -> (hv, f, grad); `v` None then only sets the point: -> (None, f, grad).  Without `g` the product
        refers to the point the last such call left: -> hv; BioenHipError (invalid state) once any other evaluation,
        optimizer or change of the matrix state has run."""
        return self._hessp(lib().bioen_hip_logw_hessp, "logw_hessp", "N", ("g", "G"), v, g, G, theta)

    def _point(self, dim, names, x, aux):
        """the two vectors of a point -- the first of length N or M (`dim`), the second of length N, `names` in the
        ValueError texts -- and what its evaluation leaves: f and grad, of the first vector's length"""
        x = (self._nvec if dim == "N" else self._mvec)(x, names[0])
        return x, self._nvec(aux, names[1]), C.c_double(0.0), np.empty(x.shape[0])

    def _hessp(self, fn, name, dim, names, v, x, aux, theta):
        """logw_hessp and forces_hessp: one call shape.  `fn` the entry, `dim` ("N" or "M") the length of a direction and of
        the point's first vector, `names` the point's two arguments and `name` the method in the ValueError texts"""
        if v is None:
            if x is None or aux is None or theta is None:
                raise ValueError("%s without v sets the point: it needs %s, %s and theta" % ((name,) + names))
            x, aux, f, grad = self._point(dim, names, x, aux)
            check(fn(self._h, ptr(x), ptr(aux), float(theta), 0, None, None, C.byref(f), ptr(grad)))
            return None, f.value, grad
        va = as_f64(v)
        size = self.n if dim == "N" else self.m
        if va.ndim not in (1, 2) or va.shape[-1] != size:
            raise ValueError("v must be (%s,) or (k, %s) with %s = %d, got %s" % (dim, dim, dim, size, (va.shape,)))
        k = 1 if va.ndim == 1 else va.shape[0]
        if k < 1 or k > 8:
            raise ValueError("%s takes 1 to 8 directions per call, got %d" % (name, k))
        hv = np.empty_like(va)
        if x is None:
            check(fn(self._h, None, None, 0.0, k, ptr(va), ptr(hv), None, None))
            return hv
        if aux is None or theta is None:
            raise ValueError("%s with %s needs %s and theta" % ((name,) + names))
        x, aux, f, grad = self._point(dim, names, x, aux)
        check(fn(self._h, ptr(x), ptr(aux), float(theta), k, ptr(va), ptr(hv), C.byref(f), ptr(grad)))
        return hv, f.value, grad

    def logw_cov(self, g=None, G=None, theta=None, cov=True):
        """C = sum_j w_j (y_j - ybar)(y_j - ybar)^T, w = softmax(g): the covariance of the observables (of the affine model if
        one is set) under the weights of a log-weights point, (m, m), bitwise symmetric, the same bits call after call --
        one compute-bound pass on the FP64 matrix cores (M <= 1024; after set_dense_panels M <= 4096 over the row panels, with
        a buffer of (sets + 1) x (M / 64)(M / 64 + 1) / 2 x 32 KiB: 0.6 GB at 4096 rows).  With `g` (and G, theta) the point is
        evaluated first, as by logw_hessp -- f and grad are its bits --, and kept on the context: -> (C, f, grad); cov=False
        then only sets the point (C is None).  Without, at the kept log-weights point (this call's, logw_hessp's or
        opt_dual_newton_logw's): -> C; BioenHipError (invalid state) as logw_hessp raises it.  The first computing call
        allocates a device buffer that stays with the context (footprint(): "logw_gram")."""
        out = self._gram(lib().bioen_logwn_cov, "logw_cov", "N", ("g", "G"), g, G, theta, cov=cov)
        return out[0] if g is None else out

    def opt_dual_newton_logw(self, g0, G, theta, params=None):
        """The dual Newton minimizer of the log-weights objective, the loop on the device side of the C ABI:
        per iteration the covariance C of the kept point, (C + theta I) z = -b factorised and solved in HBM, one centred
        adjoint pass, one evaluation per trial alpha = 1, 1/2, ...; params: gtol, max_iterations and the constants of
        LOGW_NEWTON_DEFAULTS.  theta > 0.  -> dict(g, status (0: max|grad| <= gtol max w, 1: max_iterations, 2: step
        exhausted at the rounding floor of f, 3: step exhausted), fmin, gmax, wmax, iterations, evaluations,
        factorisations).  g is in the gauge the steps leave it in: compare weights.  The returned point is the context's
        kept point: logw_cov() and logw_hessp(v) right after serve it."""
        if logw_newton_source((params or {}).get("hessian", "gram")):       # "gram_bf16": a series of one theta
            return self.opt_dual_newton_logw_series([theta], g0, G, params, hessian="gram_bf16")[0]
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        cfg = logw_newton_config(params)
        out = np.empty(self.n)
        res = LogwNewtonResult()
        check(lib().bioen_logwn_opt(self._h, ptr(g0), ptr(G), float(theta), C.byref(cfg), ptr(out), C.byref(res)))
        return dict(g=out, status=res.status, fmin=res.fmin, gmax=res.gmax, wmax=res.wmax, iterations=res.iterations,
                    evaluations=res.evaluations, factorisations=res.factorisations)

    def logw_laplace(self, g=None, G=None, theta=None, observables=None, matrices=True, vectors=True):
        """The Laplace error bars at a log-weights point, formed on the device (bioen_logwn_laplace; M <= 1024):
        C from logw_cov's pass, C + theta I factorised and inverted in HBM, the inverse handed to forces_colquad's pass
        where it stands.  With `g` (and G) the point is evaluated first, as by logw_cov, and kept; without, the kept
        log-weights point is served -- right after opt_dual_newton_logw at no further evaluation -- (BioenHipError as
        logw_hessp raises it).  theta > 0 is required either way.  -> dict: info (LAPACK dpotrf's; != 0: every array below
        is None and logdet, min_pivot are nan), logdet = ln det (C + theta I), min_pivot, std_averages (m,), cov_averages
        ((m, m), bitwise symmetric; None with matrices=False), w, leverage, var_logw, std_w ((n,) each; None with
        vectors=False, and the pass over the matrix does not run), and with g also f and grad.  `observables`, (n,) or
        (k, n): per-structure quantities that were not fitted; obs_averages and var_observables, (k,), are their refined
        averages and the variances of those (more than 8 are served in chunks of 8 at the kept point).  A single weight is
        poorly determined whenever theta w_j << 1 (std_w_j / w_j ~ 1 / sqrt(theta w_j)): read the averages."""
        if theta is None:
            raise ValueError("logw_laplace needs theta")
        if g is not None and G is None:
            raise ValueError("logw_laplace with g needs G")
        m, n = self.m, self.n
        obs = None
        if observables is not None:
            obs = as_f64(observables)
            if obs.ndim == 1:
                obs = obs.reshape(1, -1)
            if obs.ndim != 2 or obs.shape[1] != n or obs.shape[0] < 1:
                raise ValueError("observables must be (N,) or (k, N) with N = %d, got %s" % (n, (np.shape(observables),)))
        kobs = 0 if obs is None else obs.shape[0]
        sa = np.empty(m)
        ca = np.empty((m, m)) if matrices else None
        vecs = [np.empty(n) if vectors else None for _ in range(4)]
        oa, vo = (np.empty(kobs), np.empty(kobs)) if kobs else (None, None)
        logdet, pivot, info = C.c_double(float("nan")), C.c_double(float("nan")), C.c_int(0)
        fn = lib().bioen_logwn_laplace

        def chunk(k0):
            k = min(8, kobs - k0)
            return (ptr(obs[k0:k0 + k]), k, ptr(oa[k0:k0 + k]), ptr(vo[k0:k0 + k])) if k > 0 else (None, 0, None, None)

        po, k, pa, pv = chunk(0)
        out = [ptr(a) if a is not None else None for a in [sa, ca] + vecs] + [pa, pv, C.byref(logdet), C.byref(pivot),
                                                                                C.byref(info)]
        res = {}
        if g is None:
            check(fn(self._h, None, None, float(theta), po, k, *(out + [None, None])))
        else:
            g, G, f, grad = self._point("N", ("g", "G"), g, G)
            check(fn(self._h, ptr(g), ptr(G), float(theta), po, k, *(out + [C.byref(f), ptr(grad)])))
            res.update(f=f.value, grad=grad)
        for k0 in range(8, kobs if info.value == 0 else 0, 8):      # the rest at the kept point: the observables' path alone
            po, k, pa, pv = chunk(k0)
            more = C.c_int(0)
            check(fn(self._h, None, None, float(theta), po, k, None, None, None, None, None, None, pa, pv, None, None,
                     C.byref(more), None, None))
            if more.value:
                info.value = more.value
        ok = info.value == 0
        res.update(info=info.value, logdet=logdet.value if ok else float("nan"), min_pivot=pivot.value if ok else float("nan"),
                   std_averages=sa if ok else None, cov_averages=ca if ok else None)
        res.update(zip(("w", "leverage", "var_logw", "std_w"), (v if ok else None for v in vecs)))
        if kobs:
            res.update(obs_averages=oa if ok else None, var_observables=vo if ok else None)
        return res

    def logw_cov_bf16(self, g=None, G=None, theta=None, cov=True):
        """logw_cov with the M x M x N product from split-BF16 operands on the BF16 matrix cores (bioen_logwn_cov_bf16;
        DESIGN 6k): the covariance the dual Newton loop's hessian="gram_bf16" factorises.  Call shape, point semantics,
        refusals and buffer are logw_cov's; f and grad are its bits; |C~ - C|_ik <= 3 * 2^-16 sqrt(G'_ii G'_kk)."""
        out = self._gram(lib().bioen_logwn_cov_bf16, "logw_cov_bf16", "N", ("g", "G"), g, G, theta, cov=cov)
        return out[0] if g is None else out

    def opt_dual_newton_logw_series(self, thetas, g0, G, params=None, hessian="gram", warm=True):
        """opt_dual_newton_logw for the thetas in the order given, in one call (bioen_logwn_series): G goes up
        once, the vectors stay in HBM, warm=True starts theta k at the point theta k - 1 returned (False: every theta at g0).
        hessian: "gram" (the FP64 covariance: bit for bit the chained / single calls) or "gram_bf16" (the split-BF16 pass;
        a step rejected at the rounding floor sends that theta's run over to the FP64 pass, once); params["hessian"], if
        present, wins.  -> a list of opt_dual_newton_logw's dicts plus bf16_passes and switched.  A theta that ends with
        status != 0 does not stop the series.  The last theta's returned point is the context's kept point."""
        p = dict(params or {})
        source = logw_newton_source(p.get("hessian", hessian))
        th = as_f64(np.asarray(thetas, dtype=np.float64).reshape(-1))
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        cfg = logw_newton_config(p)
        out = np.empty((max(len(th), 1), self.n))
        res = (LogwNewtonSeriesResult * max(len(th), 1))()
        check(lib().bioen_logwn_series(self._h, ptr(g0), ptr(G), ptr(th), int(len(th)), C.byref(cfg), source, int(bool(warm)),
                                       ptr(out), res))
        return [dict(g=out[k].copy(), status=r.status, fmin=r.fmin, gmax=r.gmax, wmax=r.wmax, iterations=r.iterations,
                     evaluations=r.evaluations, factorisations=r.factorisations, bf16_passes=r.bf16_passes,
                     switched=bool(r.switched)) for k, r in enumerate(res)]

    def opt_dual_newton_logw_profile_series(self, thetas, g0, G, params=None, groups=None, row_offset=None, hessian="gram",
                                            warm=True):
        """opt_dual_newton_logw_series with the nuisance scales of the affine model profiled out
        (bioen_logwn_profile_series): the resident matrix is the parameter-independent one, `groups` a list of
        row-index arrays (None: one group of all rows; rows in no group keep the scale 1; at most 64 groups), one
        least-squares scale per group -- nuisance.refit_scales at the point's raw averages -- formed inside every
        evaluation, the Newton step from the projected covariance.  One run per theta replaces the alternation optimise /
        refit.  -> a list of opt_dual_newton_logw_series's dicts plus scales (one per group), chi2 and kl.  Afterwards the
        context's affine model is (row_offset, the last theta's scales) and the last returned point is the kept point:
        logw_hessp, logw_cov and logw_laplace without g serve it at those fixed scales.  set_affine(None, None) removes
        the model."""
        p = dict(params or {})
        source = logw_newton_source(p.get("hessian", hessian))
        th = as_f64(np.asarray(thetas, dtype=np.float64).reshape(-1))
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        if groups is None:
            groups = [np.arange(self.m)]
        group = np.full(self.m, -1, dtype=np.int32)
        for k, ix in enumerate(groups):
            ix = np.asarray(ix, dtype=np.int64).reshape(-1)
            if ix.size and (ix.min() < 0 or ix.max() >= self.m):
                raise ValueError("groups: row %d outside 0 .. %d" % (ix.min() if ix.min() < 0 else ix.max(), self.m - 1))
            if (group[ix] >= 0).any() or np.unique(ix).size != ix.size:
                raise ValueError("groups must be disjoint")
            group[ix] = k
        off = None if row_offset is None else self._mvec(row_offset, "row_offset")
        cfg = logw_newton_config(p)
        nt, ng = max(len(th), 1), max(len(groups), 1)
        out, scales, chi2, kl = np.empty((nt, self.n)), np.empty((nt, ng)), np.empty(nt), np.empty(nt)
        res = (LogwNewtonSeriesResult * nt)()
        check(lib().bioen_logwn_profile_series(self._h, ptr(g0), ptr(G), ptr(th), int(len(th)), C.byref(cfg), source,
                                               int(bool(warm)), ptr(off) if off is not None else None,
                                               group.ctypes.data_as(ip), int(len(groups)), ptr(out), ptr(scales), ptr(chi2),
                                               ptr(kl), res))
        return [dict(g=out[k].copy(), status=r.status, fmin=r.fmin, gmax=r.gmax, wmax=r.wmax, iterations=r.iterations,
                     evaluations=r.evaluations, factorisations=r.factorisations, bf16_passes=r.bf16_passes,
                     switched=bool(r.switched), scales=[float(s) for s in scales[k]], chi2=float(chi2[k]), kl=float(kl[k]))
                for k, r in enumerate(res)]

    def opt_lbfgs_logw(self, g0, G, theta, params, verbose=False, debug=False, want_weights=True):
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        cfg = lbfgs_config(params)
        vis = VisualParams(int(bool(debug)), int(bool(verbose)))
        res = np.empty(self.n)
        w = np.empty(self.n) if want_weights else None
        info = OptResult()
        check(lib().bioen_hip_opt_lbfgs_logw(self._h, ptr(g0), ptr(G), float(theta), C.byref(cfg), C.byref(vis),
                                             ptr(res), ptr(w) if want_weights else None, C.byref(info)))
        return res, w, info

    def opt_gsl_logw(self, g0, G, theta, algorithm, params, verbose=False, debug=False, want_weights=True):
        """GSL-style minimizer (conjugate_fr/pr, bfgs2, bfgs, steepest_descent) with all vectors in HBM.
        -> (gopt, w or None, OptResult with the GSL status in .lbfgs_code)"""
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        cfg = gsl_config(algorithm, params)
        vis = VisualParams(int(bool(debug)), int(bool(verbose)))
        res = np.empty(self.n)
        w = np.empty(self.n) if want_weights else None
        info = OptResult()
        check(lib().bioen_hip_opt_gsl_logw(self._h, ptr(g0), ptr(G), float(theta), C.byref(cfg), C.byref(vis),
                                           ptr(res), ptr(w) if want_weights else None, C.byref(info)))
        return res, w, info

    def opt_lbfgs_logw_batch(self, thetas, g0, G, params, max_batch=8, verbose=False, debug=False,
                             want_weights=True):
        """Solve a whole theta series; up to `max_batch` (<= 8) thetas share every pass over yTilde.
        g0: (n,) shared start or (ntheta, n) one start per theta.
        -> (results[ntheta, n], weights[ntheta, n] or None, [OptResult] * ntheta)"""
        thetas = as_f64(thetas).ravel()
        nt = thetas.size
        g0 = as_f64(g0)
        if g0.size == self.n:
            g0, stride = g0.ravel(), 0
        elif g0.shape == (nt, self.n):
            stride = self.n
        else:
            raise ValueError("g0 must have shape (n,) or (ntheta, n)")
        G = self._nvec(G, "G")
        cfg = lbfgs_config(params)
        vis = VisualParams(int(bool(debug)), int(bool(verbose)))
        res = np.empty((nt, self.n))
        w = np.empty((nt, self.n)) if want_weights else None
        infos = (OptResult * nt)()
        check(lib().bioen_hip_opt_lbfgs_logw_batch(self._h, nt, ptr(thetas), ptr(g0), stride, ptr(G), C.byref(cfg),
                                                   C.byref(vis), int(max_batch), ptr(res),
                                                   ptr(w) if want_weights else None, infos))
        return res, w, list(infos)

    # -- dense inverse-Hessian BFGS (scipy's fmin_bfgs on the device: bioen_amd/bfgs.py) --------------------------------
    def bfgs_logw(self, g0, G, theta, gtol=1e-5, norm=np.inf, maxiter=None, c1=1e-4, c2=0.9, xrtol=0, disp=False):
        """scipy.optimize.fmin_bfgs of the log-weights objective with H, the N x N inverse Hessian, in HBM: scipy's loop
        and line searches on the host (bioen_amd.bfgs), every vector on the device.  Unsharded contexts only.
        -> (gopt, w, info); info: fmin, iterations, func_calls, grad_calls, warnflag, message, chi2, kl"""
        from . import bfgs
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        backend = bfgs.DeviceBackend(self, g0, G, theta)
        try:
            res = bfgs.minimize(backend, self.n, gtol=gtol, norm=norm, maxiter=maxiter, c1=c1, c2=c2, xrtol=xrtol,
                                disp=disp)
        except BaseException:
            self._bfgs_abandon()
            raise
        g, w, end = backend.finish()
        res.chi2, res.kl = end.chi2, end.kl
        return g, w, res

    def _bfgs_abandon(self):
        if self._h is not None and "bfgs_hinv" in self.footprint()[0]:
            try:
                self.bfgs_end()
            except BioenHipError:
                pass

    def bfgs_begin(self, g0, G, theta, norm_inf=True):
        """-> (f0, |g0| (max norm if norm_inf, else 2-norm), |g0|_2, g0.p0) -- bioen_hip_bfgs_logw_begin"""
        g0, G = self._nvec(g0, "g0"), self._nvec(G, "G")
        o = [C.c_double(0.0) for _ in range(4)]
        check(lib().bioen_hip_bfgs_logw_begin(self._h, ptr(g0), ptr(G), float(theta), int(bool(norm_inf)),
                                              *[C.byref(v) for v in o]))
        return tuple(v.value for v in o)

    def bfgs_trial(self, alpha, need_grad):
        """-> (f(x + alpha p), g(alpha).p or None)"""
        f, d = C.c_double(0.0), C.c_double(0.0)
        check(lib().bioen_hip_bfgs_logw_trial(self._h, float(alpha), int(bool(need_grad)), C.byref(f), C.byref(d)))
        return f.value, (d.value if need_grad else None)

    def bfgs_accept(self, alpha, norm_inf=True):
        """-> (|g|, |p|_2, |x|_2) at the accepted point"""
        o = [C.c_double(0.0) for _ in range(3)]
        check(lib().bioen_hip_bfgs_logw_accept(self._h, float(alpha), int(bool(norm_inf)), *[C.byref(v) for v in o]))
        return tuple(v.value for v in o)

    def bfgs_update(self):
        """-> (g.p of the next direction, whether y.s == 0 made rho = 1000)"""
        d, fb = C.c_double(0.0), C.c_int(0)
        check(lib().bioen_hip_bfgs_logw_update(self._h, C.byref(d), C.byref(fb)))
        return d.value, bool(fb.value)

    def bfgs_end(self):
        """-> (x, w, OptResult with fmin, chi2, kl at x); frees H"""
        g, w = np.empty(self.n), np.empty(self.n)
        info = OptResult()
        check(lib().bioen_hip_bfgs_logw_end(self._h, ptr(g), ptr(w), C.byref(info)))
        return g, w, info

    def bfgs_read_hinv(self, row0=0, rows=None, padded=False):
        """rows [row0, row0 + rows) of the session's current inverse Hessian (debug / tests); padded: the stored form,
        ld = N rounded up to 16 columns, pad rows and columns included"""
        height = (self.n + 15) // 16 * 16 if padded else self.n
        rows = height - row0 if rows is None else int(rows)
        out = np.empty((rows, height))
        check(lib().bioen_hip_bfgs_logw_read_hinv(self._h, int(row0), rows, int(bool(padded)), ptr(out)))
        return out

    BFGS_VECTORS = {"x": 0, "g": 1, "p": 2, "s": 3, "y": 4, "u": 5}

    def bfgs_read_vec(self, which):
        """a session vector: 'x', 'g', 'p', 's' (newest step), 'y' (newest), 'u' (H y of the pending update)"""
        out = np.empty(self.n)
        check(lib().bioen_hip_bfgs_logw_read_vec(self._h, self.BFGS_VECTORS[which], ptr(out)))
        return out

    # -- forces -------------------------------------------------------------------
    def forces_weights(self, forces, w0):
        """w_j = w0_j exp(x_j) / Z with x = yTilde_eff^T forces -- of the affine model if one is set (set_affine)"""
        f, w0 = self._mvec(forces, "forces"), self._nvec(w0, "w0")
        w = np.empty(self.n)
        check(lib().bioen_hip_forces_weights(self._h, ptr(f), ptr(w0), ptr(w)))
        return w

    def forces_fdf(self, forces, w0, theta, need_f=True, need_grad=True):
        """-> (f, grad[m]) of the forces objective on the resident matrix, or on row_offset + row_scale * matrix
        where set_affine has set a model (the gradient is then the one with respect to the forces of that model)"""
        fo, w0 = self._mvec(forces, "forces"), self._nvec(w0, "w0")
        f = C.c_double(0.0)
        grad = np.empty(self.m) if need_grad else None
        check(lib().bioen_hip_forces_fdf(self._h, ptr(fo), ptr(w0), float(theta), C.byref(f),
                                         ptr(grad) if need_grad else None))
        return (f.value if need_f else None), grad

    def forces_hessp(self, v, forces=None, w0=None, theta=None):
        """Hessian-vector products H(forces) v of the forces objective (of the affine model if one is set) for up to 8
        directions in one call: `v` is (m,) or (k, m), the result has its shape.  With `forces` (and w0, theta) the point
        is evaluated first, as by forces_fdf -- f and grad are its bits --, and kept on the context: -> (hv, f, grad); `v`
        None then only sets the point: -> (None, f, grad).  Without `forces` the product refers to the point the last such
        call left (two fused matrix passes, whatever k): -> hv; BioenHipError (invalid state) once any other evaluation,
        optimizer or change of the matrix state has run, or when the context's point is a log-weights point."""
        return self._hessp(lib().bioen_hip_forces_hessp, "forces_hessp", "M", ("forces", "w0"), v, forces, w0, theta)

    def forces_hessian(self, forces=None, w0=None, theta=None):
        """The dense Hessian (m, m) of the forces objective: ceil(m / 8) forces_hessp calls with unit directions.  With
        `forces` the point is set first: -> (H, f, grad); without, at the kept point: -> H.  The result is symmetrised as
        (H + H^T) / 2: the products' own asymmetry -- the two matrix passes of a product add in different orders for a
        row and for a column -- is rounding, checked here to be at most 1e-10 of the largest entry (measured: see DESIGN 6d)."""
        out = None
        if forces is not None:
            _, f, grad = self.forces_hessp(None, forces=forces, w0=w0, theta=theta)
            out = (f, grad)
        m = self.m
        H = np.empty((m, m))
        eye = np.eye(m)
        for i0 in range(0, m, 8):
            H[i0:i0 + 8] = self.forces_hessp(eye[i0:i0 + 8])
        scale = np.abs(H).max()
        asym = np.abs(H - H.T).max()
        if not asym <= 1e-10 * scale:
            raise BioenHipError("forces_hessian: the products are not symmetric: max |H - H^T| = %.3g, max |H| = %.3g"
                                % (asym, scale))
        H = 0.5 * (H + H.T)
        return H if out is None else (H, out[0], out[1])

    def forces_gram(self, forces=None, w0=None, theta=None, cov=True, hess=True):
        """(C, H): the covariance of the observables under the weights, C = d ybar / d forces, and the dense Hessian of the
        forces objective (of the affine model if one is set), both (m, m) and bitwise symmetric, from ONE compute-bound
        pass over the matrix (M <= 1024; forces_hessian builds H from 2 ceil(m / 8) bandwidth-bound ones).  A matrix not
        asked for is None.  With `forces` (and w0, theta) the point is evaluated first, as by forces_fdf -- f and grad are
        its bits --, and kept on the context: -> (C, H, f, grad).  Without, at the point the last such call (or
        forces_hessp with forces) left: -> (C, H); BioenHipError (invalid state) as forces_hessp raises it.
        The first call allocates a device buffer for the partial sums that stays with the context (footprint():
        "forces_gram"): O(sets x m^2) whatever n is -- 117 MB at m = 256, 139 MB at m = 512, 168 MB at m = 1024 -- so with
        many small contexts prefer forces_hessian."""
        return self._gram(lib().bioen_hip_forces_gram, "forces_gram", "M", ("forces", "w0"), forces, w0, theta, cov=cov, hess=hess)

    def forces_gram_bf16(self, forces=None, w0=None, theta=None, cov=True, hess=True):
        """(C~, H~): forces_gram's C and H with the two M x M x N products formed from split-BF16 operands (every operand
        hi + lo, two bfloat16 numbers; hi hi + hi lo + lo hi accumulated in f32) on the BF16 matrix cores, at 32 x the FP64
        matrix rate (M <= 1024).  The result is a MINIMIZER's Hessian, good to about 1e-5 ... 1e-4 of max|H|: it
        shapes a Newton step (scipy:hessian=gram_bf16), while f and grad stay forces_fdf's FP64 bits and decide the
        optimum.  laplace_error_bars keeps using forces_gram, whose results this call leaves bitwise alone.  Arguments,
        return shapes, point semantics and refusals are forces_gram's: with `forces` (and w0, theta) -> (C~, H~, f, grad) and
        the point is kept; without -> (C~, H~) at the kept point.  Both matrices are bitwise symmetric and the same bits
        call after call.  The first computing call allocates a device buffer of forces_gram's size that stays with the
        context (footprint(): "forces_gram_bf16")."""
        return self._gram(lib().bioen_hip_forces_gram_bf16, "forces_gram_bf16", "M", ("forces", "w0"), forces, w0, theta, cov=cov,
                          hess=hess)

    def _gram(self, fn, name, dim, names, x, aux, theta, **want):
        """forces_gram, forces_gram_bf16 and logw_cov: one call shape.  `fn` the entry, `name` the method in the ValueError
        texts, `dim` and `names` the point's as in _hessp, `want` which of the entry's (m, m) matrices are asked for, by
        the method's flags in the entry's order.  -> the matrices (None where not wanted), with a point then f and grad"""
        mats = [np.empty((self.m, self.m)) if on else None for on in want.values()]
        ptrs = [ptr(a) if a is not None else None for a in mats]
        if x is None:
            if not any(want.values()):
                raise ValueError("%s without %s needs %s" % (name, names[0], " or ".join(want)))
            check(fn(self._h, None, None, 0.0, *ptrs, None, None))
            return tuple(mats)
        if aux is None or theta is None:
            raise ValueError("%s with %s needs %s and theta" % ((name,) + names))
        x, aux, f, grad = self._point(dim, names, x, aux)
        check(fn(self._h, ptr(x), ptr(aux), float(theta), *ptrs, C.byref(f), ptr(grad)))
        return (*mats, f.value, grad)

    def forces_newton_factor(self, A=None, source="gram", lam=0.0, want_L=True):
        """(L or None, info): the FP64 Cholesky factorisation A + lam I = L L^T on the device (M <= 1024).  A: an
        (m, m) matrix of which only the lower triangle is read; A=None: the Hessian of the kept forces point from `source`
        ("gram": forces_gram's H, "gram_bf16": forces_gram_bf16's), computed now and not downloaded.  info is LAPACK
        dpotrf's: 0, or k + 1 where pivot k was <= 0 or not finite (an ordinary result: L is None then and
        forces_newton_solve is refused until a factorisation succeeds).  The same bits in give the same bits out.  Keeps
        point and session; the first call allocates a device buffer that stays with the context (footprint():
        "forces_newton")."""
        m = self.m
        pa = None
        if A is not None:
            A = as_f64(A)
            if A.shape != (m, m):
                raise ValueError("A must have shape (%d, %d)" % (m, m))
            pa = ptr(A)
        L = np.zeros((m, m)) if want_L else None
        info = C.c_int(0)
        check(lib().bioen_hip_forces_newton_factor(self._h, pa, 0 if A is not None else newton_source(source), float(lam),
                                                   ptr(L) if want_L else None, C.byref(info)))
        return (L if info.value == 0 else None), info.value

    def forces_newton_solve(self, B):
        """X = (L L^T)^-1 B with the factor of the last forces_newton_factor call; B: (m,) or (k, m), k <= 8 right-hand
        sides as rows.  A row's result does not depend on k."""
        B = as_f64(B)
        one = B.ndim == 1
        B2 = np.ascontiguousarray(B.reshape(1, -1) if one else B)
        if B2.ndim != 2 or B2.shape[1] != self.m:
            raise ValueError("B must have shape (m,) or (k, m)")
        X = np.empty_like(B2)
        check(lib().bioen_hip_forces_newton_solve(self._h, int(B2.shape[0]), ptr(B2), ptr(X)))
        return X[0] if one else X

    def opt_newton_forces(self, forces0, w0, theta, params=None, want_weights=True):
        """Regularised Newton on the forces objective, the loop on the device side of the C ABI: H from
        params["hessian"] ("gram" | "gram_bf16") at the kept point, factorised and solved in HBM; params: gtol,
        max_iterations, hessian and the damping constants (NEWTON_DEFAULTS).  -> dict(forces, weights (or None), status
        (0: max|g| <= gtol, 1: max_iterations, 2: at the minimum to the rounding of f, 3: lambda out of range), fmin, gmax,
        lam, iterations, evaluations, hessians, factorisations, switched).  The returned point is the context's kept
        point: forces_gram() right after serves it."""
        f0, w0 = self._mvec(forces0, "forces0"), self._nvec(w0, "w0")
        cfg = newton_config(params)
        out = np.empty(self.m)
        w = np.empty(self.n) if want_weights else None
        res = NewtonResult()
        check(lib().bioen_hip_opt_newton_forces(self._h, ptr(f0), ptr(w0), float(theta), C.byref(cfg), ptr(out),
                                                ptr(w) if want_weights else None, C.byref(res)))
        return dict(forces=out, weights=w, status=res.status, fmin=res.fmin, gmax=res.gmax, lam=res.lam,
                    iterations=res.iterations, evaluations=res.evaluations, hessians=res.hessians,
                    factorisations=res.factorisations, switched=bool(res.switched))

    def forces_inverse(self, A=None):
        """(Ainv or None, logdet, info): the inverse of a symmetric positive definite (m, m) matrix A (only its lower triangle
        is read) from its FP64 Cholesky factor, on the device (M <= 1024): Ainv = W^T W with W = L^-1, bitwise
        symmetric, and logdet = 2 sum ln L_ii.  A=None: the Hessian (forces_gram's) of the kept forces point; the inverse
        then stays on the device and None is returned for it.  info is LAPACK dpotrf's: 0, or k + 1 where pivot k was <= 0
        or not finite -- an ordinary result: (None, nan, info).  The factor becomes the context's: forces_newton_solve
        afterwards solves with it.  The same bits in give the same bits out.  Keeps point and session; the first call
        allocates a device buffer of 4 padded m^2 doubles that stays with the context (footprint(): "forces_laplace")."""
        m = self.m
        pa, Ainv = None, None
        if A is not None:
            A = as_f64(A)
            if A.shape != (m, m):
                raise ValueError("A must have shape (%d, %d)" % (m, m))
            pa = ptr(A)
            Ainv = np.empty((m, m))
        logdet, info = C.c_double(float("nan")), C.c_int(0)
        check(lib().bioen_laplace_forces_inverse(self._h, pa, ptr(Ainv) if Ainv is not None else None, C.byref(logdet),
                                                 C.byref(info)))
        return (Ainv if info.value == 0 else None), logdet.value, info.value

    def forces_laplace(self, forces=None, w0=None, theta=None, matrices=True):
        """The Laplace error bars at a forces point, formed on the device (M <= 1024): H from forces_gram's pass,
        factorised and inverted in HBM, the inverse handed to forces_colquad's pass where it stands.  With `forces` (and w0,
        theta) the point is evaluated first, as by forces_fdf, and kept; without, the kept forces point is served
        (BioenHipError as forces_hessp raises it).  -> dict: info (LAPACK dpotrf's; != 0: every array below is None and
        logdet_H, min_pivot are nan), std_forces (m,), std_averages (m,), var_logw (n,), logdet_H, min_pivot = min L_ii^2,
        cov_forces and cov_averages ((m, m), bitwise symmetric; None with matrices=False, when nothing of size m^2 comes
        down), and with forces f and grad.  The first call allocates a device buffer that stays with the context
        (footprint(): "forces_laplace")."""
        m = self.m
        sf, sa, vl = np.empty(m), np.empty(m), np.empty(self.n)
        cf = np.empty((m, m)) if matrices else None
        ca = np.empty((m, m)) if matrices else None
        logdet, pivot, info = C.c_double(float("nan")), C.c_double(float("nan")), C.c_int(0)
        out = [ptr(sf), ptr(sa), ptr(vl), ptr(cf) if matrices else None, ptr(ca) if matrices else None, C.byref(logdet),
               C.byref(pivot), C.byref(info)]
        res = {}
        if forces is None:
            check(lib().bioen_laplace_forces(self._h, None, None, 0.0, *(out + [None, None])))
        else:
            if w0 is None or theta is None:
                raise ValueError("forces_laplace with forces needs w0 and theta")
            fo, w0 = self._mvec(forces, "forces"), self._nvec(w0, "w0")
            f = C.c_double(0.0)
            grad = np.empty(m)
            check(lib().bioen_laplace_forces(self._h, ptr(fo), ptr(w0), float(theta), *(out + [C.byref(f), ptr(grad)])))
            res.update(f=f.value, grad=grad)
        ok = info.value == 0
        res.update(info=info.value, logdet_H=logdet.value, min_pivot=pivot.value,
                   std_forces=sf if ok else None, std_averages=sa if ok else None, var_logw=vl if ok else None,
                   cov_forces=cf if ok else None, cov_averages=ca if ok else None)
        return res

    def forces_colquad(self, P, forces=None, w0=None, theta=None):
        """v[j] = a_j^T P a_j for every structure j, a_j = y_j - ybar the structure's observables (of the affine model if one
        is set) centred on the averages under the point's weights, P a symmetric (m, m) matrix: ONE compute-bound pass
        over the matrix (M <= 1024).  Since d ln w_j / d forces = a_j, P = inv(H) gives the Laplace variance of ln w_j
        (forces.laplace_error_bars), P = inv(C) a structure's Mahalanobis distance from the refined ensemble, P = I its
        spread.  With `forces` (and w0, theta) the point is evaluated first, as by forces_fdf -- f and grad are its bits --,
        and kept on the context: -> (v, f, grad).  Without, at the point the last such call (or forces_hessp / forces_gram
        with forces) left: -> v; BioenHipError (invalid state) as forces_hessp raises it.  ValueError for a P of the wrong
        shape or one that is not symmetric (|P_ij - P_ji| > 1e-12 max |P|).  The first call allocates a device buffer of
        16-padded m^2 + n doubles that stays with the context (footprint(): "forces_colquad")."""
        fn = lib().bioen_hip_forces_colquad
        m = self.m
        Pa = as_f64(P)
        if Pa.shape != (m, m):
            raise ValueError("P must be (M, M) with M = %d, got %s" % (m, (Pa.shape,)))
        if np.abs(Pa - Pa.T).max() > 1e-12 * np.abs(Pa).max():      # (the entry's own gate; non-finite entries pass, as there)
            raise ValueError("P is not symmetric: max |P - P^T| = %.3g, max |P| = %.3g"
                             % (np.abs(Pa - Pa.T).max(), np.abs(Pa).max()))
        v = np.empty(self.n)
        if forces is None:
            check(fn(self._h, None, None, 0.0, ptr(Pa), ptr(v), None, None))
            return v
        if w0 is None or theta is None:
            raise ValueError("forces_colquad with forces needs w0 and theta")
        fo, w0 = self._mvec(forces, "forces"), self._nvec(w0, "w0")
        f = C.c_double(0.0)
        grad = np.empty(m)
        check(fn(self._h, ptr(fo), ptr(w0), float(theta), ptr(Pa), ptr(v), C.byref(f), ptr(grad)))
        return v, f.value, grad

    def forces_fdf_batch(self, forces, w0, thetas, need_grad=True):
        """K <= 8 evaluations sharing every matrix pass.  forces: (K, m), thetas: (K,) -> (f[K], grad[K, m] or None).
        Every column is the single call's result bit for bit, with or without an affine model."""
        thetas = as_f64(thetas).ravel()
        k = thetas.size
        fo = as_f64(forces).reshape(k, self.m)
        w0 = self._nvec(w0, "w0")
        f = np.empty(k)
        grad = np.empty((k, self.m)) if need_grad else None
        check(lib().bioen_hip_forces_fdf_batch(self._h, k, ptr(fo), ptr(w0), ptr(thetas), ptr(f),
                                               ptr(grad) if need_grad else None))
        return f, grad

    def opt_lbfgs_forces(self, forces0, w0, theta, params, verbose=False, debug=False, want_weights=True):
        """L-BFGS on the forces objective (of the affine model if one is set) -> (forces, weights or None, OptResult);
        last_average() then hands out the averages at the returned point (nuisance.series_forces refits on them)"""
        f0, w0 = self._mvec(forces0, "forces0"), self._nvec(w0, "w0")
        cfg = lbfgs_config(params)
        vis = VisualParams(int(bool(debug)), int(bool(verbose)))
        res = np.empty(self.m)
        w = np.empty(self.n) if want_weights else None
        info = OptResult()
        check(lib().bioen_hip_opt_lbfgs_forces(self._h, ptr(f0), ptr(w0), float(theta), C.byref(cfg), C.byref(vis),
                                               ptr(res), ptr(w) if want_weights else None, C.byref(info)))
        return res, w, info

    def opt_gsl_forces(self, forces0, w0, theta, algorithm, params, verbose=False, debug=False, want_weights=True):
        """the GSL-style minimizers on the forces objective (of the affine model if one is set)"""
        f0, w0 = self._mvec(forces0, "forces0"), self._nvec(w0, "w0")
        cfg = gsl_config(algorithm, params)
        vis = VisualParams(int(bool(debug)), int(bool(verbose)))
        res = np.empty(self.m)
        w = np.empty(self.n) if want_weights else None
        info = OptResult()
        check(lib().bioen_hip_opt_gsl_forces(self._h, ptr(f0), ptr(w0), float(theta), C.byref(cfg), C.byref(vis),
                                             ptr(res), ptr(w) if want_weights else None, C.byref(info)))
        return res, w, info

    def opt_lbfgs_forces_batch(self, thetas, forces0, w0, params, max_batch=8, verbose=False, debug=False,
                               want_weights=True):
        """theta series of the forces method; up to `max_batch` (<= 8) thetas share every matrix pass.
        forces0: (m,) shared start or (ntheta, m).  -> (forces[ntheta, m], weights[ntheta, n] or None, infos).
        An affine model (set_affine) applies to every theta of the series."""
        thetas = as_f64(thetas).ravel()
        nt = thetas.size
        f0 = as_f64(forces0)
        if f0.size == self.m:
            f0, stride = f0.ravel(), 0
        elif f0.shape == (nt, self.m):
            stride = self.m
        else:
            raise ValueError("forces0 must have shape (m,) or (ntheta, m)")
        w0 = self._nvec(w0, "w0")
        cfg = lbfgs_config(params)
        vis = VisualParams(int(bool(debug)), int(bool(verbose)))
        res = np.empty((nt, self.m))
        w = np.empty((nt, self.n)) if want_weights else None
        infos = (OptResult * nt)()
        check(lib().bioen_hip_opt_lbfgs_forces_batch(self._h, nt, ptr(thetas), ptr(f0), stride, ptr(w0), C.byref(cfg),
                                                     C.byref(vis), int(max_batch), ptr(res),
                                                     ptr(w) if want_weights else None, infos))
        return res, w, list(infos)

    # -- shared -------------------------------------------------------------------
    def last_average(self):
        """(yraw, yeff) of the most recent single-problem call on this context: yraw = yTilde . w of the
        resident matrix at the point that call ended on, yeff = row_offset + row_scale * yraw.  Only
        2 m doubles cross PCIe (no weights)."""
        yraw, yeff = np.empty(self.m), np.empty(self.m)
        check(lib().bioen_hip_last_average(self._h, ptr(yraw), ptr(yeff)))
        return yraw, yeff

    def chi_squared(self, w):
        """-> (0.5 |y_eff - YTilde|^2, yave).  With an affine row model set (set_affine) chi^2 is that of the
        effective observables off + sc * (yTilde . w), while yave is the RAW product yTilde . w of the
        resident matrix (what a nuisance refit needs); last_average() returns both."""
        w = self._nvec(w, "w")
        yave = np.empty(self.m)
        chi2 = C.c_double(0.0)
        check(lib().bioen_hip_chi_squared(self._h, ptr(w), ptr(yave), C.byref(chi2)))
        return chi2.value, yave

    # -- measurement ---------------------------------------------------------------
    def kernel_stats_enable(self, on=True):
        check(lib().bioen_hip_kernel_stats_enable(self._h, 1 if on else 0))

    def kernel_stats_reset(self):
        check(lib().bioen_hip_kernel_stats_reset(self._h))

    def kernel_stats(self):
        out = {}
        for which, name in ((0, "forward"), (1, "adjoint"), (2, "hessp_dots"), (3, "hessp_tangent"), (4, "hessp_combine"),
                            (5, "hessp_epilogue"), (6, "forces_hessp_tangent"), (7, "forces_hessp_product")):
            ms = C.c_double(0.0)
            cnt = C.c_longlong(0)
            pp = C.c_longlong(0)
            check(lib().bioen_hip_kernel_stats_ex(self._h, which, C.byref(ms), C.byref(cnt), C.byref(pp)))
            out[name] = {"total_ms": ms.value, "launches": cnt.value, "problem_passes": pp.value}
        return out

    def speculation_stats(self):
        """(issued, adopted): speculative line-search evaluations of the batch engines (both methods) so far"""
        a, b = C.c_longlong(0), C.c_longlong(0)
        check(lib().bioen_hip_speculation_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- RCCL ------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_ubyte * 128)()
        check(lib().bioen_hip_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check(lib().bioen_hip_comm_init(self._h, buf, int(rank), int(nranks)))

    def set_force_exchange(self, on=True):
        """world = 1 only: execute the stage all-gathers of the sharded code path anyway (needs comm_init(id, 0, 1)
        or set_exchange); results do not change by a bit.  Puts the RCCL stage path under single-GPU tests."""
        check(lib().bioen_hip_ctx_set_force_exchange(self._h, 1 if on else 0))

    def set_mirror_exchange(self, on=True):
        """Measurement aid: the stage all-gathers of this rank-r-of-world context copy ITS part over every other rank's --
        the work one rank of a `world`-GPU run does per round, alone on one GPU (include/bioen_hip.h)."""
        check(lib().bioen_hip_ctx_set_mirror_exchange(self._h, 1 if on else 0))

    def exchange_counts(self):
        """(through RCCL, through the host callback): stage all-gathers executed on this context so far"""
        a, b = C.c_longlong(0), C.c_longlong(0)
        check(lib().bioen_hip_exchange_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exchange_probe(self, count=1024, reps=50):
        """microseconds per stage exchange (all-gather of `count` doubles per rank)"""
        us = C.c_double(0.0)
        check(lib().bioen_hip_exchange_probe(self._h, int(count), int(reps), C.byref(us)))
        return us.value

    def read_probe(self, reps=10, form=0):
        """-> (GB/s of a plain read-only stream over the resident matrix, its bytes): the box's measured read ceiling.
        form: 0 = whichever is resident, 1 = row-major, 2 = row-sum strips, 4 = column-sum strips"""
        gbs, nbytes = C.c_double(0.0), C.c_longlong(0)
        check(lib().bioen_hip_read_probe(self._h, int(form), int(reps), C.byref(gbs), C.byref(nbytes)))
        return gbs.value, nbytes.value

    def comm_destroy(self):
        check(lib().bioen_hip_comm_destroy(self._h))

    # -- peer-to-peer stage exchange (hipIpc mailboxes, one kernel per all-gather) ------------------
    def p2p_export(self):
        """64-byte hipIpc handle of this rank's mailbox (allocated on first call)"""
        buf = (C.c_ubyte * 64)()
        check(lib().bioen_hip_p2p_export(self._h, buf))
        return bytes(buf)

    def p2p_attach(self, handles):
        """handles: the `world` mailbox handles in rank order (this rank's own is ignored); None for world = 1"""
        if handles is None:
            check(lib().bioen_hip_p2p_attach(self._h, None))
            return
        blob = b"".join(bytes(h) for h in handles)
        if len(blob) != 64 * self.world:
            raise ValueError("p2p_attach needs world = %d handles of 64 bytes" % self.world)
        buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
        check(lib().bioen_hip_p2p_attach(self._h, buf))

    def p2p_detach(self):
        check(lib().bioen_hip_p2p_detach(self._h))

    TRANSPORTS = {0: "none", 1: "rccl", 2: "host", 3: "p2p"}

    def exchange_transport(self):
        """'none' | 'rccl' | 'host' | 'p2p': what the next stage exchange of this context goes through"""
        return self.TRANSPORTS[lib().bioen_hip_exchange_transport(self._h)]

    def exchange_selftest(self, reps=40):
        """`reps` back-to-back stage exchanges of varying size with a (rank, exchange, index) pattern, checked on the
        device; -> number of wrong doubles (0 = the active transport delivers)"""
        bad = C.c_longlong(0)
        check(lib().bioen_hip_exchange_selftest(self._h, int(reps), C.byref(bad)))
        return bad.value

    def exchange_counts3(self):
        """(RCCL, host callback, peer-to-peer): stage all-gathers executed on this context so far"""
        a, b, c3 = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(lib().bioen_hip_exchange_counts3(self._h, C.byref(a), C.byref(b), C.byref(c3)))
        return a.value, b.value, c3.value

    def set_wait_timeout(self, seconds):
        """bound (s) of every wait on a round or a peer; past it the call fails instead of hanging"""
        check(lib().bioen_hip_ctx_set_wait_timeout(self._h, float(seconds)))

    def comm_allgather(self, send, nranks):
        send = as_f64(send).ravel()
        recv = np.empty(send.size * nranks)
        check(lib().bioen_hip_comm_allgather(self._h, ptr(send), send.size, ptr(recv)))
        return recv.reshape(nranks, send.size)

"""What every entry of the C ABI does to the two pieces of state other calls must respect: the point of
the Hessian-vector products and the dense BFGS session.  One row per entry that takes a context: ENTRIES below, and the
ENTRIES of every tests/test_abi_<feature>.py (found by glob: a new feature brings its rows in a new file of that name, and
nothing here is edited); the CPU test keeps their union complete against include/bioen_hip.h, the GPU tests here check
every row of ENTRIES below that one process on one GPU can run, the feature files theirs.  The rows were written from the
sources BEFORE the entries got their common guard and hold for both."""
import ctypes as C
import glob
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, LBFGS_DEFAULTS
from entry_rules import ALPHA, BETA, P, Row, estate

HEADER = os.path.join(ROOT, "include", "bioen_hip.h")

LBFGS_SHORT = dict(LBFGS_DEFAULTS, max_iterations=3)
GSL_SHORT = dict(step_size=0.01, tol=0.1, max_iterations=2)


def raw(name, *args):
    """-> a call of the raw binding: the context's handle first, the return code checked"""
    def call(c):
        from bioen_amd import _lib
        _lib.check(getattr(_lib.lib(), name)(c._h, *args))
    return call


def _shape(c):
    m, n = C.c_int(0), C.c_int(0)
    raw("bioen_hip_ctx_shape", C.byref(m), C.byref(n))(c)
    assert (m.value, n.value) == (c.m, c.n_local)


def _kernel_stats(c):
    ms, cnt = C.c_double(0.0), C.c_longlong(0)
    raw("bioen_hip_kernel_stats", 0, C.byref(ms), C.byref(cnt))(c)


def _pass_probe(c):
    f, a = C.c_double(0.0), C.c_double(0.0)
    raw("bioen_hip_debug_pass_probe", 1, 1, C.byref(f), C.byref(a))(c)


def _p():
    return P.get()


ENTRIES = {
    # ---- queries and settings: nothing on the device, nothing to the state
    "bioen_hip_ctx_set_exchange_callback": Row("keeps", "keeps", lambda c: c.set_exchange(None)),
    "bioen_hip_ctx_shard": Row("keeps", "keeps", lambda c: c._query_shard()),
    "bioen_hip_ctx_set_force_exchange": Row("keeps", "keeps", lambda c: c.set_force_exchange(False)),
    "bioen_hip_ctx_set_mirror_exchange": Row("keeps", "keeps", lambda c: c.set_mirror_exchange(False)),
    "bioen_hip_exchange_counts": Row("keeps", "keeps", lambda c: c.exchange_counts()),
    "bioen_hip_exchange_counts3": Row("keeps", "keeps", lambda c: c.exchange_counts3()),
    "bioen_hip_exchange_transport": Row("keeps", "keeps", lambda c: c.exchange_transport()),
    "bioen_hip_ctx_shape": Row("keeps", "keeps", _shape),
    "bioen_hip_ctx_footprint": Row("keeps", "keeps", lambda c: c.footprint()),
    "bioen_hip_ctx_layout": Row("keeps", "keeps", lambda c: c.layout()),
    "bioen_hip_ctx_strip_plan": Row("keeps", "keeps", lambda c: (c.strip_plan(0), c.strip_plan(1))),
    "bioen_hip_ctx_set_direction_mode": Row("keeps", "keeps", lambda c: c.set_direction_mode("auto")),
    "bioen_hip_ctx_set_wait_timeout": Row("keeps", "keeps", lambda c: c.set_wait_timeout(30.0)),
    "bioen_hip_kernel_stats_enable": Row("keeps", "keeps", lambda c: c.kernel_stats_enable(False)),
    "bioen_hip_speculation_stats": Row("keeps", "keeps", lambda c: c.speculation_stats()),
    "bioen_hip_comm_destroy": Row("keeps", "keeps", lambda c: c.comm_destroy()),
    # ---- device work that leaves the state alone
    "bioen_hip_synchronize": Row("keeps", "keeps", lambda c: c.synchronize()),
    "bioen_hip_ctx_read_ytilde": Row("keeps", "keeps", lambda c: c.read_ytilde(1, 3, 5, 7)),
    "bioen_hip_last_average": Row("keeps", "keeps", lambda c: c.last_average()),
    "bioen_hip_kernel_stats": Row("keeps", "keeps", _kernel_stats),
    "bioen_hip_kernel_stats_ex": Row("keeps", "keeps", lambda c: c.kernel_stats()),
    "bioen_hip_kernel_stats_reset": Row("keeps", "keeps", lambda c: c.kernel_stats_reset()),
    "bioen_hip_debug_strip_stamps": Row("keeps", "keeps", raw("bioen_hip_debug_strip_stamps", 0, None, 0)),
    "bioen_hip_exchange_probe": Row("keeps", "keeps", lambda c: c.exchange_probe(8, 1)),
    "bioen_hip_exchange_selftest": Row("keeps", "keeps", lambda c: c.exchange_selftest(2)),
    "bioen_hip_read_probe": Row("keeps", "keeps", lambda c: c.read_probe(1)),
    "bioen_hip_p2p_export": Row("keeps", "keeps", lambda c: c.p2p_export()),
    "bioen_hip_p2p_attach": Row("keeps", "keeps", lambda c: c.p2p_attach(None), prepare=lambda c: c.p2p_export()),
    "bioen_hip_p2p_detach": Row("keeps", "keeps", lambda c: c.p2p_detach()),
    # ---- changes of the matrix state: the point goes, a session stays
    "bioen_hip_ctx_set_ytilde_target": Row("drops", "keeps", lambda c: c.set_target(_p().YT)),
    "bioen_hip_ctx_set_affine": Row("drops", "keeps", lambda c: c.set_affine(None, None)),
    "bioen_hip_ctx_set_storage": Row("drops", "keeps", lambda c: c.set_storage("f64")),
    "bioen_hip_ctx_set_one_copy": Row("drops", "keeps", lambda c: c.set_one_copy(False)),
    "bioen_hip_debug_pass_probe": Row("drops", "keeps", _pass_probe),
    # ---- evaluations and optimisers: the point goes, a session ends
    "bioen_hip_logw_weights": Row("drops", "ends", lambda c: c.logw_weights(_p().x)),
    "bioen_hip_logw_fdf": Row("drops", "ends", lambda c: c.logw_fdf(_p().x, _p().G, _p().theta)),
    "bioen_hip_chi_squared": Row("drops", "ends", lambda c: c.chi_squared(_p().w0)),
    "bioen_hip_opt_lbfgs_logw": Row("drops", "ends", lambda c: c.opt_lbfgs_logw(_p().x, _p().G, _p().theta, LBFGS_SHORT)),
    "bioen_hip_opt_lbfgs_logw_batch": Row("drops", "ends", lambda c: c.opt_lbfgs_logw_batch([10.0, 1.0], _p().x, _p().G,
                                                                                           LBFGS_SHORT)),
    "bioen_hip_opt_gsl_logw": Row("drops", "ends", lambda c: c.opt_gsl_logw(_p().x, _p().G, _p().theta, "bfgs2", GSL_SHORT)),
    "bioen_hip_forces_weights": Row("drops", "ends", lambda c: c.forces_weights(_p().f0, _p().w0)),
    "bioen_hip_forces_fdf": Row("drops", "ends", lambda c: c.forces_fdf(_p().f0, _p().w0, _p().theta)),
    "bioen_hip_forces_fdf_batch": Row("drops", "ends", lambda c: c.forces_fdf_batch(np.zeros((2, _p().m)), _p().w0, [10.0, 1.0])),
    "bioen_hip_opt_lbfgs_forces": Row("drops", "ends", lambda c: c.opt_lbfgs_forces(_p().f0, _p().w0, _p().theta, LBFGS_SHORT)),
    "bioen_hip_opt_lbfgs_forces_batch": Row("drops", "ends", lambda c: c.opt_lbfgs_forces_batch([10.0, 1.0], _p().f0, _p().w0,
                                                                                               LBFGS_SHORT)),
    "bioen_hip_opt_gsl_forces": Row("drops", "ends", lambda c: c.opt_gsl_forces(_p().f0, _p().w0, _p().theta, "bfgs2", GSL_SHORT)),
    # ---- Hessian-vector products: with g the call is an evaluation that leaves a new point; without g it serves the kept one
    "bioen_hip_logw_hessp": [Row("sets", "ends", lambda c: c.logw_hessp(_p().v, g=_p().x, G=_p().G, theta=_p().theta)),
                             Row("needs", "keeps", lambda c: c.logw_hessp(_p().v))],
    # ---- the BFGS session: every call of it drops the point, with or without a session to serve
    "bioen_hip_bfgs_logw_begin": Row("drops", "starts", lambda c: c.bfgs_begin(_p().x, _p().G, _p().theta)),
    "bioen_hip_bfgs_logw_trial": Row("drops", "needs", lambda c: c.bfgs_trial(BETA, True)),
    "bioen_hip_bfgs_logw_accept": Row("drops", "needs", lambda c: c.bfgs_accept(ALPHA)),
    "bioen_hip_bfgs_logw_update": Row("drops", "needs", lambda c: c.bfgs_update(), prepare=lambda c: c.bfgs_accept(ALPHA)),
    "bioen_hip_bfgs_logw_end": Row("drops", "needs", lambda c: c.bfgs_end(), closes=True),
    "bioen_hip_bfgs_logw_read_hinv": Row("drops", "needs", lambda c: c.bfgs_read_hinv(0, 2)),
    "bioen_hip_bfgs_logw_read_vec": Row("drops", "needs", lambda c: c.bfgs_read_vec("p")),
    # ---- not runnable here (none of them evaluates, optimises, starts or serves a session, or changes the matrix state)
    "bioen_hip_ctx_destroy": Row("keeps", "keeps", None, why="ends the context itself; nothing is left to ask"),
    "bioen_hip_comm_init": Row("keeps", "keeps", None, why="needs the ranks of an RCCL communicator (seconds to set up)"),
    "bioen_hip_comm_allgather": Row("keeps", "keeps", None, why="needs an initialised RCCL communicator"),
}

NO_CONTEXT = {
    "bioen_hip_version", "bioen_hip_device_count", "bioen_hip_strerror", "bioen_hip_last_error", "bioen_hip_lbfgs_strerror",
    "bioen_hip_gsl_strerror", "bioen_hip_set_fast_openmp_flag", "bioen_hip_get_fast_openmp_flag",
    "bioen_hip_ctx_create", "bioen_hip_ctx_create_synthetic", "bioen_hip_ctx_create_sharded",
    "bioen_hip_ctx_create_synthetic_sharded", "bioen_hip_ctx_create_raw",
    "bioen_hip_selftest_lbfgs", "bioen_hip_selftest_multimin", "bioen_hip_multimin_host",
    "bioen_hip_comm_unique_id", "bioen_hip_comm_init_abandoned",
}


def rows():
    for name, r in sorted(ENTRIES.items()):
        for i, row in enumerate(r if isinstance(r, list) else (r,)):
            if row.how is not None:                         # (the others: classified, with the reason in the row)
                yield pytest.param(row, id=name[len("bioen_hip_"):] + ("-%d" % i if isinstance(r, list) else ""))


def declared_entries():
    """-> {name: takes a context} of include/bioen_hip.h (parsed as tests/test_abi.py does); the `bioen_hip_ctx**` of the
    create functions is a result, not a context to act on"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: re.search(r"\bbioen_hip_ctx\s*\*(?!\s*\*)", args) is not None
            for name, args in re.findall(r"\b(bioen_\w+)\s*\(([^()]*)\)", src)}


def all_entries():
    """-> {name: rows}: ENTRIES above with the ENTRIES of every tests/test_abi_<feature>.py, the modules found by glob and
    loaded by path (one that pytest has imported already is taken as it is); no entry has rows in two places"""
    out, owner = dict(ENTRIES), dict.fromkeys(ENTRIES, "test_entry_effects")
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_abi_*.py"))):
        stem = os.path.splitext(os.path.basename(path))[0]
        mod = sys.modules.get(stem)
        if mod is None or os.path.abspath(getattr(mod, "__file__", "")) != os.path.abspath(path):
            spec = importlib.util.spec_from_file_location(stem, path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        assert isinstance(getattr(mod, "ENTRIES", None), dict), "%s has no ENTRIES" % stem
        for name, r in mod.ENTRIES.items():
            assert name not in out, "%s has rows in %s and in %s" % (name, owner[name], stem)
            out[name], owner[name] = r, stem
    return out


def test_every_entry_is_classified():
    decl = declared_entries()
    assert decl["bioen_hip_logw_fdf"] and not decl["bioen_hip_ctx_create"]
    with_ctx = {n for n, takes in decl.items() if takes}
    entries = all_entries()
    assert not with_ctx - set(entries), "takes a context, but has no row in an ENTRIES (here or in a tests/test_abi_*.py): %s" % sorted(
        with_ctx - set(entries))
    assert not set(decl) - with_ctx - NO_CONTEXT, "not in NO_CONTEXT: %s" % sorted(set(decl) - with_ctx - NO_CONTEXT)
    assert not set(entries) - with_ctx, "in ENTRIES, but no declared entry with a context: %s" % sorted(set(entries) - with_ctx)
    assert not NO_CONTEXT - (set(decl) - with_ctx), "in NO_CONTEXT, but no declared entry without a context: %s" % sorted(
        NO_CONTEXT - (set(decl) - with_ctx))
    assert len(decl) >= 86          # (after the comparisons, so that an entry that went missing is named by them)
    for name, r in entries.items():     # (a feature file holds its own rows to narrower conditions besides: EntryRules.check_classified)
        for row in (r if isinstance(r, list) else (r,)):
            assert row.point in ("keeps", "drops", "sets", "needs") and row.session in ("keeps", "ends", "needs", "starts")
            assert (row.how is None) == (row.why is not None), name
            if row.how is None:     # the condition on what may stay unexercised
                assert (row.point, row.session) == ("keeps", "keeps"), name


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


@pytest.mark.gpu
@pytest.mark.parametrize("row", rows())
def test_effect_on_the_point(bioen_amd, row):
    p = P.get()
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hv, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        assert np.array_equal(ctx.logw_hessp(p.v), hv)
        if row.session == "needs":                          # no session to serve: refused, and the point is gone all the same
            estate(lambda: row.how(ctx), "no BFGS session")
        else:
            if row.prepare:
                row.prepare(ctx)
            row.how(ctx)
        if row.point == "drops":
            estate(lambda: ctx.logw_hessp(p.v), "is gone")
        else:
            assert np.array_equal(ctx.logw_hessp(p.v), hv)  # the same bits at the kept (sets: the same, new) point


@pytest.mark.gpu
@pytest.mark.parametrize("row", rows())
def test_effect_on_a_session(bioen_amd, row):
    p = P.get()
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        ctx.logw_fdf(p.x, p.G, p.theta)                     # the matrix takes its evaluation form first
        start = ctx.footprint()
        ctx.bfgs_begin(p.x, p.G, p.theta)
        ctx.bfgs_trial(ALPHA, True)
        assert "bfgs_hinv" in ctx.footprint()[0]
        if row.prepare:
            row.prepare(ctx)
        if row.point == "needs":                            # (the session's own calls have dropped every point)
            estate(lambda: row.how(ctx))
        else:
            row.how(ctx)
        if row.session == "ends":
            estate(lambda: ctx.bfgs_trial(BETA, False), "ended by another call")
            assert ctx.footprint() == start
        elif row.closes:
            estate(lambda: ctx.bfgs_trial(BETA, False), "no BFGS session")
            assert ctx.footprint() == start
        else:
            f, _ = ctx.bfgs_trial(2 * BETA, False)
            assert np.isfinite(f)


@pytest.mark.gpu
def test_a_rejected_call_has_its_effects_all_the_same(bioen_amd):
    """bioen_hip_logw_fdf without g: BIOEN_HIP_EINVAL (-1) -- and the point and the session are gone, as they always were"""
    from bioen_amd import _lib
    p = P.get()
    f = C.c_double(0.0)
    for with_session in (False, True):
        with bioen_amd.Context(p.yT, p.YT) as ctx:
            ctx.logw_fdf(p.x, p.G, p.theta)
            start = ctx.footprint()
            if with_session:
                ctx.bfgs_begin(p.x, p.G, p.theta)
                ctx.bfgs_trial(ALPHA, True)
            else:
                ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
            rc = _lib.lib().bioen_hip_logw_fdf(ctx._h, None, _lib.ptr(p.G), p.theta, C.byref(f), None)
            assert rc == -1
            if with_session:
                estate(lambda: ctx.bfgs_trial(BETA, False), "ended by another call")
                assert ctx.footprint() == start
            else:
                estate(lambda: ctx.logw_hessp(p.v), "is gone")

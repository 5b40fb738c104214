"""The dual Newton theta series with the nuisance scales profiled out, bioen_logwn_profile_series, held to
the rules of tests/entry_rules.py as tests/test_abi_logw_series.py holds the entry it builds on: declared in
include/bioen_hip.h, a C caller (examples/logw_profile_demo.c) compiles against it as plain C, links and runs, the binding
has the header's argument list, and the entry has its effect row (tests/test_entry_effects.py reads it
from here), exercised on the GPU on a LOG-WEIGHTS point."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT
from entry_rules import EntryRules, P, Row, bioen_amd, estate      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_logwn_profile_series"]


def _p():
    return P.get()


def _groups():
    m = _p().m
    return [np.arange(0, m // 2), np.arange(m // 2, m - 4)]


# the row of DESIGN section 6c: the series evaluates, and leaves the last theta's returned point as the new point.  The
# call leaves an affine model; removing it (a change of the matrix state) drops the point
ENTRIES = {
    "bioen_logwn_profile_series": [
        Row("sets", "ends", lambda c: c.opt_dual_newton_logw_profile_series([10.0, _p().theta], _p().x, _p().G,
                                                                            dict(max_iterations=2), groups=_groups(),
                                                                            hessian="gram_bf16")),
    ],
}

RULES = EntryRules(NAMES, "logw_profile_demo", ENTRIES, points=("sets", "needs"))


def test_entries_are_declared_and_classified():
    """(exported and bound: tests/test_abi.py, for every declared name at once)"""
    assert not set(NAMES) - set(declared_functions())
    RULES.check_classified()


def test_binding_has_the_headers_argument_list():
    from bioen_amd import _lib
    with open(ROOT + "/include/bioen_hip.h") as f:
        text = f.read()
    decl = re.search(r"int bioen_logwn_profile_series\((.*?)\);", text, re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    restype, argtypes = _lib._SIGNATURES["bioen_logwn_profile_series"]
    assert restype is C.c_int and len(argtypes) == len(args) == 16

    def kind(a):
        if a.startswith("bioen_hip_ctx*"):
            return _lib.ctx_p
        if "bioen_logwn_config*" in a:
            return C.POINTER(_lib.LogwNewtonConfig)
        if "bioen_logwn_series_result*" in a:
            return C.POINTER(_lib.LogwNewtonSeriesResult)
        if "double*" in a:
            return _lib.dp
        if "int*" in a:
            return _lib.ip
        assert a.startswith("int "), a
        return C.c_int
    assert [kind(a) for a in args] == list(argtypes)
    # the series' result struct and sources are the entry's (tests/test_abi_logw_series.py checks their layout)
    assert _lib.logw_newton_source("gram") == 0 and _lib.logw_newton_source("gram_bf16") == 1


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_profiled_series(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """`sets` leaves a new log-weights point -- the returned one, on the model the call left --, replaces a forces point, and
    an evaluation drops it"""
    p = P.get()
    f = 1e-3 * np.random.default_rng(3).standard_normal(p.m)
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        hv, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        row.how(ctx)
        assert not np.array_equal(ctx.logw_hessp(p.v), hv)                  # a product at the point the series left
        ctx.set_affine(None, None)
        estate(lambda: ctx.logw_hessp(p.v), "is gone", "bioen_hip_ctx_set_affine")
        ctx.forces_hessp(np.ones(p.m), forces=f, w0=p.w0, theta=p.theta)    # ... and on a FORCES point
        row.how(ctx)
        estate(lambda: ctx.forces_hessp(np.ones(p.m)), "log-weights point")
        ctx.logw_fdf(p.x, p.G, p.theta)                                     # an evaluation drops what it left
        estate(lambda: ctx.logw_cov(), "is gone", "bioen_hip_logw_fdf")


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

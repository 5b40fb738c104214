"""The log-weights theta series by dual Newton and the split-BF16 covariance, bioen_logwn_series and bioen_logwn_cov_bf16
(DESIGN section 6k), held to the rules of tests/entry_rules.py as tests/test_abi_logw_newton.py holds the two entries they
build on: declared in include/bioen_hip.h, a C caller (examples/logw_series_demo.c) compiles against it as plain C, links
and runs, the new struct has the layout of its ctypes class, and every entry has its effect rows (DESIGN section 6c;
tests/test_entry_effects.py reads them from here), exercised on the GPU on a LOG-WEIGHTS point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from entry_rules import EntryRules, P, Row, bioen_amd, estate      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_logwn_cov_bf16", "bioen_logwn_series"]


def _p():
    return P.get()


# the rows of DESIGN section 6c: the split-BF16 covariance is bioen_logwn_cov's; the series evaluates, and leaves the last
# theta's returned point as the new point
ENTRIES = {
    "bioen_logwn_cov_bf16": [
        Row("sets", "ends", lambda c: c.logw_cov_bf16(g=_p().x, G=_p().G, theta=_p().theta)),
        Row("needs", "keeps", lambda c: c.logw_cov_bf16()),
    ],
    "bioen_logwn_series": [
        Row("sets", "ends", lambda c: c.opt_dual_newton_logw_series([10.0, _p().theta], _p().x, _p().G,
                                                                    dict(max_iterations=2), hessian="gram_bf16")),
    ],
}

RULES = EntryRules(NAMES, "logw_series_demo", ENTRIES, points=("sets", "needs"))


def test_entries_are_declared_and_classified():
    """(exported and bound: tests/test_abi.py, for every declared name at once)"""
    assert not set(NAMES) - set(declared_functions())
    RULES.check_classified()


STRUCT_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bioen_hip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("bioen_logwn_series_result %zu\n", sizeof(bioen_logwn_series_result));
    F(bioen_logwn_series_result, fmin); F(bioen_logwn_series_result, gmax); F(bioen_logwn_series_result, wmax);
    F(bioen_logwn_series_result, status); F(bioen_logwn_series_result, iterations); F(bioen_logwn_series_result, evaluations);
    F(bioen_logwn_series_result, factorisations); F(bioen_logwn_series_result, bf16_passes);
    F(bioen_logwn_series_result, switched);
    return 0;
}
"""


def test_struct_layout_matches_the_ctypes_class(tmp_path):
    from bioen_amd import _lib
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(STRUCT_PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    cls = _lib.LogwNewtonSeriesResult
    want = {"bioen_logwn_series_result": str(C.sizeof(cls))}
    for field, _ in cls._fields_:
        want["bioen_logwn_series_result.%s" % field] = str(getattr(cls, field).offset)
    assert got == want
    # the common part is bioen_logwn_result's, field for field
    assert cls._fields_[:len(_lib.LogwNewtonResult._fields_)] == _lib.LogwNewtonResult._fields_
    assert _lib.logw_newton_source("gram") == 0 and _lib.logw_newton_source("GRAM_BF16") == 1
    with pytest.raises(RuntimeError, match="dual_newton:hessian=fp32 not recognized"):
        _lib.logw_newton_source("fp32")


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_series(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """`needs` serves the kept log-weights point, leaves it alone, and fails without one or on a forces point, naming the
    entry; `sets` leaves a new log-weights point: the covariance at the same g the same products, the series others"""
    p = P.get()
    f = 1e-3 * np.random.default_rng(3).standard_normal(p.m)
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        if row.point == "needs":
            estate(lambda: row.how(ctx), "no point on this context", "bioen_logwn_cov_bf16")
        hv, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        row.how(ctx)
        if row is ENTRIES["bioen_logwn_series"][0]:
            assert not np.array_equal(ctx.logw_hessp(p.v), hv)              # a product at the point the series left
        else:
            assert np.array_equal(ctx.logw_hessp(p.v), hv)                  # the same bits at the kept (sets: the same, new) point
        ctx.forces_hessp(np.ones(p.m), forces=f, w0=p.w0, theta=p.theta)    # ... and on a FORCES point
        if row.point == "needs":
            estate(lambda: row.how(ctx), "forces point", "bioen_logwn_cov_bf16")
            assert np.isfinite(ctx.forces_hessp(np.ones(p.m))).all()
        else:
            row.how(ctx)
            estate(lambda: ctx.forces_hessp(np.ones(p.m)), "log-weights point")
        ctx.logw_fdf(p.x, p.G, p.theta)                                     # an evaluation drops what they left
        estate(lambda: ctx.logw_cov_bf16(), "is gone", "bioen_hip_logw_fdf")


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

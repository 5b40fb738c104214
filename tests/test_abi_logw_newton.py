"""The log-weights method's dual Newton minimizer and the covariance it is built on, bioen_logwn_*, held to the rules of
tests/entry_rules.py: the entries are declared in include/bioen_hip.h, a C caller compiles against it as plain C and links,
their two structs have the layout of the ctypes classes, and every entry has its effect rows (DESIGN section 6c;
tests/test_entry_effects.py reads them from here), exercised on the GPU.  The point these entries set and need is a
LOG-WEIGHTS point, so the check of the effect on the point is this file's own (the rules' one starts from a forces point)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from entry_rules import EntryRules, P, Row, bioen_amd, estate      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_logwn_cov", "bioen_logwn_opt"]


def _p():
    return P.get()


# the rows of DESIGN section 6c for these entries: the covariance with g is an evaluation that leaves a new point, without it
# serves the kept log-weights point; the minimizer evaluates, and leaves its optimum as the new point
ENTRIES = {
    "bioen_logwn_cov": [
        Row("sets", "ends", lambda c: c.logw_cov(g=_p().x, G=_p().G, theta=_p().theta)),
        Row("needs", "keeps", lambda c: c.logw_cov()),
    ],
    "bioen_logwn_opt": [
        Row("sets", "ends", lambda c: c.opt_dual_newton_logw(_p().x, _p().G, _p().theta, dict(max_iterations=2))),
    ],
}

RULES = EntryRules(NAMES, "c_abi_logw_newton_demo", ENTRIES, points=("sets", "needs"))


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
    printf("bioen_logwn_config %zu\nbioen_logwn_result %zu\n", sizeof(bioen_logwn_config), sizeof(bioen_logwn_result));
    F(bioen_logwn_config, gtol); F(bioen_logwn_config, armijo); F(bioen_logwn_config, floor_ulps);
    F(bioen_logwn_config, max_iterations); F(bioen_logwn_config, max_halvings);
    F(bioen_logwn_result, fmin); F(bioen_logwn_result, gmax); F(bioen_logwn_result, wmax); F(bioen_logwn_result, status);
    F(bioen_logwn_result, iterations); F(bioen_logwn_result, evaluations); F(bioen_logwn_result, factorisations);
    return 0;
}
"""


def test_struct_layouts_match_the_ctypes_classes(tmp_path):
    from bioen_amd import _lib
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(STRUCT_PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    classes = {"bioen_logwn_config": _lib.LogwNewtonConfig, "bioen_logwn_result": _lib.LogwNewtonResult}
    want = {}
    for cname, cls in classes.items():
        want[cname] = str(C.sizeof(cls))
        for field, _ in cls._fields_:
            want["%s.%s" % (cname, field)] = str(getattr(cls, field).offset)
    assert got == want
    cfg = _lib.logw_newton_config(dict(gtol=1e-7))
    assert (cfg.gtol, cfg.max_iterations, cfg.armijo, cfg.floor_ulps, cfg.max_halvings) == (1e-7, 200, 1e-4, 8.0, 60)


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_loop(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """`needs` serves the kept log-weights point, leaves it alone, and fails without one or on a forces point, naming the
    entry; `sets` leaves a new log-weights point: at the same g the same products, after the optimiser others"""
    p = P.get()
    f = 1e-3 * np.random.default_rng(3).standard_normal(p.m)
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        if row.point == "needs":
            estate(lambda: row.how(ctx), "no point on this context", "bioen_logwn_cov")
        hv, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        row.how(ctx)
        if row is ENTRIES["bioen_logwn_opt"][0]:
            assert not np.array_equal(ctx.logw_hessp(p.v), hv)              # a product at the point the optimiser left
        else:
            assert np.array_equal(ctx.logw_hessp(p.v), hv)                  # the same bits at the kept (sets: the same, new) point
        ctx.forces_hessp(np.ones(p.m), forces=f, w0=p.w0, theta=p.theta)    # ... and on a FORCES point
        if row.point == "needs":
            estate(lambda: row.how(ctx), "forces point", "bioen_logwn_cov")
            assert np.isfinite(ctx.forces_hessp(np.ones(p.m))).all()
        else:
            row.how(ctx)
            estate(lambda: ctx.forces_hessp(np.ones(p.m)), "log-weights point")
        ctx.logw_fdf(p.x, p.G, p.theta)                                     # an evaluation drops what they left
        estate(lambda: ctx.logw_cov(), "is gone", "bioen_hip_logw_fdf")


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

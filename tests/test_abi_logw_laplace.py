"""The log-weights method's Laplace error bars, bioen_logwn_laplace, held to the rules of
tests/entry_rules.py as tests/test_abi_logw_newton.py holds the entries it builds on: declared in include/bioen_hip.h, a C
caller (examples/logw_laplace_demo.c) compiles against it as plain C, links and runs, and the entry has its effect rows
(tests/test_entry_effects.py reads them from here), exercised on the GPU on a LOG-WEIGHTS point."""
import numpy as np
import pytest

from entry_rules import EntryRules, P, Row, bioen_amd, estate      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_logwn_laplace"]


def _p():
    return P.get()


def _obs():
    return np.random.default_rng(5).standard_normal((2, _p().n))


# the rows of DESIGN section 6c: bioen_logwn_cov's -- with g an evaluation that leaves a new point, without it the kept
# log-weights point is served
ENTRIES = {
    "bioen_logwn_laplace": [
        Row("sets", "ends", lambda c: c.logw_laplace(g=_p().x, G=_p().G, theta=_p().theta, observables=_obs())),
        Row("needs", "keeps", lambda c: c.logw_laplace(theta=_p().theta, observables=_obs())),
    ],
}

RULES = EntryRules(NAMES, "logw_laplace_demo", ENTRIES, points=("sets", "needs"))


def test_entries_are_declared_and_classified():
    """(exported and bound: tests/test_abi.py, for every declared name at once)"""
    assert not set(NAMES) - set(declared_functions())
    RULES.check_classified()


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_error_bars(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """`needs` serves the kept log-weights point, leaves it alone, and fails without one or on a forces point, naming the
    entry; `sets` leaves a new log-weights point: at the same g the same products"""
    p = P.get()
    f = 1e-3 * np.random.default_rng(3).standard_normal(p.m)
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        if row.point == "needs":
            estate(lambda: row.how(ctx), "no point on this context", "bioen_logwn_laplace")
        hv, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        row.how(ctx)
        assert np.array_equal(ctx.logw_hessp(p.v), hv)                      # the same bits at the kept (sets: the same, new) point
        ctx.forces_hessp(np.ones(p.m), forces=f, w0=p.w0, theta=p.theta)    # ... and on a FORCES point
        if row.point == "needs":
            estate(lambda: row.how(ctx), "forces point", "bioen_logwn_laplace")
            assert np.isfinite(ctx.forces_hessp(np.ones(p.m))).all()
        else:
            row.how(ctx)
            estate(lambda: ctx.forces_hessp(np.ones(p.m)), "log-weights point")
        ctx.logw_fdf(p.x, p.G, p.theta)                                     # an evaluation drops what they left
        estate(lambda: ctx.logw_laplace(theta=p.theta), "is gone", "bioen_hip_logw_fdf")


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

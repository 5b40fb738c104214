"""The switch of the log-weights dual Newton's pass over row panels, bioen_hip_ctx_set_dense_panels,
held to the rules of tests/entry_rules.py: declared in include/bioen_hip.h, exported and bound, its effect row (DESIGN
section 6c; tests/test_entry_effects.py reads it from here) -- a setting: it keeps the point and a session -- exercised on
the GPU, and its argument check.  What the switch switches: tests/test_hip_logw_panels.py."""
import ctypes as C

import numpy as np
import pytest

from entry_rules import EntryRules, P, Row, bioen_amd      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_hip_ctx_set_dense_panels"]


def _toggle(c):
    c.set_dense_panels(True)
    c.set_dense_panels(False)


ENTRIES = {
    "bioen_hip_ctx_set_dense_panels": [Row("keeps", "keeps", _toggle)],
}

RULES = EntryRules(NAMES, None, ENTRIES, points=("keeps",))


def test_entry_is_declared_exported_and_classified():
    from bioen_amd import _lib
    assert not set(NAMES) - set(declared_functions())
    fn = getattr(C.CDLL(_lib.LIB_PATH), NAMES[0])           # exported by the library itself, not only bound
    assert fn is not None
    assert _lib._SIGNATURES[NAMES[0]][1][1:] == [C.c_int]
    RULES.check_classified()


@pytest.mark.gpu
def test_on_is_zero_or_one(bioen_amd):      # noqa: F811
    from bioen_amd import _lib
    p = P.get()
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        assert ctx.dense_panels is False
        for bad in (-1, 2, 7):
            assert _lib.lib().bioen_hip_ctx_set_dense_panels(ctx._h, bad) == -1       # BIOEN_HIP_EINVAL
            assert "0 or 1" in _lib.lib().bioen_hip_last_error().decode()
        ctx.set_dense_panels()
        assert ctx.dense_panels is True
        # M <= 1024 is served as before, on or off: the same bits
        Con, _, _ = ctx.logw_cov(g=p.x, G=p.G, theta=p.theta)
        ctx.set_dense_panels(False)
        assert ctx.dense_panels is False
        assert np.array_equal(ctx.logw_cov(), Con)            # (the point was kept)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_the_point(bioen_amd, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

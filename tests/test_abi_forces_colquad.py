"""The fourth public header, include/bioen_hip_forces_colquad.h, held to the rules of tests/abi_header_rules.py: what it
declares is exported and bound (in _lib.py's fourth table, and in no other), it is plain C and a C caller links against it,
and every entry has an effect row that is exercised on the GPU."""
import numpy as np
import pytest

from abi_header_rules import HeaderRules, bioen_amd, f, v      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_entry_effects import P, Row

# the rows of DESIGN section 6c for this header: with forces the call is an evaluation that leaves a new point; without, it
# serves the kept one
ENTRIES = {
    "bioen_hip_forces_colquad": [
        Row("sets", "ends", lambda c: c.forces_colquad(np.eye(P.get().m), forces=f(), w0=P.get().w0, theta=P.get().theta)),
        Row("needs", "keeps", lambda c: c.forces_colquad(np.eye(P.get().m))),
    ],
}

RULES = HeaderRules("bioen_hip_forces_colquad.h", ["bioen_hip_forces_colquad"], "forces_colquad", "c_abi_forces_colquad_demo", ENTRIES)


def test_every_declared_symbol_is_exported_bound_and_classified():
    from bioen_amd import _lib
    names, _ = RULES.check_declared_exported_bound_and_classified()
    assert not set(names) & set(_lib.exported_symbols_forces_hessp())     # ... and the other three tables are their headers' alone
    assert not set(names) & set(_lib.exported_symbols_forces_gram())
    assert _lib.exported_symbols_forces_hessp() == ["bioen_hip_forces_hessp"]
    assert _lib.exported_symbols_forces_gram() == ["bioen_hip_forces_gram"]


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_pass(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """as tests/test_abi_forces_gram.py checks bioen_hip_forces_gram: `sets` leaves the same, new point, `needs` serves the
    kept one -- and fails without one; the point is the products' own"""
    RULES.check_effect_on_the_point(bioen_amd, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

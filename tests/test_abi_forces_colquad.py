"""One quadratic form per structure at a kept forces point, bioen_hip_forces_colquad, held to the rules of
tests/entry_rules.py: the entry is declared in include/bioen_hip.h, a C caller compiles against it as plain C and links, and
the entry has its effect rows (tests/test_entry_effects.py reads them from here), exercised on the GPU."""
import numpy as np
import pytest

from entry_rules import EntryRules, P, Row, bioen_amd, f, v      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_hip_forces_colquad"]

# the rows of DESIGN section 6c for this entry: with forces the call is an evaluation that leaves a new point; without, it
# serves the kept one
ENTRIES = {
    "bioen_hip_forces_colquad": [
        Row("sets", "ends", lambda c: c.forces_colquad(np.eye(P.get().m), forces=f(), w0=P.get().w0, theta=P.get().theta)),
        Row("needs", "keeps", lambda c: c.forces_colquad(np.eye(P.get().m))),
    ],
}

RULES = EntryRules(NAMES, "c_abi_forces_colquad_demo", ENTRIES)


def test_entries_are_declared_and_classified():
    """(exported and bound: tests/test_abi.py, for every declared name at once)"""
    assert not set(NAMES) - set(declared_functions())
    RULES.check_classified()


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

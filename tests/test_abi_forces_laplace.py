"""The Laplace error bars of the forces method without leaving the device, bioen_laplace_*, held to the rules of
tests/entry_rules.py: the entries are declared in include/bioen_hip.h, a C caller compiles against it as plain C and links,
and every entry has its effect rows (tests/test_entry_effects.py reads them from here), exercised on the
GPU."""
import numpy as np
import pytest

from entry_rules import EntryRules, P, Row, bioen_amd, f      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_laplace_forces", "bioen_laplace_forces_inverse"]


def _spd():
    m = P.get().m
    B = np.random.default_rng(4).standard_normal((m, m))
    return B.dot(B.T) / m + np.eye(m)


# the rows of DESIGN section 6c for these entries: the inverse keeps point and session (with A=None it needs a forces point);
# the error bars with forces are an evaluation that leaves a new point, without they serve the kept one
ENTRIES = {
    "bioen_laplace_forces_inverse": [
        Row("keeps", "keeps", lambda c: c.forces_inverse(_spd())),
        Row("needs", "keeps", lambda c: c.forces_inverse()),
    ],
    "bioen_laplace_forces": [
        Row("sets", "ends", lambda c: c.forces_laplace(forces=f(), w0=P.get().w0, theta=P.get().theta)),
        Row("needs", "keeps", lambda c: c.forces_laplace(matrices=False)),
    ],
}

RULES = EntryRules(NAMES, "c_abi_forces_laplace_demo", ENTRIES, points=("keeps", "sets", "needs"))


def test_entries_are_declared_and_classified():
    """(exported and bound: tests/test_abi.py, for every declared name at once)"""
    assert not set(NAMES) - set(declared_functions())
    RULES.check_classified()


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """`keeps` leaves the products' point alone, `needs` serves the kept forces point and fails without one, naming the entry,
    `sets` leaves a new forces point (the same forces: the same products)"""
    RULES.check_effect_on_the_point(bioen_amd, row, needles=("bioen_laplace_forces",))


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

"""The second public header, include/bioen_hip_forces_hessp.h, held to the rules of tests/abi_header_rules.py: what it
declares is exported and bound (in _lib.py's second table), it is plain C and a C caller links against it, and every entry
has an effect row that is exercised on the GPU."""
import pytest

from abi_header_rules import HeaderRules, bioen_amd, f, v      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_entry_effects import P, Row

# the rows of DESIGN section 6c for this header: with forces the call is an evaluation that leaves a new point; without, it
# serves the kept one
ENTRIES = {
    "bioen_hip_forces_hessp": [
        Row("sets", "ends", lambda c: c.forces_hessp(v(), forces=f(), w0=P.get().w0, theta=P.get().theta)),
        Row("needs", "keeps", lambda c: c.forces_hessp(v())),
    ],
}

RULES = HeaderRules("bioen_hip_forces_hessp.h", ["bioen_hip_forces_hessp"], "forces_hessp", "c_abi_forces_hessp_demo", ENTRIES)


def test_every_declared_symbol_is_exported_bound_and_classified():
    RULES.check_declared_exported_bound_and_classified()                  # (the first table is bioen_hip.h's alone: among the rules)


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_products(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """as tests/test_entry_effects.py checks bioen_hip_logw_hessp, on a forces point: `sets` leaves the same, new point,
    `needs` serves the kept one -- and fails without one"""
    RULES.check_effect_on_the_point(bioen_amd, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

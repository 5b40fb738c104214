"""The seventh public header, include/bioen_hip_forces_laplace.h, held to the rules of tests/abi_header_rules.py: what it
declares is exported and bound (in _lib.py's seventh table, and in no other), it is plain C and a C caller links against
it, and every entry has its effect rows, exercised on the GPU.  Its entries are bioen_laplace_*: the
bioen_hip_* names are closed over the six earlier tables (tests/test_abi_forces_newton.py), so the rules' pattern is
widened here."""
import re

import numpy as np
import pytest

from abi_header_rules import HeaderRules, bioen_amd, f      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_entry_effects import P, Row

PREFIX = "bioen_laplace_"
NAMES = ["bioen_laplace_forces", "bioen_laplace_forces_inverse"]


class LaplaceRules(HeaderRules):
    """the header's entries carry PREFIX where the rules expect bioen_hip_"""

    def declared_functions(self):
        src = re.sub(r"/\*.*?\*/", "", open(self.header).read(), flags=re.S)
        assert not re.findall(r"\b(bioen_hip_\w+)\s*\(", src)            # nothing of the closed namespace is declared here
        return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % PREFIX, src)))

    def rows(self):
        return [pytest.param(row, id="%s-%d" % (name[len(PREFIX):], i))
                for name in self.names for i, row in enumerate(self.entries[name])]


def _spd():
    m = P.get().m
    B = np.random.default_rng(4).standard_normal((m, m))
    return B.dot(B.T) / m + np.eye(m)


# the rows of DESIGN section 6c for this header: the inverse keeps point and session (with A=None it needs a forces point);
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

RULES = LaplaceRules("bioen_hip_forces_laplace.h", NAMES, "forces_laplace", "c_abi_forces_laplace_demo", ENTRIES,
                     points=("keeps", "sets", "needs"))


def test_every_declared_symbol_is_exported_bound_and_classified():
    from bioen_amd import _lib
    names, exported = RULES.check_declared_exported_bound_and_classified()
    others = (_lib.exported_symbols(), _lib.exported_symbols_forces_hessp(), _lib.exported_symbols_forces_gram(),
              _lib.exported_symbols_forces_colquad(), _lib.exported_symbols_forces_gram_bf16(),
              _lib.exported_symbols_forces_newton())
    for table in others:                                                  # the other six tables are their headers' alone
        assert not set(names) & set(table)
        assert not [n for n in table if n.startswith(PREFIX)]
    # the other direction: every bioen_hip_* or bioen_laplace_* symbol the library exports is bound in one of the seven tables
    bound = set(names).union(*others)
    assert not sorted(n for n in exported if n.startswith(("bioen_hip_", PREFIX)) and n not in bound)
    assert sorted(n for n in exported if n.startswith(PREFIX)) == NAMES


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

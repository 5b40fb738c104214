"""The device-resident Newton minimizer of the forces method, its factorisation and solves, held to the rules of
tests/entry_rules.py: the entries are declared in include/bioen_hip.h, a C caller compiles against it as plain C and links,
their two structs have the layout of the ctypes classes, and every entry has its effect rows (DESIGN section 6c;
tests/test_entry_effects.py reads them from here), exercised on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from entry_rules import EntryRules, P, Row, bioen_amd, f, v      # noqa: F401 -- bioen_amd is the GPU tests' fixture
from test_abi import declared_functions

NAMES = ["bioen_hip_forces_newton_factor", "bioen_hip_forces_newton_solve", "bioen_hip_opt_newton_forces"]


def _spd():
    m = P.get().m
    B = np.random.default_rng(4).standard_normal((m, m))
    return B.dot(B.T) / m + np.eye(m)


def _factor_then_solve(c):
    c.forces_newton_factor(_spd(), want_L=False)
    c.forces_newton_solve(v())


# the rows of DESIGN section 6c for these entries: the factorisation and the solve keep point and session (with A=None the
# factorisation needs a forces point); the minimizer evaluates, and leaves its optimum as the new point
ENTRIES = {
    "bioen_hip_forces_newton_factor": [
        Row("keeps", "keeps", lambda c: c.forces_newton_factor(_spd())),
        Row("needs", "keeps", lambda c: c.forces_newton_factor(None, source="gram")),
    ],
    "bioen_hip_forces_newton_solve": [Row("keeps", "keeps", _factor_then_solve)],
    "bioen_hip_opt_newton_forces": [
        Row("sets", "ends", lambda c: c.opt_newton_forces(f(), P.get().w0, P.get().theta, dict(max_iterations=2))),
    ],
}


RULES = EntryRules(NAMES, "c_abi_forces_newton_demo", ENTRIES, points=("keeps", "sets", "needs"))


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
    printf("bioen_newton_config %zu\nbioen_newton_result %zu\n", sizeof(bioen_newton_config), sizeof(bioen_newton_result));
    F(bioen_newton_config, gtol); F(bioen_newton_config, armijo); F(bioen_newton_config, rho_good);
    F(bioen_newton_config, lambda_factor); F(bioen_newton_config, lambda_first); F(bioen_newton_config, lambda_max);
    F(bioen_newton_config, lambda_zero); F(bioen_newton_config, floor_ulps); F(bioen_newton_config, max_iterations);
    F(bioen_newton_config, hessian);
    F(bioen_newton_result, fmin); F(bioen_newton_result, gmax); F(bioen_newton_result, lambda); F(bioen_newton_result, status);
    F(bioen_newton_result, iterations); F(bioen_newton_result, evaluations); F(bioen_newton_result, hessians);
    F(bioen_newton_result, factorisations); F(bioen_newton_result, switched);
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
    classes = {"bioen_newton_config": _lib.NewtonConfig, "bioen_newton_result": _lib.NewtonResult}
    want = {}
    for cname, cls in classes.items():
        want[cname] = str(C.sizeof(cls))
        for field, _ in cls._fields_:
            want["%s.%s" % (cname, "lambda" if field == "lam" else field)] = str(getattr(cls, field).offset)
    assert got == want
    cfg = _lib.newton_config(dict(hessian="gram_bf16", gtol=1e-7))
    assert (cfg.hessian, cfg.gtol, cfg.max_iterations, cfg.lambda_factor, cfg.floor_ulps) == (1, 1e-7, 200, 4.0, 8.0)
    with pytest.raises(RuntimeError, match="newton:hessian=products not recognized"):
        _lib.newton_config(dict(hessian="products"))


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    RULES.check_header_is_plain_c_and_a_c_caller_links(tmp_path)


@pytest.mark.gpu
def test_c_caller_runs_the_loop(tmp_path):
    RULES.check_c_caller_runs(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_the_point(bioen_amd, row):      # noqa: F811
    """`keeps` leaves the products' point alone, `needs` serves the kept forces point and fails without one, naming the entry,
    `sets` leaves a new forces point: the optimiser has moved"""
    RULES.check_effect_on_the_point(bioen_amd, row, needles=("bioen_hip_forces_newton_factor",), sets_moves=True)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RULES.rows())
def test_effect_on_a_session(bioen_amd, row):      # noqa: F811
    RULES.check_effect_on_a_session(bioen_amd, row)

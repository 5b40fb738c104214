"""The sixth public header, include/bioen_hip_forces_newton.h, held to the rules tests/test_abi_forces_gram_bf16.py holds the
fifth to: what it declares is exported and bound (in _lib.py's sixth table, and in no other), it is plain C and a C caller
links against it, its two structs have the layout of the ctypes classes, and every entry has an effect row (DESIGN section
6c) that is exercised on the GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_entry_effects import ALPHA, BETA, P, Row, estate

HEADER = os.path.join(ROOT, "include", "bioen_hip_forces_newton.h")
NAMES = ["bioen_hip_forces_newton_factor", "bioen_hip_forces_newton_solve", "bioen_hip_opt_newton_forces"]


def _v():
    return np.random.default_rng(2).standard_normal(P.get().m)


def _f():
    return 1e-3 * np.random.default_rng(3).standard_normal(P.get().m)


def _spd():
    m = P.get().m
    B = np.random.default_rng(4).standard_normal((m, m))
    return B.dot(B.T) / m + np.eye(m)


def _factor_then_solve(c):
    c.forces_newton_factor(_spd(), want_L=False)
    c.forces_newton_solve(_v())


# the rows of DESIGN section 6c for this header: the factorisation and the solve keep point and session (with A=None the
# factorisation needs a forces point); the minimizer evaluates, and leaves its optimum as the new point
ENTRIES = {
    "bioen_hip_forces_newton_factor": [
        Row("keeps", "keeps", lambda c: c.forces_newton_factor(_spd())),
        Row("needs", "keeps", lambda c: c.forces_newton_factor(None, source="gram")),
    ],
    "bioen_hip_forces_newton_solve": [Row("keeps", "keeps", _factor_then_solve)],
    "bioen_hip_opt_newton_forces": [
        Row("sets", "ends", lambda c: c.opt_newton_forces(_f(), P.get().w0, P.get().theta, dict(max_iterations=2))),
    ],
}


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bioen_hip_\w+)\s*\(", src)))


def test_every_declared_symbol_is_exported_bound_and_classified():
    from bioen_amd import _lib
    names = declared_functions()
    assert names == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert not [n for n in names if n not in exported]
    assert sorted(_lib.exported_symbols_forces_newton()) == names         # bound in the sixth table, nothing else there
    others = (_lib.exported_symbols(), _lib.exported_symbols_forces_hessp(), _lib.exported_symbols_forces_gram(),
              _lib.exported_symbols_forces_colquad(), _lib.exported_symbols_forces_gram_bf16())
    for table in others:                                                  # ... and the other five tables are their headers' alone
        assert not set(names) & set(table)
    assert [t for t in others[1:]] == [["bioen_hip_forces_hessp"], ["bioen_hip_forces_gram"], ["bioen_hip_forces_colquad"],
                                       ["bioen_hip_forces_gram_bf16"]]
    # the other direction: every bioen_hip_* symbol the library exports is declared in one of the six tables
    bound = set(names).union(*others)
    assert not sorted(n for n in exported if n.startswith("bioen_hip_") and n not in bound)
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib._SIGNATURES_FORCES_NEWTON[n][1]
    assert set(ENTRIES) == set(names)                                     # every entry has its effect rows
    for rows in ENTRIES.values():
        for row in rows:
            assert row.how is not None and row.point in ("keeps", "sets", "needs") and row.session in ("ends", "keeps")


STRUCT_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bioen_hip_forces_newton.h"
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


def _build_c_demo(tmp_path):
    from bioen_amd import _lib
    exe = str(tmp_path / "c_abi_forces_newton_demo")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_forces_newton_demo.c"), "-L", libdir, "-lbioen_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe], check=True)
    return exe


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    exe = _build_c_demo(tmp_path)
    import bioen_amd
    if bioen_amd.device_count() == 0:
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 77 and "no HIP device" in p.stdout


@pytest.mark.gpu
def test_c_caller_runs_the_loop(tmp_path):
    p = subprocess.run([_build_c_demo(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout, p.stderr)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


ROWS = [pytest.param(row, id="%s-%d" % (name[len("bioen_hip_"):], i)) for name in NAMES for i, row in enumerate(ENTRIES[name])]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS)
def test_effect_on_the_point(bioen_amd, row):
    """`keeps` leaves the products' point alone, `needs` serves the kept forces point and fails without one, `sets` leaves a
    new forces point"""
    p = P.get()
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        if row.point == "needs":
            estate(lambda: row.how(ctx), "no point on this context", "bioen_hip_forces_newton_factor")
        hv, _, _ = ctx.forces_hessp(_v(), forces=_f(), w0=p.w0, theta=p.theta)
        row.how(ctx)
        if row.point == "sets":
            assert not np.array_equal(ctx.forces_hessp(_v()), hv)         # a product at the new point (the optimiser has moved)
        else:
            assert np.array_equal(ctx.forces_hessp(_v()), hv)
        # ... and on a LOG-WEIGHTS point: `sets` replaces it, `needs` is refused and leaves it, `keeps` leaves it
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        if row.point == "sets":
            row.how(ctx)
            estate(lambda: ctx.logw_hessp(p.v), "forces point")
        else:
            if row.point == "needs":
                estate(lambda: row.how(ctx), "log-weights point", "bioen_hip_forces_newton_factor")
            else:
                row.how(ctx)
            assert np.array_equal(ctx.logw_hessp(p.v), hl)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS)
def test_effect_on_a_session(bioen_amd, row):
    p = P.get()
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        ctx.logw_fdf(p.x, p.G, p.theta)
        ctx.bfgs_begin(p.x, p.G, p.theta)
        ctx.bfgs_trial(ALPHA, True)
        assert "bfgs_hinv" in ctx.footprint()[0]
        if row.point == "needs":                            # (the session's own calls have dropped every point)
            estate(lambda: row.how(ctx))
        else:
            row.how(ctx)
        if row.session == "ends":
            estate(lambda: ctx.bfgs_trial(BETA, False), "ended by another call")
            assert "bfgs_hinv" not in ctx.footprint()[0]
        else:
            f, _ = ctx.bfgs_trial(2 * BETA, False)
            assert np.isfinite(f)

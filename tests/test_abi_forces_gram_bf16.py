"""The fifth public header, include/bioen_hip_forces_gram_bf16.h, held to the rules tests/test_abi_forces_colquad.py holds
the fourth to: what it declares is exported and bound (in _lib.py's fifth table, and in no other), it is plain C and a C
caller links against it, and every entry has an effect row that is exercised on the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_entry_effects import ALPHA, BETA, P, Row, estate

HEADER = os.path.join(ROOT, "include", "bioen_hip_forces_gram_bf16.h")


def _v():
    return np.random.default_rng(2).standard_normal(P.get().m)


def _f():
    return 1e-3 * np.random.default_rng(3).standard_normal(P.get().m)


# the rows of DESIGN section 6c for this header: with forces the call is an evaluation that leaves a new point; without, it
# serves the kept one
ENTRIES = {
    "bioen_hip_forces_gram_bf16": [
        Row("sets", "ends", lambda c: c.forces_gram_bf16(forces=_f(), w0=P.get().w0, theta=P.get().theta)),
        Row("needs", "keeps", lambda c: c.forces_gram_bf16()),
    ],
}


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bioen_hip_\w+)\s*\(", src)))


def test_every_declared_symbol_is_exported_bound_and_classified():
    from bioen_amd import _lib
    names = declared_functions()
    assert names == ["bioen_hip_forces_gram_bf16"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert not [n for n in names if n not in exported]
    assert sorted(_lib.exported_symbols_forces_gram_bf16()) == names      # bound in the fifth table, nothing else there
    assert not set(names) & set(_lib.exported_symbols())                  # ... and the other four tables are their headers' alone
    assert not set(names) & set(_lib.exported_symbols_forces_hessp())
    assert not set(names) & set(_lib.exported_symbols_forces_gram())
    assert not set(names) & set(_lib.exported_symbols_forces_colquad())
    assert _lib.exported_symbols_forces_colquad() == ["bioen_hip_forces_colquad"]
    assert _lib.exported_symbols_forces_hessp() == ["bioen_hip_forces_hessp"]
    assert _lib.exported_symbols_forces_gram() == ["bioen_hip_forces_gram"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib._SIGNATURES_FORCES_GRAM_BF16[n][1]
    assert set(ENTRIES) == set(names)                                     # every entry has its effect rows
    for rows in ENTRIES.values():
        for row in rows:
            assert row.how is not None and row.point in ("sets", "needs") and row.session in ("ends", "keeps")


def _build_c_demo(tmp_path):
    from bioen_amd import _lib
    exe = str(tmp_path / "c_abi_forces_gram_bf16_demo")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_forces_gram_bf16_demo.c"), "-L", libdir, "-lbioen_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe], check=True)
    return exe


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    exe = _build_c_demo(tmp_path)
    import bioen_amd
    if bioen_amd.device_count() == 0:
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 77 and "no HIP device" in p.stdout


@pytest.mark.gpu
def test_c_caller_runs_the_pass(tmp_path):
    p = subprocess.run([_build_c_demo(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout, p.stderr)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


ROWS = [pytest.param(row, id="forces_gram_bf16-%d" % i) for i, row in enumerate(ENTRIES["bioen_hip_forces_gram_bf16"])]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS)
def test_effect_on_the_point(bioen_amd, row):
    """as tests/test_abi_forces_gram.py checks bioen_hip_forces_gram: `sets` leaves the same, new point, `needs` serves the
    kept one -- and fails without one; the point is the products' own"""
    p = P.get()
    with bioen_amd.Context(p.yT, p.YT) as ctx:
        if row.point == "needs":
            estate(lambda: row.how(ctx), "no point on this context")
        hv, _, _ = ctx.forces_hessp(_v(), forces=_f(), w0=p.w0, theta=p.theta)
        assert np.array_equal(ctx.forces_hessp(_v()), hv)
        row.how(ctx)
        assert np.array_equal(ctx.forces_hessp(_v()), hv)
        # ... and on a LOG-WEIGHTS point: `sets` replaces it, `needs` is refused and leaves it
        hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
        if row.point == "sets":
            row.how(ctx)
            estate(lambda: ctx.logw_hessp(p.v), "forces point")
        else:
            estate(lambda: row.how(ctx), "log-weights point")
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

"""The rules every public header beside include/bioen_hip.h is held to -- those tests/test_abi.py and
tests/test_entry_effects.py hold that one to: what it declares is exported and bound in its own table of _lib.py, it is
plain C and a C caller links against it, and every entry has an effect row that is exercised on the GPU.
Not a test module: tests/test_abi_forces_*.py each describe their header with a HeaderRules, call these checks from test
functions of their own (so every file keeps its test ids) and add what they check beyond them."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_entry_effects import ALPHA, BETA, P, estate


def v():
    return np.random.default_rng(2).standard_normal(P.get().m)


def f():
    return 1e-3 * np.random.default_rng(3).standard_normal(P.get().m)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


class HeaderRules(object):
    """header: the file under include/; names: what it declares, sorted; table: the suffix of _lib.py's
    exported_symbols_<table>() and _SIGNATURES_<TABLE>; demo: the C caller under examples/, without .c; entries: name ->
    [Row]; points: the values a row's point may take"""

    def __init__(self, header, names, table, demo, entries, points=("sets", "needs")):
        self.header = os.path.join(ROOT, "include", header)
        self.names, self.table, self.demo, self.entries, self.points = names, table, demo, entries, points

    def declared_functions(self):
        src = re.sub(r"/\*.*?\*/", "", open(self.header).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(bioen_hip_\w+)\s*\(", src)))

    def rows(self):
        """the parameters of the effect tests: <entry without bioen_hip_>-<index of the row>"""
        return [pytest.param(row, id="%s-%d" % (name[len("bioen_hip_"):], i))
                for name in self.names for i, row in enumerate(self.entries[name])]

    def check_declared_exported_bound_and_classified(self):
        """-> (names, every symbol the library exports), for what a file checks about the other tables"""
        from bioen_amd import _lib
        names = self.declared_functions()
        assert names == self.names
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        assert not [n for n in names if n not in exported]
        assert sorted(getattr(_lib, "exported_symbols_" + self.table)()) == names      # bound in its table, nothing else there
        assert not set(names) & set(_lib.exported_symbols())                           # ... and the first table is bioen_hip.h's alone
        L = _lib.lib()
        for n in names:
            assert getattr(L, n).argtypes == getattr(_lib, "_SIGNATURES_" + self.table.upper())[n][1]
        assert set(self.entries) == set(names)                                         # every entry has its effect rows
        for rows in self.entries.values():
            for row in rows:
                assert row.how is not None and row.point in self.points and row.session in ("ends", "keeps")
        return names, exported

    def build_c_demo(self, tmp_path):
        from bioen_amd import _lib
        exe = str(tmp_path / self.demo)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", self.demo + ".c"), "-L", libdir, "-lbioen_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe], check=True)
        return exe

    def check_header_is_plain_c_and_a_c_caller_links(self, tmp_path):
        exe = self.build_c_demo(tmp_path)
        import bioen_amd
        if bioen_amd.device_count() == 0:
            p = subprocess.run([exe], capture_output=True, text=True)
            assert p.returncode == 77 and "no HIP device" in p.stdout

    def check_c_caller_runs(self, tmp_path):
        p = subprocess.run([self.build_c_demo(tmp_path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout, p.stderr)

    @staticmethod
    def check_effect_on_the_point(bioen_amd, row, needles=(), sets_moves=False):
        """on a forces point, the products' own: `sets` leaves a new point -- the same one, or with sets_moves another --,
        `needs` serves the kept one and fails without one (the message holds the needles), `keeps` leaves it alone"""
        p = P.get()
        with bioen_amd.Context(p.yT, p.YT) as ctx:
            if row.point == "needs":
                estate(lambda: row.how(ctx), "no point on this context", *needles)
            hv, _, _ = ctx.forces_hessp(v(), forces=f(), w0=p.w0, theta=p.theta)
            assert np.array_equal(ctx.forces_hessp(v()), hv)
            row.how(ctx)
            if row.point == "sets" and sets_moves:
                assert not np.array_equal(ctx.forces_hessp(v()), hv)     # a product at the new point
            else:
                assert np.array_equal(ctx.forces_hessp(v()), hv)
            # ... and on a LOG-WEIGHTS point: `sets` replaces it, `needs` is refused and leaves it, `keeps` leaves it
            hl, _, _ = ctx.logw_hessp(p.v, g=p.x, G=p.G, theta=p.theta)
            if row.point == "sets":
                row.how(ctx)
                estate(lambda: ctx.logw_hessp(p.v), "forces point")
            else:
                if row.point == "needs":
                    estate(lambda: row.how(ctx), "log-weights point", *needles)
                else:
                    row.how(ctx)
                assert np.array_equal(ctx.logw_hessp(p.v), hl)

    @staticmethod
    def check_effect_on_a_session(bioen_amd, row):
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
                fv, _ = ctx.bfgs_trial(2 * BETA, False)
                assert np.isfinite(fv)

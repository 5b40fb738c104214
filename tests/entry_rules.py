"""What the tests of the C ABI's entries share: the effect row, the problem the rows run on, and the
checks tests/test_abi_<feature>.py hold a feature's entries to -- every entry has its effect rows, a C caller compiles
against include/bioen_hip.h as strict C99, links and runs, and every row is exercised on the GPU.  Not a test module:
tests/test_entry_effects.py reads the rows of every tests/test_abi_*.py, and those describe their entries with an
EntryRules and call its checks from test functions of their own (so every file keeps its test ids)."""
import os
import re
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from conftest import ROOT, load_golden

# point:   keeps | drops | sets (leaves a new one) | needs (fails without one, keeps it)
# session: keeps | ends | needs (fails without one, keeps it; closes=True: its regular end) | starts
# how:     the call on a bioen_amd.Context (the raw binding where it has no method); None + why: not runnable in one process on one GPU
# prepare: what a live session (or the context) needs before the call can succeed
Row = namedtuple("Row", "point session how prepare closes why", defaults=(None, False, None))

ALPHA, BETA = 1e-3, 2e-3           # the trial the session is left at; another one


class P(object):
    """the problem of the tests: synth_logw_M64xN2000 (state logic: the shape does not matter)"""
    _d = None

    @classmethod
    def get(cls):
        if cls._d is None:
            d = load_golden("synth_logw_M64xN2000.npz")
            p = cls._d = cls()
            p.yT, p.YT = d["yTilde"], d["YTilde"].reshape(-1)
            p.G, p.theta, p.x = d["G"].reshape(-1), float(d["theta"]), d["GInit"].reshape(-1)
            p.m, p.n = p.yT.shape
            p.v = np.random.default_rng(1).standard_normal(p.n)
            p.w0 = np.full(p.n, 1.0 / p.n)
            p.f0 = np.zeros(p.m)
        return cls._d


def estate(call, *needles):
    from bioen_amd._lib import BioenHipError
    with pytest.raises(BioenHipError) as e:
        call()
    assert "(-6)" in str(e.value) and all(s in str(e.value) for s in needles), str(e.value)


def v():
    return np.random.default_rng(2).standard_normal(P.get().m)


def f():
    return 1e-3 * np.random.default_rng(3).standard_normal(P.get().m)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


def short_name(name):
    """an entry without its namespace -- bioen_ and the word after it: bioen_hip_, bioen_laplace_, bioen_logwn_ --: what
    the ids of the effect tests are made of"""
    return re.sub(r"^bioen_[a-z0-9]+_", "", name)


class EntryRules(object):
    """names: a feature's entries, sorted; demo: its C caller under examples/, without .c; entries: name -> [Row];
    points: the values a row's point may take"""

    def __init__(self, names, demo, entries, points=("sets", "needs")):
        self.names, self.demo, self.entries, self.points = names, demo, entries, points

    def rows(self):
        """the parameters of the effect tests: <entry without its prefix>-<index of the row>"""
        return [pytest.param(row, id="%s-%d" % (short_name(name), i))
                for name in sorted(self.entries) for i, row in enumerate(self.entries[name])]

    def check_classified(self):
        assert set(self.entries) == set(self.names)                                    # every entry has its effect rows
        for rows in self.entries.values():
            for row in rows:
                assert row.how is not None and row.point in self.points and row.session in ("ends", "keeps")

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

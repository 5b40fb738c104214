"""The host logic of the dual Newton beyond 1024 observables that lives in Python, on fakes: the
kept API's calls (ext/c_bioen.py: bioen_opt_dual_newton_logw, bioen_opt_dual_newton_logw_series) turn the context's switch
on for the call when M > 1024 and put it back as it was -- whatever the call does --, and leave it alone when M <= 1024 or
when the holder of the context has set it.  The device side: tests/test_hip_logw_panels.py."""
import numpy as np
import pytest

from bioen_amd.optimize.ext import c_bioen


class FakeContext(object):
    """what c_bioen's two calls touch of a Context: m, dense_panels, set_dense_panels and the two minimizers, which record
    the switch as they find it"""

    def __init__(self, m, on=False, fail=False):
        self.m, self.dense_panels, self.fail, self._h = m, on, fail, object()
        self.sets, self.seen = [], []

    def set_dense_panels(self, on=True):
        self.sets.append(bool(on))
        self.dense_panels = bool(on)

    def _run(self):
        self.seen.append(self.dense_panels)
        if self.fail:
            raise RuntimeError("device says no")
        return dict(g=np.zeros(3), status=0, fmin=1.5, gmax=0.0, wmax=1.0, iterations=1, evaluations=2, factorisations=1)

    def opt_dual_newton_logw(self, g, G, theta, params):
        return self._run()

    def opt_dual_newton_logw_series(self, thetas, g, G, params, warm=True):
        return [self._run() for _ in thetas]


@pytest.fixture
def served(monkeypatch):
    """c_bioen serves the calls from the fake handed to it"""
    box = {}
    monkeypatch.setattr(c_bioen, "_context_for", lambda yT, YT: (box["ctx"], True))
    monkeypatch.setattr(c_bioen, "_release", lambda ctx, cached: None)
    return box


def single():
    return c_bioen.bioen_opt_dual_newton_logw(np.zeros(3), np.zeros(3), None, None, 10.0, dict(params={}))


def series():
    return c_bioen.bioen_opt_dual_newton_logw_series(np.zeros(3), np.zeros(3), None, None, [100.0, 10.0], dict(params={}))


@pytest.mark.parametrize("call,runs", [(single, 1), (series, 2)], ids=["single", "series"])
def test_switch_is_on_for_the_call_and_back_afterwards(served, call, runs):
    ctx = served["ctx"] = FakeContext(1100)
    call()
    assert ctx.seen == [True] * runs and ctx.sets == [True, False] and ctx.dense_panels is False


@pytest.mark.parametrize("call", [single, series], ids=["single", "series"])
def test_switch_is_put_back_when_the_call_raises(served, call):
    ctx = served["ctx"] = FakeContext(4096, fail=True)
    with pytest.raises(RuntimeError, match="device says no"):
        call()
    assert ctx.seen == [True] and ctx.sets == [True, False] and ctx.dense_panels is False


@pytest.mark.parametrize("call", [single, series], ids=["single", "series"])
def test_a_holders_setting_is_left_alone(served, call):
    ctx = served["ctx"] = FakeContext(1100, on=True)
    call()
    assert ctx.sets == [] and ctx.dense_panels is True and all(ctx.seen)


@pytest.mark.parametrize("m", [1, 1024])
def test_no_switch_is_touched_up_to_1024_rows(served, m):
    ctx = served["ctx"] = FakeContext(m)
    single()
    series()
    assert ctx.sets == [] and ctx.seen == [False] * 3


def test_a_closed_context_is_not_called_again(served):
    """a context that went away inside the call (its handle gone) is not asked to put anything back"""
    ctx = served["ctx"] = FakeContext(1100)
    with c_bioen._dense_panels(ctx):
        ctx._h = None
    assert ctx.sets == [True]

"""The opening of a series on the host-driven log-weights engine (engine_logw.inl): while the slowest problem is in its
first iterations, more than two batch slots are kept back and all of them evaluate the steps lb::speculative_lattice
foresees for it.  Fewer lock-step rounds, not a bit changed.

The shape is small (M = 64 x N = 20000, where the device-resident engine would be the default), so every run asks for
the host-driven engine, the one the headline runs on: BIOEN_HIP_DEVICE_LS=0."""
import numpy as np
import pytest

from conftest import LBFGS_DEFAULTS

pytestmark = pytest.mark.gpu

M, N = 64, 20000
THETAS = list(np.logspace(3, -0.5, 8))

# What the oracle's restatement (oracle_binding.opt_lbfgs_logw, CPU) counts for these series, (iterations, evaluations) per
# theta in the order of THETAS, and the evaluations of the smallest theta's first line searches (from runs capped at
# 1, 2, 3 ... iterations).  A search of e evaluations has e - 1 rejections; all but the first are "second-level" ones,
# which two shadows cannot cover.
#   seed 9:  (6, 7) (7, 9) (17, 23) (46, 57) (82, 95) (136, 150) (172, 188) (208, 225); the smallest theta is the slowest by
#            37 evaluations; its searches take 6, 3, 5, 1, 1 ... evaluations: 4 + 1 + 3 = 8 second-level rejections within
#            its first 40 evaluations
#   seed 77: (6, 7) (8, 10) (27, 55) (45, 75) (79, 96) (149, 180) (210, 239) (174, 196); the slowest member is theta = 1, not
#            the smallest theta; searches of 6, 3, 2, 2, 1 ... evaluations: 5 second-level rejections
POLICIES = {
    "unspeculated": {"BIOEN_HIP_SPECULATE": "0"},
    "parent": {"BIOEN_HIP_HOST_SHADOWS": "2", "BIOEN_HIP_RESERVE": "2"},     # two slots kept back, two shadows per round, throughout
    "default": {},
}


@pytest.fixture(scope="module")
def hip():
    import bioen_amd
    assert bioen_amd.device_count() >= 1, "no MI355X visible"
    return bioen_amd


def problem(seed):
    rng = np.random.default_rng(seed)
    YTrue = rng.uniform(1, 10, M)
    y = rng.normal(YTrue[:, None], 0.5 * YTrue[:, None], (M, N)) / (0.1 * YTrue[:, None])
    YT = rng.normal(YTrue, 0.1 * YTrue) / (0.1 * YTrue)
    return y, YT


def series(hip, monkeypatch, seed, policy):
    """-> (everything the series returns, as comparable values; lock-step rounds)"""
    y, YT = problem(seed)
    G = np.zeros(N)
    with monkeypatch.context() as mp:
        mp.setenv("BIOEN_HIP_DEVICE_LS", "0")
        for k in ("BIOEN_HIP_SPECULATE", "BIOEN_HIP_HOST_SHADOWS", "BIOEN_HIP_RESERVE"):
            mp.delenv(k, raising=False)
        for k, v in POLICIES[policy].items():
            mp.setenv(k, v)
        with hip.Context(y, YT) as ctx:
            ctx.kernel_stats_enable(True)
            ctx.kernel_stats_reset()
            res, w, infos = ctx.opt_lbfgs_logw_batch(THETAS, G, G, LBFGS_DEFAULTS, max_batch=8)
            ctx.synchronize()
            rounds = ctx.kernel_stats()["forward"]["launches"]
    out = dict(res=res.tobytes(), w=w.tobytes(), it=[i.iterations for i in infos], ev=[i.evaluations for i in infos],
               fmin=[i.fmin for i in infos], chi2=[i.chi2 for i in infos], S=[-i.kl for i in infos],
               code=[i.lbfgs_code for i in infos])
    return out, rounds


def test_opening_shadows_save_rounds_and_change_no_bit(hip, monkeypatch):
    runs = {p: series(hip, monkeypatch, 9, p) for p in POLICIES}
    for p, (out, rounds) in runs.items():
        print(p, "rounds", rounds, "iterations", out["it"], "evaluations", out["ev"])
    ref = runs["unspeculated"][0]
    assert all(c in (0, 1) for c in ref["code"]), ref["code"]
    assert int(np.argmax(ref["ev"])) == len(THETAS) - 1            # the smallest theta is the series' slowest member
    for p in ("parent", "default"):
        for key in ref:
            assert runs[p][0][key] == ref[key], (p, key)
    assert runs["default"][1] < runs["parent"][1] < runs["unspeculated"][1], {p: r[1] for p, r in runs.items()}


def test_held_back_thetas_finish_within_the_slowest_members_rounds(hip, monkeypatch):
    """ntheta = 8 on max_batch = 8: five thetas wait during the opening.  They all finish, with the unspeculated run's bits,
    and the sweep takes no more rounds than its slowest member evaluates on its own -- here theta = 1, not the smallest
    theta the opening is held for."""
    ref, plain_rounds = series(hip, monkeypatch, 77, "unspeculated")
    out, rounds = series(hip, monkeypatch, 77, "default")
    print("rounds", rounds, "unspeculated", plain_rounds, "evaluations", ref["ev"])
    assert all(c in (0, 1) for c in out["code"]) and all(i > 0 for i in out["it"]), (out["code"], out["it"])
    for key in ref:
        assert out[key] == ref[key], key
    assert rounds <= max(ref["ev"]), (rounds, ref["ev"])

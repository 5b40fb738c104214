"""GPU tests of the log-weights dual Newton beyond 1024 observables: Context.set_dense_panels, the Gram
passes over row panels (csrc/fgram.hpp: FGramPanelArgs; csrc/kernels_logw_newton.hip: k_logw_gram_panels,
k_logw_gram_bf16_panels), the solve beyond 1024 unknowns (csrc/kernels_forces_newton_wide.hip: k_fnewton_solve_wide) and the
kept API (log_weights.find_optimum with Parameters("dual_newton")).  The shapes are the smallest at which each part can go
wrong:

  1025 x 400     a second panel of one row: 16 strip rows, one slice of one row block
  1100 x 2000    the last panel's slices of 64 + 12 rows, and the solve beyond column 1088
  2100 x 400     three panels: cross tiles between panels that are not neighbours
  4096 x 300     four full panels, the limit
  1100 x 2000 under BIOEN_HIP_SEGMENTS=1     one canonical segment
  4100 x 64      the refusal that names 4096;  1100 x 2000 with the switch off: the old refusal

The gates are those of the M <= 1024 tests: GATE of tests/test_hip_forces_gram.py for the covariance, the documented
3 * 2^-16 sqrt(G'_ii G'_kk) and tests/test_hip_logw_gram_bf16.py's 48 tg 2^-23 s_ik for the split-BF16 pass, 1e-10 max|u|
for the step.  -b has no entry of its own: it is held through the step, from either source (the FP64 step against the
80-bit step; the split pass's step against the 80-bit step from the device's own C~, which leaves -b, the factor, the solve
and the adjoint as the only things that can differ).  tests/README_logw_panels.md has the measured figures."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_hip_forces_gram import GATE
from test_hip_forces_hessp import estate, problem
from test_hip_logw_gram_bf16 import U16, held as held_bf16, restated, scale_matrix
from test_hip_logw_newton_loops import L, point_longdouble, rows_times, times_columns
from test_logw_dual_newton import PARAMS
from test_logw_series import counts, weights

from bioen_amd import optimize
from bioen_amd.optimize import log_weights, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

THETA = 10.0
SHAPES = [(1025, 400), (1100, 2000), (2100, 400), (4096, 300)]
TALL = (1100, 2000)
THREE = (2100, 400)


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    c_bioen.clear_cache()


_DATA, _LD, _HOST = {}, {}, {}


def data(shape):
    """-> dict(yT, YT, G, g): tests/test_hip_forces_hessp.py's problem and tests/test_hip_logw_dual_newton.py's point
    G + f^T yTilde (standard deviation 1: weights over a few decades, not an optimum), once per shape"""
    if shape not in _DATA:
        yT, YT, w0, f, _ = problem(shape)
        G = np.log(w0)
        _DATA[shape] = dict(yT=yT, YT=YT, G=G, g=G + f @ yT)
    return _DATA[shape]


def affine_model(m):
    rng = np.random.default_rng(3)                   # tests/test_hip_logw_dual_newton.py: test_cov_with_an_affine_model
    return rng.normal(0.0, 0.5, m), rng.uniform(0.5, 1.5, m)


def sampled_rows(m):
    """the first and the last 64 rows of every panel of 1024"""
    rows = []
    for p0 in range(0, m, 1024):
        p1 = min(m, p0 + 1024)
        rows += list(range(p0, min(p0 + 64, p1))) + list(range(max(p0, p1 - 64), p1))
    return np.array(sorted(set(rows)))


def cov_rows_longdouble(key, A, g, rows):
    """rows of C = sum_j w_j (a_j - abar)(a_j - abar)^T, w = softmax(g), against all columns in numpy.longdouble (row
    blocks on eight threads), once per problem"""
    if key not in _LD:
        gl = g.astype(L)
        e = np.exp(gl - gl.max())
        w = e / e.sum()
        a = A - (A @ w)[:, None]
        aw, at = a[rows] * w[None, :], a.T.copy()
        blocks = [b for b in np.array_split(np.arange(rows.size), 8) if b.size]
        with ThreadPoolExecutor(8) as workers:
            _LD[key] = np.vstack(list(workers.map(lambda b: aw[b] @ at, blocks))).astype(np.float64)
    return _LD[key]


def check_cov(ctx, key, d, model=None):
    """logw_cov over panels: sampled rows against longdouble, the whole matrix against the FP64 restatement, at GATE;
    bitwise symmetric, the same bits call after call, f and grad logw_fdf's bits"""
    yT, YT, G, g = d["yT"], d["YT"], d["G"], d["g"]
    m = yT.shape[0]
    if model is None:
        y, y64 = yT.astype(L), yT
    else:
        y = model[0][:, None].astype(L) + model[1][:, None].astype(L) * yT.astype(L)
        y64 = y.astype(np.float64)
        ctx.set_affine(*model)
    rows = sampled_rows(m)
    ref_rows = cov_rows_longdouble(key, y, g, rows)
    p = log_weights._dual_newton_point(g, G, y64, YT, THETA, 0.0)
    ref = log_weights.dual_newton_covariance(p, y64)
    f0, g0 = ctx.logw_fdf(g, G, THETA)
    C, fv, grad = ctx.logw_cov(g=g, G=G, theta=THETA)
    S = float(np.abs(ref).max())
    d_ld = float(np.abs(C[rows] - ref_rows).max()) / S
    d_64 = float(np.abs(C - ref).max()) / S
    print("%s: %d sampled rows |C - C_ld| = %.3g max|C|; all of it |C - C_fp64| = %.3g max|C|" % (key, rows.size, d_ld, d_64))
    assert fv == f0 and np.array_equal(grad, g0)
    assert np.array_equal(C, C.T)
    assert d_ld <= GATE and d_64 <= GATE
    assert np.array_equal(ctx.logw_cov(), C)
    assert np.array_equal(ctx.logw_cov(g=g, G=G, theta=THETA)[0], C)
    return C


# ---- 1. the covariance from k_logw_gram_panels ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_cov_over_panels(bioen_amd, shape):
    d = data(shape)
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        check_cov(ctx, case_id(shape), d)
        assert {"strips", "logw_gram"} <= ctx.footprint()[0]


def test_cov_over_panels_with_an_affine_model(bioen_amd):
    d = data(THREE)
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        plain, _, _ = ctx.logw_cov(g=d["g"], G=d["G"], theta=THETA)
        C = check_cov(ctx, "affine " + case_id(THREE), d, affine_model(THREE[0]))
        assert not np.array_equal(C, plain)
        ctx.set_affine(np.zeros(THREE[0]), np.ones(THREE[0]))            # (o, s) = (0, 1): the plain model's bits
        assert np.array_equal(ctx.logw_cov(g=d["g"], G=d["G"], theta=THETA)[0], plain)


def test_cov_over_panels_on_one_canonical_segment(bioen_amd, monkeypatch):
    d = data(TALL)
    monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        assert ctx.strip_plan(0)["local_segments"] == 1
        check_cov(ctx, case_id(TALL), d)


# ---- 3. the split-BF16 covariance -----------------------------------------------------------------------------------------
def panels_tg(ctx, m):
    """the longest chain of strips a set adds up, from the plan counted over all panels (logw_gram_plan)"""
    p = ctx.strip_plan(0)
    t = (-(-m // 64) + 1) // 2
    gs = max(1, min(p["sps"], -(-512 // (p["local_segments"] * (t * (t + 1) // 2)))))
    return -(-p["sps"] // gs)


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_bf16_cov_over_panels(bioen_amd, shape):
    """the documented bound against logw_cov at the same kept point, element by element (plus the FP64 floor of
    tests/test_hip_logw_gram_bf16.py for the two sides' ybar); at 1100 x 2000 and 2100 x 400 the restatement at that
    file's gate besides"""
    d = data(shape)
    yT, YT, G, g = d["yT"], d["YT"], d["G"], d["g"]
    S, floor = scale_matrix(yT, YT, g)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_dense_panels()
        f0, g0 = ctx.logw_fdf(g, G, THETA)
        Cb, fv, grad = ctx.logw_cov_bf16(g=g, G=G, theta=THETA)
        Cf = ctx.logw_cov()
        ratio = float((np.abs(Cb - Cf)[S > 0] / S[S > 0]).max())
        print("%dx%d: |C~ - C| = %.3g s_ik (bound %.3g)" % (shape + (ratio, 3 * U16)))
        assert fv == f0 and np.array_equal(grad, g0)
        assert (np.abs(Cb - Cf) <= 3 * U16 * S + floor).all()
        assert np.abs(Cb - Cf).max() > 0.0 and np.array_equal(Cb, Cb.T)
        assert np.array_equal(ctx.logw_cov_bf16(), Cb)
        assert np.array_equal(ctx.logw_cov(), Cf)                        # the FP64 pass keeps its bits beside it
        if shape in (TALL, THREE):
            held_bf16(case_id(shape), Cb, Cf, restated(yT, YT, G, g, THETA), (S, floor), panels_tg(ctx, shape[0]))


# ---- 2, 4. one accepted step: -b, the factor, the solve beyond 1024, the operand, the adjoint -----------------------------
def step_longdouble(key, d, Ct=None):
    """-> dict(u, w, sweeps, last): the dual Newton step at the point d["g"] in 80-bit arithmetic, (C + theta I) z = -b by
    iterative refinement on a float64 Cholesky factor with the residual in longdouble (tests/test_hip_logw_newton_loops.py:
    step_longdouble).  Ct None: the operator Yc (w o Yc^T v) + theta v applied in longdouble, C never formed; Ct: that
    matrix is the covariance, with no other float64 on the path (tests/test_hip_logw_gram_bf16.py: step_from)"""
    import scipy.linalg
    if Ct is None and key in _LD:
        return _LD[key]
    y, theta, m = d["yT"].astype(L), L(THETA), d["yT"].shape[0]
    p = point_longdouble(y, d["YT"], d["G"], d["g"], THETA)
    w, ybar = p["w"], p["ybar"]

    def centred_adjoint(v):
        return times_columns(v, y) - ybar @ v

    def centred_forward(t):
        return rows_times(y, t) - ybar * t.sum()

    if Ct is None:
        p64 = log_weights._dual_newton_point(d["g"], d["G"], d["yT"], d["YT"], THETA, 0.0)
        pre = log_weights.dual_newton_covariance(p64, d["yT"])

        def A(v):
            return centred_forward(w * centred_adjoint(v)) + theta * v
    else:
        pre, Cl = Ct, Ct.astype(L)

        def A(v):
            return Cl @ v + theta * v
    factor = scipy.linalg.cho_factor(pre + THETA * np.eye(m), lower=True)
    negb = -centred_forward(p["grad"])
    z, sweeps, last = np.zeros(m, dtype=L), 0, np.inf
    while sweeps < 8 and last > 1e-17:
        res = negb - A(z) if sweeps else negb
        dz = scipy.linalg.cho_solve(factor, res.astype(np.float64)).astype(L)
        z = z + dz
        sweeps += 1
        last = float(np.abs(dz).max() / np.abs(z).max())
    out = dict(u=-((p["dev"] - p["P"]) + centred_adjoint(p["r"] + z) / theta), w=w, sweeps=sweeps, last=last)
    if Ct is None:
        _LD[key] = out
    return out


def converged(ref):
    """the reference's own condition, asserted before anything is compared with it: the last correction of the refinement
    <= 1e-15 max|z|, five decades under the step's gate.  (tests/test_hip_logw_newton_loops.py asks 1e-17 within 5 sweeps of
    its M <= N problems; at 2100 x 400 C has rank 400, C + theta I the condition 1 + lambda_max / theta, and the rounding
    of the 80-bit residual times that condition is where the corrections stop shrinking: 7e-17 measured.)"""
    assert ref["last"] <= 1e-15 and ref["sweeps"] <= 8, (ref["sweeps"], ref["last"])


def check_step(label, d, res, ref):
    converged(ref)
    assert res["status"] == 1 and res["iterations"] == 1 and res["factorisations"] == 1
    alpha = 2.0 ** -(res["evaluations"] - 2)
    u_dev = (res["g"] - d["g"]) / alpha
    S = float(np.abs(ref["u"]).max())
    err = float(np.abs(u_dev.astype(L) - ref["u"]).max()) / S
    gauge = abs(float(ref["w"] @ u_dev.astype(L))) / S
    print("%s: alpha %g, |u - u_ld| = %.3g max|u|, |w . u| = %.3g max|u|; reference: %d sweeps, last correction %.3g max|z|"
          % (label, alpha, err, gauge, ref["sweeps"], ref["last"]))
    assert err <= 1e-10
    assert gauge <= 1e-12


@pytest.mark.parametrize("shape", [TALL, THREE], ids=case_id)
def test_one_step_against_longdouble(bioen_amd, shape):
    d = data(shape)
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        one = dict(PARAMS, max_iterations=1)
        res = ctx.opt_dual_newton_logw(d["g"], d["G"], THETA, one)
        check_step(case_id(shape), d, res, step_longdouble(("step", shape), d))
        # the returned point is the kept point
        C_kept = ctx.logw_cov()
        C, f, grad = ctx.logw_cov(g=res["g"], G=d["G"], theta=THETA)
        assert np.array_equal(C_kept, C) and res["fmin"] == f and res["gmax"] == np.abs(grad).max()
        # the split pass's step from the device's own C~: -b from that source, the factor, the solve, the adjoint
        Ct, _, _ = ctx.logw_cov_bf16(g=d["g"], G=d["G"], theta=THETA)
        resb = ctx.opt_dual_newton_logw(d["g"], d["G"], THETA, dict(one, hessian="gram_bf16"))
        assert resb["bf16_passes"] == 1
        check_step(case_id(shape) + " from C~", d, resb, step_longdouble(None, d, Ct))
        assert not np.array_equal(resb["g"], res["g"])


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------
def host_loop(theta, g0=None):
    """the numpy restatement's run at 1100 x 2000 from g0 (None: G), once per (theta, start)"""
    d = data(TALL)
    key = (theta, None if g0 is None else g0.tobytes())
    if key not in _HOST:
        _HOST[key] = log_weights.dual_newton_bioen_log_posterior_base(d["G"] if g0 is None else g0, d["G"], d["yT"], d["YT"],
                                                                      theta, PARAMS)
    return _HOST[key]


@pytest.mark.parametrize("theta", [100.0, 10.0, 1.0])
def test_loop_against_the_restatement(bioen_amd, theta):
    d = data(TALL)
    host = host_loop(theta)
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        res = ctx.opt_dual_newton_logw(d["G"], d["G"], theta, PARAMS)
        resb = ctx.opt_dual_newton_logw(d["G"], d["G"], theta, dict(PARAMS, hessian="gram_bf16"))
    dw = float(np.abs(weights(res["g"]) - weights(host["g"])).max() / weights(host["g"]).max())
    print("theta %g: device status %d, %d / %d / %d; restatement status %d, %d / %d / %d; fmin %.15g, restatement %.15g; "
          "max|dw| = %.3g max w; gram_bf16: status %d, %d / %d / %d, %d BF16 passes, switched %s, fmin %.15g"
          % ((theta, res["status"]) + counts(res) + (host["status"],) + counts(host) + (res["fmin"], host["fmin"], dw,
             resb["status"]) + counts(resb) + (resb["bf16_passes"], resb["switched"], resb["fmin"])))
    assert host["status"] == 0
    assert (res["status"],) + counts(res) == (host["status"],) + counts(host)
    assert abs(res["fmin"] - host["fmin"]) <= 1e-9 * abs(host["fmin"])
    assert dw <= 1e-5
    assert resb["status"] == 0 and abs(resb["fmin"] - res["fmin"]) <= 1e-9 * abs(res["fmin"])


def test_warm_series_equals_chained_single_calls(bioen_amd):
    d = data(TALL)
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        series = ctx.opt_dual_newton_logw_series([100.0, 10.0], d["G"], d["G"], PARAMS, hessian="gram")
        a = ctx.opt_dual_newton_logw(d["G"], d["G"], 100.0, PARAMS)
        b = ctx.opt_dual_newton_logw(a["g"], d["G"], 10.0, PARAMS)
    for s, single in zip(series, (a, b)):
        assert s["status"] == 0 and (s["status"],) + counts(s) == (single["status"],) + counts(single)
        assert np.array_equal(s["g"], single["g"]) and s["fmin"] == single["fmin"] and s["gmax"] == single["gmax"]
        assert s["bf16_passes"] == 0 and not s["switched"]


# ---- 6. the kept API, the refusals, the footprint ----------------------------------------------------------------------------
def plan_bytes(ctx, m):
    """logw_gram_plan's buffer, by hand: (sets + 1) x [sub-tiles x 32 KiB + the slices' row sums + 8] + C + 8 scalars"""
    p = ctx.strip_plan(0)
    panels = -(-m // 1024)
    last_rows = -(-(m - 1024 * (panels - 1)) // 16) * 16               # the last panel's strip rows
    nsl = 16 * (panels - 1) + -(-last_rows // 64)
    t = (nsl + 1) // 2
    gs = max(1, min(p["sps"], -(-512 // (p["local_segments"] * (t * (t + 1) // 2)))))
    stride = nsl * (nsl + 1) // 2 * 4096 + nsl * 64 + 8
    return 8 * ((p["local_segments"] * gs + 1) * stride + m * m + 8)


def test_find_optimum_serves_beyond_1024_and_puts_the_switch_back(bioen_amd):
    d = data(TALL)
    yT, YT, G = d["yT"], d["YT"], d["G"]
    v = np.random.default_rng(1).standard_normal(TALL[1])
    cfg = minimize.Parameters("dual_newton")
    cfg.update(verbose=False)
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_dense_panels()
        direct = ctx.opt_dual_newton_logw(G, G, THETA, PARAMS)
    with optimize.resident(yT, YT):
        ctx = c_bioen._HELD[id(yT)][1]
        assert ctx.dense_panels is False
        out = log_weights.find_optimum(G.reshape(-1, 1), G.reshape(-1, 1), yT, yT, YT.reshape(1, -1), THETA, cfg)
        info = dict(c_bioen.last_opt_info)
        assert info["status"] == 0 and counts(info) == counts(direct)
        assert out[4] == direct["fmin"] and np.array_equal(info["g"], direct["g"])
        # the switch is back as the holder left it: the old refusal
        assert ctx.dense_panels is False
        estate(lambda: ctx.logw_cov(g=G, G=G, theta=THETA), "bioen_logwn_cov", "M <= 1024")
        log_weights.find_optimum_series(G.reshape(-1, 1), G.reshape(-1, 1), yT, yT, YT.reshape(1, -1), [100.0, THETA], cfg)
        assert [r["status"] for r in c_bioen.last_opt_info] == [0, 0] and ctx.dense_panels is False
        # a holder's own setting stays
        ctx.set_dense_panels()
        log_weights.find_optimum(G.reshape(-1, 1), G.reshape(-1, 1), yT, yT, YT.reshape(1, -1), THETA, cfg)
        assert ctx.dense_panels is True
        # with the switch on the other dense entries keep their words, and the point of a run is the kept point
        forms, before = ctx.footprint()
        res = ctx.opt_dual_newton_logw(G, G, THETA, PARAMS)
        assert np.array_equal(res["g"], direct["g"])
        C, hv = ctx.logw_cov(), ctx.logw_hessp(v)
        C2, f2, _ = ctx.logw_cov(g=res["g"], G=G, theta=THETA)
        assert np.array_equal(C, C2) and f2 == res["fmin"] and np.array_equal(ctx.logw_hessp(v), hv)
        estate(lambda: ctx.logw_laplace(theta=THETA), "bioen_logwn_laplace", "M <= 1024")
        estate(lambda: ctx.opt_dual_newton_logw_profile_series([THETA], G, G, PARAMS), "bioen_logwn_profile_series", "M <= 1024")
        estate(lambda: ctx.forces_gram(forces=np.zeros(TALL[0]), w0=np.exp(G), theta=THETA), "M <= 1024")
        assert np.array_equal(ctx.logw_cov(), C)                          # (refused calls leave the point alone)


def test_the_buffer_is_the_plans_and_is_in_the_footprint(bioen_amd):
    d = data(TALL)
    with bioen_amd.Context(d["yT"], d["YT"]) as ctx:
        ctx.set_dense_panels()
        ctx.logw_cov(g=d["g"], G=d["G"], theta=THETA, cov=False)         # only sets the point
        forms, before = ctx.footprint()
        assert "logw_gram" not in forms
        ctx.logw_cov()
        forms, after = ctx.footprint()
        assert "logw_gram" in forms and after - before == plan_bytes(ctx, TALL[0])
        ctx.logw_cov_bf16()                                              # the split pass's sets go where the FP64 pass's went
        assert ctx.footprint() == (forms, after)


def test_refusals(bioen_amd, monkeypatch):
    d = data(TALL)
    yT, YT, G = d["yT"], d["YT"], d["G"]
    calls = (("bioen_logwn_cov", lambda c: c.logw_cov(g=G, G=G, theta=THETA)),
             ("bioen_logwn_cov_bf16", lambda c: c.logw_cov_bf16(g=G, G=G, theta=THETA)),
             ("bioen_logwn_opt", lambda c: c.opt_dual_newton_logw(G, G, THETA)),
             ("bioen_logwn_series", lambda c: c.opt_dual_newton_logw_series([THETA], G, G)))
    with bioen_amd.Context(yT, YT) as ctx:                              # the switch off: the old refusal
        for name, call in calls:
            estate(lambda: call(ctx), name, "M <= 1024")
        ctx.set_dense_panels()
        ctx.set_dense_panels(False)
        estate(lambda: calls[0][1](ctx), "bioen_logwn_cov", "M <= 1024")
        assert "logw_gram" not in ctx.footprint()[0]
    rng = np.random.default_rng(4100)                                    # beyond four panels: the refusal names 4096
    big, bigY = rng.standard_normal((4100, 64)) + 3.0, rng.standard_normal(4100) + 3.0
    Gb = np.full(64, -np.log(64.0))
    with bioen_amd.Context(big, bigY) as ctx:
        ctx.set_dense_panels()
        for name, call in (("bioen_logwn_cov", lambda: ctx.logw_cov(g=Gb, G=Gb, theta=THETA)),
                           ("bioen_logwn_cov_bf16", lambda: ctx.logw_cov_bf16(g=Gb, G=Gb, theta=THETA)),
                           ("bioen_logwn_opt", lambda: ctx.opt_dual_newton_logw(Gb, Gb, THETA)),
                           ("bioen_logwn_series", lambda: ctx.opt_dual_newton_logw_series([THETA], Gb, Gb))):
            estate(call, name, "4096")
        assert "logw_gram" not in ctx.footprint()[0]
    monkeypatch.setenv("BIOEN_HIP_PANELS", "0")                          # the panels' strip copies must be resident
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_dense_panels()
        f0, _ = ctx.logw_fdf(G, G, THETA)
        assert np.isfinite(f0)
        for name, call in calls:
            estate(lambda: call(ctx), name, "strip copies")
    monkeypatch.delenv("BIOEN_HIP_PANELS")
    monkeypatch.setenv("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", "1")           # the streaming fallback
    with bioen_amd.Context(yT, YT) as ctx:
        ctx.set_dense_panels()
        ctx.logw_fdf(G, G, THETA)
        for name, call in calls:
            estate(lambda: call(ctx), name, "strip copies")

"""GPU tests of the STREAMING PAIR on the row-major matrix (csrc/kernels_matrix.hip: k_fwd_partial / k_adj and their row
reductions) where A COLUMN TILE RUNS MANY 128-COLUMN STEPS -- tests/test_hip_strip_loops.py's question for the third pass
family, the one a context runs on whenever it has no strip copies: an allocation failed while they were built (the device
was full), M > 16384 (more than kMaxPanels row panels), BIOEN_HIP_PANELS=0, BIOEN_HIP_FWD_STREAM=1.  api.hip's
choose_fwd_tiling makes tiles of one step, rounded up to two, at every other file's streaming shape (N <= 4000).  New here:

  k_fwd_partial, K <= 6      the software-pipelined loop through three and more turns, its refill `loadY(ya, t + 2)`, the
                             odd-count tail on a refilled register set (a last tile of 5 steps)
  k_fwd_partial, K = 7, 8    the plain loop through 4, 6, 10 and 16 steps
  the segment clamp          a segment's last tile cut to one step where the other tiles run 4 and 10
  the NT instantiations      more than 192 MiB per context (non-temporal loads), held bit for bit to the cached-load ones by
                             the thread ranks, whose share of the same matrix is below the threshold
  k_adj                      528 and 4104 rows per wave: the LDS operand staging of K = 4 ... 7 restaged 17 and 129 times, a
                             ragged last staging of 16 and of 8 rows; the forces method's passes through it (F1, F3)
  k_fwd_rows_local           its grid capped at kMaxPartials, several rows per wave (16400 rows)

Every test asserts its regime first and from the library: the plan through Context.strip_plan(2) (the context fields the
launchers pass), then, after the first evaluation (the copies are built lazily), footprint() == {"rowmajor"} and one forward
and one adjoint launch per pass through kernel_stats -- no strip copies, no row panels.  STREAM_REGIMES is the table.

Data, truth and gates are those of tests/test_hip_strip_loops.py (its helpers, imported; the 80-bit values are cached per
shape there, and three of the four shapes are that file's and tests/test_hip_panel_loops.py's): rel(f) < 1e-12, gradients
1e-10 max|grad| or gradient_ok's condition clause, products 1e-10 S, bit equality wherever the project claims it."""
import numpy as np
import pytest

from test_hip_edgecases import rel
from test_hip_forces_hessp import estate
from test_hip_panel_loops import case_id, check_forces_column, check_logw, hessp_problem, launches
from test_hip_strip_loops import (CAPPED, LOGW_THETA, THETAS, assert_ranks_equal_single, data, forces_average_truth,
                                  forces_truth, logw_problem, logw_truth, on_thread_ranks, ordered, stat)

pytestmark = pytest.mark.gpu

L = np.longdouble
ODD, CLAMPED, RAGGED, DEEP = (1024, 9000), (1024, 33700), (2100, 9000), (16400, 2000)
SHARDED = (1100, 33700)                 # the refusal of the forces method: two ranks whose tiles are still four steps
NO_COPIES = {"BIOEN_HIP_TEST_FAIL_STRIP_ALLOC": "1"}       # the first allocation of a strip copy fails: a full device
# shape -> how it gets onto the family, segments (1: BIOEN_HIP_SEGMENTS=1), plan = (sps: steps per segment, gs: tiles per
# segment, tc: steps per tile, nch: rows a wave of k_adj walks, nt), and the condition that makes it this file's shape --
# on the plan p and `last`, the steps of a segment's last tile after the clamp
STREAM_REGIMES = {
    # three turns of the pipelined loop with the refill taken; the tail runs on a refilled register set; cached loads
    ODD: dict(env=NO_COPIES, segments=1, plan=(71, 12, 6, 256, 0),
              regime=lambda p, last: p["tc"] >= 6 and last >= 3 and last % 2 == 1 and p["fold"] == 0),
    # the clamp cuts the last tile of all eight segments to one step; the NT instantiations
    CLAMPED: dict(env=NO_COPIES, segments=8, plan=(33, 9, 4, 256, 1),
                  regime=lambda p, last: p["tc"] >= 4 and last == 1 and p["fold"] == 1),
    # ten steps per tile, the last tile one; k_adj's last LDS staging is of 16 rows
    RAGGED: dict(env={"BIOEN_HIP_PANELS": "0"}, segments=1, plan=(71, 8, 10, 528, 0),
                 regime=lambda p, last: p["tc"] == 10 and last == 1 and p["nch"] % 32 == 16 and p["fold"] == 0),
    # 17 row panels: one tile of 16 steps; 513 turns of k_adj, 129 stagings, the last of 8 rows; k_fwd_rows_local's grid
    # (nch blocks, capped at kMaxPartials = 1024) with several rows per wave; NT
    DEEP: dict(env={}, segments=1, plan=(16, 1, 16, 4104, 1),
               regime=lambda p, last: p["gs"] == 1 and p["tc"] == 16 and p["nch"] % 32 == 8 and p["nch"] > 1024
               and p["fold"] == 1),
    # (tests/test_hip_panel_loops.py's shape on the streaming pair: a rank of two holds four segments of 33 steps)
    SHARDED: dict(env={"BIOEN_HIP_PANELS": "0"}, segments=8, plan=(33, 9, 4, 280, 1),
                  regime=lambda p, last: p["tc"] >= 4 and last == 1),
}
SHAPES = [ODD, CLAMPED, RAGGED, DEEP]
SERIES_SHAPES = [CLAMPED, RAGGED]
FORCES_CASES = [(ODD, "generated"), (CLAMPED, "generated"), (CLAMPED, "ascending"), (CLAMPED, "descending"),
                (RAGGED, "generated"), (DEEP, "generated")]


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


# ---- regimes ---------------------------------------------------------------------------------------------------------
def enter_regime(monkeypatch, shape):
    """the environment a shape's contexts are created in"""
    want = STREAM_REGIMES[shape]
    for name, value in want["env"].items():
        monkeypatch.setenv(name, value)
    if want["segments"] == 1:
        monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")


def assert_stream_regime(ctx, shape, local_segments=None):
    """the plan of the streaming pair from the library, not recomputed: the table's, and the table's condition.  A thread
    rank holds local_segments of the eight segments and at most 138 MB of the matrix: cached loads"""
    want, p = STREAM_REGIMES[shape], ctx.strip_plan(2)
    sps, gs, tc, nch, nt = want["plan"]
    on_a_rank = local_segments is not None and local_segments != want["segments"]
    assert p["local_segments"] == (local_segments if on_a_rank else want["segments"]), p
    assert (p["sps"], p["gs"], p["tc"], p["nch"]) == (sps, gs, tc, nch), p
    assert p["fold"] == (0 if on_a_rank else nt), p
    last = p["sps"] - (p["gs"] - 1) * p["tc"]
    assert p["tc"] > 2 and 0 < last <= p["tc"], p               # a tile of more than the two steps of every other file
    assert want["regime"](dict(p, fold=nt), last), (p, last)
    return p


def enter_stream(ctx, shape, call, passes=(1, 1), local_segments=None):
    """the regime of a test, before its first numerical assertion: the plan; then `call`, an evaluation of passes =
    (forward, adjoint) matrix passes (logw_fdf: 1, 1; forces_fdf: 2, 2), made that many launches -- no row panels -- and
    left the row-major matrix as the only resident form.  -> call()"""
    assert_stream_regime(ctx, shape, local_segments)
    out, n = launches(ctx, call)
    assert n == passes, n
    assert ctx.footprint()[0] == {"rowmajor"}
    return out


# ---- (a) against the high-precision value ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,order", FORCES_CASES, ids=case_id)
def test_forces_batches_of_every_width_against_longdouble(bioen_amd, monkeypatch, shape, order):
    """forces_fdf_batch at K = 1 ... 8 on the first K problems: every column within 1e-12 / gradient_ok of the 80-bit value
    and bit for bit the single call's -- which holds k_adj's LDS-staged operands (K = 4 ... 7) to the scalar path of K = 1
    and k_fwd_partial's plain loop (K = 7, 8) to the pipelined one, in F1 / F3 and F2 / the centred pass 4.  1024 x 33700:
    columns as generated and sorted by x both ways.  Then last_average: refused after the K = 8 call, and after the single
    call of problem 0 yTilde . w of the truth at tests/test_hip_panel_loops.py's gate"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, F, th = ordered(shape, order)
    forces_truth(shape)
    worst_f = worst_g = 0.0
    with bioen_amd.Context(yT, YT) as ctx:
        first = enter_stream(ctx, shape, lambda: ctx.forces_fdf(F[0], w0, th[0]), passes=(2, 2))
        single = [first] + [ctx.forces_fdf(F[a], w0, th[a]) for a in range(1, 8)]
        for K in range(1, 9):
            (fb, gb), n = launches(ctx, lambda: ctx.forces_fdf_batch(F[:K], w0, th[:K]))
            assert n == (2, 2), (K, n)
            for a in range(K):
                err_f, err_g = check_forces_column(shape, a, fb[a], gb[a])
                worst_f, worst_g = max(worst_f, err_f), max(worst_g, err_g)
                assert fb[a] == single[a][0] and np.array_equal(gb[a], single[a][1]), (K, a)
        with pytest.raises(bioen_amd.BioenHipError):
            ctx.last_average()
        f0, g0 = ctx.forces_fdf(F[0], w0, th[0])
        assert f0 == fb[0] and np.array_equal(g0, gb[0])
        yraw, yeff = ctx.last_average()
        ref = forces_average_truth(shape)[0]
        err_y = float(np.abs(yraw - ref).max() / np.abs(ref).max())
        assert err_y <= 1e-12 and np.array_equal(yraw, yeff), err_y
        assert ctx.footprint()[0] == {"rowmajor"}
    print("forces %dx%d %s: worst rel(f) %.3g, worst |grad - ld| %.3g max|grad|, |ybar - ld| %.3g max|ybar|"
          % (shape + (order, worst_f, worst_g, err_y)))


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_logw_evaluation_and_products_against_longdouble(bioen_amd, monkeypatch, shape):
    """logw_fdf to 1e-12 / 1e-10 max|grad|; logw_hessp with k = 1 ... 8 directions at the kept point to 1e-10 S, a
    direction's bits the same at any width; one forward and one adjoint launch per pass"""
    enter_regime(monkeypatch, shape)
    yT, YT, G, x, pool = logw_problem(shape)
    f_true, g_true, hv_true = logw_truth(shape)
    S = float(np.abs(hv_true).max())
    with bioen_amd.Context(yT, YT) as ctx:
        f, grad = enter_stream(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        (hv8, f2, grad2), n = launches(ctx, lambda: ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA))
        assert n == (2, 2), n                                                    # the evaluation and the product
        err_f, err_g, worst = check_logw(shape, f, grad, hv8)
        assert f2 == f and np.array_equal(grad2, grad)
        for k in range(1, 9):
            got, n = launches(ctx, lambda: ctx.logw_hessp(pool[8 - k:] if k > 1 else pool[7]))
            assert n == (1, 1), (k, n)
            want = hv_true[8 - k:] if k > 1 else hv_true[7]
            assert got.shape == want.shape
            worst = max(worst, float(np.abs(got - want).max()) / S)
            assert np.array_equal(got, hv8[8 - k:] if k > 1 else hv8[7]), k      # a direction's bits: any width
        assert ctx.footprint()[0] == {"rowmajor"}
    print("logw %dx%d: rel(f) %.3g, |grad - ld| %.3g max|grad|, worst |hv - ld| %.3g S" % (shape + (err_f, err_g, worst)))
    assert worst <= 1e-10


@pytest.mark.parametrize("shape", [ODD, DEEP], ids=case_id)
def test_chi_squared_of_the_longdouble_weights(bioen_amd, monkeypatch, shape):
    """chi_squared (api.hip's K = 1 forward launch, uncentred) of the 80-bit softmax weights: 0.5 |y w - Y|^2 against
    y @ w in longdouble at the scalar gate, yave at last_average's"""
    enter_regime(monkeypatch, shape)
    yT, YT, G, x, pool = logw_problem(shape)
    xl = x.astype(L)
    e = np.exp(xl - xl.max())
    w = (e / e.sum()).astype(np.float64)
    ref = yT.astype(L) @ w.astype(L)
    chi_ref = float(L(0.5) * ((ref - YT.astype(L)) ** 2).sum())
    ref = ref.astype(np.float64)
    with bioen_amd.Context(yT, YT) as ctx:
        chi2, yave = enter_stream(ctx, shape, lambda: ctx.chi_squared(w), passes=(1, 0))
        err_y = float(np.abs(yave - ref).max() / np.abs(ref).max())
        print("chi_squared %dx%d: rel(chi2) %.3g, |yave - ld| %.3g max|yave|" % (shape + (rel(chi2, chi_ref), err_y)))
        assert rel(chi2, chi_ref) < 1e-12, (chi2, chi_ref)
        assert err_y <= 1e-12, err_y
        chi2b, yaveb = ctx.chi_squared(w)
        assert chi2b == chi2 and np.array_equal(yaveb, yave)


# ---- (b) bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_ls", ["0", "1"])
@pytest.mark.parametrize("shape", SERIES_SHAPES, ids=case_id)
def test_logw_series_equals_its_single_runs(bioen_amd, monkeypatch, shape, device_ls):
    enter_regime(monkeypatch, shape)
    monkeypatch.setenv("BIOEN_HIP_DEVICE_LS", device_ls)
    yT, YT, G, x, pool = logw_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        enter_stream(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        res, w, infos = ctx.opt_lbfgs_logw_batch(THETAS, x, G, CAPPED, max_batch=8)
        for a in range(8):
            g1, w1, i1 = ctx.opt_lbfgs_logw(x, G, THETAS[a], CAPPED)
            assert stat([infos[a]]) == stat([i1]), a
            assert np.array_equal(res[a], g1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) >= 5
        assert ctx.footprint()[0] == {"rowmajor"}


@pytest.mark.parametrize("shape", SERIES_SHAPES, ids=case_id)
def test_forces_series_equals_its_single_runs(bioen_amd, monkeypatch, shape):
    enter_regime(monkeypatch, shape)
    yT, YT, w0, F, th = ordered(shape, "generated")
    with bioen_amd.Context(yT, YT) as ctx:
        enter_stream(ctx, shape, lambda: ctx.forces_fdf(F[0], w0, th[0]), passes=(2, 2))
        res, w, infos = ctx.opt_lbfgs_forces_batch(th, 0.2 * F[0], w0, CAPPED, max_batch=8)
        for a in range(8):
            f1, w1, i1 = ctx.opt_lbfgs_forces(0.2 * F[0], w0, th[a], CAPPED)
            assert stat([infos[a]]) == stat([i1]), a
            assert np.array_equal(res[a], f1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) >= 5
        assert ctx.footprint()[0] == {"rowmajor"}


def everything(ctx, shape, n_theta, forces=True, local_segments=None):
    """what neither a second call, a second context nor (log-weights) the GPU count may change: logw_fdf, logw_hessp at
    k = 8, a capped series of n_theta thetas; forces_fdf_batch at K = 8 and a capped series of the forces method"""
    yT, YT, G, x, pool = logw_problem(shape)
    out = {}
    out["f"], out["grad"] = enter_stream(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA), local_segments=local_segments)
    out["hv"], _, _ = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
    out["res"], out["w"], infos = ctx.opt_lbfgs_logw_batch(THETAS[:n_theta], x, G, CAPPED, max_batch=8)
    out["stat"] = np.array(stat(infos))
    if forces:
        _, _, w0, F, th = ordered(shape, "generated")
        out["forces f"], out["forces grad"] = ctx.forces_fdf_batch(F, w0, th)
        out["forces res"], out["forces w"], infos = ctx.opt_lbfgs_forces_batch(th[:n_theta], 0.2 * F[0], w0, CAPPED, max_batch=8)
        out["forces stat"] = np.array(stat(infos))
    assert ctx.footprint()[0] == {"rowmajor"}
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_a_second_call_and_a_second_context_give_the_same_bits(bioen_amd, monkeypatch, shape):
    """every reduction of the family has a fixed shape (kernels_matrix.hip's header): run to run, context to context"""
    enter_regime(monkeypatch, shape)
    yT, YT = data(shape)[:2]
    with bioen_amd.Context(yT, YT) as ctx:
        first = everything(ctx, shape, 3)
        assert_ranks_equal_single([everything(ctx, shape, 3)], first)
    with bioen_amd.Context(yT, YT) as ctx:
        assert_ranks_equal_single([everything(ctx, shape, 3)], first)


_SINGLE = {}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [8, 2])
def test_logw_thread_ranks_equal_the_single_context(bioen_amd, monkeypatch, world):
    """1024 x 33700 with no strip copies on any rank (the switch is process-wide: every rank falls back together): a rank
    runs the tiles of its 8 // world segments, each with its clamped last tile, and the cached-load instantiations (34 and
    138 MB); the single context runs all 72 tiles and the NT ones -- "the GPU count changes no bit" where a tile is four
    steps, and "NT changes no bit": logw_fdf, logw_hessp at k = 8, a five-theta capped series"""
    shape = CLAMPED
    enter_regime(monkeypatch, shape)
    yT, YT = data(shape)[:2]
    if shape not in _SINGLE:
        with bioen_amd.Context(yT, YT) as ctx:
            assert ctx.strip_plan(2)["fold"] == 1
            _SINGLE[shape] = everything(ctx, shape, 5, forces=False)

    def workload(ctx, local_segments):
        assert local_segments == 8 // world and ctx.strip_plan(2)["fold"] == 0
        return everything(ctx, shape, 5, forces=False, local_segments=local_segments)

    assert_ranks_equal_single(on_thread_ranks(bioen_amd, world, yT, YT, workload), _SINGLE[shape])


@pytest.mark.timeout(600)
def test_forces_method_stays_refused_on_a_sharded_streaming_context(bioen_amd, monkeypatch):
    """held by tests/test_hip_panel_loops.py past the panel limit; here with BIOEN_HIP_PANELS=0 at 1100 x 33700: two thread
    ranks on four-step tiles are told that the strip copies are missing, and stay on the row-major matrix"""
    shape = SHARDED
    enter_regime(monkeypatch, shape)
    yT, YT, G, w0, f = data(shape)[:5]

    def workload(ctx, local_segments):
        assert_stream_regime(ctx, shape, local_segments=local_segments)
        assert local_segments == 4
        estate(lambda: ctx.forces_fdf(f, w0, 10.0), "needs the strip copies")
        assert ctx.footprint()[0] == {"rowmajor"}
        return {"refused": 1}

    assert_ranks_equal_single(on_thread_ranks(bioen_amd, 2, yT, YT, workload), {"refused": 1})


# ---- (c) the fallback itself, at depth -----------------------------------------------------------------------------------
def test_fallback_keeps_the_matrix_and_refuses_the_forces_products(bioen_amd, monkeypatch):
    """1024 x 9000 after the first strip-copy allocation failed: read_ytilde returns the caller's numbers after evaluations
    of both methods; forces_hessp and forces_gram are refused with BIOEN_HIP_ESTATE (the streaming kernels have neither
    product); the context then answers with the bits it gave before"""
    shape = ODD
    enter_regime(monkeypatch, shape)
    yT, YT, G, x, pool = logw_problem(shape)
    _, _, w0, F, th = ordered(shape, "generated")
    fh, V = hessp_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        f, grad = enter_stream(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        ff, fg = ctx.forces_fdf(F[0], w0, th[0])
        assert np.array_equal(ctx.read_ytilde(), yT)
        r0, c0, rows, cols = 1000, shape[1] // 3, 17, 37
        assert np.array_equal(ctx.read_ytilde(r0, rows, c0, cols), yT[r0:r0 + rows, c0:c0 + cols])
        estate(lambda: ctx.forces_hessp(V[0], forces=fh, w0=w0, theta=10.0), "bioen_hip_forces_hessp", "streaming")
        estate(lambda: ctx.forces_hessp(V[0]), "bioen_hip_forces_hessp", "streaming")
        estate(lambda: ctx.forces_gram(forces=fh, w0=w0, theta=10.0), "bioen_hip_forces_gram", "streaming")
        ff2, fg2 = ctx.forces_fdf(F[0], w0, th[0])
        assert ff2 == ff and np.array_equal(fg2, fg)
        f2, grad2 = ctx.logw_fdf(x, G, LOGW_THETA)
        assert f2 == f and np.array_equal(grad2, grad)
        assert ctx.footprint()[0] == {"rowmajor"}
        assert np.array_equal(ctx.read_ytilde(), yT)

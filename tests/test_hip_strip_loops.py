"""GPU tests of the strip passes (csrc/kernels_strip512.hip: k_strip, kernels_strip1024.hip: k_strip2, kernels_strip_logw.hip:
k_strip_fwd / k_strip_adj) where ONE BLOCK SLOT RUNS SEVERAL STRIPS OF A COLUMN SEGMENT -- the regime of every production
size, which the small-shape tests (N <= 9000: one strip per group and segment, one strip per forward chunk) never enter:

  k_strip, DEPTH 3 (K > 4)   the deferred row-sum product of strip s running beside P2 of strip s + 1 on the other parity's
                             tv / scale buffers (`if (!first) p3(...)`)
  k_strip, DEPTH 2           the two register sets alternating through segments of odd length
  k_strip / k_strip2         the online softmax carried from strip to strip: accumulators rescaled by 0 < sc < 1, the wave-wide
                             skip when no maximum moved, a wave whose problems disagree about it
  k_strip_fwd, fold          chunk ends with tc >= 2, a group's shorter last chunk, the empty last chunk of a short group
  canonical order            "the GPU count changes no bit" where a chunk is more than one strip

Every test first asserts its regime through Context.strip_plan (bioen_hip_ctx_strip_plan: what the launchers compute), so
a later change of the launch plan cannot silently turn it back into a one-strip test.  REGIMES is the table.

Data: SURVEY 8(d)'s recipe (tests/test_hip_hessp.py: recipe), non-uniform prior.  Forces: one vector f scaled so that
x = yTilde^T f has standard deviation 5; the eight problems of a batch are s f, s in SCALES, with eight thetas.  Column
orders (ORDERS): as generated; sorted by x ascending -- every strip of a group raises the running maximum of the problems
with s > 0 and rescales what came before, while those with s < 0 never move after a segment's first strip and s = 0 never
moves at all, all in one wave --; sorted descending, the mirror image.

The truth is the formula of DESIGN section 2 (6b for the products) in numpy.longdouble, written out below, computed once
per shape and cached.  A forces value and gradient do not depend on the order of the columns, so the three orders of a
shape share one truth (its own sums differ by the order at 1e-19).  Gates, the project's own: rel(f) < 1e-12, gradients
1e-10 max|grad| of the truth or test_hip_edgecases.gradient_ok's condition-number clause, products 1e-10 S, and bit
equality wherever the project claims it."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import LBFGS_DEFAULTS
from test_hip_edgecases import gradient_ok, rel
from test_hip_hessp import recipe

pytestmark = pytest.mark.gpu

L = np.longdouble
SCALES = (1.0, 0.5, -1.0, -0.5, 0.25, 2.0, -2.0, 0.0)
THETAS = (10.0, 0.3, 100.0, 3.0, 1.0, 30.0, 0.1, 1000.0)
ORDERS = ("generated", "ascending", "descending")
CAPPED = dict(LBFGS_DEFAULTS, max_iterations=10)
LOGW_THETA = 10.0

# shape -> segments (1: BIOEN_HIP_SEGMENTS=1), forces (gs, most strips of a group per segment; the other groups one fewer),
# forward (gs, tc, nch, fold); None: the pass is not under test at this shape
REGIMES = {
    (64, 131500): dict(segments=8, forces=(1024, 2), forward=(128, 2, 5, 1)),     # k_strip, 2 waves, four blocks per CU
    (160, 70000): dict(segments=8, forces=(512, 2), forward=(128, 1, 5, 1)),      # k_strip, 4 waves (3 live)
    (300, 66000): dict(segments=8, forces=(256, 3), forward=(96, 1, 6, 1)),       # k_strip, 5 waves, mps = 304; odd tg
    (600, 33700): dict(segments=8, forces=(256, 2), forward=(32, 2, 5, 1)),       # k_strip2, ragged last wave
    (1024, 33700): dict(segments=8, forces=(256, 2), forward=(32, 2, 5, 1)),      # log-weights: 16 full waves, chunks 2 2 2 2 1 | 2 2 2 2 0
    (300, 9000): dict(segments=1, forces=(256, 3), forward=(96, 1, 6, 0)),        # the same loops with no flush inside them
    (1024, 9000): dict(segments=1, forces=(256, 3), forward=(32, 3, 6, 0)),
    # three strips per group on the 2- and 4-wave blocks too: a deferred product whose rescale factor is not a segment's
    # first (that one multiplies accumulators that are zero) needs a third strip
    (64, 33000): dict(segments=1, forces=(1024, 3), forward=None),
    (160, 17000): dict(segments=1, forces=(512, 3), forward=None),
}
K_STRIP_SHAPES = [(64, 131500), (160, 70000), (300, 66000), (300, 9000), (64, 33000), (160, 17000)]
SORTED_SHAPES = [(300, 66000), (600, 33700)]
FORCES_CASES = [(s, o) for s in [(64, 131500), (160, 70000), (300, 66000), (600, 33700), (300, 9000), (64, 33000), (160, 17000)]
                for o in (ORDERS if s in SORTED_SHAPES else ORDERS[:1])]
LOGW_SHAPES = [(1024, 33700), (64, 131500), (1024, 9000)]
FOLDED_SHAPES = [(1024, 33700), (64, 131500)]


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


# ---- regimes ---------------------------------------------------------------------------------------------------------
def enter_regime(monkeypatch, shape, regimes=None):
    """the environment a shape's contexts are created in (regimes: another file's table, tests/test_hip_panel_loops.py)"""
    if (regimes or REGIMES)[shape]["segments"] == 1:
        monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")


def assert_forces_regime(ctx, shape, local_segments=None):
    """some groups of the forces passes run tg >= 2 strips of a segment, the others tg - 1: from the plan, not recomputed"""
    want, p = REGIMES[shape], ctx.strip_plan(1)
    gs, tg = want["forces"]
    assert p["local_segments"] == (want["segments"] if local_segments is None else local_segments), p
    assert (p["gs"], p["tc"]) == (gs, tg) and tg >= 2, p
    long_groups = p["sps"] - p["gs"] * (p["tc"] - 1)           # groups g < long_groups own strips g, g + gs, ..., tg of them
    assert 0 < long_groups < p["gs"], p
    if shape == (300, 66000):
        # the last segment's valid columns end inside its groups' second strips: a group's third strip there is padding only
        valid = -(-(shape[1] - 7 * p["sps"] * 16) // 16)
        assert p["gs"] < valid <= 2 * p["gs"] < p["sps"], (p, valid)
    return p


def assert_forward_regime(ctx, shape, fold=None, local_segments=None, regimes=None):
    want, p = (regimes or REGIMES)[shape], ctx.strip_plan(0)
    gs, tc, nch, dflt_fold = want["forward"]
    assert p["local_segments"] == (want["segments"] if local_segments is None else local_segments), p
    assert (p["gs"], p["tc"], p["nch"]) == (gs, tc, nch), p
    assert p["fold"] == (dflt_fold if fold is None else fold), p
    tmax = -(-p["sps"] // p["gs"])
    assert tmax >= 2, p                                         # a slot's second strip of a segment
    if tc >= 2 and want["segments"] == 8:
        # groups of tmax strips end on a shorter chunk, groups of tmax - 1 on an empty one
        long_groups = p["sps"] - p["gs"] * (tmax - 1)
        last_of_long, last_of_short = tmax - tc * (nch - 1), tmax - 1 - tc * (nch - 1)
        assert 0 < long_groups < p["gs"] and 0 < last_of_long < tc and last_of_short == 0, p
    return p


# ---- data and the truth, once per shape ------------------------------------------------------------------------------
_DATA, _FORCES_TRUTH, _FORCES_YBAR, _LOGW_TRUTH, _DEFAULT_BITS = {}, {}, {}, {}, {}


def data(shape):
    """-> yTilde, YTilde, G (log prior), w0, f (x = yTilde^T f has standard deviation 5), x"""
    if shape not in _DATA:
        M, N = shape
        yT, YT, G = recipe(M, N, 1000 * M + N)
        f = np.random.default_rng(5 + M).standard_normal(M)
        x = f @ yT
        f *= 5.0 / x.std()
        _DATA[shape] = (yT, YT, G, np.exp(G), f, f @ yT)
    return _DATA[shape]


def ordered(shape, order):
    """-> yTilde, YTilde, w0, F[8, M], thetas[8] with the columns in `order`"""
    yT, YT, G, w0, f, x = data(shape)
    F, th = np.outer(SCALES, f), np.array(THETAS)
    if order == "generated":
        return yT, YT, w0, F, th
    perm = np.argsort(x, kind="stable")
    if order == "descending":
        perm = perm[::-1]
    xs = x[perm]
    assert (np.diff(xs) >= 0).all() if order == "ascending" else (np.diff(xs) <= 0).all()
    return np.ascontiguousarray(yT[:, perm]), YT, np.ascontiguousarray(w0[perm]), F, th


def forces_truth(shape):
    """DESIGN section 2, forces, in 80-bit arithmetic for the eight problems: -> [(L, grad, cond())]; cond: the gradient's
    condition (test_hip_edgecases), formed only where the plain gate is missed"""
    if shape in _FORCES_TRUTH:
        return _FORCES_TRUTH[shape]
    yT, YT, G, w0, f, _ = data(shape)
    yl, Yl, w0l = yT.astype(L), YT.astype(L), w0.astype(L)
    x1 = f.astype(L) @ yl
    def one(s, theta):
        x = L(s) * x1
        e = w0l * np.exp(x - x.max())
        w = e / e.sum()
        ybar = yl @ w
        r = ybar - Yl
        lw = np.log(w) - np.log(w0l)
        t = (L(theta) * (1 + lw) + r @ yl) * w
        grad = np.array([(yl[i] - ybar[i]) @ t for i in range(shape[0])])
        obj = L(theta) * (w * lw).sum() + L(0.5) * (r * r).sum()

        def cond():
            return (np.abs(yT.astype(L) - Yl[:, None]) @ np.abs(t) + np.abs(r) * abs(t.sum())).astype(np.float64)
        return float(obj), grad.astype(np.float64), cond, ybar.astype(np.float64)
    with ThreadPoolExecutor(8) as pool:                         # (numpy's longdouble products release the interpreter lock)
        out = list(pool.map(one, SCALES, THETAS))
    _FORCES_TRUTH[shape] = [o[:3] for o in out]
    _FORCES_YBAR[shape] = [o[3] for o in out]
    return _FORCES_TRUTH[shape]


def forces_average_truth(shape):
    """yTilde . w of the eight problems, from the same 80-bit evaluation (Context.last_average is held to it)"""
    forces_truth(shape)
    return _FORCES_YBAR[shape]


def logw_problem(shape):
    yT, YT, G = data(shape)[:3]
    N = shape[1]
    rng = np.random.default_rng(77 + shape[0])
    x = G + 0.3 * rng.standard_normal(N)
    pool = rng.standard_normal((8, N))
    pool[6] = 1.0                       # v = 1: H 1 = 0
    pool[7] = 0.0
    pool[7, N // 3] = 1.0               # a unit vector: one column of H
    return yT, YT, G, x, pool


def logw_truth(shape):
    """DESIGN sections 2 and 6b, log-weights, in 80-bit arithmetic at theta = LOGW_THETA: -> (L, grad, H pool)"""
    if shape in _LOGW_TRUTH:
        return _LOGW_TRUTH[shape]
    yT, YT, G, x, pool = logw_problem(shape)
    y, xl, Gl, Yl, theta = yT.astype(L), x.astype(L), G.astype(L), YT.astype(L), L(LOGW_THETA)

    def lse(v):
        return v.max() + np.log(np.exp(v - v.max()).sum())
    e = np.exp(xl - xl.max())
    w = e / e.sum()
    ybar = y @ w
    r = ybar - Yl
    dev = xl - Gl
    P = w @ dev
    obj = theta * (P - lse(xl) + lse(Gl)) + L(0.5) * (r * r).sum()
    grad = w * (theta * (dev - P) + (r @ y - ybar @ r))
    def product(v):
        dv = v - w @ v
        dr = y @ (w * dv)
        return dv * grad + w * (theta * dv + (dr @ y - ybar @ dr) - v @ grad)
    with ThreadPoolExecutor(8) as workers:
        hv = list(workers.map(product, pool.astype(L)))
    _LOGW_TRUTH[shape] = (float(obj), grad.astype(np.float64), np.array(hv).astype(np.float64))
    return _LOGW_TRUTH[shape]


def stat(infos):
    return [(i.fmin, i.iterations, i.evaluations, i.lbfgs_code, i.chi2, i.kl) for i in infos]


# ---- (a) against the high-precision value; a batch column = the single call ------------------------------------------
@pytest.mark.parametrize("shape,order", FORCES_CASES, ids=case_id)
def test_forces_batches_of_every_width_against_longdouble(bioen_amd, monkeypatch, shape, order):
    """forces_fdf_batch at K = 1 ... 8 on the first K problems: every column within 1e-12 / gradient_ok of the 80-bit value,
    and bit for bit the single call's -- K <= 4 runs the two register sets (DEPTH 2), K > 4 the deferred row-sum product
    (DEPTH 3); 600 rows: k_strip2"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, F, th = ordered(shape, order)
    truth = forces_truth(shape)
    worst_f = worst_g = 0.0
    with bioen_amd.Context(yT, YT) as ctx:
        assert_forces_regime(ctx, shape)
        single = [ctx.forces_fdf(F[a], w0, th[a]) for a in range(8)]
        for K in range(1, 9):
            fb, gb = ctx.forces_fdf_batch(F[:K], w0, th[:K])
            for a in range(K):
                f_true, g_true, cond = truth[a]
                err = float(np.abs(gb[a] - g_true).max() / np.abs(g_true).max())
                worst_f, worst_g = max(worst_f, rel(fb[a], f_true)), max(worst_g, err)
                assert rel(fb[a], f_true) < 1e-12, (K, a, fb[a], f_true)
                assert err <= 1e-10 or gradient_ok(gb[a], g_true, g_true, cond()), (K, a, err)
                assert fb[a] == single[a][0] and np.array_equal(gb[a], single[a][1]), (K, a)
    print("forces %dx%d %s: worst rel(f) %.3g, worst |grad - ld| %.3g max|grad|" % (shape + (order, worst_f, worst_g)))


@pytest.mark.parametrize("one_copy", [False, True], ids=["twocopy", "onecopy"])
@pytest.mark.parametrize("shape", LOGW_SHAPES, ids=case_id)
def test_logw_evaluation_and_products_against_longdouble(bioen_amd, monkeypatch, shape, one_copy):
    """logw_fdf to 1e-12 / 1e-10 max|grad|; logw_hessp with k = 1 ... 8 directions at the kept point to 1e-10 S (both
    passes at every width); two strip copies (k_strip_adj) and one (the forces kernels' ADJ form)"""
    enter_regime(monkeypatch, shape)
    yT, YT, G, x, pool = logw_problem(shape)
    f_true, g_true, hv_true = logw_truth(shape)
    S = float(np.abs(hv_true).max())
    with bioen_amd.Context(yT, YT) as ctx:
        if one_copy:
            ctx.set_one_copy(True)
        assert_forward_regime(ctx, shape)
        f, grad = ctx.logw_fdf(x, G, LOGW_THETA)
        err_g = float(np.abs(grad - g_true).max() / np.abs(g_true).max())
        assert rel(f, f_true) < 1e-12 and err_g <= 1e-10, (f, f_true, err_g)
        hv8, f2, grad2 = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        assert f2 == f and np.array_equal(grad2, grad)
        worst = float(np.abs(hv8 - hv_true).max())
        for k in range(1, 9):
            got = ctx.logw_hessp(pool[8 - k:] if k > 1 else pool[7])
            want = hv_true[8 - k:] if k > 1 else hv_true[7]
            assert got.shape == want.shape
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.array_equal(got, hv8[8 - k:] if k > 1 else hv8[7]), k      # a direction's bits: any width
        assert ctx.layout()["one_copy"] == int(one_copy)
    print("logw %dx%d %s: rel(f) %.3g, |grad - ld| %.3g max|grad|, worst |hv - ld| %.3g S"
          % (shape + ("one copy" if one_copy else "two copies", rel(f, f_true), err_g, worst / S)))
    assert worst <= 1e-10 * S


# ---- (b) bits: the forms ---------------------------------------------------------------------------------------------
def forces_form_workload(bioen_amd, shape):
    """what a k_strip form must not change: the K = 5 ... 8 batches, and a six-theta series capped at 10 iterations"""
    yT, YT, w0, F, th = ordered(shape, "generated")
    with bioen_amd.Context(yT, YT) as ctx:
        assert_forces_regime(ctx, shape)
        out = []
        for K in range(5, 9):
            fb, gb = ctx.forces_fdf_batch(F[:K], w0, th[:K])
            out += [fb.tobytes(), gb.tobytes()]
        res, w, infos = ctx.opt_lbfgs_forces_batch(th[:6], 0.2 * F[0], w0, CAPPED, max_batch=6)
    return out + [res.tobytes(), w.tobytes(), stat(infos)]


@pytest.mark.parametrize("switch", [("BIOEN_HIP_STRIP_DEPTH5", "1"), ("BIOEN_HIP_STRIP_DEPTH5", "2"), ("BIOEN_HIP_NVEC_NT", "0"),
                                    ("BIOEN_HIP_NVEC_NT", "1")], ids=lambda s: "%s=%s" % s)
@pytest.mark.parametrize("shape", K_STRIP_SHAPES, ids=case_id)
def test_k_strip_forms_give_the_same_bits(bioen_amd, monkeypatch, shape, switch):
    """the K > 4 forms of k_strip -- DEPTH 3 (default), 2 and 1 -- and both cache policies of the N-vector kernels: the same
    bits where a slot runs two and three strips of a segment (a context per setting, created after the variable is set)"""
    enter_regime(monkeypatch, shape)
    if shape not in _DEFAULT_BITS:
        _DEFAULT_BITS[shape] = forces_form_workload(bioen_amd, shape)
    monkeypatch.setenv(*switch)
    assert forces_form_workload(bioen_amd, shape) == _DEFAULT_BITS[shape]


def logw_fold_workload(bioen_amd, shape, fold):
    yT, YT, G, x, pool = logw_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        assert_forward_regime(ctx, shape, fold=fold)
        f, grad = ctx.logw_fdf(x, G, LOGW_THETA)
        hv, _, _ = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        res, w, infos = ctx.opt_lbfgs_logw_batch(THETAS, x, G, CAPPED, max_batch=8)
    return [f, grad.tobytes(), hv.tobytes(), res.tobytes(), w.tobytes(), stat(infos)]


@pytest.mark.parametrize("shape", FOLDED_SHAPES, ids=case_id)
def test_unfolded_forward_pass_gives_the_folded_bits(bioen_amd, monkeypatch, shape):
    """BIOEN_HIP_STRIP_FOLD=0 (one chunk per slot, the chunks added up by the consumer: what a rank of eight runs) against
    the default (a slot runs its group and adds the chunks of tc = 2 strips in registers): logw_fdf, logw_hessp at k = 8,
    an eight-theta series capped at 10 iterations"""
    folded = logw_fold_workload(bioen_amd, shape, 1)
    monkeypatch.setenv("BIOEN_HIP_STRIP_FOLD", "0")
    assert logw_fold_workload(bioen_amd, shape, 0) == folded


# ---- (b) bits: a batched series = its single runs ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", SORTED_SHAPES, ids=case_id)
def test_forces_series_equals_its_single_runs(bioen_amd, shape):
    yT, YT, w0, F, th = ordered(shape, "generated")
    with bioen_amd.Context(yT, YT) as ctx:
        assert_forces_regime(ctx, shape)
        res, w, infos = ctx.opt_lbfgs_forces_batch(th, 0.2 * F[0], w0, CAPPED, max_batch=8)
        for a in range(8):
            f1, w1, i1 = ctx.opt_lbfgs_forces(0.2 * F[0], w0, th[a], CAPPED)
            assert stat([infos[a]]) == stat([i1]), a
            assert np.array_equal(res[a], f1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) >= 5


@pytest.mark.parametrize("device_ls", ["0", "1"])
@pytest.mark.parametrize("shape", FOLDED_SHAPES, ids=case_id)
def test_logw_series_equals_its_single_runs(bioen_amd, monkeypatch, shape, device_ls):
    monkeypatch.setenv("BIOEN_HIP_DEVICE_LS", device_ls)
    yT, YT, G, x, pool = logw_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        assert_forward_regime(ctx, shape)
        res, w, infos = ctx.opt_lbfgs_logw_batch(THETAS, x, G, CAPPED, max_batch=8)
        for a in range(8):
            g1, w1, i1 = ctx.opt_lbfgs_logw(x, G, THETAS[a], CAPPED)
            assert stat([infos[a]]) == stat([i1]), a
            assert np.array_equal(res[a], g1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) >= 5


# ---- (b) bits: the GPU count -----------------------------------------------------------------------------------------
def on_thread_ranks(bioen_amd, world, yT, YT, workload):
    """-> the workload's result on each of `world` ranks, threads of this process on device 0 (sweep.ThreadComm)"""
    from bioen_amd import sweep
    comms = sweep.ThreadComm.create(world)
    results, errors = [None] * world, [None] * world

    def rank_main(r):
        try:
            ctx = bioen_amd.Context(yT, YT, device=0, rank=r, world=world)
            try:
                ctx.set_exchange(comms[r])
                results[r] = workload(ctx, 8 // world)
            finally:
                ctx.close()
        except BaseException as e:          # noqa: B902 -- reported below; the other ranks leave through the barrier's bound
            errors[r] = e
            try:
                comms[r]._s.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a rank did not finish"
    assert all(e is None for e in errors), errors
    return results


def assert_ranks_equal_single(results, single):
    for r, res in enumerate(results):
        for key, val in single.items():
            assert np.array_equal(np.asarray(res[key]), np.asarray(val)), (r, key)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [8, 2])
def test_logw_thread_ranks_equal_the_single_context(bioen_amd, world):
    """1024 x 33700: a rank of eight runs one chunk of tc = 2 strips per slot and its one segment; the single context folds
    the chunks of all eight segments in registers -- logw_fdf, logw_hessp at k = 8, a five-theta capped series"""
    shape = (1024, 33700)
    yT, YT, G, x, pool = logw_problem(shape)

    def workload(ctx, local_segments):
        assert_forward_regime(ctx, shape, fold=int(local_segments == 8), local_segments=local_segments)
        out = {}
        out["f"], out["grad"] = ctx.logw_fdf(x, G, LOGW_THETA)
        out["hv"], _, _ = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        out["res"], out["w"], infos = ctx.opt_lbfgs_logw_batch(THETAS[:5], x, G, CAPPED, max_batch=8)
        out["stat"] = np.array(stat(infos))
        return out

    with bioen_amd.Context(yT, YT) as ctx:
        single = workload(ctx, 8)
    assert_ranks_equal_single(on_thread_ranks(bioen_amd, world, yT, YT, workload), single)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [8, 2])
def test_forces_thread_ranks_equal_the_single_context(bioen_amd, world):
    """300 x 66000: a rank of eight runs a group's two or three strips and flushes once; the single context runs them
    through eight segments and flushes eight times -- forces_fdf_batch at K = 8, a five-theta capped series"""
    shape = (300, 66000)
    yT, YT, w0, F, th = ordered(shape, "generated")

    def workload(ctx, local_segments):
        assert_forces_regime(ctx, shape, local_segments=local_segments)
        out = {}
        out["f"], out["grad"] = ctx.forces_fdf_batch(F, w0, th)
        out["res"], out["w"], infos = ctx.opt_lbfgs_forces_batch(th[:5], 0.2 * F[0], w0, CAPPED, max_batch=8)
        out["stat"] = np.array(stat(infos))
        return out

    with bioen_amd.Context(yT, YT) as ctx:
        single = workload(ctx, 8)
    assert_ranks_equal_single(on_thread_ranks(bioen_amd, world, yT, YT, workload), single)

"""GPU tests of the ROW-PANEL passes (M > 1024: strip.hpp's panels of 1024 rows; csrc/strip_plan.cpp: launch_fwd_strip /
launch_adj_strip over the panel list, api.hip: enqueue_forces_eval with psets > 0, api_forces_hessp.cpp's panel path) where
ONE BLOCK SLOT RUNS SEVERAL STRIPS OF A COLUMN SEGMENT -- tests/test_hip_strip_loops.py's question for the other pass family.
At eight segments the forward plan on panels is 32 groups per segment, so up to N = 4096 a slot runs one strip, one chunk;
every other file's M > 1024 shapes stay below that or have two panels and tc = 1.  What is new here:

  k_strip_fwd on panels      chunks of two and three strips written at fwd_partial + p * 1024 * K with pstride = mp, the
                             context's sets in every panel, a short last panel whose blocks have 2 waves instead of 16
  k_strip_adj across panels  `accumulate = p > 0` where a block loops over strips (256 blocks, 2107 resp. 568 strips), and the
                             one-copy form (k_strip / k_strip2 ADJ, 256 groups of 264 resp. 568 strips per segment)
  the forces panel passes    k_forces_seg_exp / k_forces_seg_t with seg_sets = gs * nch unfolded (a rank of eight, a
                             one-segment context), the per-segment softmax merge with segments whose maxima all differ
  the forces products        api_forces_hessp.cpp's four passes with k_fhp_seg_t on the same sets
  canonical order            "the GPU count changes no bit" on panels where a chunk is more than one strip
  the panel limit            16 panels (M = 16384: the last the strip kernels serve) and 17 (the streaming kernels)

Every test asserts its regime first and from the library: the plan through Context.strip_plan, the panel count through
kernel_stats (an evaluation's forward / adjoint launches), the resident forms through footprint.  REGIMES is the table.

Data, truth and gates are those of tests/test_hip_strip_loops.py (its helpers, imported): the formulas of DESIGN sections 2,
6b and 6d in numpy.longdouble, once per shape; rel(f) < 1e-12, gradients 1e-10 max|grad| or gradient_ok's condition clause,
products 1e-10 S, bit equality wherever the project claims it."""
import numpy as np
import pytest

from test_hip_edgecases import gradient_ok, rel
from test_hip_forces_hessp import WIDTHS, directions, estate, hessp_longdouble
from test_hip_hessp import recipe
from test_hip_strip_loops import (CAPPED, LOGW_THETA, THETAS, assert_forward_regime, assert_ranks_equal_single, data,
                                  enter_regime, forces_average_truth, forces_truth, logw_problem, logw_truth, on_thread_ranks,
                                  ordered, stat)

pytestmark = pytest.mark.gpu

L = np.longdouble
TWO, THREE, FULL, OVER = (1100, 33700), (2100, 9000), (16384, 300), (16400, 300)
OVER_SHARDED = (16400, 600)             # 300 columns are too few to shard over two ranks (runs of four segments of 128)
# shape -> segments (1: BIOEN_HIP_SEGMENTS=1), row panels, strips per segment, forward (gs, tc, nch, fold)
REGIMES = {
    TWO: dict(segments=8, panels=2, sps=264, forward=(32, 2, 5, 1)),      # chunks 2 2 2 2 1 | 2 2 2 2 0; panel 1: 80 strip rows
    THREE: dict(segments=1, panels=3, sps=568, forward=(32, 3, 6, 0)),    # chunks of three, unfolded; panel 2: 64 strip rows
    FULL: dict(segments=8, panels=16, sps=8, forward=(8, 1, 1, 1)),       # the last admissible panel count, one strip per slot
}
LOOP_SHAPES = [TWO, THREE]
FORCES_CASES = [(TWO, "generated"), (TWO, "ascending"), (THREE, "generated")]
HESSP_THETAS = (10.0, 1000.0)
COPIES = pytest.mark.parametrize("one_copy", [False, True], ids=["twocopy", "onecopy"])


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    return bioen_amd


# ---- regimes ---------------------------------------------------------------------------------------------------------
def assert_plan(ctx, shape, fold=None, local_segments=None):
    want = REGIMES[shape]
    gs, tc, nch, dflt_fold = want["forward"]
    if shape in LOOP_SHAPES:        # tmax >= 2; at eight segments a group's shorter and empty last chunk
        p = assert_forward_regime(ctx, shape, fold=fold, local_segments=local_segments, regimes=REGIMES)
    else:
        p = ctx.strip_plan(0)
    assert (p["sps"], p["gs"], p["tc"], p["nch"], p["fold"]) == (want["sps"], gs, tc, nch, dflt_fold if fold is None else fold), p
    assert p["local_segments"] == (want["segments"] if local_segments is None else local_segments), p
    assert ctx.strip_plan(1)["gs"] == 0                         # the forces strip passes (M <= 1024) do not apply
    return p


def launches(ctx, call):
    """-> call(), (forward, adjoint) launches it made"""
    ctx.kernel_stats_enable(True)
    ctx.kernel_stats_reset()
    out = call()
    st = ctx.kernel_stats()
    ctx.kernel_stats_enable(False)
    return out, (st["forward"]["launches"], st["adjoint"]["launches"])


def enter_panels(ctx, shape, call, passes=1, one_copy=False, fold=None, local_segments=None):
    """the regime of a test, before its first numerical assertion: the plan; the panel count from the launches of `call`,
    an evaluation of `passes` forward and adjoint passes per panel (logw_fdf: 1, forces_fdf: 2); the resident forms.
    -> call()"""
    assert_plan(ctx, shape, fold=fold, local_segments=local_segments)
    out, n = launches(ctx, call)
    panels = REGIMES[shape]["panels"]
    assert n == (passes * panels, passes * panels), (n, panels)
    assert ctx.footprint()[0] == ({"strips"} if one_copy else {"strips", "strips_colsum"})
    assert ctx.layout()["one_copy"] == int(one_copy)
    return out


# ---- the truth of the forces products, once per shape ----------------------------------------------------------------
_HESSP_TRUTH = {}


def hessp_problem(shape):
    """-> forces (x = yTilde^T f has standard deviation 1, as tests/test_hip_forces_hessp.py's loop cases), directions"""
    return data(shape)[4] / 5.0, directions(shape[0], 3 + shape[0])


def forces_hessp_truth(shape):
    """DESIGN section 6d in 80-bit arithmetic: theta -> (H V, L, grad); HESSP_THETAS at the loop shapes, else theta = 10"""
    if shape not in _HESSP_TRUTH:
        yT, YT, G, w0 = data(shape)[:4]
        f, V = hessp_problem(shape)
        A = yT.astype(L)
        thetas = HESSP_THETAS if shape in LOOP_SHAPES else HESSP_THETAS[:1]
        _HESSP_TRUTH[shape] = {th: hessp_longdouble(A, YT, w0, f, th, V) for th in thetas}
    return _HESSP_TRUTH[shape]


def check_logw(shape, f, grad, hv8=None):
    """-> rel(f), gradient error / max|grad|, worst product error / S against the 80-bit values, gated"""
    f_true, g_true, hv_true = logw_truth(shape)
    err_g = float(np.abs(grad - g_true).max() / np.abs(g_true).max())
    assert rel(f, f_true) < 1e-12 and err_g <= 1e-10, (f, f_true, err_g)
    S = float(np.abs(hv_true).max())
    worst = 0.0 if hv8 is None else float(np.abs(hv8 - hv_true).max())
    assert worst <= 1e-10 * S, worst / S
    return rel(f, f_true), err_g, worst / S


def check_forces_column(shape, a, f, grad):
    f_true, g_true, cond = forces_truth(shape)[a]
    err = float(np.abs(grad - g_true).max() / np.abs(g_true).max())
    assert rel(f, f_true) < 1e-12, (a, f, f_true)
    assert err <= 1e-10 or gradient_ok(grad, g_true, g_true, cond()), (a, err)
    return rel(f, f_true), err


# ---- 1. log-weights against the high-precision value -------------------------------------------------------------------
@COPIES
@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=case_id)
def test_logw_evaluation_and_products_against_longdouble(bioen_amd, monkeypatch, shape, one_copy):
    """logw_fdf to 1e-12 / 1e-10 max|grad|; logw_hessp with k = 1 ... 8 directions at the kept point to 1e-10 S, a
    direction's bits the same at any width; two strip copies (k_strip_adj continued across panels, 256 blocks looping over
    the strips) and one (the forces kernels' ADJ form on panels: 256 groups of 264 resp. 568 strips)"""
    enter_regime(monkeypatch, shape, REGIMES)
    yT, YT, G, x, pool = logw_problem(shape)
    f_true, g_true, hv_true = logw_truth(shape)
    S = float(np.abs(hv_true).max())
    with bioen_amd.Context(yT, YT) as ctx:
        if one_copy:
            ctx.set_one_copy(True)
        f, grad = enter_panels(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA), one_copy=one_copy)
        hv8, f2, grad2 = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        err_f, err_g, worst = check_logw(shape, f, grad, hv8)
        assert f2 == f and np.array_equal(grad2, grad)
        for k in range(1, 9):
            got = ctx.logw_hessp(pool[8 - k:] if k > 1 else pool[7])
            want = hv_true[8 - k:] if k > 1 else hv_true[7]
            assert got.shape == want.shape
            worst = max(worst, float(np.abs(got - want).max()) / S)
            assert np.array_equal(got, hv8[8 - k:] if k > 1 else hv8[7]), k      # a direction's bits: any width
        assert ctx.layout()["one_copy"] == int(one_copy)
    print("logw %dx%d %s: rel(f) %.3g, |grad - ld| %.3g max|grad|, worst |hv - ld| %.3g S"
          % (shape + ("one copy" if one_copy else "two copies", err_f, err_g, worst)))
    assert worst <= 1e-10


# ---- 2. the forces evaluation's four panel passes ----------------------------------------------------------------------
def assert_segment_maxima_rise(shape):
    """columns sorted by x ascending: the maxima of the eight canonical segments rise strictly (fall, for s < 0), so the
    per-segment softmax merge rescales every segment's share but the last one's (the first one's)"""
    xs = np.sort(data(shape)[5])
    segcols = -(-(-(-shape[1] // 8)) // 128) * 128
    maxima = [xs[v * segcols:(v + 1) * segcols].max() for v in range(8)]
    minima = [xs[v * segcols:(v + 1) * segcols].min() for v in range(8)]
    assert len(xs[7 * segcols:]) > 0 and (np.diff(maxima) > 0).all() and (np.diff(minima) > 0).all()


@COPIES
@pytest.mark.parametrize("shape,order", FORCES_CASES, ids=case_id)
def test_forces_batches_of_every_width_against_longdouble(bioen_amd, monkeypatch, shape, order, one_copy):
    """forces_fdf_batch at K = 1 ... 8 on the first K problems: every column within 1e-12 / gradient_ok of the 80-bit value
    and bit for bit the single call's; launch_adj_strip takes the one-copy form here too.  2100 x 9000 on one segment:
    seg_sets = 32 x 6 unfolded.  Sorted columns: every segment's maximum differs, both ways in one batch.  Then
    last_average: refused after the K = 8 call (a multi-problem call), and after the single call of problem 0 -- the K = 8
    call's column 0 bit for bit -- yTilde . w of the truth at tests/test_hip_api.py::test_last_average_after_forces_calls'
    gate (the panel path keeps ybar - centre and adds the centre back)"""
    enter_regime(monkeypatch, shape, REGIMES)
    yT, YT, w0, F, th = ordered(shape, order)
    forces_truth(shape)
    if order == "ascending":
        assert_segment_maxima_rise(shape)
    worst_f = worst_g = 0.0
    with bioen_amd.Context(yT, YT) as ctx:
        if one_copy:
            ctx.set_one_copy(True)
        first = enter_panels(ctx, shape, lambda: ctx.forces_fdf(F[0], w0, th[0]), passes=2, one_copy=one_copy)
        single = [first] + [ctx.forces_fdf(F[a], w0, th[a]) for a in range(1, 8)]
        for K in range(1, 9):
            fb, gb = ctx.forces_fdf_batch(F[:K], w0, th[:K])
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
        assert ctx.layout()["one_copy"] == int(one_copy)
    print("forces %dx%d %s %s: worst rel(f) %.3g, worst |grad - ld| %.3g max|grad|, |ybar - ld| %.3g max|ybar|"
          % (shape + (order, "one copy" if one_copy else "two copies", worst_f, worst_g, err_y)))


# ---- 3. the forces products' panel path --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [THREE, TWO], ids=case_id)
def test_forces_products_against_longdouble(bioen_amd, monkeypatch, shape):
    """forces_hessp at the widths of WIDTHS, theta = 10 and 1000, against DESIGN 6d in 80-bit arithmetic to 1e-10 S; a
    direction's bits the same at any width; the point-setting call returns forces_fdf's f and gradient"""
    enter_regime(monkeypatch, shape, REGIMES)
    yT, YT, G, w0 = data(shape)[:4]
    f, pool = hessp_problem(shape)
    truth = forces_hessp_truth(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        enter_panels(ctx, shape, lambda: ctx.forces_fdf(f, w0, HESSP_THETAS[0]), passes=2)
        for theta in HESSP_THETAS:
            ref, fref, gref = truth[theta]
            S = float(np.abs(ref).max())
            f0, g0 = ctx.forces_fdf(f, w0, theta)
            hv8, fv, grad = ctx.forces_hessp(pool, forces=f, w0=w0, theta=theta)
            assert fv == f0 and np.array_equal(grad, g0)
            assert rel(fv, fref) < 1e-12 and np.abs(grad - gref).max() <= 1e-10 * np.abs(gref).max()
            assert not hv8[5].any()                                                      # H 0 = 0
            worst = float(np.abs(hv8 - ref).max())
            for k in WIDTHS:
                got = ctx.forces_hessp(pool[8 - k:] if k > 1 else pool[7])
                want = ref[8 - k:] if k > 1 else ref[7]
                assert got.shape == want.shape
                worst = max(worst, float(np.abs(got - want).max()))
                assert np.array_equal(got, hv8[8 - k:] if k > 1 else hv8[7]), k
            print("forces products %dx%d theta %g: max |hv - ld| = %.3g S" % (shape + (theta, worst / S)))
            assert worst <= 1e-10 * S


@pytest.mark.parametrize("shape", [TWO, FULL], ids=case_id)
def test_forces_products_after_logw_products_on_one_context(bioen_amd, shape):
    """the two methods' products share their N-vector buffers: the log-weights adjoint leaves its constant in a buffer's
    padding (columns n ... ld: 92 here, 724 at 16384 x 300), which the forces products' row-sum pass on the centred copy
    multiplies with (0 - centre) unless k_fhp_seg_t has written it as zero -- the FIRST forces product after a log-weights
    product was wrong by 267 S at 16384 x 300 before it did"""
    yT, YT, G, x, pool = logw_problem(shape)
    w0 = data(shape)[3]
    f, V = hessp_problem(shape)
    ref, fref, gref = forces_hessp_truth(shape)[10.0]
    S = float(np.abs(ref).max())
    with bioen_amd.Context(yT, YT) as ctx:
        enter_panels(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        first, fv, grad = ctx.forces_hessp(V, forces=f, w0=w0, theta=10.0)
        err = float(np.abs(first - ref).max()) / S
        print("forces products after log-weights products %dx%d: max |hv - ld| = %.3g S" % (shape + (err,)))
        assert err <= 1e-10
        assert np.array_equal(ctx.forces_hessp(V), first)


# ---- 4. - 6. bits --------------------------------------------------------------------------------------------------------
def everything(ctx, shape, n_logw, fold=None, local_segments=None):
    """what neither the fold nor the GPU count may change: logw_fdf, logw_hessp at k = 8, forces_fdf_batch at K = 8,
    forces_hessp at k = 8, a capped series of n_logw thetas of the log-weights method and of five of the forces method"""
    yT, YT, G, x, pool = logw_problem(shape)
    _, _, w0, F, th = ordered(shape, "generated")
    fh, V = hessp_problem(shape)
    out = {}
    out["f"], out["grad"] = enter_panels(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA), fold=fold,
                                         local_segments=local_segments)
    out["hv"], _, _ = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
    out["forces f"], out["forces grad"] = ctx.forces_fdf_batch(F, w0, th)
    out["forces hv"], out["point f"], out["point grad"] = ctx.forces_hessp(V, forces=fh, w0=w0, theta=10.0)
    out["res"], out["w"], infos = ctx.opt_lbfgs_logw_batch(THETAS[:n_logw], x, G, CAPPED, max_batch=8)
    out["stat"] = np.array(stat(infos))
    out["forces res"], out["forces w"], infos = ctx.opt_lbfgs_forces_batch(th[:5], 0.2 * F[0], w0, CAPPED, max_batch=8)
    out["forces stat"] = np.array(stat(infos))
    return out


def test_unfolded_passes_give_the_folded_bits(bioen_amd, monkeypatch):
    """1100 x 33700, BIOEN_HIP_STRIP_FOLD=0 in a fresh context (one chunk per slot, seg_sets = 32 x 5 in the forces passes:
    what a rank of eight runs) against the default (a slot adds its group's chunks of two strips in registers)"""
    yT, YT = data(TWO)[:2]
    with bioen_amd.Context(yT, YT) as ctx:
        folded = everything(ctx, TWO, 8, fold=1)
    monkeypatch.setenv("BIOEN_HIP_STRIP_FOLD", "0")
    with bioen_amd.Context(yT, YT) as ctx:
        unfolded = everything(ctx, TWO, 8, fold=0)
    assert_ranks_equal_single([unfolded], folded)


@pytest.mark.parametrize("device_ls", ["0", "1"])
def test_logw_series_equals_its_single_runs(bioen_amd, monkeypatch, device_ls):
    monkeypatch.setenv("BIOEN_HIP_DEVICE_LS", device_ls)
    yT, YT, G, x, pool = logw_problem(TWO)
    with bioen_amd.Context(yT, YT) as ctx:
        enter_panels(ctx, TWO, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        res, w, infos = ctx.opt_lbfgs_logw_batch(THETAS, x, G, CAPPED, max_batch=8)
        for a in range(8):
            g1, w1, i1 = ctx.opt_lbfgs_logw(x, G, THETAS[a], CAPPED)
            assert stat([infos[a]]) == stat([i1]), a
            assert np.array_equal(res[a], g1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) >= 5


def test_forces_series_equals_its_single_runs(bioen_amd):
    yT, YT, w0, F, th = ordered(TWO, "generated")
    with bioen_amd.Context(yT, YT) as ctx:
        enter_panels(ctx, TWO, lambda: ctx.forces_fdf(F[0], w0, th[0]), passes=2)
        res, w, infos = ctx.opt_lbfgs_forces_batch(th[:5], 0.2 * F[0], w0, CAPPED, max_batch=8)
        for a in range(5):
            f1, w1, i1 = ctx.opt_lbfgs_forces(0.2 * F[0], w0, th[a], CAPPED)
            assert stat([infos[a]]) == stat([i1]), a
            assert np.array_equal(res[a], f1) and np.array_equal(w[a], w1), a
        assert max(i.iterations for i in infos) >= 5


_SINGLE = {}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [8, 2])
def test_thread_ranks_equal_the_single_context(bioen_amd, world):
    """1100 x 33700: a rank of eight runs one chunk of two strips per slot on its one segment, in both panels, and the
    forces passes with seg_sets = 160; the single context folds the chunks of all eight segments in registers"""
    yT, YT = data(TWO)[:2]
    if TWO not in _SINGLE:
        with bioen_amd.Context(yT, YT) as ctx:
            _SINGLE[TWO] = everything(ctx, TWO, 5, fold=1)

    def workload(ctx, local_segments):
        return everything(ctx, TWO, 5, fold=int(local_segments == 8), local_segments=local_segments)

    assert_ranks_equal_single(on_thread_ranks(bioen_amd, world, yT, YT, workload), _SINGLE[TWO])


# ---- 7. read-back ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [THREE, FULL], ids=case_id)
def test_read_back_from_the_panel_copies(bioen_amd, monkeypatch, shape):
    """read_ytilde after the strip copies have replaced the row-major matrix: the caller's numbers, gathered from 3 and
    16 panels; and a block whose rows start and end inside panels"""
    enter_regime(monkeypatch, shape, REGIMES)
    yT, YT, G, x, pool = logw_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        enter_panels(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA))     # footprint: no "rowmajor" from here on
        assert np.array_equal(ctx.read_ytilde(), yT)
        r0, c0 = 1000, shape[1] // 3
        rows, cols = shape[0] - r0 - 10, 37                           # ends inside the last panel
        assert np.array_equal(ctx.read_ytilde(r0, rows, c0, cols), yT[r0:r0 + rows, c0:c0 + cols])
        assert "rowmajor" not in ctx.footprint()[0]


# ---- 8. the panel limit ------------------------------------------------------------------------------------------------
def test_sixteen_panels_are_served_by_the_strip_kernels(bioen_amd):
    """16384 x 300: kMaxPanels row panels, every one full -- both methods and both products against the 80-bit values"""
    shape = FULL
    yT, YT, G, x, pool = logw_problem(shape)
    _, _, w0, F, th = ordered(shape, "generated")
    fh, V = hessp_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        f, grad = enter_panels(ctx, shape, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        hv8, f2, grad2 = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        assert f2 == f and np.array_equal(grad2, grad)
        errs = check_logw(shape, f, grad, hv8)
        (f1, g1), n = launches(ctx, lambda: ctx.forces_fdf_batch(F[:1], w0, th[:1]))
        assert n == (32, 32), n
        worst_f, worst_g = check_forces_column(shape, 0, f1[0], g1[0])
        fb, gb = ctx.forces_fdf_batch(F, w0, th)
        assert fb[0] == f1[0] and np.array_equal(gb[0], g1[0])
        for a in range(8):
            err_f, err_g = check_forces_column(shape, a, fb[a], gb[a])
            worst_f, worst_g = max(worst_f, err_f), max(worst_g, err_g)
        ref, fref, gref = forces_hessp_truth(shape)[10.0]
        S = float(np.abs(ref).max())
        fhv, fv, fgrad = ctx.forces_hessp(V, forces=fh, w0=w0, theta=10.0)
        assert rel(fv, fref) < 1e-12 and np.abs(fgrad - gref).max() <= 1e-10 * np.abs(gref).max()
        err_h = float(np.abs(fhv - ref).max()) / S
        print("16384x300: logw rel(f) %.3g, grad %.3g, products %.3g S; forces rel(f) %.3g, grad %.3g, products %.3g S"
              % (errs + (worst_f, worst_g, err_h)))
        assert err_h <= 1e-10
        assert ctx.footprint()[0] == {"strips", "strips_colsum"}


def test_seventeen_panels_are_served_by_the_streaming_kernels(bioen_amd):
    """16400 x 300, past the limit: the row-major matrix stays, one forward and one adjoint launch per gradient, the values
    at the same gates; the forces products are refused with BIOEN_HIP_ESTATE and the context stays usable"""
    shape = OVER
    yT, YT, G, x, pool = logw_problem(shape)
    _, _, w0, F, th = ordered(shape, "generated")
    fh, V = hessp_problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        assert ctx.strip_plan(1)["gs"] == 0
        (f, grad), n = launches(ctx, lambda: ctx.logw_fdf(x, G, LOGW_THETA))
        assert n == (1, 1), n
        assert ctx.footprint()[0] == {"rowmajor"}
        hv8, f2, grad2 = ctx.logw_hessp(pool, g=x, G=G, theta=LOGW_THETA)
        assert f2 == f and np.array_equal(grad2, grad)
        errs = check_logw(shape, f, grad, hv8)
        ff, fg = ctx.forces_fdf(F[0], w0, th[0])
        worst = check_forces_column(shape, 0, ff, fg)
        estate(lambda: ctx.forces_hessp(V[0], forces=fh, w0=w0, theta=10.0), "bioen_hip_forces_hessp", "streaming")
        estate(lambda: ctx.forces_hessp(V[0]), "bioen_hip_forces_hessp", "streaming")
        estate(lambda: ctx.forces_gram(forces=fh, w0=w0, theta=10.0), "bioen_hip_forces_gram", "M <= 1024")
        ff2, fg2 = ctx.forces_fdf(F[0], w0, th[0])                   # ... and serves what it served
        assert ff2 == ff and np.array_equal(fg2, fg)
        f3, grad3 = ctx.logw_fdf(x, G, LOGW_THETA)
        assert f3 == f and np.array_equal(grad3, grad)
        assert ctx.footprint()[0] == {"rowmajor"}
    print("16400x300: logw rel(f) %.3g, grad %.3g, products %.3g S; forces rel(f) %.3g, grad %.3g" % (errs + worst))


@pytest.mark.timeout(600)
def test_seventeen_panels_refuse_the_forces_method_on_a_sharded_context(bioen_amd):
    """the streaming kernels' partial sums are not in canonical segments: two thread ranks are told what is missing"""
    M, N = OVER_SHARDED
    yT, YT, G = recipe(M, N, 1000 * M + N)
    w0, f = np.exp(G), 1e-3 * np.random.default_rng(5).standard_normal(M)

    def workload(ctx, local_segments):
        assert local_segments == 4 and ctx.strip_plan(1)["gs"] == 0
        estate(lambda: ctx.forces_fdf(f, w0, 10.0), "needs the strip copies")
        assert ctx.footprint()[0] == {"rowmajor"}
        return {"refused": 1}

    assert_ranks_equal_single(on_thread_ranks(bioen_amd, 2, yT, YT, workload), {"refused": 1})

"""GPU tests of the forces method's dense kernels WHERE THEIR LOOPS RUN LONG (csrc/fgram.hpp: fgram_pass / fgram16_pass at the
forces point, csrc/kernels_forces_gram.hip: k_fgram_sum_sets, csrc/kernels_forces_colquad.hip, csrc/api_forces_laplace.cpp,
csrc/api_forces_newton.cpp): Context.forces_gram, forces_gram_bf16, forces_colquad, forces_laplace and opt_newton_forces at
the shapes of tests/test_hip_strip_loops.py's REGIMES at which a set chains 16 ... 132 strips, a block of the quadratic-form
pass runs 4 ... 17 panels, and the sum of the sets meets more than eight groups on eight segments.  The ordinary test files
of these entries reach chains of 7 and a block's second panel.  tests/README_forces_dense_loops.md has the regime table, the
measured errors and the wrong builds the file was run against.

Every test asserts its regime first, from what the launchers compute: Context.strip_plan(3) (the Gram passes' sets) and
strip_plan(4) (the quadratic-form pass's grid).

The point is f / 5 of data(shape), x with standard deviation 1; the thetas are tests/test_hip_forces_gram.py's.

Truth (tests/test_forces_dense_truth.py, pinned there on the CPU).  A full M x M x N product in 80-bit arithmetic is
affordable at 64 x 131500 only; elsewhere two truths together:
  a band of 16 rows, exact -- rows of C, and of T = theta C + G2 (H without C C): the device's H enters as H_dev - C_dev
    C_dev, that product formed in longdouble on the host from the device's own C.  What this leaves unsaid about H is
    C_dev C_dev - C C, at most 2 M max|C| |C_dev - C|, and C's band and products are held by themselves;
  every element, through products -- C_dev V and H_dev V for eight seeded directions, formed on the host in longdouble,
    against the matrix-free C V and H V: GATE of max|C V|, max|H V|.

The split-BF16 gate, derived (as tests/test_hip_logw_gram_bf16.py derives its own; CAP and REST of
tests/test_hip_forces_gram_bf16.py were measured at chains of <= 7 and are printed beside it, not asserted).  With a = Y -
centre, G'[u] = sum_j u_j a_j a_j^T in FP64 on the host, s1_ik = sqrt(G'[w]_ii G'[w]_kk) and s2_ik the same with |u2| (u2 =
w (q - <q>) has both signs; every summand of element (i, k) is bounded relative to s_ik by Cauchy-Schwarz), tg the longest
chain from strip_plan(3):
  (ii) each set product against the restatement (the same split products summed in FP64): b2 = 48 tg 2^-23 of s -- 48 f32
       additions per strip and accumulator (3 instructions of depth 16), one unit of the last place each;
  (i)  against the FP64 pass: b1 = b2 + 3 . 2^-16 of s -- each operand keeps 16 significant bits, lo lo is dropped.
  Through H~ = theta C~ + G2~ + C~ C~ with E1 = b s1 + F, E2 = b s2 + GATE s2 + (1 + 2 sum|u2|) F:
       |dC| <= E1,    |dH| <= theta E1 + E2 + E1 |C| + (|C| + E1) E1          (matrix products of absolute values)
  F is scale_matrix's FP64 floor 4 n eps max|y_i| max|y_k| (the two sides form ybar', and g = sum u2 a, in different orders);
  GATE s2 covers u2 itself, formed in FP64 in another order on the host.  Against the FP64 pass its own GATE max|H| is added.

The Newton step's truth: H p = -g, g and H p in longdouble (matrix-free), solved by iterative refinement on a float64
Cholesky factor of the restatement's H; asserted converged before anything is compared."""
from concurrent.futures import ThreadPoolExecutor
import time

import numpy as np
import pytest
import scipy.linalg

from test_forces_colquad import GATE as CQ_GATE, colquad_ld, matrices
from test_forces_dense_truth import L, band_ld, objective_ld, point_ld, products_ld, refine_solve
from test_hip_forces_gram import GATE, THETAS, gram_longdouble
from test_hip_forces_gram_bf16 import CAP, REST
from test_hip_forces_laplace import EPS, GATE as GATE_SOLVE
from test_hip_logw_gram_bf16 import U16, U23, gram_tg
from test_hip_logw_newton_loops import GRAM_CHAIN
from test_hip_strip_loops import REGIMES, data, enter_regime

from bioen_amd.optimize import forces, minimize
from bioen_amd.optimize.ext import c_bioen

pytestmark = pytest.mark.gpu

SHAPES = [(64, 131500), (600, 33700), (1024, 9000), (1024, 33700)]
# shape -> (gs, the longest chain; the other sets one strip fewer, at 1024 x 33700 none) of the Gram passes
GRAM = {(64, 131500): (64, 17), (600, 33700): (5, 53), (1024, 9000): (15, 38), (1024, 33700): (2, 132)}
# shape -> (NB, panels, the fewest panels a block runs; the others one more) of the quadratic-form pass
COLQUAD = {(64, 131500): (1, 4110, 16), (600, 33700): (10, 1054, 4), (1024, 9000): (16, 282, 1), (1024, 33700): (16, 1054, 4)}
BF16_SHAPES = [(600, 33700), (1024, 9000), (1024, 33700)]
# where forces.hessian_gram_bf16_bioen_log_posterior_base takes under about 5 s on the host, measured (the README has the
# times): comparison (ii) runs there, (i) alone at the others
RESTATED = {(600, 33700): True, (1024, 9000): True, (1024, 33700): False}
STEP_SHAPES = [(64, 131500), (600, 33700), (1024, 9000)]
LOOP_SHAPES = [(600, 33700), (64, 131500)]
# forces0 = STEP_SCALE f at STEP_THETA: the restatement accepts its first step with one factorisation and lambda = 0, cond(H)
# = 1.2, 2.6 and 12 at the three shapes (measured on the CPU).  Not theta = 10: there H is indefinite at every scaled copy of
# the test point, f = 0 included (smallest eigenvalue -6.4 at 600 x 33700, -2.1e3 at 1024 x 9000), and the first step is a
# damped one after 19 factorisations
STEP_THETA = 1000.0
STEP_SCALE = 0.5
# the float64 einsum of the every-column check lies within 0.1 COARSE CQ_GATE scale of the longdouble value on the sample
# (measured on the CPU: the README has the figures); the device may use CQ_GATE scale itself, so 2 leaves it that and more
COARSE = 2.0


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def bioen_amd():
    import bioen_amd
    assert bioen_amd.device_count() >= 1
    yield bioen_amd
    c_bioen.clear_cache()
    _A.clear()
    _TRUTH.clear()


# ---- regimes -----------------------------------------------------------------------------------------------------------
def assert_gram_regime(ctx, shape, local_segments=None):
    """the sets of the Gram passes from the plan: strip_plan(3) is forces_gram_plan's answer, GRAM_CHAIN and gram_tg the
    log-weights files' arithmetic for the same gram_plan"""
    p = ctx.strip_plan(3)
    segments = REGIMES[shape]["segments"] if local_segments is None else local_segments
    assert p["local_segments"] == segments, p
    if local_segments is None:
        assert (p["gs"], p["tc"]) == GRAM[shape], p
        assert p["tc"] == GRAM_CHAIN[shape] == gram_tg(ctx, shape[0]) and p["tc"] >= 16, p
        assert p["nch"] == segments * p["gs"], p
        if shape == (64, 131500):
            assert p["gs"] > 8 and segments == 8, p              # groups g >= 8 of segments v >= 1 in the sum of the sets
    return p


def assert_colquad_regime(ctx, shape):
    p = ctx.strip_plan(4)
    nb, panels, least = COLQUAD[shape]
    assert p["sps"] == panels == -(-shape[1] // 32), p
    assert p["gs"] == min(panels, 256) and p["nch"] == nb, p
    assert panels // p["gs"] == least and p["tc"] == -(-panels // p["gs"]), p
    if shape != (1024, 9000):
        assert least >= 3, p                                     # every block runs a third panel and more
    else:
        assert p["tc"] == 2 and REGIMES[shape]["segments"] == 1, p
    if shape[0] == 600:
        assert p["fold"] == 608 and p["fold"] % 64 == 32, p       # the last slice short: 8 of its 16 steps
    return p


# ---- data and the truths, once per shape -------------------------------------------------------------------------------
_A, _TRUTH = {}, {}


def problem(shape):
    yT, YT, G, w0, f, x = data(shape)
    return yT, YT, w0, f / 5.0


def matrix_ld(shape):
    """the matrix in longdouble; one shape's at a time (552 MB at 1024 x 33700)"""
    if shape not in _A:
        _A.clear()
        _A[shape] = problem(shape)[0].astype(L)
    return _A[shape]


def band_rows(m):
    """16 rows: the first and last row of the first 64-row slice, the first and last valid row of the last slice, both sides
    of a 128-row tile boundary, a row of a diagonal tile's off-diagonal sub-tile (rows 64 ... 127 of tile 0), the rest
    seeded at random"""
    rows = {0, min(63, m - 1), 64 * ((m - 1) // 64), m - 1}
    if m > 128:
        rows |= {127, 128, 100}
    rng = np.random.default_rng(m)
    while len(rows) < 16:
        rows.add(int(rng.integers(0, m)))
    return np.array(sorted(rows))


def truth(shape):
    if shape not in _TRUTH:
        yT, YT, w0, f = problem(shape)
        A = matrix_ld(shape)
        t0 = time.time()
        pt = point_ld(A, YT, w0, f)
        rows = band_rows(shape[0])
        V = np.random.default_rng(8 + shape[0]).standard_normal((8, shape[0]))
        _TRUTH[shape] = dict(pt=pt, rows=rows, band=band_ld(A, pt, rows), V=V, prod=products_ld(A, pt, V),
                             fg=objective_ld(A, pt))
        print("%dx%d: the truths took %.1f s" % (shape + (time.time() - t0,)))
    return _TRUTH[shape]


def against_the_truths(shape, theta, C, H, label):
    """band and products (the module docstring); -> the worst figures, for the README"""
    t = truth(shape)
    rows, (Cb, Gxb, Gbb) = t["rows"], t["band"]
    Cl, Hl, V = C.astype(L), H.astype(L), t["V"].astype(L)
    SC, SH = float(np.abs(C).max()), float(np.abs(H).max())
    Tb = L(theta) * (Cb + Gxb) + Gbb
    dc = float(np.abs(Cl[rows] - Cb).max()) / SC
    dt = float(np.abs(Hl[rows] - Cl[rows] @ Cl - Tb).max()) / SH
    CV, HV = t["prod"](theta)
    pc = float(np.abs(Cl @ V.T - CV).max() / np.abs(CV).max())
    ph = float(np.abs(Hl @ V.T - HV).max() / np.abs(HV).max())
    print("%s: band |C - C_ld| = %.3g max|C|, |H - C C - T_ld| = %.3g max|H|; products |C V - (C V)_ld| = %.3g max|C V|, "
          "|H V - (H V)_ld| = %.3g max|H V|" % (label, dc, dt, pc, ph))
    assert dc <= GATE and dt <= GATE
    assert pc <= GATE and ph <= GATE


# ---- 1. forces_gram -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_gram_against_both_truths(bioen_amd, monkeypatch, shape):
    """C and H bitwise symmetric, the band and the products at every theta, H against forces_hessian() at the same kept
    point (ceil(M / 8) batched products: milliseconds at these sizes, kept at every shape), at 64 x 131500 the full
    longdouble matrices as well; a second call and a fresh context return the same bits"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, f = problem(shape)
    full = gram_longdouble(("dense loops", shape), matrix_ld(shape), YT, w0, f) if shape == (64, 131500) else None
    with bioen_amd.Context(yT, YT) as ctx:
        plan = assert_gram_regime(ctx, shape)
        for theta in THETAS:
            C, H, fv, grad = ctx.forces_gram(forces=f, w0=w0, theta=theta)
            label = "%dx%d theta %g (gs %d, chains of %d)" % (shape + (theta, plan["gs"], plan["tc"]))
            assert np.array_equal(C, C.T) and np.array_equal(H, H.T)
            against_the_truths(shape, theta, C, H, label)
            Hp = ctx.forces_hessian()
            dp = float(np.abs(H - Hp).max() / np.abs(H).max())
            print("%s: |H - H_products| = %.3g max|H|" % (label, dp))
            assert dp <= GATE
            if full is not None:
                Cf, Hf = full(theta)
                dc, dh = float(np.abs(C - Cf).max() / np.abs(Cf).max()), float(np.abs(H - Hf).max() / np.abs(Hf).max())
                print("%s: full |C - C_ld| = %.3g max|C|, |H - H_ld| = %.3g max|H|" % (label, dc, dh))
                assert dc <= GATE and dh <= GATE
            C2, H2 = ctx.forces_gram()
            assert np.array_equal(C2, C) and np.array_equal(H2, H)
    with bioen_amd.Context(yT, YT) as fresh:                     # theta = THETAS[-1]
        C3, H3, _, _ = fresh.forces_gram(forces=f, w0=w0, theta=THETAS[-1])
        assert np.array_equal(C3, C) and np.array_equal(H3, H)


def test_eight_segments_against_one(bioen_amd, monkeypatch):
    """600 x 33700: the order of the sum differs (8 x 5 sets of 53 | 52 strips against 35 of 61 | 60), nothing else"""
    shape = (600, 33700)
    yT, YT, w0, f = problem(shape)
    out = {}
    for segments in (8, 1):
        if segments == 1:
            monkeypatch.setenv("BIOEN_HIP_SEGMENTS", "1")
        with bioen_amd.Context(yT, YT) as ctx:
            p = assert_gram_regime(ctx, shape, local_segments=segments)
            assert p["tc"] >= 16, p
            out[segments] = ctx.forces_gram(forces=f, w0=w0, theta=10.0)[:2] + (p,)
    (C8, H8, p8), (C1, H1, p1) = out[8], out[1]
    dc, dh = float(np.abs(C8 - C1).max() / np.abs(C1).max()), float(np.abs(H8 - H1).max() / np.abs(H1).max())
    print("600x33700: 8 segments (gs %d, chains of %d) against 1 (gs %d, chains of %d): |dC| = %.3g max|C|, |dH| = %.3g max|H|"
          % (p8["gs"], p8["tc"], p1["gs"], p1["tc"], dc, dh))
    assert dc <= GATE and dh <= GATE


# ---- 2. forces_gram_bf16 -----------------------------------------------------------------------------------------------------
def bf16_bounds(yT, YT, w0, f, theta, tg, C):
    """the module docstring's bounds: -> {"i": (E_C, E_H), "ii": (E_C, E_H)} as matrices, from FP64 host quantities and
    |C| of the side compared with"""
    w = forces.get_weights_from_forces(w0, yT, f)[:, 0]
    ybar = yT.dot(w)
    x = yT.T.dot(f)
    q = theta * (x - w.dot(x)) + yT.T.dot(ybar - YT)
    u2 = w * (q - w.dot(q))
    a = yT - YT[:, None]
    d1, d2 = np.einsum("ij,j,ij->i", a, w, a), np.einsum("ij,j,ij->i", a, np.abs(u2), a)
    s1, s2 = np.sqrt(np.outer(d1, d1)), np.sqrt(np.outer(d2, d2))
    top = np.abs(yT).max(axis=1)
    F = 4 * yT.shape[1] * EPS * np.outer(top, top)
    Ca = np.abs(C)
    out = {}
    for name, b in (("ii", 48 * tg * U23), ("i", 48 * tg * U23 + 3 * U16)):
        E1 = b * s1 + F
        E2 = b * s2 + GATE * s2 + (1.0 + 2.0 * np.abs(u2).sum()) * F
        out[name] = (E1, theta * E1 + E2 + E1.dot(Ca) + (Ca + E1).dot(E1))
    return out


@pytest.mark.parametrize("shape", BF16_SHAPES, ids=case_id)
def test_gram_bf16_at_depth(bioen_amd, monkeypatch, shape):
    """C~ and H~ inside the derived bounds -- (i) against the FP64 pass at every theta, (ii) against the restatement where
    RESTATED says it is affordable, at theta = 10 --, not the FP64 pass's bits, bitwise symmetric, the same bits again, and
    forces_gram() afterwards returns the FP64 bits it returned before"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, f = problem(shape)
    with bioen_amd.Context(yT, YT) as ctx:
        tg = assert_gram_regime(ctx, shape)["tc"]
        for theta in THETAS:
            C, H, _, _ = ctx.forces_gram(forces=f, w0=w0, theta=theta)
            Cb, Hb = ctx.forces_gram_bf16()
            label = "%dx%d theta %g, chains of %d" % (shape + (theta, tg))
            SC, SH = float(np.abs(C).max()), float(np.abs(H).max())
            bounds = bf16_bounds(yT, YT, w0, f, theta, tg, C)
            EC, EH = bounds["i"]
            dC, dH = np.abs(Cb - C), np.abs(Hb - H)
            print("%s: (i) |C~ - C| = %.3g of its bound, %.3g max|C| (%.3g CAP); |H~ - H| = %.3g of its bound, %.3g max|H| "
                  "(%.3g CAP)" % (label, float((dC / EC).max()), dC.max() / SC, dC.max() / SC / CAP,
                                  float((dH / (EH + GATE * SH)).max()), dH.max() / SH, dH.max() / SH / CAP))
            assert np.array_equal(Cb, Cb.T) and np.array_equal(Hb, Hb.T)
            assert (dC <= EC + GATE * SC).all() and (dH <= EH + GATE * SH).all()
            assert dC.max() > 0.0 and dH.max() > 0.0
            if RESTATED[shape] and theta == 10.0:
                t0 = time.time()
                Cr, Hr = forces.hessian_gram_bf16_bioen_log_posterior_base(f, w0, yT, YT, theta)
                spent = time.time() - t0
                EC, EH = bf16_bounds(yT, YT, w0, f, theta, tg, Cr)["ii"]
                rC, rH = np.abs(Cb - Cr), np.abs(Hb - Hr)
                print("%s: (ii) |C~ - C~_rest| = %.3g of its bound, %.3g max|C| (%.3g REST); |H~ - H~_rest| = %.3g of its bound, "
                      "%.3g max|H| (%.3g REST); the restatement took %.1f s"
                      % (label, float((rC / EC).max()), rC.max() / SC, rC.max() / SC / REST, float((rH / EH).max()),
                         rH.max() / SH, rH.max() / SH / REST, spent))
                assert (rC <= EC).all() and (rH <= EH).all()
            Cb2, Hb2 = ctx.forces_gram_bf16()
            assert np.array_equal(Cb2, Cb) and np.array_equal(Hb2, Hb)
            C2, H2 = ctx.forces_gram()
            assert np.array_equal(C2, C) and np.array_equal(H2, H)


# ---- 3. forces_colquad ---------------------------------------------------------------------------------------------------------
def column_sample(shape, sps, segments):
    """all 32 columns of panel 0, of panels 255, 256 and 257 (the end of a block's first round, the start of its second), of
    the first panel of the third round, of the last full panel and the ragged last one; the 32 columns either side of
    every segment boundary; 200 columns seeded at random"""
    n = shape[1]
    panels = -(-n // 32)
    cols = set(np.random.default_rng(n).integers(0, n, 200).tolist())
    for p in (0, 255, 256, 257, 512, n // 32 - 1, panels - 1):
        if 0 <= p < panels:
            cols |= set(range(32 * p, min(32 * p + 32, n)))
    for v in range(1, segments):
        edge = v * sps * 16
        cols |= set(range(max(0, edge - 32), min(edge + 32, n)))
    return np.array(sorted(cols))


def spread_ld(A, ybar):
    """(a . a).sum(0) for every column in longdouble, column blocks on eight threads: O(M N)"""
    blocks = [b for b in np.array_split(np.arange(A.shape[1]), 32) if b.size]
    with ThreadPoolExecutor(8) as workers:
        return np.concatenate(list(workers.map(lambda c: ((A[:, c[0]:c[-1] + 1] - ybar[:, None]) ** 2).sum(axis=0), blocks)))


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_colquad_where_a_block_runs_many_panels(bioen_amd, monkeypatch, shape):
    """the four kinds of P: sampled columns against longdouble at CQ_GATE scale; every column against a float64 einsum at
    COARSE CQ_GATE scale (scale: the sample's, no larger than all columns'); P = 0 exact zeros; P = I against (a . a).sum(0)
    in longdouble for every column; a second call the same bits"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, f = problem(shape)
    m, n = shape
    A, pt = matrix_ld(shape), truth(shape)["pt"]
    mats, u = matrices(m, 11 + m)
    a64 = yT - pt["ybar"].astype(np.float64)[:, None]
    with bioen_amd.Context(yT, YT) as ctx:
        plan = assert_colquad_regime(ctx, shape)
        segments = ctx.strip_plan(1)["local_segments"]
        assert segments == REGIMES[shape]["segments"]
        cols = column_sample(shape, ctx.strip_plan(1)["sps"], segments)
        a = A[:, cols] - pt["ybar"][:, None]
        ctx.forces_hessp(None, forces=f, w0=w0, theta=10.0)
        for name, P in mats.items():
            v = ctx.forces_colquad(P)
            assert v.shape == (n,) and np.array_equal(ctx.forces_colquad(P), v)
            if name == "0":
                assert not v.any()
                continue
            ref, scale = colquad_ld(a, P)
            err = float(np.abs(v[cols] - ref).max()) / scale
            if name == "I":
                every = spread_ld(A, pt["ybar"]).astype(np.float64)
            elif name == "uu^T":
                every = ((u.astype(L) @ A - u.astype(L) @ pt["ybar"]) ** 2).astype(np.float64)
            else:
                every = np.einsum("ij,ij->j", P.dot(a64), a64)
            drift = float(np.abs(every[cols] - ref).max()) / scale
            coarse = float(np.abs(v - every).max()) / scale
            print("%dx%d (NB %d, %d panels on %d blocks), P = %s: %d sampled columns |v - v_ld| = %.3g scale; every column "
                  "|v - v_every| = %.3g scale (the comparison itself on the sample: %.3g)"
                  % (shape + (plan["nch"], plan["sps"], plan["gs"], name, cols.size, err, coarse, drift)))
            assert err <= CQ_GATE
            assert drift <= 0.1 * COARSE * CQ_GATE
            assert coarse <= COARSE * CQ_GATE


# ---- 4. forces_laplace -----------------------------------------------------------------------------------------------------------
def test_laplace_at_depth(bioen_amd):
    """600 x 33700 at the optimum opt_newton_forces finds (gtol 1e-8): matrices=True against False the same bits; var_logw
    against forces_colquad(cov_forces) on the same context; var_logw on the column sample against a_j^T H^-1 a_j in
    longdouble, H^-1 = forces._laplace_inverse of the device's H (test 1 holds H; forming H through 600 matrix-free
    products would take a minute); logdet_H against slogdet"""
    shape = (600, 33700)
    yT, YT, w0, _ = problem(shape)
    m, n = shape
    theta = 10.0
    with bioen_amd.Context(yT, YT) as ctx:
        assert_gram_regime(ctx, shape)
        assert_colquad_regime(ctx, shape)
        res = ctx.opt_newton_forces(np.zeros(m), w0, theta, dict(gtol=1e-8), want_weights=False)
        assert res["status"] in (0, 2)
        fopt = res["forces"]
        got = ctx.forces_laplace(forces=fopt, w0=w0, theta=theta)
        lean = ctx.forces_laplace(forces=fopt, w0=w0, theta=theta, matrices=False)
        assert got["info"] == lean["info"] == 0
        for k in ("std_forces", "std_averages", "var_logw"):
            assert np.array_equal(got[k], lean[k]), k
        assert got["logdet_H"] == lean["logdet_H"] and lean["cov_forces"] is None
        again = ctx.forces_colquad(got["cov_forces"])
        top = float(np.abs(got["var_logw"]).max())
        d = float(np.abs(got["var_logw"] - again).max()) / top
        C, H = ctx.forces_gram()
        cols = column_sample(shape, ctx.strip_plan(1)["sps"], 8)
    Hi = forces._laplace_inverse(H, theta)
    cond = float(np.linalg.cond(H))
    gate = GATE_SOLVE * m * EPS * cond
    pt = point_ld(matrix_ld(shape), YT, w0, fopt)
    ref, scale = colquad_ld(matrix_ld(shape)[:, cols] - pt["ybar"][:, None], Hi)
    err = float(np.abs(got["var_logw"][cols] - ref).max()) / scale
    sign, ld = np.linalg.slogdet(H)
    print("600x33700: |var_logw - colquad(cov_forces)| = %.3g of its largest entry; on %d sampled columns |var_logw - a^T H^-1 a| "
          "= %.3g scale (gate %.3g = %.3g m eps cond, cond(H) = %.3g); logdet_H %.17g, slogdet %.17g"
          % (d, cols.size, err, gate, GATE_SOLVE, cond, got["logdet_H"], ld))
    assert d <= 1e-8
    assert gate <= 1e-6                                          # a wrong panel cannot hide in it
    assert err <= gate
    assert sign == 1.0 and abs(got["logdet_H"] - ld) <= 1e-12 * abs(ld)


# ---- 5. the Newton step ------------------------------------------------------------------------------------------------------------
ONE = dict(max_iterations=1)
_STEP = {}


def step_truth(shape):
    """-> dict(p, g, H64, host: {source: the restatement's one-iteration run}, sweeps, last) at forces0 = STEP_SCALE f"""
    if shape not in _STEP:
        yT, YT, w0, f = problem(shape)
        f0 = STEP_SCALE * f
        A = matrix_ld(shape)
        pt = point_ld(A, YT, w0, f0)
        g = objective_ld(A, pt)(STEP_THETA)[1]
        C64, H64 = forces.hessian_gram_bioen_log_posterior_base(f0, w0, yT, YT, STEP_THETA)
        factor = scipy.linalg.cho_factor(H64, lower=True)
        p, sweeps, last = refine_solve(lambda z: products_ld(A, pt, z[None, :])(STEP_THETA)[1][:, 0], -g, factor)
        # (the restatement from the FP64 Hessian; its split-BF16 run costs 3 s more per shape and says the same of a step
        # that differs by 1e-6: the device's own counts are asserted for both sources)
        host = forces.newton_bioen_log_posterior_base(f0, w0, yT, YT, STEP_THETA, dict(ONE, hessian="gram"))
        _STEP[shape] = dict(f0=f0, p=p, g=g, C64=C64, H64=H64, host=host, sweeps=sweeps, last=last)
    return _STEP[shape]


def first_step_taken(r):
    """one accepted step from one factorisation with lambda = 0"""
    return (r["status"], r["iterations"], r["evaluations"], r["hessians"], r["factorisations"], r["lam"]) == (1, 1, 2, 1, 1, 0.0)


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=case_id)
def test_newton_step_direction(bioen_amd, monkeypatch, shape):
    """opt_newton_forces with max_iterations = 1 from both Hessian sources: the returned forces minus forces0 is the device's
    p (to the rounding of that sum, 2 eps max|f|).  gram: within GATE_SOLVE m eps cond(H) max|p| of the 80-bit step, a
    bound asserted to be <= 1e-8 max|p| here.  gram_bf16: a descent direction, within |H^-1| |dH| |p~| of it (dH: test 2's
    bound (i); exact, not first order: (H + dH) p~ = -g gives p~ - p = -H^-1 dH p~), and not the FP64 step's bits"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, f = problem(shape)
    m = shape[0]
    ref = step_truth(shape)
    assert ref["last"] <= 1e-17 and ref["sweeps"] <= 5, (ref["sweeps"], ref["last"])
    assert first_step_taken(ref["host"]), ref["host"]
    f0, p, H64 = ref["f0"], ref["p"], ref["H64"]
    S = float(np.abs(p).max())
    cond = float(np.linalg.cond(H64))
    gate = GATE_SOLVE * m * EPS * cond
    assert gate <= 1e-8, (cond, gate)
    with bioen_amd.Context(yT, YT) as ctx:
        tg = assert_gram_regime(ctx, shape)["tc"]
        out = {}
        for s in ("gram", "gram_bf16"):
            res = ctx.opt_newton_forces(f0, w0, STEP_THETA, dict(ONE, hessian=s), want_weights=False)
            assert first_step_taken(res) and not res["switched"], (s, res)
            out[s] = res["forces"]
    sum_rounding = 2 * EPS * float(max(np.abs(f0).max(), np.abs(out["gram"]).max()))
    p64 = (out["gram"] - f0).astype(L)
    err = float(np.abs(p64 - p).max())
    p16 = out["gram_bf16"] - f0
    EH = bf16_bounds(yT, YT, w0, f0, STEP_THETA, tg, ref["C64"])["i"][1] + GATE * np.abs(H64).max()
    bound16 = np.abs(np.linalg.inv(H64)).dot(EH.dot(np.abs(p16)))
    d16 = np.abs(p16.astype(L) - p).astype(np.float64)
    descent = float(ref["g"] @ p16.astype(L))
    print("%dx%d: chains of %d; reference: %d sweeps, last correction %.3g max|p|; cond(H) = %.3g, gate %.3g max|p|; gram |p - "
          "p_ld| = %.3g max|p|; gram_bf16 |p~ - p_ld| = %.3g max|p|, %.3g of its bound, g . p~ = %.3g"
          % (shape + (tg, ref["sweeps"], ref["last"], cond, gate, err / S, float(d16.max()) / S,
                      float((d16 / (bound16 + gate * S + sum_rounding)).max()), descent)))
    assert err <= gate * S + sum_rounding
    assert descent < 0.0
    assert (d16 <= bound16 + gate * S + sum_rounding).all()
    assert not np.array_equal(out["gram_bf16"], out["gram"])


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------------
def bits(res):
    return (res["forces"].tobytes(), res["fmin"], res["gmax"], res["status"], res["iterations"], res["evaluations"],
            res["hessians"], res["factorisations"], res["switched"])


@pytest.mark.parametrize("theta", (10.0, 1000.0))
@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=case_id)
def test_loop_at_depth(bioen_amd, monkeypatch, shape, theta):
    """both sources from forces = 0: status 0 or 2; fmin not above scipy's trust-exact (hessian=gram) on the device objective,
    by tests/test_hip_forces_newton.py's margin; the returned point judged on its own: the 80-bit gradient there passes the
    stop test (status 0: max|grad| <= gtol, status 2: the reported maximum) up to the FP64 evaluation's rounding -- 64 ulp
    of the gradient's condition, tests/test_hip_edgecases.py's clause --, fmin is the 80-bit objective to 1e-12; a second run
    and a fresh context return the same bits"""
    enter_regime(monkeypatch, shape)
    yT, YT, w0, _ = problem(shape)
    m = shape[0]
    c_bioen.clear_cache()
    cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:hessian=gram,scipy:gtol=1e-6")
    cfg.update(verbose=False)
    trust = forces.find_optimum(np.zeros((m, 1)), w0.reshape(-1, 1), yT, yT, YT.reshape(1, -1), theta, cfg)
    c_bioen.clear_cache()
    A = matrix_ld(shape)
    for source in ("gram", "gram_bf16"):
        params = dict(hessian=source)
        with bioen_amd.Context(yT, YT) as ctx:
            plan = assert_gram_regime(ctx, shape)
            res = ctx.opt_newton_forces(np.zeros(m), w0, theta, params, want_weights=False)
            second = ctx.opt_newton_forces(np.zeros(m), w0, theta, params, want_weights=False)
        with bioen_amd.Context(yT, YT) as fresh:
            third = fresh.opt_newton_forces(np.zeros(m), w0, theta, params, want_weights=False)
        pt = point_ld(A, YT, w0, res["forces"])
        f_ld, g_ld = objective_ld(A, pt)(theta)
        w64 = pt["w"].astype(np.float64)
        t = np.abs((theta * (1.0 + np.log(w64 / w0)) + (pt["r"].astype(np.float64)).dot(yT)) * w64)
        rounding = 64 * 2.0 ** -52 * float((np.abs(yT - YT[:, None]).dot(t)).max())
        gmax = float(np.abs(g_ld).max())
        print("%dx%d theta %g %s (chains of %d): status %d, %d iterations, %d factorisations, switched %s; fmin %.15g (trust-exact "
              "%.15g), |fmin - f_ld| = %.3g |f|; 80-bit max|grad| = %.3g (reported %.3g, rounding allowance %.3g)"
              % (shape + (theta, source, plan["tc"], res["status"], res["iterations"], res["factorisations"], res["switched"],
                          res["fmin"], trust[4], abs(float(res["fmin"] - f_ld)) / abs(float(f_ld)), gmax, res["gmax"], rounding)))
        assert res["status"] in (0, 2)
        assert res["fmin"] <= trust[4] + 1e-9 * abs(trust[4])
        assert gmax <= (1e-6 if res["status"] == 0 else res["gmax"]) + rounding
        assert abs(gmax - res["gmax"]) <= rounding
        assert abs(float(res["fmin"] - f_ld)) <= 1e-12 * abs(float(f_ld))
        assert bits(second) == bits(res) and bits(third) == bits(res)

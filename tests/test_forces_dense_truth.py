"""The truths tests/test_hip_forces_dense_loops.py holds the forces method's dense kernels to at shapes where a full
M x M x N product in 80-bit arithmetic is out of reach, and their own tests on the CPU, at 129 x 257 and 64 x 2000, before
they are trusted:

  point_ld        the kept point's pieces in numpy.longdouble: w, ybar, r, and the two halves of q - <q> = theta xq + bq
                  (the weights do not depend on theta, q is linear in it)
  band_ld         rows of C = G[w], Gx = G[w xq], Gb = G[w bq] from the definitions (tests/test_hip_forces_gram.py:
                  gram_longdouble's formulas restricted to rows), so that rows of T(theta) = theta C + theta Gx + Gb -- H
                  without C C -- are exact; the device's H is compared as H_dev - C_dev C_dev with that product formed in
                  longdouble on the host from the device's own C, whose band is held by itself
  products_ld     C V and H V matrix-free, O(M N) per direction: H V = theta C V + C (C V) + theta Gx V + Gb V
  objective_ld    the objective and its gradient g = theta gx + gb
  refine_solve    A z = rhs by iterative refinement: the operator applied in longdouble, the corrections from a float64
                  Cholesky factor
  cholesky_solve_ld   a dense longdouble solve written out (numpy.linalg takes no longdouble): what refine_solve is held to

Nothing here touches the device; the matrix is only ever multiplied in row or column blocks on eight threads (numpy's
longdouble products release the interpreter lock)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_hip_forces_hessp import problem

L = np.longdouble
THETAS = (0.1, 10.0, 1000.0)


def _blocks(n):
    return [b for b in np.array_split(np.arange(n), 8) if b.size]


def rows_times(A, t):
    """A t in longdouble (t: (N,) or (N, k)): column chunks of about 512 on eight threads, their partial sums added as a
    tree -- numpy adds a longdouble product's N terms one after the other, and a chain of 33700 rounds to 2e-17 of its
    terms, above the 1e-17 the refinement's last correction is held to; chunked, 3e-18"""
    n = A.shape[1]
    chunks = [c for c in np.array_split(np.arange(n), max(1, n // 512)) if c.size]
    with ThreadPoolExecutor(8) as workers:
        parts = list(workers.map(lambda c: A[:, c[0]:c[-1] + 1] @ t[c[0]:c[-1] + 1], chunks))
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def times_columns(v, A):
    """v A in longdouble (v: (M,) or (k, M)), column blocks on eight threads"""
    with ThreadPoolExecutor(8) as workers:
        return np.concatenate(list(workers.map(lambda cols: v @ A[:, cols[0]:cols[-1] + 1], _blocks(A.shape[1]))), axis=-1)


def point_ld(A, YT, w0, f):
    """A: the model's matrix in longdouble.  -> dict(w, ybar, r, x, xq = x - <x>, bq = b - <b> with b = A^T r)"""
    x = times_columns(f.astype(L), A)
    e = w0.astype(L) * np.exp(x - x.max())
    w = e / e.sum()
    ybar = rows_times(A, w)
    r = ybar - YT.astype(L)
    b = times_columns(r, A)
    return dict(w=w, ybar=ybar, r=r, x=x, xq=x - w @ x, bq=b - w @ b, w0=w0.astype(L))


def band_ld(A, pt, rows):
    """-> (C, Gx, Gb)[rows, :] in longdouble: sum_j u_j a_ij a_kj with a = A - ybar, u = w, w xq, w bq; the centring of
    the second factor is taken off as a rank-one term (a_r u) A^T - (sum_j a_rj u_j) ybar^T, which costs 1e-19 here"""
    rows = np.asarray(rows)
    ar = A[rows] - pt["ybar"][rows, None]
    lhs = np.concatenate([ar * u[None, :] for u in (pt["w"], pt["w"] * pt["xq"], pt["w"] * pt["bq"])])
    with ThreadPoolExecutor(8) as workers:
        out = np.concatenate(list(workers.map(lambda blk: lhs @ A[blk[0]:blk[-1] + 1].T, _blocks(A.shape[0]))), axis=1)
    out -= np.outer(lhs.sum(axis=1), pt["ybar"])
    k = rows.size
    return out[:k], out[k:2 * k], out[2 * k:]


def _weighted(A, pt, T, weights):
    """[a (u o t_i) for u in weights], T: (k, N) -> list of (M, k)"""
    k = T.shape[0]
    stacked = np.concatenate([(u[None, :] * T) for u in weights]).T           # (N, k len(weights))
    out = rows_times(A, stacked) - np.outer(pt["ybar"], stacked.sum(axis=0))
    return [out[:, i * k:(i + 1) * k] for i in range(len(weights))]


def _centred_adjoint(A, pt, V):
    """a^T v for the rows v of V (k, M): -> (k, N)"""
    return times_columns(V, A) - (V @ pt["ybar"])[:, None]


def products_ld(A, pt, V):
    """V: (k, M) directions as rows.  -> theta -> (C V, H V), each (M, k) in longdouble, the matrices never formed"""
    V = np.atleast_2d(V).astype(L)
    w = pt["w"]
    CV, GxV, GbV = _weighted(A, pt, _centred_adjoint(A, pt, V), (w, w * pt["xq"], w * pt["bq"]))
    CCV, = _weighted(A, pt, _centred_adjoint(A, pt, CV.T), (w,))

    def at(theta):
        return CV, L(theta) * CV + CCV + L(theta) * GxV + GbV
    return at


def objective_ld(A, pt):
    """-> theta -> (f, grad) in longdouble at the point: f = theta sum w ln(w / w0) + |r|^2 / 2, grad = a (w (q - <q>))"""
    w = pt["w"]
    kl = (w * (np.log(w) - np.log(pt["w0"]))).sum()
    chi = L(0.5) * (pt["r"] * pt["r"]).sum()
    gx, gb = _weighted(A, pt, np.ones((1, w.size), dtype=L), (w * pt["xq"], w * pt["bq"]))

    def at(theta):
        return L(theta) * kl + chi, L(theta) * gx[:, 0] + gb[:, 0]
    return at


def refine_solve(apply, rhs, factor, sweeps_max=5, done=1e-17):
    """A z = rhs: z <- z + cho_solve(factor, rhs - A z) with the residual in longdouble.  -> (z, sweeps, last: max|dz| /
    max|z| of the last correction).  The caller asserts last <= 1e-17 within 5 sweeps before it compares anything"""
    import scipy.linalg
    z, sweeps, last = np.zeros(rhs.size, dtype=L), 0, np.inf
    while sweeps < sweeps_max and last > done:
        res = rhs - apply(z) if sweeps else rhs
        dz = scipy.linalg.cho_solve(factor, res.astype(np.float64)).astype(L)
        z = z + dz
        sweeps += 1
        last = float(np.abs(dz).max() / np.abs(z).max())
    return z, sweeps, last


def cholesky_solve_ld(A, b):
    """A z = b for a symmetric positive definite A, every operation in longdouble"""
    A, m = A.astype(L), A.shape[0]
    Lo = np.zeros((m, m), dtype=L)
    for j in range(m):
        Lo[j, j] = np.sqrt(A[j, j] - Lo[j, :j] @ Lo[j, :j])
        Lo[j + 1:, j] = (A[j + 1:, j] - Lo[j + 1:, :j] @ Lo[j, :j]) / Lo[j, j]
    y = np.zeros(m, dtype=L)
    for i in range(m):
        y[i] = (b[i] - Lo[i, :i] @ y[:i]) / Lo[i, i]
    z = np.zeros(m, dtype=L)
    for i in range(m - 1, -1, -1):
        z[i] = (y[i] - Lo[i + 1:, i] @ z[i + 1:]) / Lo[i, i]
    return z


# ---- the helpers against the full matrices ----------------------------------------------------------------------------------
SHAPES = [(129, 257), (64, 2000)]
ULPS = 64 * np.finfo(L).eps          # "a few longdouble ulps" of the largest entry: the sums differ by their order alone


def full(shape):
    """tests/test_hip_forces_gram.py's gram_longdouble pieces at problem(shape)'s point, kept in longdouble"""
    from test_hip_forces_gram import _gram_ld
    yT, YT, w0, f, _ = problem(shape)
    A = yT.astype(L)
    x = f.astype(L) @ A
    e = w0.astype(L) * np.exp(x - x.max())
    w = e / e.sum()
    ybar = A @ w
    b = (ybar - YT.astype(L)) @ A
    a = A - ybar[:, None]
    C, Gx, Gb = _gram_ld(a, w), _gram_ld(a, w * (x - w @ x)), _gram_ld(a, w * (b - w @ b))
    return A, point_ld(A, YT, w0, f), C, Gx, Gb


def close(got, want, scale=None):
    return float(np.abs(got - want).max()) <= ULPS * float(np.abs(want).max() if scale is None else scale)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_band_equals_the_rows_of_the_full_matrices(shape):
    from test_hip_forces_gram import gram_longdouble
    yT, YT, w0, f, _ = problem(shape)
    A, pt, C, Gx, Gb = full(shape)
    rows = [0, shape[0] - 1, shape[0] // 2, 63, min(64, shape[0] - 1)]
    Cb, Gxb, Gbb = band_ld(A, pt, rows)
    assert close(Cb, C[rows], np.abs(C).max()) and close(Gxb, Gx[rows], np.abs(Gx).max())
    # b = A^T r itself rounds on the scale of |A|^T |r| (its terms cancel), and the two sides add it up in different orders
    a = np.abs(A - pt["ybar"][:, None])
    assert close(Gbb, Gb[rows], ((a[rows] * (pt["w"] * (np.abs(pt["r"]) @ np.abs(A)))) @ a.T).max())
    ref = gram_longdouble(("truth", shape), A, YT, w0, f)
    for theta in THETAS:
        C64, H64 = ref(theta)
        Hb = L(theta) * (Cb + Gxb) + Gbb + Cb @ C
        assert np.abs(Cb.astype(np.float64) - C64[rows]).max() <= 4 * np.finfo(np.float64).eps * np.abs(C64).max()
        assert np.abs(Hb.astype(np.float64) - H64[rows]).max() <= 4 * np.finfo(np.float64).eps * np.abs(H64).max()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_matrix_free_products_equal_the_matrices_times_v(shape):
    A, pt, C, Gx, Gb = full(shape)
    V = np.random.default_rng(shape[0]).standard_normal((8, shape[0])).astype(L)
    prod = products_ld(A, pt, V)
    for theta in THETAS:
        H = L(theta) * (C + Gx) + Gb + C @ C
        CV, HV = prod(theta)
        assert CV.shape == HV.shape == (shape[0], 8)
        assert close(CV, C @ V.T) and close(HV, H @ V.T)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_objective_and_gradient_against_the_written_out_formula(shape):
    """tests/test_hip_strip_loops.py: forces_truth's formula, t = (theta (1 + ln w / w0) + r A) w, grad = (A - ybar) t"""
    yT, YT, w0, f, _ = problem(shape)
    A, pt = yT.astype(L), None
    pt = point_ld(A, YT, w0, f)
    fg = objective_ld(A, pt)
    for theta in THETAS:
        lw = np.log(pt["w"]) - np.log(w0.astype(L))
        t = (L(theta) * (1 + lw) + pt["r"] @ A) * pt["w"]
        a = A - pt["ybar"][:, None]
        grad = a @ t
        obj = L(theta) * (pt["w"] * lw).sum() + L(0.5) * (pt["r"] * pt["r"]).sum()
        got_f, got_g = fg(theta)
        # the written-out t carries a constant (theta (1 - log s) + <b>) that the centred a removes: ITS sum rounds on the
        # scale of |a| |t|, not of the gradient
        assert abs(got_f - obj) <= ULPS * abs(obj) and close(got_g, grad, (np.abs(a) @ np.abs(t)).max())


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_refinement_reproduces_a_longdouble_solve(shape):
    """problem()'s point is no minimum and H indefinite there: the system is H + s I, s lifting the smallest eigenvalue to a
    tenth of the largest (cond about 10, as at the points the GPU tests solve at: the corrections end at cond eps_longdouble,
    and the callers' 1e-17 needs that below it); the operator is the matrix-free one"""
    import scipy.linalg
    A, pt, C, Gx, Gb = full(shape)
    theta = 10.0
    H = L(theta) * (C + Gx) + Gb + C @ C
    H64 = H.astype(np.float64)
    ev = np.linalg.eigvalsh(H64)
    s = max(0.0, -ev[0]) + 0.1 * ev[-1]
    prod = products_ld(A, pt, np.zeros((1, shape[0])))          # (shape check of the single direction path)
    assert prod(theta)[1].shape == (shape[0], 1)

    def apply(z):
        return products_ld(A, pt, z[None, :])(theta)[1][:, 0] + L(s) * z
    rhs = -objective_ld(A, pt)(theta)[1]
    factor = scipy.linalg.cho_factor(H64 + s * np.eye(shape[0]), lower=True)
    z, sweeps, last = refine_solve(apply, rhs, factor)
    assert last <= 1e-17 and sweeps <= 5, (sweeps, last)
    want = cholesky_solve_ld(H + L(s) * np.eye(shape[0], dtype=L), rhs)
    err = float(np.abs(z - want).max() / np.abs(want).max())
    cond = np.linalg.cond(H64 + s * np.eye(shape[0]))
    print("%dx%d: %d sweeps, last %.3g; |z - z_ld| = %.3g max|z|, cond %.3g" % (shape + (sweeps, last, err, cond)))
    assert err <= 64 * shape[0] * np.finfo(L).eps * cond

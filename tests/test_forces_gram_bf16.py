"""The forces Hessian from split-BF16 operands, on the CPU: the numpy restatement
(forces.hessian_gram_bf16_bioen_log_posterior_base) against the FP64 Gram Hessian, its bitwise symmetry, scipy's
trust-exact fed by it through find_optimum, and the refusals of the scipy parameter `hessian`."""
import numpy as np
import pytest

from conftest import FORCES_GOLDEN, load_golden
from test_forces_gram import SEEDED, seeded_problem
from test_forces_hessp import DRIVER_CASES, check_optimum, forces_case, run_driver

from bioen_amd.optimize import forces, minimize

# of max|H| (of max|C| for C).  A cap, not a measurement: a bfloat16 pair hi + lo carries 16 bits of an operand, so the
# three products drop terms of 2^-16 ... 2^-17 of |a| |t| each, which sum like the terms themselves where they have one
# sign (an offset the rank corrections take off).  Measured here: 1.1e-6 ... 1.2e-5; a dropped lo product leaves 2^-9 per term
CAP = 1e-3


def check_against_fp64(x, args, label):
    C, H = forces.hessian_gram_bioen_log_posterior_base(x, *args)
    Cb, Hb = forces.hessian_gram_bf16_bioen_log_posterior_base(x, *args)
    m = x.size
    assert Cb.shape == (m, m) and Hb.shape == (m, m)
    assert np.array_equal(Cb, Cb.T) and np.array_equal(Hb, Hb.T)
    eh, ec = np.abs(Hb - H).max() / np.abs(H).max(), np.abs(Cb - C).max() / np.abs(C).max()
    print("%s: max |H~ - H| = %.3g max|H|, max |C~ - C| = %.3g max|C|" % (label, eh, ec))
    assert eh <= CAP and ec <= CAP
    assert eh > 0.0                          # ... and it IS the split product, not the FP64 one under another name


@pytest.mark.parametrize("name", FORCES_GOLDEN)
def test_restatement_against_the_fp64_hessian_on_the_goldens(name):
    d, args, x, _ = forces_case(name)
    check_against_fp64(x, args, name)


@pytest.mark.parametrize("shape,theta", SEEDED, ids=["%dx%d" % s for s, _ in SEEDED])
def test_restatement_against_the_fp64_hessian_away_from_the_optimum(shape, theta):
    x, args = seeded_problem(shape, theta)
    check_against_fp64(x, args, "%dx%d theta %g" % (shape + (theta,)))


def test_the_rounding_is_bfloat16_round_to_nearest_even():
    """the integer rounding against hand-made cases: ties go to the even neighbour, the split is hi + lo to 2^-17"""
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -7)                                   # bfloat16 keeps 8 significant bits
    v = np.array([1.0, 1.0 + ulp / 2, 1.0 + ulp * 1.5, 1.0 + ulp * 0.75, -(1.0 + ulp / 2), 0.0], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2 * ulp, 1.0 + ulp, -1.0, 0.0], dtype=np.float32)
    assert np.array_equal(forces._bf16_round(v), want) and one == 1.0
    x = np.random.default_rng(0).standard_normal(1000) * 10.0 ** np.random.default_rng(1).uniform(-6, 6, 1000)
    hi, lo = forces._bf16_split(x)
    for part in (hi, lo):
        bits = part.astype(np.float32).view(np.uint32)
        assert np.array_equal(part.astype(np.float32).astype(np.float64), part) and not (bits & 0xffff).any()
    assert np.all(np.abs(hi + lo - x) <= 2.0 ** -16 * np.abs(x))


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_trust_exact_with_the_bf16_hessian_on_the_numpy_objective(name):
    """the same minimum as every other driver: the gradient is FP64, the Hessian only shapes the step"""
    check_optimum(*run_driver(name, "trust_exact", False, mod="scipy:gtol=1e-6,scipy:hessian=gram_bf16"))


def test_the_source_is_recognized():
    cfg = minimize.Parameters("scipy", "scipy:algorithm=trust_exact,scipy:hessian=gram_bf16")
    assert forces._hessian_source(cfg) == "gram_bf16"
    assert "gram_bf16" in forces._HESSIAN_SOURCES


@pytest.mark.parametrize("mod,needle", [("scipy:algorithm=fmin_bfgs,scipy:hessian=gram_bf16", "trust_exact"),
                                        ("scipy:algorithm=trust_exact,scipy:hessian=dense", "not recognized.*gram_bf16")],
                         ids=["wrong-algorithm", "unknown-value"])
@pytest.mark.parametrize("use_c", [False, True], ids=["numpy", "device"])
def test_refusals_come_before_anything_is_evaluated(monkeypatch, mod, needle, use_c):
    from bioen_amd.optimize.ext import c_bioen

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(c_bioen, "hold", touched)
    monkeypatch.setattr(c_bioen, "_context_for", touched)
    monkeypatch.setattr(forces, "bioen_log_posterior_base", touched)
    d = load_golden("ref_data_forces_M64xN64.npz")
    cfg = minimize.Parameters("scipy", mod)
    cfg.update(verbose=False, use_c_functions=use_c)
    with pytest.raises(RuntimeError, match=needle):
        forces.find_optimum(d["forces_init"], d["w0"], d["y"], d["yTilde"], d["YTilde"].reshape(1, -1), d["theta"], cfg)

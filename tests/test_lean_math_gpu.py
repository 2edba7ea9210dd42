"""The lean FP64 functions, the Philox generator and the boundary maps of csrc/common.h on the device, against exact references.

What runs is the HEADER's code under the library's compiler and flags: a HipCallbacks plugin includes common.h before the user's
source, so a derived() may call tph_log, tph_rng, tph_gamma_mt, bc_periodic ... directly (two probes, tests/lean_math_cases.py,
compiled once each).  It is not the instruction sequence inside any particular library kernel: there the compiler schedules and
contracts the same expressions among their neighbours.  The truth is mpmath at 40 digits on the same doubles and Philox words; the
bounds are the project's own statements (common.h, KERNELS.md section 3a) or derived from them in the docstrings, never fitted to
what the device returns.  Every test also evaluates its first rows at n = 1, 63, 64, 65 and 1000 and wants the batch's bits."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import philox as px
from oracle import ps
from tests import lean_math_cases as L

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")]

U = L.U


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _probe(name):
    import tempest_amd as tp
    source, n_dim, n_derived = L.PROBES[name]
    return tp.HipCallbacks(source, n_dim, n_derived=n_derived)


@pytest.fixture(scope="module")
def math_probe():
    return _probe("math")


@pytest.fixture(scope="module")
def rng_probe():
    return _probe("rng")


def evaluate(cb, x):
    """derived() over all rows in one batch; the first rows again at every launch shape: the same bits."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    got = cb.derived(x)
    assert got.shape == (x.shape[0], cb.n_derived)
    for n in L.SIZES:
        n = min(n, x.shape[0])
        np.testing.assert_array_equal(L.bits(cb.derived(x[:n])), L.bits(got[:n]), err_msg=f"n = {n}")
    return got


def math_columns(cb, a, b=None):
    a = np.asarray(a, dtype=np.float64)
    out = evaluate(cb, np.stack([a, np.ones_like(a) if b is None else np.asarray(b, dtype=np.float64)], axis=1))
    return lambda name: L.column(L.MATH_COLUMNS, out, name)


def report(name, err, where, unit):
    k = int(np.argmax(err))
    print(f"{name}: largest error {float(err[k]):.4g} {unit} at {where[k]!r}, mean {float(err.mean()):.3g} over {err.size} values")
    return float(err[k])


# ------------------------------------------------------------------------------------------------------- reciprocal and division
def test_rcp_and_div_within_one_ulp(math_probe):
    """common.h: "1 ulp (sqrt, division)" on the arguments of the call sites (L.DIV_SITES, L.RCP_SITES); a zero numerator gives
    exactly 0, a subnormal numerator over 1.0 (tph_log1p_unit below exp's underflow) itself."""
    b = L.sample_rcp()
    got = math_columns(math_probe, b)("rcp")
    assert np.all(np.isfinite(got))
    assert report("tph_rcp", L.ulp_error(got, L.truth_rcp()), b, "ulp") <= 1.0
    a, b = L.sample_div()
    got = math_columns(math_probe, a, b)("div")
    assert np.all(np.isfinite(got))
    assert (a == 0.0).sum() >= 6 and np.all(got[a == 0.0] == 0.0)
    sub = (np.abs(a) < 2.0 ** -1022) & (a != 0.0) & (b == 1.0)
    assert sub.sum() >= 2
    np.testing.assert_array_equal(L.bits(got[sub]), L.bits(a[sub]))
    assert report("tph_div", L.ulp_error(got, L.truth_div()), list(zip(a, b)), "ulp") <= 1.0


# ------------------------------------------------------------------------------------------------------------------------ square root
def test_sqrt_within_one_ulp_and_zero(math_probe):
    """common.h: "1 ulp (sqrt, division)"; +0 and -0 give +0; the normal at u1 = 1, tph_sqrt(-2.0 * tph_log(1.0)), is +0 and not NaN."""
    x = L.sample_sqrt()
    col = math_columns(math_probe, np.concatenate([x, [1.0]]))
    got = col("sqrt")[:-1]
    zero = x == 0.0
    assert zero.sum() == 2 and np.signbit(x[zero]).sum() == 1
    np.testing.assert_array_equal(L.bits(got[zero]), L.bits(np.zeros(2)))
    assert L.bits(col("log")[-1:])[0] == 0, "tph_log(1.0) is +0"
    assert L.bits(col("radius")[-1:])[0] == 0, "the radius at u1 = 1 is +0"
    assert np.all(np.isfinite(got))
    assert report("tph_sqrt", L.ulp_error(got, L.truth_sqrt()), x, "ulp") <= 1.0


# ------------------------------------------------------------------------------------------------------------------------- logarithm
def test_log_below_one_ulp(math_probe):
    """common.h: "Errors stay below 1 ulp (log)" on L.sample_log(); exactly 0 at the argument 1 (k = 2^53 - 1 and r = 2^32 - 1)."""
    x = L.sample_log()
    got = math_columns(math_probe, x)("log")
    assert np.all(np.isfinite(got))
    one = x == 1.0
    assert one.sum() >= 2 and np.all(got[one] == 0.0)
    assert report("tph_log", L.ulp_error(got, L.truth_log()), x, "ulp") < 1.0


# ------------------------------------------------------------------------------------------------------------------------- sincospi
def test_sincospi_absolute_error_and_unit_circle(math_probe):
    """KERNELS.md 3a / common.h: errors "< 1 ulp of 1": |error| <= 2^-52 on each output.  At the quarter turns t = j / 2 the values
    are 0 or +-1 and must be exact (an odd j / 4 is a tie of rint(2 t): there the bound holds, on either side's kernel).  Second
    check: sn^2 + cs^2 within 4 x 2^-53 of 1."""
    t = L.sample_sincospi()
    col = math_columns(math_probe, t)
    sn, cs = col("sinpi"), col("cospi")
    ts, tc = L.truth_sincospi()
    turn = np.isin(t, L.QUARTERS[::2])
    assert turn.sum() >= 5 and np.isin(t, L.QUARTERS[1::2]).sum() >= 4
    np.testing.assert_array_equal(sn[turn], ts.near[turn])
    np.testing.assert_array_equal(cs[turn], tc.near[turn])
    es = report("tph_sincospi sin", L.abs_error(sn, ts) / 2.0 ** -52, t, "x 2^-52")
    ec = report("tph_sincospi cos", L.abs_error(cs, tc) / 2.0 ** -52, t, "x 2^-52")
    defect = report("tph_sincospi sn^2 + cs^2 - 1", np.abs(L.unit_circle_defect(sn, cs)) / 2.0 ** -53, t, "x 2^-53")
    assert es <= 1.0 and ec <= 1.0
    assert defect <= 4.0


# ----------------------------------------------------------------------------------------------------------- log1p_unit, logaddexp
def test_log1p_unit_and_logaddexp(math_probe):
    """tph_log1p_unit(e), 0 <= e <= 1: |error| <= 3 U log1p(e) + 4 U^2 (L.bound_log1p: tph_log's ulp on log u, the final sum, and the
    second-order terms of c / u).  tph_logaddexp(x, y): |error| <= U (|r| + (2 + |t|) q + 3 log1p(E)) + 8 U^2 + 5e-324 with t = x - y,
    E = exp(-|t|), q = E / (1 + E) (L.truth_logaddexp: the rounding of t, one ulp for the library exp, log1p_unit, the final sum).
    On L.logaddexp_specials() the bits are np.logaddexp's."""
    e = L.sample_log1p()
    got = math_columns(math_probe, e)("log1p_unit")
    truth = L.truth_log1p()
    err, bound = L.abs_error(got, truth), L.bound_log1p(truth)
    report("tph_log1p_unit", err / np.spacing(np.abs(truth.near)), e, "ulp")
    assert report("tph_log1p_unit error / bound", err / bound, e, "") <= 1.0
    assert got[e == 0.0][0] == 0.0 and got[e == 5e-324][0] == 5e-324

    x, y = L.sample_logaddexp()
    got = math_columns(math_probe, x, y)("logaddexp")
    truth, bound = L.truth_logaddexp()
    err = L.abs_error(got, truth)
    report("tph_logaddexp", err / np.spacing(np.abs(truth.near)), list(zip(x, y)), "ulp")
    assert report("tph_logaddexp error / bound", err / bound, list(zip(x, y)), "") <= 1.0

    x, y = L.logaddexp_specials()
    got = math_columns(math_probe, x, y)("logaddexp")
    with np.errstate(invalid="ignore"):
        want = np.logaddexp(x, y)
        far = np.abs(x - y) > 745.0
    assert np.isnan(want).sum() == 5 and np.isinf(want).sum() >= 4
    assert far.sum() >= 6 and np.all(want[far & np.isfinite(x) & np.isfinite(y)] == np.maximum(x, y)[far & np.isfinite(x) & np.isfinite(y)])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(L.bits(got), L.bits(want))


# --------------------------------------------------------------------------------------------------------------------- boundary maps
def test_boundary_maps_bit_for_bit(math_probe):
    """bc_periodic is NumPy's v % 1.0 and bc_reflective the reference's formula as oracle/ps.py restates it, bit for bit; both lie in
    [0, 1] for finite input (-1e-17 % 1.0 is 1.0); NaN gives NaN."""
    v = L.sample_bc()
    col = math_columns(math_probe, np.concatenate([v, [np.nan]]))
    per, ref = col("bc_periodic"), col("bc_reflective")
    assert np.isnan(per[-1]) and np.isnan(ref[-1])
    per, ref = per[:-1], ref[:-1]
    want_per = ps.apply_boundary_conditions(v[:, None], periodic=[0])[:, 0]
    want_ref = ps.apply_boundary_conditions(v[:, None], reflective=[0])[:, 0]
    np.testing.assert_array_equal(L.bits(want_per), L.bits(v % 1.0))
    assert want_per[v == -1e-17][0] == 1.0
    for name, got, want in (("bc_periodic", per, want_per), ("bc_reflective", ref, want_ref)):
        np.testing.assert_array_equal(L.bits(got), L.bits(want), err_msg=name)
        assert np.all((got >= 0.0) & (got <= 1.0)), name
    print(f"bc_periodic, bc_reflective: {v.size} values bit for bit")


# ---------------------------------------------------------------------------------------------------------------- RNG, bit for bit
def test_philox_words_and_uniforms_bit_for_bit(rng_probe):
    """tph_philox's four words and tph_rng::uniform2 on Random123's three known-answer vectors, the counter corners (item 2^32 is
    item 0) and 4096 random counters: the published words, and elsewhere the oracle's."""
    c = L.corner_counters()
    out = evaluate(rng_probe, L.probe_rows(c))
    col = lambda name: L.column(L.RNG_COLUMNS, out, name)
    words = [col(f"w{k}") for k in range(4)]
    for row, (_, _, want) in enumerate(L.KAT):
        assert tuple(int(w[row]) for w in words) == want, f"known-answer vector {row}"
    want = L.oracle_words(c)
    for k in range(4):
        np.testing.assert_array_equal(words[k], want[k].astype(np.float64), err_msg=f"word {k}")
    for name, u in zip(("u_a", "u_b"), L.by_seed(c, px.uniform_pair, 2)):
        np.testing.assert_array_equal(L.bits(col(name)), L.bits(u), err_msg=name)
    k53 = ((c.item & np.uint64(L.MASK32)) >> np.uint64(5) << np.uint64(26)) | (c.draw >> np.uint64(6))
    np.testing.assert_array_equal(col("k53"), k53.astype(np.float64))
    assert col("k53").max() == 2.0 ** 53 - 1.0
    print(f"tph_philox, uniform2, tph_k53: {c.item.size} counters bit for bit")


# ------------------------------------------------------------------------------------------------------------------- RNG, analytic
def test_normal2_and_gamma_candidate_against_mpmath(rng_probe):
    """normal2 (both outputs) and gamma_candidate's x: |error| <= 6 x 2^-53 x sqrt(-2 ln u1).  With U = 2^-53 and one ulp of relative
    error counted as 2 U: tph_log contributes 2 U, which the square root halves to U; tph_sqrt's own error adds 2 U, so the radius is
    within 3 U; tph_sincospi adds 2 U absolute on an exact angle; the product's rounding U |z|: rad (3 U |trig| + 2 U) + U rad <=
    6 U rad.  gamma_candidate's logu is tph_log of an exact argument: within one ulp.  On 2 x 10^4 ordinary counters and the extreme
    blocks of a 2^22-item scan: the smallest and largest u1, u2 next to every multiple of 1/8."""
    c, t = L.normal_counters(), L.truth_normals()
    assert c.item.size == 20000 + 11 * 32
    out = evaluate(rng_probe, L.probe_rows(c))
    bound = L.bound_normal(t.rad)
    assert np.all(bound > 0.0) and t.rad.max() > 5.3 and t.rad.min() < 1e-3
    worst = 0.0
    for name, truth in (("z0", t.z0), ("z1", t.z1), ("cand_x", t.x)):
        got = L.column(L.RNG_COLUMNS, out, name)
        assert np.all(np.isfinite(got))
        worst = max(worst, report(f"tph_rng {name} error / (6 U rad)", L.abs_error(got, truth) / bound, list(zip(c.item, c.draw)), ""))
    err = report("tph_rng cand_logu", L.ulp_error(L.column(L.RNG_COLUMNS, out, "cand_logu"), t.logu), list(zip(c.item, c.draw)), "ulp")
    assert worst <= 1.0
    assert err <= 1.0


@pytest.mark.parametrize("shape", L.GAMMA_SHAPES)
def test_gamma_mt_accepts_the_exact_attempt(rng_probe, shape):
    """tph_gamma_mt over items 0 .. 3999 (seed 7, tick 3): the device's value lies within the bound propagated from the candidate's,
    |dv| / v <= 3 |d(1 + c x)| / (1 + c x) (L.truth_gamma derives every term), of the value that the EXACT evaluation of Marsaglia-
    Tsang's test accepts first.  The values of two attempts differ by far more than that, so this pins the accepted attempt too.  An
    item may be left out only where its exact acceptance margin is below the rounding bound of the inequality: none is, and that is
    asserted.  The fallback after 64 rejected attempts cannot be reached by choosing counters (an attempt is rejected with
    probability below 0.05) and stays untested."""
    truth, kept = L.truth_gamma()[shape]
    print(f"shape {shape}: {truth.left_out} left out, smallest margin {truth.min_margin:.3g} d, "
          f"attempts used up to {int(truth.attempts.max())}, {int((truth.attempts > 0).sum())} items past the first")
    assert truth.left_out == 0 and kept.all()
    if shape < 10.0:                       # the rejection rate falls with the shape: 3 items in 4000 at 50.5, none at 5e5
        assert (truth.attempts > 0).sum() >= 20
    got = L.column(L.RNG_COLUMNS, evaluate(rng_probe, L.gamma_rows(shape)), "gamma")
    assert np.all(np.isfinite(got) & (got > 0.0))
    err = L.abs_error(got, truth.value)
    report(f"tph_gamma_mt({shape}) relative error / U", err / np.abs(truth.value.near) / U, np.arange(got.size), "")
    assert report(f"tph_gamma_mt({shape}) error / bound", err / truth.bound, np.arange(got.size), "") <= 1.0

"""Pareto-smoothed importance-sampling LOO (HipCallbacks(pointwise="psis")), the part that needs neither a
compiler nor a GPU: the oracle of tests/psis_cases.py held against what is known of the estimator, the record of the new plugin
part (-D list, key, text, prototypes), what the constructors accept and refuse, the sizing function and compare_pointwise."""
import ctypes as C
import math

import numpy as np
import pytest

from tempest_amd import hipcallbacks as H
from tempest_amd._cdecl import prototypes
from tempest_amd._lib import TempestHipError
from tests import psis_cases as pc

TABLES = (("A", 2),)


# ------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("k_true", [0.1, 0.5, 0.9])
def test_fit_recovers_the_shape_on_the_quantile_grid(k_true):
    N = 3000
    p = (np.arange(1, N + 1) - 0.5) / N
    x = np.expm1(-k_true * np.log1p(-p)) / k_true               # GPD(k, sigma = 1) quantiles, ascending
    k, sigma = pc.gpd_fit(x)
    print(f"k = {k_true}: fitted {k:.4f}, sigma {sigma:.4f}")
    assert abs(k - k_true) <= 0.05 and abs(sigma - 1.0) <= 0.1


def test_khat_of_a_gaussian_ratio_follows_the_variance():
    """a = -z^2 / 2 with z ~ N(0, s^2): the ratios exp(-a) have a Pareto tail of shape s^2."""
    rng = np.random.default_rng(5)
    for s2, lo, hi in ((0.25, 0.0, 0.5), (1.0, 0.6, 1.4)):
        k = np.median([pc.psis_column(-0.5 * s2 * rng.standard_normal(4000) ** 2)[0] for _ in range(9)])
        assert lo < k < hi, (s2, k)


def test_unsmoothed_cases_are_plain_importance_sampling():
    cases = {"S=20": pc.gauss_case(20, 7)}
    cases.update((k, v) for k, v in pc.tie_cases().items() if k != "runs_of_8")
    for name, A in cases.items():
        for a in A:
            k, elpd, ess = pc.psis_column(a)
            v = np.exp(a.min() - a)
            assert k == np.inf, name
            assert abs(elpd - pc.is_loo_column(a)) <= 1e-13 * max(1.0, abs(elpd)), name
            assert abs(ess - v.sum() ** 2 / (v * v).sum()) <= 1e-12 * ess, name
    assert all(np.isfinite(pc.psis_oracle(pc.tie_cases()["runs_of_8"])["pareto_k"]))
    assert pc.tail_len(20) == 4 and pc.tail_len(21) == 5 and pc.tail_len(24) == 5 and pc.tail_len(1000) == 95


def test_special_values_of_the_oracle():
    got = pc.psis_oracle(pc.special_case())
    for k in pc.KEYS:
        assert np.isnan(got[k][1]) and np.isfinite(got[k][0]) and np.isfinite(got[k][3]) and np.isfinite(got[k][5])
    assert got["elpd_psis"][2] == -np.inf and got["elpd_psis"][4] == np.inf
    assert np.isnan(got["pareto_k"][[2, 4]]).all() and np.isnan(got["ess_psis"][[2, 4]]).all()


def test_the_recorded_bound_is_eight_times_a_figure_below_the_conditioning_limit():
    assert set(pc.PSIS_RTOL) == set(pc.KEYS)
    for k in pc.KEYS:
        assert pc.PSIS_RTOL[k] == 8.0 * pc.PSIS_MEASURED[k] and pc.PSIS_MEASURED[k] < 1e-10
    ref = pc.psis_oracle(pc.gauss_case(257, 7))
    got = pc.psis_oracle(pc.gauss_case(257, 7), ops=pc.Perturbed(0))
    for k in pc.KEYS:
        pc.close(got[k], ref[k], k)


def test_tail_length_and_threshold_are_the_oracles():
    for n in (1, 2, 20, 21, 24, 25, 100, 1000, 4096, 131072, 1_864_135, 1_864_136, 10 ** 7):
        assert H.psis_tail_len(n) == pc.tail_len(n, H.PSIS_MAX_TAIL), n
    assert H.psis_tail_len(1_864_135) == 4096 and 3.0 * math.sqrt(1_864_135) < 4096 < 3.0 * math.sqrt(1_864_136)
    assert H.PSIS_MAX_TAIL == pc.MAX_TAIL >= 4096
    for n in (100, 1000, 131072):
        assert H.psis_k_threshold(n) == pc.k_threshold(n)
    assert H.psis_k_threshold(100) == 0.5 and H.psis_k_threshold(10 ** 6) == 0.7


# ------------------------------------------------------------------------------------ the plugin part
def test_the_part_record_of_a_psis_plugin():
    p = H._Parts.of(pc.SOURCE, TABLES, term=True, pointwise="psis")
    assert p.pointwise is True and p.psis is True and p._fields[-1] == "psis"
    assert p.defines(2)[-2:] == ["-DTPHU_POINTWISE", "-DTPHU_PSIS"]
    assert p.key(2).endswith("|pointwise|psis")
    assert p.build_args()["pointwise"] == "psis" and "psis" not in p.build_args()
    assert H._Parts.of(pc.SOURCE, **p.build_args()) == p
    text = p.text(pc.SOURCE)
    assert "int tphu_psis(" in text and "int tphu_psis_layout(" in text and "//@" not in text
    assert f"#define TPHU_PSIS_MAXTAIL {H.PSIS_MAX_TAIL} " in text
    for kernel in ("k_user_psis_hist", "k_user_psis_sweep", "k_user_psis_fit", "k_user_predict_narrow", "k_user_pw_range"):
        assert f" {kernel}(" in text, kernel
    assert "void __launch_bounds__(256) k_user_predict_hist(" not in text           # predict()'s own kernels stay out
    restype, argtypes = prototypes(text, "tphu_")["tphu_psis"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                        C.c_int64, C.c_void_p]
    part = {q.name: q for q in H._PARTS}["psis"]
    assert part.layout == H.PREDICT_SUM_LAYOUT + (H.POINTWISE_MAX_TILE, H.PREDICT_TABLES, H.PSIS_MAX_TAIL)
    assert H.PSIS_KEYS == pc.KEYS


def test_pointwise_true_keeps_its_text_key_and_defines():
    plain = H._Parts.of(pc.SOURCE, TABLES, True, 0, False, True)
    assert plain.psis is False and plain.build_args()["pointwise"] is True
    text = plain.text(pc.SOURCE)
    assert text == H.plugin_source(pc.SOURCE, TABLES, True, pointwise=True) and "psis" not in text.lower()
    assert plain.defines(2) == ["-DN_DIM=2", "-DTPHU_POINTWISE"] and plain.key(2).endswith("|pointwise")
    assert plain.key(2) + "|psis" == H._Parts.of(pc.SOURCE, TABLES, True, 0, False, "psis").key(2)
    assert H._Parts.of(pc.SOURCE, TABLES, True, 0, False, "PSIS").psis is False


class _Stop(Exception):
    pass


@pytest.fixture
def no_compiler(monkeypatch):
    seen = {}

    def build_plugin(source, n_dim, verbose=False, **kw):
        seen.update(kw)
        raise _Stop
    monkeypatch.setattr(H, "build_plugin", build_plugin)
    return seen


def test_the_constructor_hands_the_level_through_pointwise(no_compiler):
    with pytest.raises(_Stop):
        H.HipCallbacks(pc.SOURCE, 2, data={"A": np.zeros((3, 4))}, n_terms=3, pointwise="psis")
    assert no_compiler["pointwise"] == "psis"
    assert set(no_compiler) == {"tables", "term", "n_derived", "predict", "pointwise", "replicate", "discrepancy"}
    no_compiler.clear()
    with pytest.raises(_Stop):
        H.HipCallbacks(pc.SOURCE, 2, data={"A": np.zeros((3, 4))}, n_terms=3, pointwise=True)
    assert no_compiler["pointwise"] is True


def test_trace_callbacks_hands_the_level_through(no_compiler):
    pytest.importorskip("torch")
    from tempest_amd.trace import trace_callbacks
    from tests.test_trace_data import prior, quad_term
    t = np.linspace(-1.0, 1.0, 5)
    D = {"t": t, "y": 0.5 * t, "s": np.ones(5)}
    with pytest.raises(_Stop):
        trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", pointwise="psis")
    assert no_compiler["pointwise"] == "psis"
    no_compiler.clear()
    with pytest.raises(_Stop):
        trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", pointwise=True)
    assert no_compiler["pointwise"] is True
    with pytest.raises(ValueError, match="HipCallbacks: pointwise must be True or False, got 'loo'"):
        trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", pointwise="loo")


@pytest.mark.parametrize("level", ["PSIS", "loo", 1])
def test_other_levels_are_refused_with_the_message_of_before(level, no_compiler):
    with pytest.raises(ValueError) as e:
        H.HipCallbacks(pc.SOURCE, 2, data={"A": np.zeros((3, 4))}, n_terms=3, pointwise=level)
    assert str(e.value) == f"HipCallbacks: pointwise must be True or False, got {level!r}"


def test_psis_without_a_term_is_refused(no_compiler):
    whole = pc.SOURCE.replace("log_likelihood_term(const double* x, int64_t r,", "log_likelihood(const double* x,").replace("r * D.A_cols + ", "")
    with pytest.raises(ValueError, match="goes with a source that defines log_likelihood_term"):
        H.HipCallbacks(whole, 2, data={"A": np.zeros((3, 4))}, pointwise="psis")


def test_psis_loo_needs_the_level():
    cb = H.HipCallbacks.__new__(H.HipCallbacks)
    cb.pointwise_enabled = True
    with pytest.raises(TempestHipError, match='built without pointwise="psis"'):
        cb.psis_loo(np.zeros((4, 2)))


def test_scratch_words_against_the_formula():
    for n, T in ((1, 1), (20, 7), (21, 7), (1000, 50), (1025, 65), (131072, 1000), (1_864_200, 2), (4096, 10 ** 6)):
        n_blocks = -(-n // 1024)
        M = math.ceil(min(0.2 * n, 3 * math.sqrt(n)))
        M = 0 if M < 5 else min(M, 4096)
        per_r = 256 + 8 + 3 * n_blocks + M
        batch = min(T, max(1, (1 << 23) // per_r))
        assert H.psis_scratch_words(n, T) == 1 + n_blocks + per_r * batch, (n, T)
    assert H.psis_scratch_words(4096, 10 ** 6) < 1 + 4 + (1 << 23) + 4500          # the cap holds: batches


def test_compare_pointwise():
    import tempest_amd as tp
    assert tp.compare_pointwise is H.compare_pointwise and "compare_pointwise" in tp.__all__
    a = {"elpd_psis": np.array([-1.0, -2.0, -4.0, -0.5]), "elpd_loo": np.array([-1.0, -2.0, -4.0, -1.5])}
    b = {"elpd_psis": np.array([-1.5, -1.0, -3.0, -0.25]), "elpd_loo": np.array([-1.0, -2.0, -4.0, -0.5])}
    d = np.array([0.5, -1.0, -1.0, -0.25])
    got = tp.compare_pointwise(a, b, key="elpd_psis")
    assert got == {"diff": -1.75, "se": float(np.sqrt(4 * np.var(d))), "n": 4}
    assert tp.compare_pointwise(a, b)["diff"] == -1.0                            # the default key: elpd_loo
    assert tp.compare_pointwise(a["elpd_psis"], b["elpd_psis"])["diff"] == -1.75
    with pytest.raises(ValueError, match="same observations"):
        tp.compare_pointwise(a, {"elpd_psis": np.zeros(3)}, key="elpd_psis")


def test_totals_count_every_k_that_is_not_below_the_threshold():
    res = {"pareto_k": np.array([0.1, 0.71, np.inf, np.nan, 0.7]), "elpd_psis": np.array([-1.0, -2.0, -3.0, -4.0, -5.0])}
    tot = H.psis_totals({k: v[[0, 1, 2, 4]] for k, v in res.items()}, 0.7)
    assert tot == {"elpd_psis": -11.0, "elpd_psis_se": float(np.sqrt(4 * np.var([-1.0, -2.0, -3.0, -5.0]))), "n_high_k": 2}
    assert H.psis_totals(res, 0.7)["n_high_k"] == 3

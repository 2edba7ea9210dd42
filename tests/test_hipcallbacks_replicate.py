"""HipCallbacks replicated data (tempest_amd/hipcallbacks.py): `replicate(x, r, g)` and `discrepancy(x, r, y)` in the
user's source; bands of y_rep, the PIT per observation and a Bayesian p-value reduced on the device over the posterior rows
(cb.replicated, Sampler.replicated).

CPU: every validation error, the //@Y lines and the key word only with replicate() in the source, and sources without it generate
the text and the key the parent commit gave them (tests/golden/replicate_parent_plugins.json, recorded there).
GPU: a Bernoulli source whose draws oracle/philox.py restates to the bit -- the host builds the whole y_rep matrix and every output
from it in the device's orders: moments in PREDICT_SUM_LAYOUT, integer weights llrint(u 2^52) for quantiles, pit and p_value (equal);
a linear Gaussian source against the NumPy Box-Muller (1e-12; pit and p_value equal away from ties); every pinned launch shape
bitwise; seeds and row identity; a well-specified model's PIT against the normal CDF; a whole run.

Two sources serve every GPU test (BERN at n_dim 3 and 9, GAUSS at n_dim 2).  The p-value's tie condition: the issue asks that no
|T_rep_i - T_obs_i| be below 1e-9 before `p_value` is compared for equality.  With 0 / 1 data and few observations a row's replicate
EQUALS the observed vector with fair probability (half the rows at n_replicate = 1), and then T_rep_i == T_obs_i exactly: both are the
same additions of the same products, on the host and on the device alike (contraction is off), so `>=` is true on both.  check_gaps
therefore admits a gap of exactly 0 where the replicated row equals the observed one element for element, and holds every other gap
to 1e-9; the seed is searched for on the CPU until that is so, and no case is left out."""
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import philox  # noqa: E402
from tests.test_hipcallbacks_predict import BASE, PRED_D, PRED_X, WHOLE_D, layout_sum, need_gpu, needs_hipcc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = (64, 16)
TAG_NORMAL, TAG_UNIFORM = 10, 11
TWO52 = 4503599627370496.0

PRIOR_ID = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
  for (int j = 0; j < N_DIM; ++j) x[j] = u[j];
}
'''
# p = 0.25 + 0.5 x[0] t[r] with x[0], t in [0, 1]: + and * alone, one rounding each (contraction is off in the user's code)
BERN = PRIOR_ID + '''
__device__ double log_likelihood(const double* x, const tphu_data& D) { return 0.0; }
__device__ double replicate(const double* x, int64_t r, const tphu_noise& g, const tphu_data& D) {
  const double p = 0.25 + 0.5 * x[0] * D.t[r];
  return g.uniform(0) < p ? 1.0 : 0.0;
}
__device__ double discrepancy(const double* x, int64_t r, double y, const tphu_data& D) {
  const double p = 0.25 + 0.5 * x[0] * D.t[r];
  const double d = y - p;
  return d * d;
}
'''
GAUSS_PRIOR = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
  x[0] = 4.0 * u[0] - 1.0;
  x[1] = 4.0 * u[1] - 1.0;
}
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double z = (D.y[r] - (x[0] + x[1] * D.t[r])) / D.s[r];
  return -0.5 * z * z;
}
'''
GAUSS_REP = '''
__device__ double replicate(const double* x, int64_t r, const tphu_noise& g, const tphu_data& D) {
  return (x[0] + x[1] * D.t[r]) + D.s[r] * g.normal(0);
}
'''
GAUSS_DISC = '''
__device__ double discrepancy(const double* x, int64_t r, double y, const tphu_data& D) {
  const double z = (y - (x[0] + x[1] * D.t[r])) / D.s[r];
  return z * z;
}
'''
GAUSS = GAUSS_PRIOR + GAUSS_REP + GAUSS_DISC
# replicate without data, observed or discrepancy (CPU tests: text and compile only)
REP_X = '''
__device__ double replicate(const double* x, int64_t r, const tphu_noise& g) { return x[0] + 0.125 * (double)r * g.normal(1); }
'''

SIZES = (1, 63, 64, 65, 256, 257, 1023, 1024, 1025, 2500)
N_REPLICATE = (1, 2, 63, 64, 65, 130)
QS = (0.025, 0.5, 0.975)
PINS = ((1, 256), (7, 512), (64, 256), (64, 2560))
KEYS = ("mean", "var", "quantiles", "pit", "p_value", "t_obs_mean", "t_rep_mean")


# ------------------------------------------------------------------------------------------------- host restatement
def int_weights(w):
    """W in the layout order, u = w / W (0 where w == 0), k = llrint(u 2^52) as int64."""
    W = layout_sum(w[None, :], LAYOUT)[0]
    u = np.where(w > 0, w / W, 0.0)
    return u, np.rint(u * TWO52).astype(np.int64)


def inverted_cdf(y, k, qs):
    """(len(qs), R): per row of y (R, n) the first sorted value at which the running integer weight reaches the target -- ceil(q 2^52)
    held inside [1, total] -- over the values with k > 0 that are no NaN; NaN where a row with u > 0 is NaN (the caller fills that)."""
    R = y.shape[0]
    out = np.full((len(qs), R), np.nan)
    total = int(k.sum())
    for r in range(R):
        keep = (k > 0) & ~np.isnan(y[r])
        if not keep.any():
            continue
        order = np.argsort(y[r][keep], kind="stable")
        ys, cum = y[r][keep][order], np.cumsum(k[keep][order])
        tot = int(cum[-1])
        for j, q in enumerate(qs):
            T = min(max(int(math.ceil(q * TWO52)), 1), tot)
            out[j, r] = ys[np.searchsorted(cum, T, side="left")]
    assert total > 0
    return out


def t_sums(disc):
    """Rows of disc (R, n) added over r in the term-form order for R <= 256 (one chunk): r order from +0.0, then + 0.0 twice."""
    assert disc.shape[0] <= 256
    tot = np.zeros(disc.shape[1])
    for r in range(disc.shape[0]):
        tot = tot + disc[r]
    return (0.0 + tot) + 0.0


def host_outputs(y, w, qs, y_obs=None, t_obs=None, t_rep=None):
    """Every output of cb.replicated from the host's y_rep matrix y (R, n), in the device's orders."""
    u, k = int_weights(w)
    pos = u > 0
    with np.errstate(invalid="ignore"):
        mean = layout_sum(np.where(pos, u * y, 0.0), LAYOUT)
        d = y - mean[:, None]
        var = layout_sum(np.where(pos, u * (d * d), 0.0), LAYOUT)
    out = {"mean": mean, "var": var, "quantiles": inverted_cdf(y, k, qs)}
    total = float(k.sum())
    if y_obs is not None:
        below = np.where(y < y_obs[:, None], k, 0).sum(axis=1).astype(np.float64)
        equal = np.where(y == y_obs[:, None], k, 0).sum(axis=1).astype(np.float64)
        out["pit"] = (below + 0.5 * equal) / total
    if t_obs is not None:
        with np.errstate(invalid="ignore"):
            out["p_value"] = float(np.where(t_rep >= t_obs, k, 0).sum()) / total
            out["t_obs_mean"] = layout_sum(np.where(pos, u * t_obs, 0.0)[None, :], LAYOUT)[0]
            out["t_rep_mean"] = layout_sum(np.where(pos, u * t_rep, 0.0)[None, :], LAYOUT)[0]
    return out


def check_gaps(y, y_obs, t_obs, t_rep, k):
    """True where the p-value cannot depend on a rounding: over the rows with k > 0 every |T_rep - T_obs| is at least 1e-9, or exactly 0
    with the replicated row equal to the observed one (module docstring)."""
    live = k > 0
    gap = np.abs(t_rep - t_obs)[live]
    same = np.all(y == y_obs[:, None], axis=0)[live]
    return bool(np.all((gap >= 1e-9) | ((gap == 0.0) & same)))


def bern_rows(n, d, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    w = rng.uniform(0.1, 3.0, n)
    w[1::3] = 0.0                                     # a third of the rows without weight (row 0 keeps its own: n = 1)
    return x, w


def bern_data(R, seed):
    rng = np.random.RandomState(1000 + seed)
    t = rng.uniform(0.0, 1.0, R)
    return {"t": t, "y": (rng.rand(R) < 0.25 + 0.25 * t).astype(np.float64)}          # (0 / 1 observations of a typical row: x[0] = 0.5)


def bern_matrix(x, D, seed):
    """y_rep (R, n), T_obs, T_rep (n) of BERN, operation by operation; NaN rows give y = 0 (the comparison is false) and NaN sums."""
    n, R = len(x), len(D["t"])
    U = philox.uniform_pair(seed, np.arange(n)[None, :], 0, np.arange(R)[:, None], TAG_UNIFORM)[0]
    with np.errstate(invalid="ignore"):
        p = 0.25 + 0.5 * x[None, :, 0] * D["t"][:, None]
        y = np.where(U < p, 1.0, 0.0)
        do, dr = D["y"][:, None] - p, y - p
        return y, t_sums(do * do), t_sums(dr * dr)


@functools.lru_cache(maxsize=None)
def bern_case(n, R, d):
    """Rows, weights, data, the seed (the first from 1 whose T gaps are clear, found on the CPU) and the host's outputs: computed once,
    shared, read-only."""
    x, w = bern_rows(n, d, seed=n + 13 * d)
    D = bern_data(R, seed=R)
    _, k = int_weights(w)
    for seed in range(1, 200):
        y, t_obs, t_rep = bern_matrix(x, D, seed)
        if check_gaps(y, D["y"], t_obs, t_rep, k):
            break
    else:
        raise AssertionError(f"no seed below 200 clears the T gaps at n={n}, R={R}")
    ref = host_outputs(y, w, QS, D["y"], t_obs, t_rep)
    for a in ref.values():                        # (x, w and the data stay writable only because torch.from_numpy warns otherwise)
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x, w, D, seed, ref


def gauss_rows(n, seed, equal=False):
    rng = np.random.RandomState(seed)
    x = np.stack([rng.uniform(1.0, 2.0, n), rng.uniform(0.5, 1.0, n)], axis=1)
    w = np.ones(n) if equal else rng.uniform(0.1, 3.0, n)
    if not equal:
        w[rng.rand(n) < 0.05] = 0.0
    return x, w


def gauss_data(R, seed, truth=(1.5, 0.75)):
    rng = np.random.RandomState(2000 + seed)
    t = np.linspace(0.0, 1.0, R) if R > 1 else np.array([0.5])
    s = 0.1 + 0.2 * rng.rand(R)
    return {"t": t, "s": s, "y": truth[0] + truth[1] * t + s * rng.randn(R)}


def gauss_matrix(x, D, seed):
    n, R = len(x), len(D["t"])
    z = philox.normal_pair(seed, np.arange(n)[None, :], 0, np.arange(R)[:, None], TAG_NORMAL)[0]
    m = x[None, :, 0] + x[None, :, 1] * D["t"][:, None]
    y = m + D["s"][:, None] * z
    zo, zr = (D["y"][:, None] - m) / D["s"][:, None], (y - m) / D["s"][:, None]
    return y, m, t_sums(zo * zo), t_sums(zr * zr)


def make(tp, src, n_dim, D, **kw):
    return tp.HipCallbacks(src, n_dim, data=D, n_replicate="t", observed="y", **kw)


def same_bits(a, b, keys=KEYS, msg=""):
    for key in keys:
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=f"{key} {msg}")


# ------------------------------------------------------------------------------------------------- CPU
T5 = {"t": np.linspace(0.0, 1.0, 5), "y": np.zeros(5), "y4": np.zeros(4), "m": np.zeros((5, 2))}


@pytest.mark.parametrize("source,kw,match", [
    (BERN, {"data": T5}, "give n_replicate="),
    (WHOLE_D, {"data": T5, "n_replicate": 5}, "n_replicate= goes with a source that defines"),
    (WHOLE_D + "// we replicate the data (see eq. 4)\n", {"data": T5, "n_replicate": 5}, "n_replicate= goes with a source that defines"),
    (BERN, {"data": T5, "n_replicate": True, "observed": "y"}, "positive int"),
    (BERN, {"data": T5, "n_replicate": 0, "observed": "y"}, "positive int"),
    (BERN, {"data": T5, "n_replicate": 2.0, "observed": "y"}, "positive int"),
    (BERN, {"data": T5, "n_replicate": "nope", "observed": "y"}, "names no data entry"),
    (BERN, {"data": T5, "n_replicate": "t", "observed": "nope"}, "observed='nope' names no data entry"),
    (BERN, {"data": T5, "n_replicate": "t", "observed": 3}, "names no data entry"),
    (BERN, {"data": T5, "n_replicate": "t", "observed": "y4"}, "1-D data entry of length n_replicate = 5"),
    (BERN, {"data": T5, "n_replicate": "t", "observed": "m"}, "1-D data entry of length n_replicate = 5"),
    (BERN, {"data": T5, "n_replicate": "t"}, "discrepancy.*give observed="),
    (WHOLE_D, {"data": T5, "observed": "y"}, "observed= goes with a source that defines replicate"),
    (WHOLE_D + GAUSS_DISC, {"data": T5}, "discrepancy.*goes with a source that defines replicate"),
])
def test_replicate_validation_raises_before_the_compiler_runs(source, kw, match, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    with pytest.raises(ValueError, match=match):
        tp.HipCallbacks(source, 3, **kw)


def test_the_words_in_a_comment_are_no_definitions():
    from tempest_amd import hipcallbacks as H
    assert not H._defines(BASE + "// we replicate( the data\n", "replicate") and not H._defines(BASE + "// double replicated(\n", "replicate")
    assert H._defines(BERN, "replicate") and H._defines(BERN, "discrepancy") and H._defines(REP_X, "replicate")
    assert not H._defines(GAUSS_PRIOR + GAUSS_REP, "discrepancy")


def test_plugin_text_and_key_carry_replicate_only_with_it():
    from tempest_amd.hipcallbacks import plugin_key, plugin_source
    tabs = (("t", 1), ("y", 1))
    with_y = plugin_source(BERN, tabs, replicate=True)
    for word in ("struct tphu_noise", "TPHU_TAG_REP_NORMAL = 10", "TPHU_TAG_REP_UNIFORM = 11", "k_user_rep_moment", "k_user_rep_hist",
                 "k_user_rep_disc", "tphu_replicated(", "tphu_replicate_layout(", "k_user_predict_wsum(", "k_user_predict_narrow(",
                 "#define TPHU_CHUNK 256"):
        assert word in with_y, word
    assert "//@" not in with_y and "@" not in with_y.replace(BERN, "")
    assert "tphu_predictive(" not in with_y and "void k_user_predict_moment" not in with_y and "k_user_pw" not in with_y
    # shared lines appear once where predict, pointwise and the term form are there too
    gt = (("t", 1), ("s", 1), ("y", 1))
    full = plugin_source(GAUSS + PRED_D, gt, True, predict=True, pointwise=True, replicate=True)
    for word in ("k_user_predict_wsum(", "k_user_predict_narrow(", "k_user_predict_fold(", "#define TPHU_PCHUNK", "#define TPHU_PRED_TAB"):
        assert full.count(word if word.startswith("#") else "void __launch_bounds__(256) " + word) == 1, word
    assert "tphu_predictive(" in full and "tphu_replicated(" in full and "@" not in full.replace(GAUSS + PRED_D, "")
    without = plugin_source(WHOLE_D + PRED_D, (("t", 1),), predict=True)
    for word in ("tphu_noise", "replicate", "k_user_rep", "TPHU_TAG_REP", "//@Y", "//@S"):
        assert word not in without, word
    assert "replicate" not in plugin_source(BASE) and "//@" not in plugin_source(BASE)
    assert plugin_source(BASE + REP_X, replicate=True).count("replicate(xx, r, g)") == 2          # no data: no trailing D
    plain = plugin_key(3)
    assert "replicate" not in plain and "discrepancy" not in plain
    assert plugin_key(3, replicate=True) == plain + "|replicate"
    assert plugin_key(3, replicate=True, discrepancy=True) == plain + "|replicate|discrepancy"
    assert plugin_key(3, predict=True, pointwise=True, replicate=True).endswith("|predict|pointwise|replicate")
    assert plugin_key(3, discrepancy=True) == plain                       # (never without replicate: the constructor refuses it)


def test_sources_without_replicate_generate_the_parent_text_and_key():
    """Plain, data + predict and term + pointwise sources: the SHA-256 of plugin_source and the key, recorded on the parent commit."""
    from tempest_amd import hipcallbacks as H
    from tests import test_hipcallbacks_data as T
    from tests import test_hipcallbacks_pointwise as W
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "replicate_parent_plugins.json")))["cases"]
    sources = {"plain": T.OLD_SRC, "data_predict": WHOLE_D + PRED_D, "term_pointwise": W.TERM_X}
    assert set(rec) == set(sources)
    for name, src in sources.items():
        c = rec[name]
        assert hashlib.sha256(src.encode()).hexdigest() == c["source_sha256"], name
        tables = None if c["tables"] is None else tuple(tuple(t) for t in c["tables"])
        text = H.plugin_source(src, tables, c["term"], predict=c["predict"], pointwise=c["pointwise"])
        assert hashlib.sha256(text.encode()).hexdigest() == c["text_sha256"], name
        assert text == H.plugin_source(src, tables, c["term"], predict=c["predict"], pointwise=c["pointwise"], replicate=False)
        key = H.plugin_key(c["n_dim"], predict=c["predict"], pointwise=c["pointwise"])
        assert key == c["key"].replace("{toolchain}", H._toolchain_id()), name
        assert key == H.plugin_key(c["n_dim"], predict=c["predict"], pointwise=c["pointwise"], replicate=False, discrepancy=False)


@needs_hipcc
def test_replicate_plugins_build_in_every_form_and_export_the_entry_point():
    import ctypes
    from tempest_amd.hipcallbacks import build_plugin
    built = (build_plugin(BERN, 3, tables=(("t", 1), ("y", 1)), replicate=True, discrepancy=True),
             build_plugin(GAUSS_PRIOR + GAUSS_REP, 2, tables=(("t", 1), ("s", 1), ("y", 1)), term=True, replicate=True),
             build_plugin(BASE + REP_X + PRED_X, 3, predict=True, replicate=True))
    assert len(set(built)) == 3
    for path in built:
        lib = ctypes.CDLL(str(path))
        for sym in ("tphu_replicated", "tphu_replicate_layout", "tphu_prior", "tphu_like", "tphu_accept", "tphu_step", "tphu_run"):
            assert hasattr(lib, sym), sym
        assert tuple(lib.tphu_replicate_layout(i) for i in range(9)) == (64, 16, 64, 24, 256, 64, 10, 11, -1) and lib.tphu_abi() == 3
    assert hasattr(ctypes.CDLL(str(built[2])), "tphu_predictive") and not hasattr(ctypes.CDLL(str(built[0])), "tphu_predictive")
    plain = ctypes.CDLL(str(build_plugin(BASE, 3)))
    assert not hasattr(plain, "tphu_replicated") and not hasattr(plain, "tphu_replicate_layout")


@needs_hipcc
def test_replicated_without_replicate_in_the_source_raises():
    import tempest_amd as tp
    from tempest_amd._lib import TempestHipError
    cb = tp.HipCallbacks(BASE, 3)
    assert cb.n_replicate == 0 and cb.observed is None
    with pytest.raises(TempestHipError, match="no replicate"):
        cb.replicated(np.zeros((4, 3)), np.ones(4))


def test_scratch_words_cover_the_layout():
    from tempest_amd.hipcallbacks import PREDICT_SCRATCH_WORDS, replicate_scratch_words
    for n in (1, 63, 1000, 3001, 1 << 20):
        for R in (1, 7, 1000, 100_000):
            for nq in (0, 3, 8):
                nb, nc = -(-n // 1024), -(-n // 64)
                fixed, per_r = 3 + 3 * nb + 3 * R + 2 * nc, nb + 258 * nq + 1
                words = replicate_scratch_words(n, R, nq)
                assert fixed + per_r <= words <= fixed + max(per_r, PREDICT_SCRATCH_WORDS)


def test_the_host_restatement_of_the_inverted_cdf():
    """inverted_cdf against np.percentile(method="inverted_cdf") for equal weights away from knife edges."""
    rng = np.random.RandomState(3)
    for n, qs in ((63, (0.025, 0.5, 0.975)), (1001, (0.3, 0.5))):
        y = rng.randn(4, n)
        k = np.full(n, int(round(TWO52 / n)), dtype=np.int64)
        want = np.percentile(y, [100 * q for q in qs], axis=1, method="inverted_cdf")
        np.testing.assert_array_equal(inverted_cdf(y, k, qs), want)


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n_dim", [3, 9])
@pytest.mark.parametrize("n", SIZES)
def test_bernoulli_every_output_against_the_host_matrix(n, n_dim):
    """n_dim 3: the rows are staged through LDS; n_dim 9: every lane reads its row from memory.  mean and var within the bound
    test_hipcallbacks_predict.py holds predictive()'s moments to (they are equal to the restatement), everything else equal."""
    import tempest_amd as tp
    need_gpu()
    for R in N_REPLICATE:
        x, w, D, seed, ref = bern_case(n, R, n_dim)
        cb = make(tp, BERN, n_dim, D)
        assert cb.n_replicate == R and cb.observed == "y" and cb.has_discrepancy
        got = cb.replicated(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), quantiles=QS, seed=seed)
        assert got["mean"].shape == got["var"].shape == got["pit"].shape == (R,) and got["quantiles"].shape == (len(QS), R)
        assert got["n_rows"] == n and got["seed"] == seed and abs(got["ess"] - w.sum() ** 2 / (w * w).sum()) <= 1e-9 * got["ess"]
        print(f"n={n} R={R} d={n_dim} seed={seed}: mean differs at {int(np.sum(got['mean'] != ref['mean']))}, var at "
              f"{int(np.sum(got['var'] != ref['var']))} indices; p_value {got['p_value']} / {ref['p_value']}")
        np.testing.assert_array_equal(got["mean"], ref["mean"])
        np.testing.assert_array_equal(got["var"], ref["var"])
        np.testing.assert_array_equal(got["quantiles"], ref["quantiles"])
        np.testing.assert_array_equal(got["pit"], ref["pit"])
        assert got["p_value"] == ref["p_value"]
        assert got["t_obs_mean"] == ref["t_obs_mean"] and got["t_rep_mean"] == ref["t_rep_mean"]


@pytest.mark.gpu
@needs_hipcc
def test_rows_without_weight_may_hold_nan():
    import tempest_amd as tp
    need_gpu()
    n, R = 257, 65
    x, w, D, seed, ref = bern_case(n, R, 3)
    y = x.copy()
    y[w == 0] = np.nan
    assert np.sum(w == 0) > 80
    cb = make(tp, BERN, 3, D)
    same_bits(cb.replicated(y, w, quantiles=QS, seed=seed), ref, msg="rows without weight set to NaN")
    # a NaN replicate WITH weight: NaN at every index for mean, var, quantiles and pit
    G = {"t": D["t"], "s": np.ones(R), "y": D["y"]}
    bad = make(tp, GAUSS, 2, dict(G, t=np.where(np.arange(R) == 2, np.nan, D["t"])), n_terms="t").replicated(x[:, :2], w, quantiles=QS, seed=seed)
    ok = make(tp, GAUSS, 2, G, n_terms="t").replicated(x[:, :2], w, quantiles=QS, seed=seed)
    keep = np.arange(R) != 2
    for key in ("mean", "var", "pit"):
        assert np.isnan(bad[key][2]) and np.all(np.isfinite(ok[key]))
        np.testing.assert_array_equal(bad[key][keep], ok[key][keep])
    assert np.all(np.isnan(bad["quantiles"][:, 2]))
    np.testing.assert_array_equal(bad["quantiles"][:, keep], ok["quantiles"][:, keep])


@functools.lru_cache(maxsize=None)
def gauss_case(n, R):
    x, w = gauss_rows(n, seed=n)
    D = gauss_data(R, seed=R)
    _, k = int_weights(w)
    for seed in range(1, 50):
        y, m, t_obs, t_rep = gauss_matrix(x, D, seed)
        if np.all(np.abs(y - D["y"][:, None]) > 1e-9 * np.abs(D["y"][:, None])) and np.all(np.abs(t_rep - t_obs)[k > 0] >= 1e-9):
            break
    else:
        raise AssertionError("no seed below 50 clears the ties")
    return x, w, D, seed, y, host_outputs(y, w, QS, D["y"], t_obs, t_rep)


@pytest.mark.gpu
@needs_hipcc
def test_linear_gaussian_against_the_numpy_box_muller():
    import tempest_amd as tp
    need_gpu()
    n, R = 700, 37
    x, w, D, seed, y, ref = gauss_case(n, R)
    cb = make(tp, GAUSS, 2, D, n_terms="t")
    got = cb.replicated(x, w, quantiles=QS, seed=seed)
    for key in ("mean", "var", "quantiles", "t_obs_mean", "t_rep_mean"):
        err = np.max(np.abs(np.asarray(got[key]) - ref[key]) / np.abs(ref[key]))
        print(f"{key}: largest relative difference {err:.3e}")
    np.testing.assert_allclose(got["mean"], ref["mean"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["var"], ref["var"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["quantiles"], ref["quantiles"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got["pit"], ref["pit"])
    assert got["p_value"] == ref["p_value"]
    np.testing.assert_allclose([got["t_obs_mean"], got["t_rep_mean"]], [ref["t_obs_mean"], ref["t_rep_mean"]], rtol=1e-12, atol=0)
    # update_data on the observed entry: the same device buffer, new values
    y2 = D["y"] + 0.05
    cb.update_data("y", y2)
    _, _, t_obs2, t_rep2 = gauss_matrix(x, dict(D, y=y2), seed)
    ref2 = host_outputs(y, w, QS, y2, t_obs2, t_rep2)
    got2 = cb.replicated(x, w, quantiles=QS, seed=seed)
    np.testing.assert_array_equal(got2["quantiles"], got["quantiles"])
    np.testing.assert_array_equal(got2["pit"], ref2["pit"])
    assert np.any(got2["pit"] != got["pit"])


@pytest.mark.gpu
@needs_hipcc
def test_no_launch_shape_changes_a_bit_and_seeds_and_row_identity():
    """cb.replicated(x[perm], w[perm]) is NOT the unpermuted result: the draws belong to the row's index (stated in its docstring)."""
    import tempest_amd as tp
    need_gpu()
    n, R = 2500, 130
    x, w = gauss_rows(n, seed=5)
    D = gauss_data(R, seed=5)
    cb = make(tp, GAUSS, 2, D, n_terms="t")
    xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    base = cb.replicated(xt, wt, quantiles=QS, seed=3)
    for pin in PINS:
        cb.predict_tile = pin
        same_bits(cb.replicated(xt, wt, quantiles=QS, seed=3), base, msg=f"at pin {pin}")
    cb.predict_tile = 0
    same_bits(cb.replicated(xt, wt, quantiles=QS, seed=3), base, msg="same seed again")
    q1 = cb.replicated(xt, wt, quantiles=(0.5,), seed=3)
    q8 = cb.replicated(xt, wt, quantiles=(0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0), seed=3)
    np.testing.assert_array_equal(q1["quantiles"][0], base["quantiles"][1])
    np.testing.assert_array_equal(q8["quantiles"][3], base["quantiles"][1])
    same_bits(q8, base, keys=("mean", "var", "pit", "p_value"))
    other = cb.replicated(xt, wt, quantiles=QS, seed=4)
    assert other["seed"] == 4 and np.any(other["quantiles"] != base["quantiles"]) and np.any(other["mean"] != base["mean"])
    perm = np.random.RandomState(0).permutation(n)
    moved = cb.replicated(x[perm], w[perm], quantiles=QS, seed=3)
    assert np.any(moved["quantiles"] != base["quantiles"]) and np.any(moved["mean"] != base["mean"])
    np.testing.assert_allclose(moved["mean"], base["mean"], atol=0.05)          # (another set of draws of the same law)
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            cb.replicated(xt, wt, seed=bad)
    assert cb.replicated(xt, wt, quantiles=(), seed=2 ** 64 - 1)["quantiles"].shape == (0, R)
    kept = cb._yscratch.data_ptr()
    cb.replicated(xt[:100], wt[:100])
    assert cb._yscratch.data_ptr() == kept


@pytest.mark.gpu
@needs_hipcc
def test_well_specified_model_pit_against_the_normal_cdf():
    """65 536 equal-weight rows around the generating parameters: pit[r] is within 0.01 of sum u Phi((y_r - m_ir) / s_r) -- 5 sigma of
    the Monte Carlo error sqrt(1 / (4 n)) ~ 0.002 -- and the chi-square discrepancy's p-value lies in (0.01, 0.99)."""
    import tempest_amd as tp
    need_gpu()
    n, R = 65536, 16
    rng = np.random.RandomState(11)
    D = gauss_data(R, seed=16)
    x = np.array([1.5, 0.75]) + 0.05 * rng.randn(n, 2)
    cb = make(tp, GAUSS, 2, D, n_terms="t")
    got = cb.replicated(x, np.ones(n), seed=9)
    m = x[None, :, 0] + x[None, :, 1] * D["t"][:, None]
    z = (D["y"][:, None] - m) / D["s"][:, None]
    want = np.mean(0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0))), axis=1)
    print("pit", got["pit"], "expected", want, "p_value", got["p_value"], got["t_obs_mean"], got["t_rep_mean"])
    assert np.all(np.abs(got["pit"] - want) < 0.01)
    assert 0.01 < got["p_value"] < 0.99
    assert abs(got["t_rep_mean"] - R) < 0.2                   # (E T_rep = n_replicate exactly; its Monte Carlo error is sqrt(2 R / n) ~ 0.02)


@pytest.mark.gpu
@needs_hipcc
def test_through_the_sampler(tmp_path):
    import tempest_amd as tp
    from tempest_amd._lib import TempestHipError
    need_gpu()
    D = gauss_data(40, seed=40)
    cb = make(tp, GAUSS, 2, D, n_terms="t")

    def sampler(c):
        return tp.Sampler(c.prior_transform, c.log_likelihood, 2, n_particles=2048, vectorize=True, clustering=False, random_state=11)
    s = sampler(cb)
    s.run(n_total=4096, progress=False)
    for case in (dict(), dict(trim_importance_weights=False)):
        x, w, _ = s.posterior(**case)
        got = s.replicated(seed=5, **case)
        direct = cb.replicated(x, w, seed=5)
        assert got["n_rows"] == len(x) and got["ess"] == direct["ess"] and got["seed"] == 5
        same_bits(got, direct)
    x, w, _ = s.posterior()
    own = s.replicated()
    assert own["seed"] == 11
    same_bits(own, cb.replicated(x, w, seed=11))
    print("pit", got["pit"], "p_value", got["p_value"])
    assert np.all((got["pit"] > 0.0) & (got["pit"] < 1.0)) and 0.0 < got["p_value"] < 1.0
    assert np.all(got["quantiles"][0] <= got["quantiles"][1]) and np.all(got["quantiles"][1] <= got["quantiles"][2])
    want = s.replicated(seed=5)
    for name in ("run.state", "run.ckpt"):
        s.save_state(tmp_path / name)
        t = sampler(cb)
        t.load_state(tmp_path / name)
        again = t.replicated(seed=5)
        x, w, _ = t.posterior()
        same_bits(again, cb.replicated(x, w, seed=5))
        # (the weights are recomputed over the reloaded history and may differ in their last bits)
        for key in ("mean", "var", "pit"):
            np.testing.assert_allclose(again[key], want[key], rtol=1e-9, atol=1e-12)
    plain = tp.HipCallbacks(GAUSS_PRIOR, 2, data=D, n_terms="t")
    with pytest.raises(TempestHipError, match="replicate"):
        sampler(plain).replicated()

"""HipCallbacks pointwise log predictive densities (tempest_amd/hipcallbacks.py): with `pointwise=True` a term-form
source gets cb.pointwise(x, w) / Sampler.pointwise(): lppd, mean, p_waic, elpd_waic, elpd_loo and ess_loo per observation, reduced on
the device over the posterior rows.

CPU: sources without the option generate the text and the file name they had (the parent's recorded hashes, three predict-form
sources among them), plugins with it compile for gfx950 in every form and export tphu_pointwise, every validation error, the tile
rule; and the float64 restatement of the summation order is held against long double sums under the bounds the device is held to.
GPU: mean and p_waic against the NumPy restatement of PREDICT_SUM_LAYOUT to the bit, lppd / elpd_loo / ess_loo against long double
within (n_blocks + 40) 2^-52 (absolute; ess_loo relative at four times that): 6 tree levels + 16 chunk additions + n_blocks block
additions + the roundings of u, the product, a <= 2 ulp exp and the log; every output bit for bit at every tile and batch; every way
the rows are loaded; special values; guard cells; streams; a closed form; a whole run; two ranks.

The term sources keep |a| below 2.5, so that an absolute bound in units of 2^-52 means what it says."""
import ctypes
import functools
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_hipcallbacks_predict import (BASE, DERIVED, PARENT_ENV, PRED_D, PRED_X, PRIOR_D, QUAD, QUAD_PRED, TERM_D, _free_port,  # noqa: E402
                                             layout_sum, need_gpu, needs_hipcc, parent_cases, quad_data, rows_and_weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("lppd", "mean", "p_waic", "elpd_waic", "elpd_loo", "ess_loo")
LAYOUT = (64, 16)

# one rounding per operation, split so that nothing could fuse; every index with r % 5 == 3 ignores x: all rows tied.  The term
# reads the first and the LAST coordinate; t <= 1.75, x[0] in [1, 2], x[-1] in [0.5, 1]: -2 <= a <= 0
TERM_X = PRIOR_D + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double t = 0.0625 * (double)(r % 29);
  if (r % 5 == 3) return -t;
  const double a = x[N_DIM - 1] * t;
  const double z = x[0] - a;
  const double q = z * z;
  return -0.5 * q;
}
'''
# rows marked by x[1] == 9 / 8 return what the tables say at that index (and every row where every[r] == 1)
TERM_SPECIAL = PRIOR_D + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  if (D.every[r] == 1.0) return D.sp[r];
  if (x[1] == 9.0) return D.sp[r];
  if (x[1] == 8.0) return D.sq[r];
  const double z = x[0] - D.c[r];
  const double q = z * z;
  return -0.5 * q;
}
'''
TERM_Y = PRIOR_D + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double z = D.y[r] - x[0];
  const double q = z * z;
  return -0.5 * q;
}
'''
WHOLE_PLAIN = BASE
DERIVED_D = '''
__device__ void derived(const double* x, double* out, const tphu_data& D) { out[0] = x[0] + x[1]; }
'''

SIZES = (1, 63, 64, 65, 700, 3001)
N_TERMS = (1, 7, 256, 1000)
BIG = (1 << 20) + 3
PINS = (1, 4, 16, 64)


def term_x(x, r0, r1):
    """TERM_X at indices r0 .. r1 - 1, operation by operation: (r1 - r0, n)."""
    r = np.arange(r0, r1)
    t = 0.0625 * (r % 29).astype(np.float64)
    a = x[None, :, -1] * t[:, None]
    z = x[None, :, 0] - a
    p = -0.5 * (z * z)
    tied = r % 5 == 3
    p[tied] = -t[tied, None]
    return p


def tolerance(n):
    return (-(-n // (LAYOUT[0] * LAYOUT[1])) + 40) * 2.0 ** -52


def mirror(a, w, layout=LAYOUT):
    """The six outputs as the kernels define them, in float64 and their summation order: a (R, n) terms, w (n) weights."""
    W = layout_sum(w[None, :], layout)[0]
    u = np.where(w > 0, w / W, 0.0)
    up = (u > 0)[None, :]
    lsum = lambda v: layout_sum(np.where(up, v, 0.0), layout)      # noqa: E731
    inf = np.inf
    with np.errstate(all="ignore"):
        isn = np.any(up & np.isnan(a), axis=1)
        M = np.max(np.where(up & ~np.isnan(a), a, -inf), axis=1) + 0.0
        m = np.min(np.where(up & ~np.isnan(a), a, inf), axis=1) + 0.0
        mean = lsum(u * a)
        d = a - mean[:, None]
        pw = lsum(u * (d * d))
        s1 = lsum(u * np.exp(a - M[:, None]))
        v = u * np.exp(m[:, None] - a)
        s2, s3 = lsum(v), lsum(v * v)
        minf, linf = np.isinf(M), np.isinf(m)
        lppd = np.where(minf, M, M + np.log(s1))
        pw = np.where(minf | linf, np.nan, pw)
        loo = np.where(linf, m, m - np.log(s2))
        ess = np.where(linf, np.nan, s2 * s2 / s3)
        out = {"lppd": lppd, "mean": mean, "p_waic": pw, "elpd_waic": lppd - pw, "elpd_loo": loo, "ess_loo": ess}
    for k in KEYS:
        out[k] = np.where(isn, np.nan, out[k])
    return out


def long_double(a, w):
    """lppd, elpd_loo, ess_loo by their definitions, summed in long double over the rows with weight (a finite there)."""
    L = np.longdouble
    keep = w > 0
    al, wl = a[:, keep].astype(L), w[keep].astype(L)
    u = wl / wl.sum()
    v = u * np.exp(-al)
    return {"lppd": np.log((u * np.exp(al)).sum(axis=1)), "elpd_loo": -np.log(v.sum(axis=1)),
            "ess_loo": v.sum(axis=1) ** 2 / (v * v).sum(axis=1)}


def within_bounds(got, ld, n):
    tol = tolerance(n)
    for k in ("lppd", "elpd_loo"):
        err = np.max(np.abs(got[k].astype(np.longdouble) - ld[k]))
        assert err <= tol, (k, n, float(err), tol)
    rel = np.max(np.abs(got["ess_loo"].astype(np.longdouble) - ld["ess_loo"]) / ld["ess_loo"])
    assert rel <= 4 * tol, ("ess_loo", n, float(rel), 4 * tol)


@functools.lru_cache(maxsize=None)
def case(n, n_terms, d=3):
    """Rows, weights, the bitwise-mirrored terms, the float64 mirror and the long double reference: computed once, shared, read-only."""
    x, w = rows_and_weights(n, seed=n + 7 * d, d=d)
    a = term_x(x, 0, n_terms)
    ref, ld = mirror(a, w), long_double(a, w)
    for arr in (a, *ref.values(), *ld.values()):       # (x and w stay writable only because torch.from_numpy warns otherwise)
        arr.setflags(write=False)
    return x, w, a, ref, ld


def all_cases():
    return [(n, R) for n in SIZES for R in N_TERMS] + [(BIG, 7)]


# ------------------------------------------------------------------------------------------------- CPU
# Three predict-form sources: SHA-256 of the text -- recorded again when the moment and select kernels became wrappers of one shared
# body each, which moved every text with predict() in it and none without -- and the file name build_plugin gave the parent of this
# feature (6ed21b6) under the recorded environment (PARENT_ENV), hashed from the text of that time
def parent_predict_cases():
    return (   # source, n_dim, tables, term, n_derived, text hash, file name
        (BASE + PRED_X, 3, None, False, 0, "eac1200fb0927cbe343b57a12f63e7adb4ee88f4850b708436d46937e6c6640b", "tphu_3d_343e121977ab325cfa63.so"),
        (TERM_D + PRED_D, 3, (("t", 1),), True, 0, "acbad4f4d592ba6c67c06021f7c73124a1830cfb3623b94bdfa928359a4bc8ec",
         "tphu_3d_ed63f11797bfe745fab2.so"),
        (BASE + DERIVED + PRED_X, 4, None, False, 1, "0cd3236e6c8e5d05fd83f30812f7de48660ed9e6d76c0068e3a7c982dce70417",
         "tphu_4d_2a0630f7e195a2552641.so"),
    )


def every_parent_case():
    return [c + (False,) for c in parent_cases()] + [c + (True,) for c in parent_predict_cases()]


def test_sources_without_pointwise_generate_the_parent_text():
    from tempest_amd.hipcallbacks import plugin_source
    for src, _, tables, term, nder, sha, _, pred in every_parent_case():
        text = plugin_source(src, tables, term, derived=nder > 0, predict=pred)
        assert hashlib.sha256(text.encode()).hexdigest() == sha
        assert text == plugin_source(src, tables, term, derived=nder > 0, predict=pred, pointwise=False)
        assert "pointwise" not in text and "k_user_pw" not in text and "//@W" not in text and "//@Q" not in text
    for src, kw in ((TERM_X, {}), (TERM_D + PRED_D, {"predict": True}), (TERM_D + DERIVED_D, {"derived": True})):
        tables = (("t", 1),) if "D.t" in src else None
        with_w = plugin_source(src, tables, True, pointwise=True, **kw)
        for word in ("k_user_pw_range", "k_user_pw_shift", "k_user_pw_sums", "k_user_pw_final", "tphu_pointwise(", "k_user_predict_wsum"):
            assert word in with_w, word
        assert "@" not in with_w.replace(src, "")
        assert with_w.count("k_user_predict_wsum(") == 1 and with_w.count("#define TPHU_PCHUNK") == 1
        assert ("tphu_predictive(" in with_w) == bool(kw.get("predict"))


@needs_hipcc
def test_sources_without_pointwise_keep_their_file_name():
    from tempest_amd import hipcallbacks as H
    deps = (H._CSRC / "common.h").read_bytes() + open(H.HEADER_PATH, "rb").read()
    recorded_env = hashlib.sha256(deps + H._toolchain_id().encode()).hexdigest() == PARENT_ENV
    flags = "-O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -ffp-contract=on -Wno-unused-function"
    for src, n_dim, tables, term, nder, sha, name, pred in every_parent_case():
        got = H.build_plugin(src, n_dim, tables=tables, term=term, n_derived=nder, predict=pred).name
        text = H.plugin_source(src, tables, term, derived=nder > 0, predict=pred)
        key = f"|{n_dim}|gfx950|{flags}|{H._toolchain_id()}" + (f"|derived={nder}" if nder else "") + ("|predict" if pred else "")
        assert got == f"tphu_{n_dim}d_{hashlib.sha256(text.encode() + deps + key.encode()).hexdigest()[:20]}.so"
        if recorded_env:
            assert got == name
    assert H.build_plugin(TERM_X, 3, term=True, pointwise=True) != H.build_plugin(TERM_X, 3, term=True)


@needs_hipcc
def test_pointwise_plugins_build_in_every_form_and_export_the_entry_point():
    from tempest_amd.hipcallbacks import POINTWISE_MAX_TILE, PREDICT_SUM_LAYOUT, build_plugin
    tabs = (("t", 1),)
    built = (build_plugin(TERM_X, 3, term=True, pointwise=True),                                       # term only
             build_plugin(TERM_D, 3, tables=tabs, term=True, pointwise=True),                          # with data tables
             build_plugin(TERM_D + DERIVED_D, 3, tables=tabs, term=True, n_derived=1, pointwise=True),   # with derived
             build_plugin(TERM_D + PRED_D, 3, tables=tabs, term=True, predict=True, pointwise=True),   # with predict
             build_plugin(TERM_X, 40, term=True, pointwise=True))                                      # too wide for the LDS staging
    for path in built:
        lib = ctypes.CDLL(str(path))
        for sym in ("tphu_pointwise", "tphu_pointwise_layout", "tphu_prior", "tphu_like", "tphu_like_split", "tphu_accept", "tphu_step", "tphu_run"):
            assert hasattr(lib, sym), sym
        assert tuple(lib.tphu_pointwise_layout(i) for i in range(3)) == PREDICT_SUM_LAYOUT + (POINTWISE_MAX_TILE,) and lib.tphu_abi() == 3
    assert hasattr(ctypes.CDLL(str(built[2])), "tphu_derived") and hasattr(ctypes.CDLL(str(built[3])), "tphu_predictive")
    for path in (build_plugin(TERM_X, 3, term=True), build_plugin(TERM_D + PRED_D, 3, tables=tabs, term=True, predict=True)):
        plain = ctypes.CDLL(str(path))
        assert not hasattr(plain, "tphu_pointwise") and not hasattr(plain, "tphu_pointwise_layout") and plain.tphu_abi() == 3


@pytest.mark.parametrize("source,kw,match", [
    (WHOLE_PLAIN, {"pointwise": True}, "log_likelihood_term"),
    (WHOLE_PLAIN + PRED_X, {"pointwise": True, "n_predict": 4}, "log_likelihood_term"),
    (TERM_X, {"pointwise": 1, "n_terms": 5}, "True or False"),
    (TERM_X, {"pointwise": "yes", "n_terms": 5}, "True or False"),
    (TERM_X, {"pointwise": None, "n_terms": 5}, "True or False"),
    (TERM_X, {"pointwise": True}, "needs n_terms="),
])
def test_pointwise_validation_raises_before_the_compiler_runs(source, kw, match, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    with pytest.raises(ValueError, match=match):
        tp.HipCallbacks(source, 3, **kw)
    with pytest.raises(TypeError):
        tp.HipCallbacks(TERM_X, 3, True, False, True, False, None, 5, None, None, True)      # keyword-only


def test_pointwise_tile_rule_and_scratch():
    from tempest_amd.hipcallbacks import (POINTWISE_MAX_TILE, POINTWISE_MIN_WORKGROUPS, POINTWISE_SCRATCH_WORDS, pointwise_scratch_words,
                                          pointwise_tiles)
    for n in (1, 63, 1000, 3001, 1 << 20, 1 << 22):
        for R in (1, 7, 100, 10_000, 100_000):
            tile = pointwise_tiles(n, R)
            n_blocks = -(-n // 1024)
            assert 1 <= tile <= POINTWISE_MAX_TILE and tile & (tile - 1) == 0
            assert tile == POINTWISE_MAX_TILE or n_blocks * -(-R // (2 * tile)) < POINTWISE_MIN_WORKGROUPS      # why it was halved
            assert tile == 1 or n_blocks * -(-R // tile) >= POINTWISE_MIN_WORKGROUPS                            # why no further
            per_r = 4 * n_blocks + 2
            words = pointwise_scratch_words(n, R)
            assert words >= 1 + n_blocks + per_r and words <= 1 + n_blocks + max(per_r, POINTWISE_SCRATCH_WORDS)
            assert (words - 1 - n_blocks) % per_r == 0 and (words - 1 - n_blocks) // per_r <= R
    assert pointwise_tiles(1000, 10_000) < POINTWISE_MAX_TILE            # few rows, many indices: smaller index tiles
    assert pointwise_tiles(1 << 20, 100) == POINTWISE_MAX_TILE
    assert pointwise_scratch_words(3001, 1000) == 1 + 3 + 14 * 1000


def test_the_summation_order_alone_stays_inside_the_bounds():
    """The float64 restatement against the long double reference, at the seeds and sizes the device test uses: the order of the sums
    (and NumPy's exp and log) leave the bounds room."""
    for n, R in all_cases():
        x, w, a, ref, ld = case(n, R)
        assert np.all(np.abs(a) <= 2.5) and np.sum(w == 0) >= (n >= 700) * 0.03 * n
        within_bounds(ref, ld, n)
        np.testing.assert_array_equal(ref["elpd_waic"], ref["lppd"] - ref["p_waic"])
        assert np.all(ref["ess_loo"] <= np.sum(w > 0) * (1 + 1e-12)) and np.all(ref["ess_loo"] >= 1 - 1e-12)


def closed_form(seed=5, T=50, n=1 << 16):
    """y_r ~ N(theta, 1), T fixed observations, n equal-weight draws from the exact posterior N(ybar, 1 / T): the rows, the data, the
    closed forms of lppd, elpd_loo and p_waic (without the constant -log(2 pi) / 2) and their delta-method standard errors from the draws."""
    rng = np.random.RandomState(seed)
    y = 0.3 + rng.randn(T)
    ybar, s2 = y.mean(), 1.0 / T
    theta = ybar + np.sqrt(s2) * rng.randn(n)
    a = -0.5 * (y[:, None] - theta[None, :]) ** 2
    delta = y - ybar
    ybar_r = (y.sum() - y) / (T - 1)

    def lognorm(v, mu, var):
        return -0.5 * np.log(var) - 0.5 * (v - mu) ** 2 / var
    want = {"lppd": lognorm(y, ybar, 1 + s2), "elpd_loo": lognorm(y, ybar_r, 1 + 1.0 / (T - 1)), "p_waic": (2 * s2 * s2 + 4 * delta ** 2 * s2) / 4}
    E, F = np.exp(a), np.exp(-a)
    var = a.var(axis=1)
    m4 = ((a - a.mean(axis=1)[:, None]) ** 4).mean(axis=1)
    se = {"lppd": E.std(axis=1) / (np.sqrt(n) * E.mean(axis=1)), "elpd_loo": F.std(axis=1) / (np.sqrt(n) * F.mean(axis=1)),
          "p_waic": np.sqrt((m4 - var ** 2) / n)}
    numpy = {"lppd": np.log(E.mean(axis=1)), "elpd_loo": -np.log(F.mean(axis=1)), "p_waic": var}
    x = np.zeros((n, 3))
    x[:, 0] = theta
    return x, {"y": y}, want, se, numpy


def test_closed_form_reference_passes_at_the_committed_seed():
    _, _, want, se, numpy = closed_form()
    for k in want:
        assert np.all(np.abs(numpy[k] - want[k]) <= 6 * se[k]), k
        assert np.all(se[k] < 0.02)


# ------------------------------------------------------------------------------------------------- GPU
def run_case(tp, n, R):
    x, w, a, ref, ld = case(n, R)
    cb = tp.HipCallbacks(TERM_X, 3, n_terms=R, pointwise=True)
    assert cb.pointwise_enabled and cb.n_terms == R and cb.pointwise_tile == 0
    got = cb.pointwise(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda())
    assert got["n_rows"] == n and abs(got["ess"] - w.sum() ** 2 / (w * w).sum()) <= 1e-9 * got["ess"]
    for k in KEYS:
        assert got[k].shape == (R,) and got[k].dtype == np.float64
    tol = tolerance(n)
    print(f"n={n} n_terms={R}: mean differs at {int(np.sum(got['mean'] != ref['mean']))}, p_waic at {int(np.sum(got['p_waic'] != ref['p_waic']))}; "
          + ", ".join(f"{k} {float(np.max(np.abs(got[k] - ld[k]))) / 2.0 ** -52:.1f}" for k in ("lppd", "elpd_loo"))
          + f" of {tol / 2.0 ** -52:.0f} x 2^-52; ess_loo rel {float(np.max(np.abs(got['ess_loo'] - ld['ess_loo']) / ld['ess_loo'])) / tol:.2f} of 4 tol")
    np.testing.assert_array_equal(got["mean"], ref["mean"])
    np.testing.assert_array_equal(got["p_waic"], ref["p_waic"])
    within_bounds(got, ld, n)
    np.testing.assert_array_equal(got["elpd_waic"], got["lppd"] - got["p_waic"])
    tot = got["totals"]
    for k in ("elpd_waic", "p_waic", "lppd", "elpd_loo"):
        assert tot[k] == math.fsum(got[k])
    assert tot["p_loo"] == tot["lppd"] - tot["elpd_loo"]
    for k in ("elpd_waic", "elpd_loo"):
        assert tot[k + "_se"] == pytest.approx(math.sqrt(R * np.var(got[k])), rel=1e-12, abs=1e-300)
    return cb, got


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n", SIZES)
def test_values_bit_for_bit_and_within_the_bounds(n):
    import tempest_amd as tp
    need_gpu()
    for R in N_TERMS:
        run_case(tp, n, R)


@pytest.mark.gpu
@needs_hipcc
def test_values_at_1025_row_blocks():
    import tempest_amd as tp
    need_gpu()
    run_case(tp, BIG, 7)


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n", (65, 3001))
def test_no_tile_and_no_batch_changes_a_bit(n, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks as H
    need_gpu()
    R = 1000
    cb, got = run_case(tp, n, R)
    x, w = case(n, R)[:2]
    xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    for pin in PINS:
        cb.pointwise_tile = pin
        other = cb.pointwise(xt, wt)
        for k in KEYS:
            np.testing.assert_array_equal(other[k], got[k], err_msg=f"{k} at tile {pin}")
    cb.pointwise_tile = 0
    per_r = 4 * -(-n // 1024) + 2
    monkeypatch.setattr(H, "POINTWISE_SCRATCH_WORDS", per_r * 400)
    words = H.pointwise_scratch_words(n, R)
    assert -(-R // ((words - 1 - -(-n // 1024)) // per_r)) >= 3                 # at least 3 batches
    for pin in (0, 4):
        cb.pointwise_tile = pin
        other = cb.pointwise(xt, wt)
        for k in KEYS:
            np.testing.assert_array_equal(other[k], got[k], err_msg=f"{k} in batches, tile {pin}")


def call_entry(cb, xbuf, g, wt, n, R, words, tile, guard=0, fill=-777.25, ifill=0x5A5A5A5A5A5A5A5A):
    obuf = torch.full((guard + 6 * R + guard,), fill, dtype=torch.float64, device="cuda")
    sbuf = torch.full((guard + words + guard,), ifill, dtype=torch.int64, device="cuda")
    rc = cb.lib.tphu_pointwise(cb._stream(xbuf), xbuf.data_ptr() + 8 * g, wt.data_ptr(), n, R, obuf.data_ptr() + 8 * guard,
                               sbuf.data_ptr() + 8 * guard, words, tile, *cb._data())
    assert rc == 0, cb.lib.tphu_last_error()
    return obuf.cpu().numpy(), sbuf.cpu().numpy()


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n_dim", [4, 10, 40])
@pytest.mark.parametrize("shift", [0, 1])
def test_every_way_the_rows_are_loaded(n_dim, shift):
    """n_dim 3 (every other test): staged through LDS at a pitch equal to n_dim; n_dim 4: at a pitch of 5 doubles; n_dim 10 and 40:
    256 rows exceed the staging buffer, every lane reads its row from memory.  shift 1: x on an address that is not 16-byte aligned
    (8-byte staging loads).  Through the entry point itself."""
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import pointwise_scratch_words
    need_gpu()
    R, g = 11, 64 + shift
    cb = tp.HipCallbacks(TERM_X, n_dim, n_terms=R, pointwise=True)
    for n in (65, 700) + ((3001,) if n_dim < 40 else ()):
        x, w, a, ref, ld = case(n, R, n_dim)
        xbuf = torch.zeros(g + n_dim * n + g, dtype=torch.float64, device="cuda")
        xbuf[g:g + n_dim * n] = torch.from_numpy(x).cuda().reshape(-1)
        wt = torch.from_numpy(w).cuda()
        first = None
        for tile in (64, 4):
            o, _ = call_entry(cb, xbuf, g, wt, n, R, pointwise_scratch_words(n, R), tile)
            res = dict(zip(KEYS, o.reshape(6, R)))
            np.testing.assert_array_equal(res["mean"], ref["mean"])
            np.testing.assert_array_equal(res["p_waic"], ref["p_waic"])
            within_bounds(res, ld, n)
            first = first or res
            for k in KEYS:
                np.testing.assert_array_equal(res[k], first[k])
        if shift == 0:
            got = cb.pointwise(x, w)
            for k in KEYS:
                np.testing.assert_array_equal(got[k], first[k])


def special_setup(n=3001, R=8, seed=9):
    x, w = rows_and_weights(n, seed=seed)
    rng = np.random.RandomState(seed + 1)
    pos = np.flatnonzero(w > 0)
    nine, eight = pos[rng.choice(len(pos), 40, replace=False)].reshape(2, 20)
    x[nine, 1], x[eight, 1] = 9.0, 8.0
    inf, nan = np.inf, np.nan
    D = {"c": np.linspace(0.5, 1.5, R),
         "sp": np.array([-0.3, nan, -inf, inf, -inf, -inf, inf, nan]),
         "sq": np.array([-0.7, -0.7, -0.7, -0.7, inf, -0.7, -0.7, -0.7]),
         "every": np.array([0, 0, 0, 0, 0, 1, 1, 1.0])}
    return x, w, D, nine, eight


def term_special(x, D):
    R = len(D["c"])
    z = x[None, :, 0] - D["c"][:, None]
    a = -0.5 * (z * z)
    a = np.where((x[None, :, 1] == 8.0), D["sq"][:, None], a)
    a = np.where((x[None, :, 1] == 9.0) | (D["every"][:, None] == 1.0), D["sp"][:, None], a)
    assert a.shape == (R, len(x))
    return a


def same_bits(a, b):
    """Equal, NaN where the other is NaN."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


@pytest.fixture(scope="module")
def special_run():
    import tempest_amd as tp
    need_gpu()
    x, w, D, nine, eight = special_setup()
    cb = tp.HipCallbacks(TERM_SPECIAL, 3, data=D, n_terms="c", pointwise=True)
    got = cb.pointwise(x, w)
    a = term_special(x, D)
    return cb, x, w, D, a, got, mirror(a, w)


def finite_part(a, w, r, drop):
    """The long double reference of index r over the rows whose term is not `drop` (their weight stays in W)."""
    L = np.longdouble
    keep = (w > 0) & (a[r] != drop)
    u = w[keep].astype(L) / w[w > 0].astype(L).sum()
    return a[r, keep].astype(L), u


@pytest.mark.gpu
@needs_hipcc
def test_special_plain_index_is_untouched(special_run):
    cb, x, w, D, a, got, ref = special_run
    assert np.all(np.isfinite(a[0][w > 0]))
    for k in ("mean", "p_waic"):
        assert got[k][0] == ref[k][0]
    within_bounds({k: got[k][:1] for k in KEYS}, {k: v[:1] for k, v in long_double(a[:1], w).items()}, len(w))


@pytest.mark.gpu
@needs_hipcc
def test_special_nan_with_weight_makes_every_output_nan(special_run):
    cb, x, w, D, a, got, ref = special_run
    for r in (1, 7):
        assert all(np.isnan(got[k][r]) for k in KEYS), r
    assert all(np.isnan(got["totals"][k]) for k in ("elpd_waic", "p_waic", "lppd", "elpd_loo", "p_loo", "elpd_waic_se", "elpd_loo_se"))


@pytest.mark.gpu
@needs_hipcc
def test_special_minus_infinity(special_run):
    cb, x, w, D, a, got, ref = special_run
    r = 2                                                    # min = -inf, the others finite
    assert got["mean"][r] == -np.inf and np.isnan(got["p_waic"][r]) and got["elpd_loo"][r] == -np.inf and np.isnan(got["ess_loo"][r])
    al, u = finite_part(a, w, r, -np.inf)
    assert abs(got["lppd"][r] - np.log((u * np.exp(al)).sum())) <= tolerance(len(w)) and np.isnan(got["elpd_waic"][r])
    r = 5                                                    # every term -inf
    assert got["lppd"][r] == -np.inf and got["mean"][r] == -np.inf and np.isnan(got["p_waic"][r])
    assert got["elpd_loo"][r] == -np.inf and np.isnan(got["ess_loo"][r])


@pytest.mark.gpu
@needs_hipcc
def test_special_plus_infinity(special_run):
    cb, x, w, D, a, got, ref = special_run
    r = 3                                                    # max = +inf, the others finite
    assert got["lppd"][r] == np.inf and got["mean"][r] == np.inf and np.isnan(got["p_waic"][r])
    al, u = finite_part(a, w, r, np.inf)
    v = u * np.exp(-al)
    tol = tolerance(len(w))
    assert abs(got["elpd_loo"][r] + np.log(v.sum())) <= tol
    ess = v.sum() ** 2 / (v * v).sum()
    assert abs(got["ess_loo"][r] - ess) <= 4 * tol * ess
    r = 4                                                    # both: lppd = +inf, elpd_loo = -inf, the mean is inf - inf
    assert got["lppd"][r] == np.inf and got["elpd_loo"][r] == -np.inf
    assert np.isnan(got["mean"][r]) and np.isnan(got["p_waic"][r]) and np.isnan(got["ess_loo"][r])
    r = 6                                                    # every term +inf
    assert got["lppd"][r] == np.inf and got["mean"][r] == np.inf and np.isnan(got["p_waic"][r]) and np.isnan(got["ess_loo"][r])
    assert got["elpd_loo"][r] == np.inf
    for k in KEYS:                                           # and the restatement has the same NaNs and infinities everywhere
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        np.testing.assert_array_equal(np.where(np.isinf(got[k]), got[k], 0.0), np.where(np.isinf(ref[k]), ref[k], 0.0), err_msg=k)


@pytest.mark.gpu
@needs_hipcc
def test_special_rows_without_weight_never_matter(special_run):
    cb, x, w, D, a, got, ref = special_run
    zero = np.flatnonzero(w == 0)
    assert len(zero) > 50
    for fill in (np.nan, 1e300, -1e300, 9.0, 8.0):           # (9 and 8: the term returns NaN / +-inf there at most indices)
        y = x.copy()
        y[zero] = fill
        other = cb.pointwise(y, w)
        for k in KEYS:
            assert same_bits(other[k], got[k]), (k, fill)


@pytest.mark.gpu
@needs_hipcc
def test_equal_weights_are_the_unweighted_formulas_and_bad_weights_raise():
    import tempest_amd as tp
    from tempest_amd._lib import TempestHipError
    need_gpu()
    n, R = 3001, 9
    x, w, a, _, _ = case(n, R)
    cb = tp.HipCallbacks(TERM_X, 3, n_terms=R, pointwise=True)
    tol = tolerance(n)
    L = np.longdouble
    al = a.astype(L)
    for wv in (1.0, 1.0 / n, 0.7):
        got = cb.pointwise(x, np.full(n, wv))
        v = np.exp(-al)
        assert np.all(np.abs(got["lppd"] - np.log(np.exp(al).mean(axis=1))) <= tol)
        assert np.all(np.abs(got["elpd_loo"] + np.log(v.mean(axis=1))) <= tol)
        ess = v.sum(axis=1) ** 2 / (v * v).sum(axis=1)
        assert np.all(np.abs(got["ess_loo"] - ess) <= 4 * tol * ess)
        assert np.all(np.abs(got["mean"] - al.mean(axis=1)) <= tol)
        assert np.all(np.abs(got["p_waic"] - al.var(axis=1)) <= tol)
        assert got["ess"] == pytest.approx(n, rel=1e-12)
    one = cb.pointwise(x[5:6], np.array([0.37]))              # one row: everything is that row's term
    for k in ("lppd", "mean", "elpd_loo", "elpd_waic"):
        np.testing.assert_array_equal(one[k], a[:, 5])
    assert np.all(one["p_waic"] == 0.0) and np.all(one["ess_loo"] == 1.0) and one["n_rows"] == 1
    for wbad in (np.zeros(n), np.where(np.arange(n) == 3, -1.0, 1.0), np.where(np.arange(n) == 3, np.inf, 1.0),
                 np.where(np.arange(n) == 3, np.nan, 1.0), np.ones(n - 1)):
        with pytest.raises(ValueError, match="pointwise"):
            cb.pointwise(x, wbad)
    with pytest.raises(ValueError, match="pointwise"):
        cb.pointwise(x[:0], w[:0])
    plain = tp.HipCallbacks(TERM_X, 3, n_terms=R)
    assert not plain.pointwise_enabled
    with pytest.raises(TempestHipError, match="pointwise=True"):
        plain.pointwise(x, w)
    s = tp.Sampler(plain.prior_transform, plain.log_likelihood, 3, n_particles=256, vectorize=True, random_state=1)
    with pytest.raises(TempestHipError, match="pointwise=True"):
        s.pointwise()


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("shift", [0, 1])
def test_guard_cells_round_output_and_scratch_and_batches_of_indices(shift):
    """The entry point itself: the output and a scratch buffer of exactly the size the package gives keep their guard cells; a scratch
    that holds 3 indices at a time (batches) gives the same bits.  shift 1: x not 16-byte aligned (8-byte loads)."""
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import pointwise_scratch_words
    need_gpu()
    R, g = 11, 64 + shift
    cb = tp.HipCallbacks(TERM_X, 3, n_terms=R, pointwise=True)
    fill, ifill = -777.25, 0x5A5A5A5A5A5A5A5A
    for n in (1, 65, 1025, 3001):
        x, w = case(n, R)[:2]
        want = cb.pointwise(x, w)
        xbuf = torch.zeros(g + 3 * n + g, dtype=torch.float64, device="cuda")
        xbuf[g:g + 3 * n] = torch.from_numpy(x).cuda().reshape(-1)
        wt = torch.from_numpy(w).cuda()
        n_blocks = -(-n // 1024)
        for words in (pointwise_scratch_words(n, R), 1 + n_blocks + 3 * (4 * n_blocks + 2)):
            for tile in (1, 64):
                o, s = call_entry(cb, xbuf, g, wt, n, R, words, tile, guard=g, fill=fill, ifill=ifill)
                assert np.all(o[:g] == fill) and np.all(o[-g:] == fill), (n, words, tile)
                assert np.all(s[:g] == ifill) and np.all(s[-g:] == ifill), (n, words, tile)
                for k, row in zip(KEYS, o[g:-g].reshape(6, R)):
                    np.testing.assert_array_equal(row, want[k])
    # checked arguments
    stream, D = cb._stream(xbuf), cb._data()
    obuf, sbuf = torch.zeros(6 * R, dtype=torch.float64, device="cuda"), torch.zeros(words, dtype=torch.int64, device="cuda")
    a = (stream, xbuf.data_ptr(), wt.data_ptr(), 4, R, obuf.data_ptr(), sbuf.data_ptr())
    assert cb.lib.tphu_pointwise(*a, 5, 64, *D) == -2 and b"scratch" in cb.lib.tphu_last_error()
    assert cb.lib.tphu_pointwise(*a, words, 65, *D) == -2 and cb.lib.tphu_pointwise(*a, words, 0, *D) == -2
    assert cb.lib.tphu_pointwise(stream, None, wt.data_ptr(), 4, R, obuf.data_ptr(), sbuf.data_ptr(), words, 64, *D) == -2
    assert cb.lib.tphu_pointwise(stream, xbuf.data_ptr(), wt.data_ptr(), 4, R + 1, obuf.data_ptr(), sbuf.data_ptr(), words, 64, *D) == -2
    # the scratch is kept between calls
    cb.pointwise(x, w)
    kept = cb._wscratch.data_ptr()
    cb.pointwise(x[:100], w[:100])
    assert cb._wscratch.data_ptr() == kept


@pytest.mark.gpu
@needs_hipcc
def test_pointwise_respects_the_stream_it_is_given():
    import tempest_amd as tp
    need_gpu()
    a = tp.HipCallbacks(TERM_X, 3, n_terms=50, pointwise=True)
    b = tp.HipCallbacks(TERM_X, 3, n_terms=50, pointwise=True)
    assert a.path == b.path
    x, w = rows_and_weights(200_000, seed=3)
    xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    want = a.pointwise(xt, wt)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(4):
        with torch.cuda.stream(sa):
            ya, va = xt * 1.0, wt * 1.0                            # produced on sa: pointwise must queue behind them on sa
            ra = a.pointwise(ya, va)
        with torch.cuda.stream(sb):
            yb, vb = xt + 0.0, wt + 0.0
            rb = b.pointwise(yb, vb)
        outs.append((ra, rb, ya, yb, va, vb))
    torch.cuda.synchronize()
    for ra, rb, *_ in outs:
        for k in KEYS:
            np.testing.assert_array_equal(ra[k], want[k])
            np.testing.assert_array_equal(rb[k], want[k])


@pytest.mark.gpu
@needs_hipcc
def test_closed_form_normal_mean():
    import tempest_amd as tp
    need_gpu()
    x, D, want, se, _ = closed_form()
    cb = tp.HipCallbacks(TERM_Y, 3, data=D, n_terms="y", pointwise=True)
    got = cb.pointwise(x, np.ones(len(x)))
    for k in want:
        z = np.abs(got[k] - want[k]) / se[k]
        print(f"{k}: at most {z.max():.2f} standard errors from the closed form")
        assert np.all(z <= 6), k
    assert np.all(got["ess_loo"] > 0.5 * len(x))
    assert abs(got["totals"]["p_waic"] - want["p_waic"].sum()) <= 6 * se["p_waic"].sum()
    assert 0.5 < got["totals"]["p_waic"] < 2.0                                   # one parameter


@pytest.mark.gpu
@needs_hipcc
def test_whole_run_and_nothing_else_changes():
    import tempest_amd as tp
    from tempest_amd._lib import TempestHipError
    need_gpu()
    D = quad_data()

    def run(cb):
        s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=512, vectorize=True, clustering=False, random_state=11)
        s.run(n_total=2048, progress=False)
        return s
    plain = run(tp.HipCallbacks(QUAD + QUAD_PRED, 3, data=D, n_terms="t", n_predict="t"))
    cb = tp.HipCallbacks(QUAD + QUAD_PRED, 3, data=D, n_terms="t", n_predict="t", pointwise=True)
    s = run(cb)
    assert s.evidence()[0] == plain.evidence()[0]
    for case_kw in (dict(), dict(trim_importance_weights=False)):
        for got, want in zip(s.posterior(**case_kw), plain.posterior(**case_kw)):
            np.testing.assert_array_equal(got, want)
        pa, pb = s.predictive(**case_kw), plain.predictive(**case_kw)
        for k in ("mean", "var", "quantiles"):
            np.testing.assert_array_equal(pa[k], pb[k])
        x, w, _ = s.posterior(**case_kw)
        pw = s.pointwise(**case_kw)
        direct = cb.pointwise(x, w)
        assert pw["n_rows"] == len(x) and pw["ess"] == direct["ess"] and pw["totals"] == direct["totals"]
        for k in KEYS:
            np.testing.assert_array_equal(pw[k], direct[k])
            assert pw[k].shape == (200,) and np.all(np.isfinite(pw[k]))
    assert np.all(pw["elpd_loo"] <= pw["lppd"]) and 0.5 < pw["totals"]["p_waic"] < 10 and 0.5 < pw["totals"]["p_loo"] < 10
    with pytest.raises(TempestHipError, match="pointwise=True"):
        plain.pointwise()


@pytest.mark.gpu
@needs_hipcc
def test_two_ranks_refuse_and_finish(tmp_path):
    need_gpu()
    import tempest_amd as tp
    tp.HipCallbacks(TERM_X, 3, n_terms=5, pointwise=True)                     # compiled once, here: the ranks find it cached
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, "-m", "tests._dist_workers_pointwise", str(r), "2", str(port), str(tmp_path)], cwd=ROOT)
             for r in (0, 1)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0]
    for r in (0, 1):
        meta = json.load(open(tmp_path / f"pointwise{r}.json"))
        assert meta["raised"] == "NotImplementedError" and "sharded" in meta["message"] and meta["rows"] > 0 and meta["finished"]

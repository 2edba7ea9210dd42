"""HipCallbacks posterior predictive (tempest_amd/hipcallbacks.py): `predict(x, r)` in the user's source, its
weighted mean, variance and quantiles over the posterior rows reduced on the device (cb.predictive, Sampler.predictive).

CPU: sources without predict() generate the text and the file name they had, plugins with it compile for gfx950 in every form and
export tphu_predictive, every validation error.  GPU: mean and var against a NumPy restatement of PREDICT_SUM_LAYOUT to the bit and at
every tile, quantiles by exact membership and rank, np.percentile(method="inverted_cdf") for equal weights, special inputs, guard
cells, two streams, a whole run, checkpoints, two ranks.

Every index of every case is checked in every way.  Host cost decides HOW at (1 << 20) + 3 rows: the restatement runs over slabs
of columns on a few threads; the weights there are 40-bit integers times 2^-38, so that membership and the exact rank sums are int64
work done with torch on the device from the NumPy-computed predictions; and the 1e-12 bound on the order of the sums is taken
against sums accumulated in long double (64-bit mantissa: a pairwise sum of 2^20 terms is good to about 1e-18), themselves held
against math.fsum at BIG_FSUM indices.  The tiles are pinned at the sizes up to 3001 and two values of n_predict, so the largest
case runs once.  (No disassembly check: the project has none for its plugins.)"""
from concurrent.futures import ThreadPoolExecutor
import ctypes
import hashlib
import json
import math
import os
import shutil
import socket
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc not available")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = '''
__device__ void prior_transform(const double* u, double* x) {
  for (int j = 0; j < N_DIM; ++j) x[j] = 20.0 * u[j] - 10.0;
}
__device__ double log_likelihood(const double* x) {
  double s = 0.0;
  for (int j = 0; j < N_DIM; ++j) s += x[j] * x[j];
  return -0.5 * s;
}
'''
# one rounding per operation, split so that nothing could fuse; every index with r % 5 == 3 ignores x: all rows tied
PRED_X = '''
__device__ double predict(const double* x, int64_t r) {
  const double t = 0.125 * (double)r;
  if (r % 5 == 3) return t;
  const double a = x[1] * t;
  return x[0] + a;
}
'''
PRIOR_D = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
  for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0;
}
'''
PRED_D = '''
__device__ double predict(const double* x, int64_t r, const tphu_data& D) {
  const double a = x[1] * D.t[r];
  return x[0] + a;
}
'''
WHOLE_D = PRIOR_D + '''
__device__ double log_likelihood(const double* x, const tphu_data& D) {
  double s = 0.0;
  for (int64_t r = 0; r < D.t_len; ++r) { const double z = x[0] - D.t[r]; s += -0.5 * z * z; }
  return s;
}
'''
TERM_D = PRIOR_D + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double z = x[0] - D.t[r];
  return -0.5 * z * z;
}
'''
DERIVED = '''
__device__ void derived(const double* x, double* out) { out[0] = x[0] + x[1]; }
'''
# the README's example: a quadratic in t with known noise
QUAD = PRIOR_D + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double m = x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r];
  const double z = (D.y[r] - m) / D.s[r];
  return -0.5 * z * z;
}
'''
QUAD_PRED = '''
__device__ double predict(const double* x, int64_t r, const tphu_data& D) {
  return x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r];
}
'''

SIZES = (1, 63, 64, 65, 700, 3001, (1 << 20) + 3)
N_PREDICT = (1, 7, 256, 1000)
QS = (0.0, 0.025, 0.5, 0.975, 1.0)
PINS = ((1, 256), (4, 512), (16, 1024), (64, 256))       # (indices per workgroup, rows per workgroup of the select)
BIG = 1 << 20
BIG_FSUM = 8
PINNED_N_PREDICT = (7, 1000)
# the other two ways the rows reach the lanes (n_dim 3 stages through LDS at a pitch equal to n_dim): predict reads the first and
# the LAST coordinate
PRED_LAST = '''
__device__ double predict(const double* x, int64_t r) {
  const double t = 0.125 * (double)r;
  if (r % 5 == 3) return t;
  const double a = x[N_DIM - 1] * t;
  return x[0] + a;
}
'''


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


W_SCALE = 2.0 ** 38


def rows_and_weights(n, seed, dyadic=False, d=3):
    """x[:, 0] in [1, 2], x[:, 1] and x[:, -1] in [0.5, 1] (positive predictions: a relative bound on the mean means something) and
    positive weights with about 5 % exact zeros; dyadic: 40-bit integers times 2^-38 -- random values in (0, 4) whose float64 sums
    still round (the order of W shows), and whose exact sums are int64 sums of w * W_SCALE."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (n, d))
    x[:, 0] = rng.uniform(1.0, 2.0, n)
    x[:, 1] = rng.uniform(0.5, 1.0, n)
    x[:, -1] = rng.uniform(0.5, 1.0, n)
    w = rng.randint(1, 1 << 40, n, dtype=np.int64) * 2.0 ** -38 if dyadic else rng.uniform(0.1, 3.0, n)
    w[rng.rand(n) < 0.05] = 0.0
    if not np.any(w > 0):
        w[0] = 1.0
    return x, w


def pred_x(x, r0, r1, col=1):
    """PRED_X (col = -1: PRED_LAST) at indices r0 .. r1 - 1, operation by operation: (r1 - r0, n)."""
    r = np.arange(r0, r1)
    t = 0.125 * r.astype(np.float64)
    a = x[None, :, col] * t[:, None]
    p = x[None, :, 0] + a
    tied = r % 5 == 3
    p[tied] = t[tied, None]
    return p


def layout_sum(v, layout):
    """Rows of v (c, n) added in the order of PREDICT_SUM_LAYOUT: chunks of `C` consecutive values by the halving tree v[:h] + v[h:2h],
    blocks of `B` chunk sums in chunk order, the block sums in block order, every level from +0.0."""
    C, B = layout
    c, n = v.shape
    nb = -(-n // (C * B))
    pad = np.zeros((c, nb * C * B))
    pad[:, :n] = v
    t = pad.reshape(c, nb, B, C)
    h = C // 2
    while h >= 1:
        t = t[..., :h] + t[..., h:2 * h]
        h //= 2
    t = t[..., 0]
    bs = np.zeros((c, nb))
    for j in range(B):
        bs = bs + t[:, :, j]
    tot = np.zeros(c)
    for b in range(nb):
        tot = tot + bs[:, b]
    return tot


def reference_moments(pred, x, w, n_predict, layout, step=64, workers=1, on_slab=None, long_double=False):
    """mean, var (n_predict,) as the kernels define them: W in the layout order, u = w / W, sum u p, then sum u (p - mean)^2.  Slabs of
    `step` columns, on `workers` threads (NumPy releases the interpreter lock in its loops); on_slab(r0, r1, p) sees every slab of
    predictions, in the thread that made it.  long_double: also (mean, var) with the same terms accumulated in long double."""
    W = layout_sum(w[None, :], layout)[0]
    pos = w > 0
    u = np.where(pos, w / W, 0.0)
    mean, var = np.empty(n_predict), np.empty(n_predict)
    hi = (np.empty(n_predict, dtype=np.longdouble), np.empty(n_predict, dtype=np.longdouble)) if long_double else None

    def slab(r0, r1):
        with np.errstate(invalid="ignore", over="ignore"):
            p = pred(x, r0, r1)
            if on_slab is not None:
                on_slab(r0, r1, p)
            term = np.where(u > 0, u * p, 0.0)
            m = layout_sum(term, layout)
            if hi:
                hi[0][r0:r1] = term.sum(axis=1, dtype=np.longdouble)
            d = p - m[:, None]
            term = np.where(u > 0, u * (d * d), 0.0)
            mean[r0:r1], var[r0:r1] = m, layout_sum(term, layout)
            if hi:
                hi[1][r0:r1] = term.sum(axis=1, dtype=np.longdouble)

    with ThreadPoolExecutor(workers) as pool:
        pending = []
        for r0 in range(0, n_predict, step):
            r1 = min(n_predict, r0 + step)
            pending.append(pool.submit(slab, r0, r1))
            while len(pending) > workers:              # (bounds the slabs of predictions alive at once)
                pending.pop(0).result()
        for f in pending:
            f.result()
    return (mean, var) + (hi if hi else ())


def exact_sum(a):
    return Fraction(math.fsum(a))


def check_quantile_column(p, w, qs, got, eps):
    """got[j] is bitwise one of p, and sum_{p < v} w <= (q + eps) W, sum_{p <= v} w >= (q - eps) W in exact arithmetic (fsum)."""
    tot = exact_sum
    W = tot(w)
    bits = p.view(np.int64)
    for q, v in zip(qs, got):
        assert np.any(bits == np.float64(v).view(np.int64)), (q, v)
        below, upto = tot(w[p < v]), tot(w[p <= v])
        assert below <= (Fraction(q) + eps) * W, (q, v, float(below / W))
        assert upto >= (Fraction(q) - eps) * W, (q, v, float(upto / W))


# ------------------------------------------------------------------------------------------------- CPU
# What the parent of this feature (3a62694) generated: SHA-256 of the text and the file name build_plugin gave it (the name also
# hashes csrc/common.h, include/tempest_hip.h and `hipcc --version`: the recorded names hold where those are the recorded ones).
PARENT_ENV = "2b62480092b80b7ec47b1333ab23a4d077792b10d3b49d36aad7954ec603477e"


def parent_cases():
    from tests import test_hipcallbacks_data as T
    from tests import test_hipcallbacks_derived as X
    return (   # source, n_dim, tables, term, n_derived, text hash, file name
        (T.OLD_SRC, 10, None, False, 0, "85422a8c6c6b7f15300384fe0cff150dc7d93d0c9030862000df9219ef6bc467", "tphu_10d_31906f1f808b4d3dacbe.so"),
        (T.REG, 3, X.REG_TABLES, True, 0, "2f76975f583edfd024e56ecb6d3fc91bdb72f594fe1beac0713e94a88e10c03d", "tphu_3d_8cf3797ac7a56213842b.so"),
        (T.WHOLE, 3, (("obs", 2),), False, 0, "2852dc283614e005b4c163dd6beed48e08e3f5a267d889d59fb34ebfe45335a1", "tphu_3d_04a943dee0844861b2bf.so"),
        (X.BASE + X.ARITH, 4, None, False, 2, "79f97f95028fa88fc7fd8bf66a10adab8d2170f5566e038241900152fa28f58c", "tphu_4d_d4e99995d6d44e316908.so"),
        (X.TERM_D + X.DERIVED_D, 3, (("tab", 2),), True, 2, "5dc548543ace24a8221df948dab017b50bd6103868ddbb22381d6bef8bca683e",
         "tphu_3d_d65ba023b41633052b2f.so"),
    )


def test_sources_without_predict_generate_the_parent_text():
    from tempest_amd.hipcallbacks import plugin_source
    for src, _, tables, term, nder, sha, _ in parent_cases():
        text = plugin_source(src, tables, term, derived=nder > 0)
        assert hashlib.sha256(text.encode()).hexdigest() == sha
        assert text == plugin_source(src, tables, term, derived=nder > 0, predict=False)
        assert "predict" not in text and "TPHU_PCHUNK" not in text and "//@P" not in text
    with_p = plugin_source(BASE + PRED_X, predict=True)
    assert "k_user_predict_moment" in with_p and "tphu_predictive(" in with_p and "//@P" not in with_p
    assert "@" not in with_p.replace(BASE + PRED_X, "")


@needs_hipcc
def test_sources_without_predict_keep_their_file_name():
    from tempest_amd import hipcallbacks as H
    deps = (H._CSRC / "common.h").read_bytes() + open(H.HEADER_PATH, "rb").read()
    recorded_env = hashlib.sha256(deps + H._toolchain_id().encode()).hexdigest() == PARENT_ENV
    for src, n_dim, tables, term, nder, sha, name in parent_cases():
        got = H.build_plugin(src, n_dim, tables=tables, term=term, n_derived=nder).name
        text = H.plugin_source(src, tables, term, derived=nder > 0)
        key = f"|{n_dim}|gfx950|-O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -ffp-contract=on -Wno-unused-function|{H._toolchain_id()}" \
            + (f"|derived={nder}" if nder else "")
        assert got == f"tphu_{n_dim}d_{hashlib.sha256(text.encode() + deps + key.encode()).hexdigest()[:20]}.so"
        if recorded_env:
            assert got == name
    assert H.build_plugin(BASE + PRED_X, 3, predict=True) != H.build_plugin(BASE + PRED_X, 4, predict=True)


@needs_hipcc
def test_predict_plugins_build_in_every_form_and_export_the_entry_point():
    from tempest_amd.hipcallbacks import PREDICT_SUM_LAYOUT, build_plugin
    tabs = (("t", 1),)
    built = (build_plugin(BASE + PRED_X, 3, predict=True),
             build_plugin(WHOLE_D + PRED_D, 3, tables=tabs, predict=True),
             build_plugin(TERM_D + PRED_D, 3, tables=tabs, term=True, predict=True),
             build_plugin(BASE + DERIVED + PRED_X, 3, n_derived=1, predict=True),
             build_plugin(BASE + PRED_X, 40, predict=True))                      # too wide for the LDS staging: rows straight from memory (run at 10)
    for path in built:
        lib = ctypes.CDLL(str(path))
        for sym in ("tphu_predictive", "tphu_predict_layout", "tphu_prior", "tphu_like", "tphu_accept", "tphu_step", "tphu_run"):
            assert hasattr(lib, sym), sym
        assert (lib.tphu_predict_layout(0), lib.tphu_predict_layout(1)) == PREDICT_SUM_LAYOUT == (64, 16) and lib.tphu_abi() == 3
    assert hasattr(ctypes.CDLL(str(built[2])), "tphu_like_split") and hasattr(ctypes.CDLL(str(built[3])), "tphu_derived")
    plain = ctypes.CDLL(str(build_plugin(BASE, 3)))
    assert not hasattr(plain, "tphu_predictive") and not hasattr(plain, "tphu_predict_layout")


T5 = {"t": np.linspace(0.0, 1.0, 5)}


@pytest.mark.parametrize("source,kw,match", [
    (BASE + PRED_X, {}, "give n_predict="),
    (BASE, {"n_predict": 4}, "goes with a source that defines"),
    (BASE + "// the band we predict (see eq. 3)\n", {"n_predict": 4}, "goes with a source that defines"),
    (BASE + PRED_X, {"n_predict": True}, "positive int"),
    (BASE + PRED_X, {"n_predict": 0}, "positive int"),
    (BASE + PRED_X, {"n_predict": -3}, "positive int"),
    (BASE + PRED_X, {"n_predict": 2.0}, "positive int"),
    (BASE + PRED_X, {"n_predict": "t"}, "names no data entry"),
    (WHOLE_D + PRED_D, {"n_predict": "y", "data": T5}, "names no data entry"),
])
def test_predict_validation_raises_before_the_compiler_runs(source, kw, match, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    with pytest.raises(ValueError, match=match):
        tp.HipCallbacks(source, 3, **kw)


def test_the_word_predict_in_a_comment_is_not_a_definition():
    from tempest_amd import hipcallbacks
    assert not hipcallbacks._defines(BASE + "// the band we predict (see eq. 3)\n", "predict")
    assert not hipcallbacks._defines(BASE + "// double predictions(\n", "predict")
    assert hipcallbacks._defines(BASE + PRED_X, "predict") and hipcallbacks._defines(WHOLE_D + PRED_D, "predict")


def test_tile_rule_and_scratch():
    from tempest_amd.hipcallbacks import (PREDICT_MAX_TILE, PREDICT_SCRATCH_WORDS, PREDICT_TABLES, predict_scratch_words,
                                          predict_tiles)
    for n in (1, 63, 1000, 3001, 1 << 20, 1 << 22):
        for R in (1, 7, 100, 10_000, 100_000):
            for nq in (0, 1, 3, 8):
                tile, slab = predict_tiles(n, R, nq)
                assert 1 <= tile <= PREDICT_MAX_TILE and slab >= 256 and slab % 256 == 0 and -(-n // slab) <= 65535
                n_blocks = -(-n // 1024)
                per_r = n_blocks + 258 * nq + 1
                words = predict_scratch_words(n, R, nq)
                assert words >= 1 + n_blocks + per_r and words <= 1 + n_blocks + max(per_r, PREDICT_SCRATCH_WORDS)
    assert predict_tiles(1000, 10_000, 3)[0] < PREDICT_MAX_TILE            # few rows, many indices: smaller index tiles ...
    tile, slab = predict_tiles(1 << 20, 100, 3)                            # ... many rows, few indices: the rows are cut for the select
    assert tile == PREDICT_MAX_TILE and slab < (1 << 20) // 32
    assert PREDICT_TABLES == 24


# ------------------------------------------------------------------------------------------------- GPU
def check_quantiles_on_device(p, w_int, qs, got, eps):
    """check_quantile_column for a slab of columns at once, with integer weights (exact int64 sums): p (c, n) NumPy predictions, got
    (len(qs), c).  The comparisons and the sums run as torch operations on the device; the verdict is integer arithmetic here."""
    pt, wi = torch.from_numpy(p).cuda(), torch.from_numpy(w_int).cuda()
    zero = torch.zeros((), dtype=torch.int64, device="cuda")
    W = int(w_int.sum())
    gt = torch.from_numpy(np.ascontiguousarray(got)).cuda()
    for j, q in enumerate(qs):
        v = gt[j][:, None]
        member = (pt.view(torch.int64) == v.view(torch.int64)).any(dim=1)
        below = torch.where(pt < v, wi, zero).sum(dim=1).cpu().numpy()
        upto = torch.where(pt <= v, wi, zero).sum(dim=1).cpu().numpy()
        assert bool(member.all()), (q, np.flatnonzero(~member.cpu().numpy()))
        hi, lo = (Fraction(q) + eps) * W, (Fraction(q) - eps) * W
        assert all(int(b) <= hi for b in below), (q, float(below.max()) / W)
        assert all(int(u) >= lo for u in upto), (q, float(upto.min()) / W)


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n", SIZES)
def test_moments_bit_for_bit_and_quantiles_by_exact_rank(n):
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import PREDICT_SUM_LAYOUT
    need_gpu()
    big = n >= BIG
    x, w = rows_and_weights(n, seed=n, dyadic=big)
    xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    eps = Fraction(2 * n, 2 ** 53)
    for n_predict in N_PREDICT:
        cb = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=n_predict)
        assert cb.predict_sum_layout == PREDICT_SUM_LAYOUT and cb.n_predict == n_predict
        pp = cb.predictive(xt, wt, quantiles=QS)
        assert pp["mean"].shape == pp["var"].shape == (n_predict,) and pp["quantiles"].shape == (len(QS), n_predict)
        assert pp["n_rows"] == n and abs(pp["ess"] - w.sum() ** 2 / (w * w).sum()) <= 1e-9 * pp["ess"]
        if big:
            w_int = (w * W_SCALE).astype(np.int64)
            assert np.array_equal(w_int / W_SCALE, w)
            mean, var, mean_hi, var_hi = reference_moments(
                pred_x, x, w, n_predict, PREDICT_SUM_LAYOUT, step=32, workers=8, long_double=True,
                on_slab=lambda r0, r1, p: check_quantiles_on_device(p, w_int, QS, pp["quantiles"][:, r0:r1], eps))
        else:
            mean, var = reference_moments(pred_x, x, w, n_predict, PREDICT_SUM_LAYOUT)
        print(f"n={n} n_predict={n_predict}: mean differs at {int(np.sum(pp['mean'] != mean))}, var at {int(np.sum(pp['var'] != var))} indices")
        np.testing.assert_array_equal(pp["mean"], mean)
        np.testing.assert_array_equal(pp["var"], var)
        if not big and n_predict in PINNED_N_PREDICT:
            for pin in PINS + (4,):
                cb.predict_tile = pin
                other = cb.predictive(xt, wt, quantiles=QS)
                for key in ("mean", "var", "quantiles"):
                    np.testing.assert_array_equal(other[key], pp[key], err_msg=f"{key} at tile {pin}")
            cb.predict_tile = 0
        W = math.fsum(w)
        if big:
            # the order itself, every index: within 1e-12 of the long double sums, which fsum vouches for at BIG_FSUM of them
            mean_hi, var_hi = mean_hi.astype(np.float64), var_hi.astype(np.float64)      # (sums of the terms u p and u (p - mean)^2)
            assert np.all(np.abs(pp["mean"] - mean_hi) <= 1e-12 * np.abs(mean_hi))
            assert np.all(np.abs(pp["var"] - var_hi) <= 1e-12 * var_hi + 1e-20 * mean_hi ** 2)
            for r in np.linspace(0, n_predict - 1, min(n_predict, BIG_FSUM)).astype(int):
                p = pred_x(x, r, r + 1)[0]
                m = math.fsum(w * p) / W
                v = math.fsum(w * (p - m) ** 2) / W
                assert abs(mean_hi[r] - m) <= 1e-13 * abs(m) and abs(var_hi[r] - v) <= 1e-13 * v + 1e-20 * m * m, r
            continue
        for r in range(n_predict):
            p = pred_x(x, r, r + 1)[0]
            # the order itself: within 1e-12 of the exactly rounded sums (var: plus the square of what n roundings can move the mean)
            m = math.fsum(w * p) / W
            v = math.fsum(w * (p - m) ** 2) / W
            assert abs(pp["mean"][r] - m) <= 1e-12 * abs(m), (r, pp["mean"][r], m)
            assert abs(pp["var"][r] - v) <= 1e-12 * v + 1e-20 * m * m, (r, pp["var"][r], v)
            check_quantile_column(p, w, QS, pp["quantiles"][:, r], eps)


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n_dim", [4, 10])
@pytest.mark.parametrize("shift", [0, 1])
def test_every_way_the_rows_are_loaded(n_dim, shift):
    """n_dim 4: staged through LDS at a pitch of 5 doubles (n_dim 3 has pitch 3 = n_dim); n_dim 10: 256 rows exceed the staging
    buffer, every lane reads its row from memory.  shift 1: x on an address that is not 16-byte aligned (8-byte staging loads).
    Moments to the bit, quantiles by membership and exact rank, through the entry point itself."""
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import PREDICT_SUM_LAYOUT, predict_scratch_words
    need_gpu()
    R, g = 11, 64 + shift
    cb = tp.HipCallbacks(BASE + PRED_LAST, n_dim, n_predict=R)
    qs = np.array(QS)
    pred = lambda x, r0, r1: pred_x(x, r0, r1, col=-1)      # noqa: E731
    for n in (65, 700, 3001):
        x, w = rows_and_weights(n, seed=n + n_dim, d=n_dim)
        mean, var = reference_moments(pred, x, w, R, PREDICT_SUM_LAYOUT)
        xbuf = torch.zeros(g + n_dim * n + g, dtype=torch.float64, device="cuda")
        xbuf[g:g + n_dim * n] = torch.from_numpy(x).cuda().reshape(-1)
        wt = torch.from_numpy(w).cuda()
        words = predict_scratch_words(n, R, len(qs))
        for tile, slab in ((64, 256), (4, 1024)):
            obuf = torch.zeros((2 + len(qs)) * R, dtype=torch.float64, device="cuda")
            sbuf = torch.zeros(words, dtype=torch.int64, device="cuda")
            rc = cb.lib.tphu_predictive(cb._stream(xbuf), xbuf.data_ptr() + 8 * g, wt.data_ptr(), n, R, qs.ctypes.data, len(qs),
                                        obuf.data_ptr(), sbuf.data_ptr(), words, tile, slab)
            assert rc == 0, cb.lib.tphu_last_error()
            res = obuf.cpu().numpy().reshape(2 + len(qs), R)
            np.testing.assert_array_equal(res[0], mean)
            np.testing.assert_array_equal(res[1], var)
            for r in range(R):
                check_quantile_column(pred(x, r, r + 1)[0], w, QS, res[2:, r], Fraction(2 * n, 2 ** 53))
        if shift == 0:
            pp = cb.predictive(x, w, quantiles=QS)
            np.testing.assert_array_equal(pp["mean"], mean)
            np.testing.assert_array_equal(pp["quantiles"], res[2:])


@pytest.mark.gpu
@needs_hipcc
def test_knife_edges_equal_weights_and_ties():
    """Equal weights with q n an integer (the cumulative weight sits ON the target) and indices where every row predicts the same
    value: membership and rank within eps, and the same values at every tile."""
    import tempest_amd as tp
    need_gpu()
    cb = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=12)
    for n in (64, 1000, 3000, 4096):
        x, _ = rows_and_weights(n, seed=n)
        x[: n // 2, :2] = x[0, :2]                                           # half the rows identical: many tied predictions
        for wv in (1.0, 0.3):
            w = np.full(n, wv)
            assert all(float(q * n).is_integer() for q in (0.0, 0.5, 1.0))
            xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
            pp = cb.predictive(xt, wt, quantiles=QS)
            for pin in PINS:
                cb.predict_tile = pin
                np.testing.assert_array_equal(cb.predictive(xt, wt, quantiles=QS)["quantiles"], pp["quantiles"])
            cb.predict_tile = 0
            for r in range(12):
                p = pred_x(x, r, r + 1)[0]
                check_quantile_column(p, w, QS, pp["quantiles"][:, r], Fraction(2 * n, 2 ** 53))
                if r % 5 == 3:
                    assert np.all(pp["quantiles"][:, r] == 0.125 * r)


UNWEIGHTED = [(n, q) for n in (63, 1001, 3001, 70_001) for q in (0.025, 0.5, 0.975, 0.3)]


@pytest.mark.gpu
@needs_hipcc
def test_equal_weights_match_numpy_inverted_cdf():
    import tempest_amd as tp
    need_gpu()
    for n, q in UNWEIGHTED:                                                  # no case on a knife edge: q n is not within eps n of an integer
        assert abs(q * n - round(q * n)) > 2 * n * 2.0 ** -53 * n, (n, q)
    cb = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=40)
    for n in sorted({n for n, _ in UNWEIGHTED}):
        qs = [q for m, q in UNWEIGHTED if m == n]
        x, _ = rows_and_weights(n, seed=n + 1)
        for wv in (1.0, 1.0 / n, 0.7):
            pp = cb.predictive(x, np.full(n, wv), quantiles=qs)
            want = np.percentile(pred_x(x, 0, 40), [100 * q for q in qs], axis=1, method="inverted_cdf")
            np.testing.assert_array_equal(pp["quantiles"], want)


@pytest.mark.gpu
@needs_hipcc
def test_special_inputs():
    import tempest_amd as tp
    from tempest_amd._lib import TempestHipError
    need_gpu()
    n, R = 3001, 9
    x, w = rows_and_weights(n, seed=9)
    cb = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=R)
    pp = cb.predictive(x, w, quantiles=QS)
    zero = np.flatnonzero(w == 0)
    assert len(zero) > 50
    for fill in (np.nan, 1e300, -1e300):                                    # rows without weight: whatever they hold changes nothing
        y = x.copy()
        y[zero] = fill
        other = cb.predictive(y, w, quantiles=QS)
        for key in ("mean", "var", "quantiles"):
            np.testing.assert_array_equal(other[key], pp[key], err_msg=f"{key}, rows without weight set to {fill}")
    # a NaN prediction with positive weight: NaN at that index, and only there
    t = np.linspace(0.0, 1.0, R)
    tn = t.copy()
    tn[2] = np.nan
    ok = tp.HipCallbacks(WHOLE_D + PRED_D, 3, data={"t": t}, n_predict="t").predictive(x, w, quantiles=QS)
    bad = tp.HipCallbacks(WHOLE_D + PRED_D, 3, data={"t": tn}, n_predict="t").predictive(x, w, quantiles=QS)
    keep = np.arange(R) != 2
    for key in ("mean", "var"):
        assert np.isnan(bad[key][2]) and np.all(np.isfinite(ok[key]))
        np.testing.assert_array_equal(bad[key][keep], ok[key][keep])
    assert np.all(np.isnan(bad["quantiles"][:, 2]))
    np.testing.assert_array_equal(bad["quantiles"][:, keep], ok["quantiles"][:, keep])
    # one row; and all the weight on one row among many
    one = cb.predictive(x[5:6], np.array([0.37]), quantiles=QS)
    p5 = pred_x(x[5:6], 0, R)[:, 0]
    np.testing.assert_array_equal(one["mean"], p5)
    assert np.all(one["var"] == 0.0) and one["n_rows"] == 1 and one["ess"] == pytest.approx(1.0)
    np.testing.assert_array_equal(one["quantiles"], np.tile(p5, (len(QS), 1)))
    w1 = np.zeros(n)
    w1[5] = 2.5
    lone = cb.predictive(x, w1, quantiles=QS)
    np.testing.assert_array_equal(lone["mean"], p5)
    assert np.all(lone["var"] == 0.0)
    np.testing.assert_array_equal(lone["quantiles"], one["quantiles"])
    # weights and quantiles that are refused
    for wbad in (np.zeros(n), np.where(np.arange(n) == 3, -1.0, 1.0), np.where(np.arange(n) == 3, np.inf, 1.0),
                 np.where(np.arange(n) == 3, np.nan, 1.0), np.ones(n - 1)):
        with pytest.raises(ValueError):
            cb.predictive(x, wbad)
    for qbad in ((-0.1,), (1.5,), (np.nan,), tuple(np.linspace(0, 1, 9))):
        with pytest.raises(ValueError, match="quantiles"):
            cb.predictive(x, w, quantiles=qbad)
    assert cb.predictive(x, w, quantiles=tuple(np.linspace(0, 1, 8)))["quantiles"].shape == (8, R)
    assert cb.predictive(x, w, quantiles=())["quantiles"].shape == (0, R)
    plain = tp.HipCallbacks(BASE, 3)
    with pytest.raises(TempestHipError, match="no predict"):
        plain.predictive(x, w)
    s = tp.Sampler(plain.prior_transform, plain.log_likelihood, 3, n_particles=256, vectorize=True, random_state=1)
    with pytest.raises(TempestHipError, match="predict"):
        s.predictive()


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("shift", [0, 1])
def test_guard_cells_round_output_and_scratch_and_batches_of_indices(shift):
    """The entry point itself: the output and a scratch buffer of exactly the size the package gives keep their guard cells; a scratch
    that holds 3 indices at a time (batches) gives the same bits.  shift 1: x not 16-byte aligned (8-byte loads)."""
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import predict_scratch_words
    need_gpu()
    R, g = 11, 64 + shift
    cb = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=R)
    qs = np.array(QS)
    fill, ifill = -777.25, 0x5A5A5A5A5A5A5A5A
    for n in (1, 65, 1025, 3001):
        x, w = rows_and_weights(n, seed=n)
        want = cb.predictive(x, w, quantiles=QS)
        xbuf = torch.zeros(g + 3 * n + g, dtype=torch.float64, device="cuda")
        xbuf[g:g + 3 * n] = torch.from_numpy(x).cuda().reshape(-1)
        wt = torch.from_numpy(w).cuda()
        stream = cb._stream(xbuf)
        n_blocks = -(-n // 1024)
        for words in (predict_scratch_words(n, R, len(qs)), 1 + n_blocks + 3 * (n_blocks + 258 * len(qs) + 1)):
            for tile, slab in ((1, 256), (64, 1024)):
                obuf = torch.full((g + (2 + len(qs)) * R + g,), fill, dtype=torch.float64, device="cuda")
                sbuf = torch.full((g + words + g,), ifill, dtype=torch.int64, device="cuda")
                rc = cb.lib.tphu_predictive(stream, xbuf.data_ptr() + 8 * g, wt.data_ptr(), n, R, qs.ctypes.data, len(qs),
                                            obuf.data_ptr() + 8 * g, sbuf.data_ptr() + 8 * g, words, tile, slab)
                assert rc == 0, cb.lib.tphu_last_error()
                o, s = obuf.cpu().numpy(), sbuf.cpu().numpy()
                assert np.all(o[:g] == fill) and np.all(o[-g:] == fill), (n, words, tile)
                assert np.all(s[:g] == ifill) and np.all(s[-g:] == ifill), (n, words, tile)
                res = o[g:-g].reshape(2 + len(qs), R)
                np.testing.assert_array_equal(res[0], want["mean"])
                np.testing.assert_array_equal(res[1], want["var"])
                np.testing.assert_array_equal(res[2:], want["quantiles"])
    # checked arguments
    a = (stream, xbuf.data_ptr(), wt.data_ptr(), 4, R, qs.ctypes.data, len(qs), obuf.data_ptr(), sbuf.data_ptr())
    assert cb.lib.tphu_predictive(*a, 10, 64, 256) == -2 and b"scratch" in cb.lib.tphu_last_error()
    assert cb.lib.tphu_predictive(*a, words, 65, 256) == -2 and cb.lib.tphu_predictive(*a, words, 0, 256) == -2
    assert cb.lib.tphu_predictive(*a, words, 64, 100) == -2
    assert cb.lib.tphu_predictive(stream, None, wt.data_ptr(), 4, R, qs.ctypes.data, len(qs), obuf.data_ptr(), sbuf.data_ptr(), words, 64, 256) == -2
    # the scratch is kept between calls
    cb.predictive(x, w)
    kept = cb._pscratch.data_ptr()
    cb.predictive(x[:100], w[:100])
    assert cb._pscratch.data_ptr() == kept


@pytest.mark.gpu
@needs_hipcc
def test_predictive_respects_the_stream_it_is_given():
    import tempest_amd as tp
    need_gpu()
    a = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=50)
    b = tp.HipCallbacks(BASE + PRED_X, 3, n_predict=50)
    assert a.path == b.path
    x, w = rows_and_weights(200_000, seed=3)
    xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    want = a.predictive(xt, wt)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(4):
        with torch.cuda.stream(sa):
            ya, va = xt * 1.0, wt * 1.0                            # produced on sa: predictive must queue behind them on sa
            ra = a.predictive(ya, va)
        with torch.cuda.stream(sb):
            yb, vb = xt + 0.0, wt + 0.0
            rb = b.predictive(yb, vb)
        outs.append((ra, rb, ya, yb, va, vb))
    torch.cuda.synchronize()
    for ra, rb, *_ in outs:
        for key in ("mean", "var", "quantiles"):
            np.testing.assert_array_equal(ra[key], want[key])
            np.testing.assert_array_equal(rb[key], want[key])


def quad_data(n_terms=200, seed=7):
    rng = np.random.RandomState(seed)
    t = np.linspace(-1.0, 1.0, n_terms)
    s = 0.5 + 0.5 * rng.rand(n_terms)
    return {"t": t, "y": 0.7 + 1.9 * t - 1.1 * t * t + s * rng.randn(n_terms), "s": s}


def run_quad(tp, cb):
    s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=2048, vectorize=True, clustering=False, random_state=11)
    s.run(n_total=4096, progress=False)
    return s


@pytest.mark.gpu
@needs_hipcc
def test_whole_run_band_and_nothing_else_changes(tmp_path):
    import tempest_amd as tp
    need_gpu()
    D = quad_data()
    plain = run_quad(tp, tp.HipCallbacks(QUAD, 3, data=D, n_terms="t"))
    cb = tp.HipCallbacks(QUAD + QUAD_PRED, 3, data=D, n_terms="t", n_predict="t")
    assert cb.n_predict == 200
    s = run_quad(tp, cb)
    # posterior(), evidence() and the run's record are those of the run without predict
    assert s.evidence()[0] == plain.evidence()[0]
    for key in ("steps", "beta", "logz"):
        np.testing.assert_array_equal(np.asarray(s.state.get_history(key)), np.asarray(plain.state.get_history(key)))
    for case in (dict(), dict(trim_importance_weights=False)):
        for got, want in zip(s.posterior(**case), plain.posterior(**case)):
            np.testing.assert_array_equal(got, want)
        x, w, _ = s.posterior(**case)
        pp = s.predictive(quantiles=(0.025, 0.5, 0.975), **case)
        direct = cb.predictive(x, w, quantiles=(0.025, 0.5, 0.975))
        assert pp["n_rows"] == len(x) and pp["ess"] == direct["ess"]
        for key in ("mean", "var", "quantiles"):
            np.testing.assert_array_equal(pp[key], direct[key])
    pp = s.predictive()
    truth = 0.7 + 1.9 * D["t"] - 1.1 * D["t"] ** 2
    inside = np.mean((pp["quantiles"][0] <= truth) & (truth <= pp["quantiles"][2]))
    print(f"generating curve inside the 95 % band at {100 * inside:.1f} % of the abscissae, {pp['n_rows']} rows, ess {pp['ess']:.0f}")
    assert inside >= 0.8
    assert np.all(pp["quantiles"][0] <= pp["quantiles"][1]) and np.all(pp["quantiles"][1] <= pp["quantiles"][2])
    assert np.all(np.abs(pp["mean"] - pp["quantiles"][1]) <= 3 * np.sqrt(pp["var"]))
    for name in ("run.state", "run.ckpt"):
        s.save_state(tmp_path / name)
        t = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=2048, vectorize=True, clustering=False, random_state=11)
        t.load_state(tmp_path / name)
        got = t.predictive()
        x, w, _ = t.posterior()
        again = cb.predictive(x, w)
        for key in ("mean", "var", "quantiles"):
            np.testing.assert_array_equal(got[key], again[key])
            # (the weights are recomputed over the reloaded history and may differ in their last bits)
            np.testing.assert_allclose(got[key], pp[key], rtol=1e-9, atol=1e-12)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
@needs_hipcc
def test_two_ranks_refuse_and_finish(tmp_path):
    need_gpu()
    import tempest_amd as tp
    tp.HipCallbacks(BASE + PRED_X, 3, n_predict=5)                           # compiled once, here: the ranks find it cached
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, "-m", "tests._dist_workers_predict", str(r), "2", str(port), str(tmp_path)], cwd=ROOT)
             for r in (0, 1)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0]
    for r in (0, 1):
        meta = json.load(open(tmp_path / f"predict{r}.json"))
        assert meta["raised"] == "NotImplementedError" and "sharded" in meta["message"] and meta["rows"] > 0 and meta["finished"]

"""Posterior marginals on the device (tempest_amd/marginals.py, csrc/marginals.hip): HipContext.marginals and
Sampler.marginals -- weighted mean, variance, range, 1-D and 2-D histograms and quantiles of every column of the posterior rows.

CPU: every ValueError of plan(), the bin rule against its definition and np.histogram, hpd_levels, the exported symbols and layout
constants, the scratch query.  GPU: every output against a NumPy restatement, bit for bit (assert_array_equal) -- W, mean and var in
MARGINAL_SUM_LAYOUT's order, k = rint(w / W 2^52), bin_index, np.add.at, sort + integer cumsum -- at every row, column and bin edge,
at every pinnable geometry, on special values and weights, with guard cells round every buffer, on two streams, once at 2^20 + 3 rows,
and through a whole run with torch, HipCallbacks and NumPy sources of the columns."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_hipcallbacks_derived import ARITH, BASE, f_arith, needs_hipcc  # noqa: E402

QS = (0.025, 0.16, 0.5, 0.84, 0.975)
TWO52 = 2.0 ** 52


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------- the restatement
def layout_sum(v, layout):
    """Rows of v (c, n) added in the order of MARGINAL_SUM_LAYOUT: chunks of `C` consecutive values by the halving tree v[:h] +
    v[h:2h], blocks of `B` chunk sums in chunk order, the block sums in block order, every level from +0.0."""
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


def restate(v, w, bins=64, rng=None, qs=QS, pairs=None, bins_2d=32):
    """What tph_marginals computes, in NumPy, operation by operation."""
    from tempest_amd.marginals import MARGINAL_SUM_LAYOUT as L, bin_index, plan
    M, c = v.shape
    p = plan(c, bins, rng, qs, pairs, bins_2d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        W = layout_sum(w[None, :], L)[0]
        u = np.where(w > 0, w / W, 0.0)
        k = np.rint(u * TWO52).astype(np.int64)
        vt = np.ascontiguousarray(v.T)
        mean = layout_sum(np.where(u > 0, u * vt, 0.0), L)
        d = vt - mean[:, None]
        var = layout_sum(np.where(u > 0, u * (d * d), 0.0), L)
    if p["range"] is not None:
        r = p["range"].copy()
    else:
        r = np.empty((c, 2))
        for j in range(c):
            fin = v[(w > 0) & np.isfinite(v[:, j]), j]
            lo, hi = (fin.min(), fin.max()) if fin.size else (0.0, 1.0)
            r[j] = (lo - 0.5, hi + 0.5) if (fin.size and lo == hi) else (lo, hi)
    idx = [bin_index(v[:, j], r[j, 0], r[j, 1], bins) for j in range(c)]
    counts, outside = np.zeros((c, bins), dtype=np.int64), np.zeros(c, dtype=np.int64)
    for j in range(c):
        ok = idx[j] >= 0
        np.add.at(counts[j], idx[j][ok], k[ok])
        outside[j] = k[~ok].sum()
    pr = p["pairs"]
    c2, o2 = np.zeros((len(pr), bins_2d, bins_2d), dtype=np.int64), np.zeros(len(pr), dtype=np.int64)
    idx2 = {}
    for n, (a, b) in enumerate(pr):
        for j in (a, b):
            if j not in idx2:
                idx2[j] = bin_index(v[:, j], r[j, 0], r[j, 1], bins_2d)
        ok = (idx2[a] >= 0) & (idx2[b] >= 0)
        np.add.at(c2[n], (idx2[a][ok], idx2[b][ok]), k[ok])
        o2[n] = k[~ok].sum()
    q = np.full((len(p["quantiles"]), c), np.nan)
    sel = k > 0
    for j in range(c):
        vals, kk = v[sel, j], k[sel]
        if vals.size == 0 or np.isnan(vals).any():
            continue
        order = np.argsort(vals, kind="stable")
        cum = np.cumsum(kk[order])
        for n, qq in enumerate(p["quantiles"]):
            T = min(max(int(math.ceil(qq * TWO52)), 1), int(cum[-1]))
            q[n, j] = vals[order][np.searchsorted(cum, T, side="left")]
    return {"mean": mean, "var": var, "quantiles": q, "range": r, "counts": counts, "outside": outside, "counts_2d": c2,
            "outside_2d": o2, "sum_k": int(k.sum()), "k": k}


EXACT = ("mean", "var", "quantiles", "range", "counts", "outside", "counts_2d", "outside_2d")


def check(got, want, v, bins, bins_2d):
    for key in EXACT:
        assert got[key].shape == want[key].shape, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["sum_k"] == want["sum_k"]
    np.testing.assert_array_equal(got["counts"].sum(axis=1) + got["outside"], np.full(v.shape[1], want["sum_k"]))
    if len(got["pairs"]):
        np.testing.assert_array_equal(got["counts_2d"].sum(axis=(1, 2)) + got["outside_2d"], np.full(len(got["pairs"]), want["sum_k"]))
    np.testing.assert_array_equal(got["mass"], got["counts"] * 2.0 ** -52)
    assert got["counts"].dtype == np.int64 and got["counts_2d"].dtype == np.int64
    assert got["edges"].shape == (v.shape[1], bins + 1) and got["edges_2d"].shape == (v.shape[1], bins_2d + 1)
    r = got["range"]
    for key, B in (("edges", bins), ("edges_2d", bins_2d)):       # lo + (hi - lo) * arange(B + 1) / B: for plotting (the last one may miss hi by an ulp)
        np.testing.assert_array_equal(got[key], r[:, :1] + (r[:, 1:] - r[:, :1]) * np.arange(B + 1)[None, :] / B)
    assert got["n_rows"] == v.shape[0]


def values_and_weights(m, c, seed, dyadic_w=False):
    """Ordinary doubles (mean and var are single-rounded operations in a fixed order) with about 5 % of exact-zero weights."""
    rs = np.random.RandomState(seed)
    v = rs.normal(size=(m, c)) * rs.uniform(0.5, 3.0, c) + rs.uniform(-2.0, 2.0, c)
    w = rs.randint(1, 1 << 40, m).astype(np.float64) * 2.0 ** -38 if dyadic_w else rs.uniform(0.1, 3.0, m)
    w[rs.rand(m) < 0.05] = 0.0
    if not np.any(w > 0):
        w[0] = 1.0
    return v, w


@pytest.fixture(scope="module")
def ctx():
    need_gpu()
    from tempest_amd.device import HipContext
    c = HipContext(2, 0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("kw, match", [
    (dict(c=3, bins=0), "bins must be"),
    (dict(c=3, bins=1025), "bins must be"),
    (dict(c=3, bins_2d=0), "bins_2d must be"),
    (dict(c=3, bins_2d=129), "bins_2d must be"),
    (dict(c=3, range=(1.0, 1.0)), "lo < hi"),
    (dict(c=3, range=(2.0, 1.0)), "lo < hi"),
    (dict(c=3, range=(0.0, np.inf)), "finite"),
    (dict(c=3, range=(np.nan, 1.0)), "finite"),
    (dict(c=3, range=np.zeros((2, 2))), "range must be"),
    (dict(c=3, range=(0.0, 1.0, 2.0)), "range must be"),
    (dict(c=3, pairs=[(1, 1)]), "two different columns"),
    (dict(c=3, pairs=[(0, 3)]), "two different columns"),
    (dict(c=3, pairs=[(-1, 2)]), "two different columns"),
    (dict(c=3, pairs="some"), "pairs must be"),
    (dict(c=3, pairs=[(0, 1, 2)]), "pairs must be"),
    (dict(c=3, pairs=[(0.0, 1.0)]), "pairs must be"),
    (dict(c=3, quantiles=np.linspace(0, 1, 9)), "quantiles must be"),
    (dict(c=3, quantiles=(0.5, 1.5)), "quantiles must be"),
    (dict(c=3, quantiles=(-0.1,)), "quantiles must be"),
    (dict(c=0), "columns"),
    (dict(c=129), "columns"),
])
def test_plan_refuses(kw, match):
    from tempest_amd.marginals import plan
    with pytest.raises(ValueError, match=match):
        plan(**kw)


def test_plan_normalises():
    from tempest_amd.marginals import plan
    p = plan(4, 10, (0.0, 2.0), (0.5,), "all", 8)
    assert p["range"].shape == (4, 2) and p["pairs"].dtype == np.int32
    assert [tuple(t) for t in p["pairs"]] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert plan(1, pairs="all")["pairs"].shape == (0, 2) and plan(3)["pairs"].shape == (0, 2) and plan(3, pairs=[])["pairs"].shape == (0, 2)
    assert [tuple(t) for t in plan(3, pairs=[(2, 0)])["pairs"]] == [(2, 0)]
    assert plan(128, 1024, None, np.linspace(0, 1, 8), None, 128)["range"] is None


def test_bin_index_follows_the_rule():
    from tempest_amd.marginals import bin_index
    lo, hi, B = -1.0, 3.0, 16
    v = np.array([lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.nan, np.inf, -np.inf, np.nextafter(hi, -np.inf), 0.0])
    np.testing.assert_array_equal(bin_index(v, lo, hi, B), [0, B - 1, -1, -1, -1, -1, -1, B - 1, 4])
    assert bin_index(0.3, 0.0, 1.0, 1) == 0 and bin_index(1.0, 0.0, 1.0, 1) == 0
    # a value below hi whose t = (v - lo) * inv rounds up to B: the last bin
    rs = np.random.RandomState(0)
    hi = rs.uniform(0.1, 10.0, 4000)
    v = np.nextafter(hi, -np.inf)
    t = (v - 0.0) * (np.float64(7) / (hi - 0.0))
    up = t >= 7
    assert up.any() and (~up).any()
    np.testing.assert_array_equal(bin_index(v[up], 0.0, hi[up], 7), 6)
    # np.histogram on values away from the edges (np.histogram decides a value near an edge by comparing with the edge array)
    v = rs.uniform(-1.0, 3.0, 10000)
    t = (v - lo) * (np.float64(B) / 4.0)
    far = np.abs(t - np.rint(t)) > 1e-9
    assert far.sum() > 9900
    np.testing.assert_array_equal(np.bincount(bin_index(v[far], lo, 3.0, B), minlength=B), np.histogram(v[far], B, (lo, 3.0))[0])


def test_hpd_levels():
    from tempest_amd.marginals import hpd_levels
    t = np.array([[10, 5, 1], [5, 20, 5], [1, 5, 8]])              # 60 in all: 20 | 30 | 38 | 58 | 60 held at t = 20, 10, 8, 5, 1
    np.testing.assert_array_equal(hpd_levels(t, (0.3, 0.5, 0.51, 0.68, 0.95, 0.97)), [20, 10, 8, 5, 5, 1])
    np.testing.assert_array_equal(hpd_levels(t, (0.0, 1.0)), [20, 1])
    np.testing.assert_array_equal(hpd_levels(t), hpd_levels(t, (0.68, 0.95)))
    ties = np.array([4, 4, 4, 4, 0, 0])                            # all or none of the tied bins
    np.testing.assert_array_equal(hpd_levels(ties, (0.0, 0.25, 0.26, 1.0)), [4, 4, 4, 4])
    np.testing.assert_array_equal(hpd_levels(np.array([[3, 3], [2, 2]]), (0.6, 0.61)), [3, 2])
    np.testing.assert_array_equal(hpd_levels(np.zeros((3, 3), dtype=np.int64)), [0, 0])
    # 2^52 + 1 in all: half of it is 2^51 + 1/2, more than the largest bin holds -- in float64 that product rounds to 2^51
    big = np.array([1 << 51, 1 << 50, 1 << 50, 1], dtype=np.int64)
    np.testing.assert_array_equal(hpd_levels(big, (0.25, 0.5, 0.75, 1.0)), [1 << 51, 1 << 50, 1 << 50, 1])
    with pytest.raises(ValueError):
        hpd_levels(np.array([0.5, 1.0]))
    with pytest.raises(ValueError):
        hpd_levels(t, (1.5,))


def test_library_exports_marginals_and_its_constants():
    from tempest_amd import _lib, marginals as mg
    lib = _lib.load()
    for sym in ("tph_marginals", "tph_marginals_layout", "tph_marginals_scratch_words"):
        assert hasattr(lib, sym), sym
    got = tuple(lib.tph_marginals_layout(i) for i in range(8))
    assert got == mg.MARGINAL_SUM_LAYOUT + (mg.MAX_MARGINAL_COLUMNS, mg.MAX_MARGINAL_BINS, mg.MAX_MARGINAL_BINS_2D, mg.MAX_QUANTILES,
                                            mg.MARGINAL_SCRATCH_WORDS, len(mg.MARGINAL_TILE_KEYS))
    assert lib.tph_marginals_layout(8) == -1
    from tempest_amd.hipcallbacks import MAX_QUANTILES, PREDICT_SUM_LAYOUT
    assert mg.MARGINAL_SUM_LAYOUT == PREDICT_SUM_LAYOUT and mg.MAX_QUANTILES == MAX_QUANTILES


def test_scratch_words_grow_with_the_request_and_respect_the_cap():
    from tempest_amd import _lib, marginals as mg
    f = _lib.load().tph_marginals_scratch_words
    base = dict(m=5000, c=10, bins=64, n_pairs=3, bins_2d=32, n_q=5)
    order = ("m", "c", "bins", "n_pairs", "bins_2d", "n_q")
    steps = dict(m=(1, 1024, 1025, 5000, 1 << 20, 1 << 24, 1 << 27), c=(1, 2, 10, 127, 128), bins=(1, 64, 1024), n_pairs=(0, 1, 45, 8128),
                 bins_2d=(1, 32, 128), n_q=(0, 1, 5, 8))
    for name, vals in steps.items():
        words = [f(*[dict(base, **{name: v})[k] for k in order]) for v in vals]
        assert all(w > 0 for w in words) and all(a <= b for a, b in zip(words, words[1:])), (name, words)
    assert f(5000, 10, 64, 45, 32, 5) > f(5000, 10, 64, 0, 32, 5)
    # the batch: whatever c, the part of the scratch that grows with the columns stays under the cap (or is one column)
    for m in (1 << 20, 1 << 24, 1 << 27):
        nblocks = -(-m // 1024)
        per_col = 3 * nblocks + 258 * 8 + 1
        fixed = f(m, 1, 64, 0, 32, 8) - per_col
        assert fixed == 1 + nblocks + 4 * 128
        assert f(m, 128, 64, 0, 32, 8) - fixed == per_col * min(128, max(1, mg.MARGINAL_SCRATCH_WORDS // per_col))
        assert f(m, 128, 64, 0, 32, 8) - fixed <= max(per_col, mg.MARGINAL_SCRATCH_WORDS)
    assert f(1 << 27, 128, 64, 0, 32, 8) < f(1 << 27, 1, 64, 0, 32, 8) * 128
    for bad in ((0, 1, 1, 0, 1, 0), (1, 0, 1, 0, 1, 0), (1, 129, 1, 0, 1, 0), (1, 1, 1025, 0, 1, 0), (1, 1, 1, 1, 129, 0), (1, 1, 1, 0, 1, 9)):
        assert f(*bad) == -1


def test_sampler_has_marginals():
    import inspect
    import tempest_amd as tp
    sig = inspect.signature(tp.Sampler.marginals)
    assert [n for n in sig.parameters][1:] == ["bins", "range", "quantiles", "pairs", "bins_2d", "derived", "trim_importance_weights",
                                               "ess_trim", "bins_trim"]
    assert sig.parameters["bins"].default == 64 and sig.parameters["bins_2d"].default == 32 and sig.parameters["derived"].default is True


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3001])
def test_row_edges(ctx, m):
    v, w = values_and_weights(m, 3, 100 + m)
    got = ctx.marginals(v, w, bins=16, pairs=[(0, 2)])
    check(got, restate(v, w, 16, pairs=[(0, 2)]), v, 16, 32)
    s1, s2 = w.sum(), (w * w).sum()
    assert abs(got["ess"] - s1 * s1 / s2) <= 1e-12 * got["ess"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 2, 10, 17, 33, 64, 127, 128])
def test_column_edges(ctx, c):
    v, w = values_and_weights(777, c, 200 + c)
    pairs = [(0, c - 1), (c - 1, (c - 1) // 2)] if c > 1 else None
    got = ctx.marginals(v, w, pairs=pairs, bins_2d=8)
    check(got, restate(v, w, pairs=pairs, bins_2d=8), v, 64, 8)


@pytest.fixture(scope="module")
def bin_case():
    return values_and_weights(2049, 4, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("bins", [1, 2, 3, 64, 255, 256, 257, 1024])
def test_bin_edges_1d(ctx, bin_case, bins):
    v, w = bin_case
    got = ctx.marginals(v, w, bins=bins, quantiles=(0.5,))
    check(got, restate(v, w, bins, qs=(0.5,)), v, bins, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("bins_2d", [1, 2, 8, 64, 65, 128])
def test_bin_edges_2d_and_the_transpose(ctx, bin_case, bins_2d):
    v, w = bin_case
    pairs = [(0, 1), (1, 0), (3, 2)]
    got = ctx.marginals(v, w, bins=8, quantiles=(), pairs=pairs, bins_2d=bins_2d)
    check(got, restate(v, w, 8, qs=(), pairs=pairs, bins_2d=bins_2d), v, 8, bins_2d)
    assert got["quantiles"].shape == (0, 4)
    np.testing.assert_array_equal(got["counts_2d"][0], got["counts_2d"][1].T)
    assert got["outside_2d"][0] == got["outside_2d"][1]


@pytest.fixture(scope="module")
def tile_case():
    v, w = values_and_weights(3001, 10, 11)
    v[5, 3], v[77, 3], v[300, 9] = np.nan, np.inf, -np.inf
    w[5] = 0.0                                                   # the NaN carries no weight: column 3 keeps its numbers
    return v, w, restate(v, w, pairs="all")


# every geometry the host chooses, pinned (MARGINAL_TILE_KEYS): 1300 words of batch scratch hold one column of this case, 4000 three
PINS = [{}, {"sweep_cols": 1}, {"sweep_cols": 3}, {"sweep_cols": 16}, {"hist_cols": 1}, {"hist_cols": 8}, {"hist_rows": 256},
        {"hist_rows": 1024}, {"hist_rows": 4096}, {"select_cols": 1}, {"select_cols": 3}, {"table_2d": 1}, {"table_2d": 2}, {"rows_2d": 256},
        {"rows_2d": 2048}, {"batch_words": 1300}, {"batch_words": 4000},
        {"sweep_cols": 5, "hist_cols": 3, "hist_rows": 512, "select_cols": 2, "table_2d": 1, "rows_2d": 768, "batch_words": 9000}]


@pytest.mark.gpu
@pytest.mark.parametrize("pin", PINS, ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()) or "auto")
def test_every_geometry_gives_the_same_bits(ctx, tile_case, pin):
    v, w, want = tile_case
    ctx.marginals_tile = pin
    try:
        got = ctx.marginals(v, w, pairs="all")
    finally:
        ctx.marginals_tile = None
    check(got, want, v, 64, 32)
    assert len(got["pairs"]) == 45


@pytest.mark.gpu
def test_bad_pins_are_errors(ctx):
    from tempest_amd._lib import TempestHipError
    v, w = values_and_weights(100, 3, 1)
    for pin in ({"sweep_cols": 17}, {"hist_cols": 9}, {"hist_rows": 100}, {"select_cols": 4}, {"table_2d": 3}, {"batch_words": (1 << 23) + 1}):
        ctx.marginals_tile = pin
        try:
            with pytest.raises(TempestHipError):
                ctx.marginals(v, w, pairs="all")
        finally:
            ctx.marginals_tile = None
    ctx.marginals_tile = {"hist_cols": 8}                         # 8 tables of 1025 cells do not fit
    try:
        with pytest.raises(TempestHipError):
            ctx.marginals(v, w, bins=1024)
    finally:
        ctx.marginals_tile = None
    with pytest.raises(ValueError):
        ctx.marginals(v, -w)
    with pytest.raises(ValueError):
        ctx.marginals(v, w[:-1])
    with pytest.raises(ValueError):
        ctx.marginals(v, w, bins=0)


@pytest.mark.gpu
def test_explicit_dyadic_range_edges_and_outside(ctx):
    # lo = -2, hi = 6, 16 bins of width 1/2: values at lo, at hi, at interior edges, next to them, and outside
    edges = -2.0 + 0.5 * np.arange(17)
    col = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-2.5, 6.5, 1e300, -1e300]])
    rs = np.random.RandomState(3)
    v = np.stack([col, rs.permutation(col), col[::-1]], axis=1)
    w = rs.randint(1, 1 << 20, len(col)).astype(np.float64) * 2.0 ** -10
    rng = np.array([[-2.0, 6.0], [-2.0, 6.0], [-4.0, 4.0]])
    got = ctx.marginals(v, w, bins=16, range=rng, pairs="all", bins_2d=16)
    want = restate(v, w, 16, rng, pairs="all", bins_2d=16)
    check(got, want, v, 16, 16)
    k = want["k"]
    assert got["counts"][0, 0] == k[0] + k[34] + k[18] and got["counts"][0, 15] == k[15] + k[16] + k[33] + k[49]      # lo .. the next edge-; the last edge .. hi
    assert got["outside"][0] == k[17] + k[50] + k[51:].sum()                                                  # lo-, hi+, the four beyond
    got1 = ctx.marginals(v, w, bins=16, range=(-2.0, 6.0))
    np.testing.assert_array_equal(got1["counts"][:2], got["counts"][:2])
    np.testing.assert_array_equal(got1["range"], np.tile([-2.0, 6.0], (3, 1)))


@pytest.mark.gpu
def test_nan_and_infinities_with_and_without_weight(ctx):
    v0, w0 = values_and_weights(700, 4, 21)
    w0[[10, 20, 30]] = 1.0
    clean = ctx.marginals(v0, w0, pairs="all")
    v = v0.copy()
    v[10, 1], v[20, 2], v[30, 2] = np.nan, np.inf, -np.inf
    got = ctx.marginals(v, w0, pairs="all")
    want = restate(v, w0, pairs="all")
    check(got, want, v, 64, 32)
    assert np.isnan(got["mean"][1]) and np.isnan(got["var"][1]) and np.isnan(got["quantiles"][:, 1]).all()
    assert np.isnan(got["mean"][2]) and np.isfinite(got["quantiles"][1:-1, 2]).all() and np.isfinite(got["range"]).all()
    assert got["outside"][1] == want["k"][10] and got["outside"][2] == want["k"][20] + want["k"][30]
    for key in ("mean", "var", "quantiles", "outside"):                           # the other columns: untouched
        np.testing.assert_array_equal(got[key][..., [0, 3]], clean[key][..., [0, 3]], err_msg=key)
    np.testing.assert_array_equal(got["counts"][[0, 3]], clean["counts"][[0, 3]])
    np.testing.assert_array_equal(got["counts_2d"][2], clean["counts_2d"][2])     # the pair (0, 3)
    # q = 0 and q = 1 reach the infinities of column 2 (they take part by their order)
    ends = ctx.marginals(v, w0, quantiles=(0.0, 1.0))["quantiles"]
    assert ends[0, 2] == -np.inf and ends[1, 2] == np.inf and ends[0, 0] == v0[w0 > 0, 0].min() and ends[1, 0] == v0[w0 > 0, 0].max()
    # the same three values without weight: no effect at all
    w = w0.copy()
    w[[10, 20, 30]] = 0.0
    v_ok = v0.copy()
    v_ok[[10, 20, 30]] = 0.25
    a, b = ctx.marginals(v, w, pairs="all"), ctx.marginals(v_ok, w, pairs="all")
    check(a, restate(v, w, pairs="all"), v, 64, 32)
    for key in EXACT:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.gpu
def test_constant_and_empty_columns_one_heavy_row_tiny_weights_and_ties(ctx):
    rs = np.random.RandomState(5)
    m = 1500
    v = rs.normal(size=(m, 5))
    v[:, 1] = 3.25                                                # constant: range 3.25 -+ 0.5
    v[:, 2] = np.where(rs.rand(m) < 0.5, np.nan, np.inf)         # no finite value with weight: range [0, 1], all outside
    v[:, 3] = rs.randint(0, 4, m) * 0.5                          # heavy ties
    w = rs.uniform(0.5, 1.5, m)
    w[::7] = 1e-17                                                # k == 0 beside u > 0: absent from counts and quantiles
    w[3] = 0.0
    got = ctx.marginals(v, w, bins=8, quantiles=(0.0, 0.3, 0.5, 1.0), pairs=[(0, 3), (1, 2)], bins_2d=4)
    want = restate(v, w, 8, qs=(0.0, 0.3, 0.5, 1.0), pairs=[(0, 3), (1, 2)], bins_2d=4)
    check(got, want, v, 8, 4)
    assert (want["k"][::7] == 0).all() and want["sum_k"] == want["k"].sum()
    np.testing.assert_array_equal(got["range"][1], [2.75, 3.75])
    np.testing.assert_array_equal(got["range"][2], [0.0, 1.0])
    assert got["counts"][2].sum() == 0 and got["outside"][2] == want["sum_k"] and got["outside_2d"][1] == want["sum_k"]
    assert got["mean"][1] == pytest.approx(3.25, rel=1e-14) and got["counts"][1, 4] == want["sum_k"]
    assert set(got["quantiles"][:, 3]) <= {0.0, 0.5, 1.0, 1.5}
    # all the weight on one row: mean = v exactly, var = 0, every quantile that row
    w1 = np.zeros(m)
    w1[777] = 0.37
    one = ctx.marginals(v[:, [0, 3]], w1, bins=8)
    check(one, restate(v[:, [0, 3]], w1, 8), v[:, [0, 3]], 8, 32)
    np.testing.assert_array_equal(one["mean"], v[777, [0, 3]])
    np.testing.assert_array_equal(one["var"], [0.0, 0.0])
    np.testing.assert_array_equal(one["quantiles"], np.tile(v[777, [0, 3]], (5, 1)))
    assert one["sum_k"] == 1 << 52 and one["ess"] == pytest.approx(1.0)
    np.testing.assert_array_equal(one["range"], np.stack([v[777, [0, 3]] - 0.5, v[777, [0, 3]] + 0.5], axis=1))


def raw_marginals(ctx, v, w, bins, qs, pairs, bins_2d, guard=128):
    """tph_marginals called directly on buffers with guard cells on both sides: (outputs, {name: the guards kept their fill})."""
    import ctypes as C
    from tempest_amd.marginals import plan
    m, c = v.shape
    p = plan(c, bins, None, qs, pairs, bins_2d)
    nq, pr = len(p["quantiles"]), p["pairs"]
    dev = ctx.device
    vd, wd = torch.from_numpy(v).to(dev), torch.from_numpy(w).to(dev)
    words = int(ctx.lib.tph_marginals_scratch_words(m, c, bins, len(pr), bins_2d, nq))
    shapes = {"moments": ((2, c), torch.float64), "range": ((c, 2), torch.float64), "quant": ((nq, c), torch.float64),
              "counts": ((c, bins), torch.int64), "outside": ((c,), torch.int64), "counts2": ((len(pr), bins_2d, bins_2d), torch.int64),
              "outside2": ((len(pr),), torch.int64), "sumk": ((1,), torch.int64), "scratch": ((words,), torch.int64)}
    bufs = {}
    for name, (shape, dt) in shapes.items():
        fill = -777.25 if dt == torch.float64 else -7777
        bufs[name] = torch.full((int(np.prod(shape)) + 2 * guard,), fill, dtype=dt, device=dev)
    ptr = {name: C.c_void_p(t.data_ptr() + 8 * guard) for name, t in bufs.items()}
    ctx.use_current_stream()
    rc = ctx.lib.tph_marginals(ctx._ctx, vd.data_ptr(), m, c, wd.data_ptr(), None, bins, pr.ctypes.data_as(C.c_void_p), len(pr), bins_2d,
                               p["quantiles"].ctypes.data_as(C.c_void_p), nq, None, ptr["scratch"], words, ptr["moments"], ptr["range"],
                               ptr["quant"], ptr["counts"], ptr["outside"], ptr["counts2"], ptr["outside2"], ptr["sumk"])
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    out, kept = {}, {}
    for name, (shape, dt) in shapes.items():
        t = bufs[name].cpu().numpy()
        fill = -777.25 if dt == torch.float64 else -7777
        kept[name] = bool((t[:guard] == fill).all() and (t[len(t) - guard:] == fill).all())
        out[name] = t[guard:len(t) - guard].reshape(shape)
    return out, kept


@pytest.mark.gpu
@pytest.mark.parametrize("m, c, bins, bins_2d", [(1, 1, 1, 1), (1025, 3, 16, 8), (3001, 10, 1024, 65), (777, 128, 7, 128)])
def test_guard_cells_keep_their_fill(ctx, m, c, bins, bins_2d):
    v, w = values_and_weights(m, c, 31 + m)
    pairs = [(0, c - 1), (c - 1, 0)] if c > 1 else None
    out, kept = raw_marginals(ctx, v, w, bins, QS, pairs, bins_2d)
    assert all(kept.values()), kept
    want = restate(v, w, bins, pairs=pairs, bins_2d=bins_2d)
    for name, key in (("range", "range"), ("quant", "quantiles"), ("counts", "counts"), ("outside", "outside"), ("counts2", "counts_2d"),
                      ("outside2", "outside_2d")):
        np.testing.assert_array_equal(out[name], want[key], err_msg=name)
    np.testing.assert_array_equal(out["moments"], np.stack([want["mean"], want["var"]]))
    assert out["sumk"][0] == want["sum_k"]


@pytest.mark.gpu
def test_two_streams_two_contexts(ctx):
    from tempest_amd.device import HipContext
    other = HipContext(3, 0)
    try:
        cases = [values_and_weights(5000, 6, 41), values_and_weights(4097, 6, 42)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = []
        for rep in range(2):
            for cx, st, (v, w) in zip((ctx, other), streams, cases):
                with torch.cuda.stream(st):
                    got.append(cx.marginals(torch.from_numpy(v).to(cx.device), torch.from_numpy(w).to(cx.device), pairs=[(0, 5)]))
        torch.cuda.synchronize()
        for n, g in enumerate(got):
            v, w = cases[n % 2]
            check(g, restate(v, w, pairs=[(0, 5)]), v, 64, 32)
    finally:
        other.close()


@pytest.mark.gpu
def test_one_large_case(ctx):
    """(1 << 20) + 3 rows x 10 columns with the default geometry: cross-workgroup atomics, 1025 row blocks.  The weights are 40-bit
    integers times 2^-38, as in the predictive test."""
    m = (1 << 20) + 3
    v, w = values_and_weights(m, 10, 51, dyadic_w=True)
    pairs = [(0, 1), (8, 9)]
    got = ctx.marginals(v, w, pairs=pairs)
    check(got, restate(v, w, pairs=pairs), v, 64, 32)


def gauss2(tp, **kw):
    mean = torch.tensor([0.5, -1.0], dtype=torch.float64, device="cuda")
    s = tp.Sampler(lambda u: 10 * u - 5, lambda x: -0.5 * (((x - mean) / 0.7) ** 2).sum(dim=1), 2, n_particles=1024, vectorize=True,
                   clustering=False, random_state=3, **kw)
    s.run(n_total=2048, progress=False)
    return s


@pytest.mark.gpu
def test_sampler_marginals_match_the_posterior_rows():
    import tempest_amd as tp
    need_gpu()
    s = gauss2(tp)
    got = s.marginals(pairs="all")
    x, w, _ = s.posterior()
    assert got["n_dim"] == 2 and got["n_derived"] == 0 and got["n_rows"] == len(x) and [tuple(p) for p in got["pairs"]] == [(0, 1)]
    check(got, restate(x, w, pairs="all"), x, 64, 32)            # the same rows and weights on both sides: every bit
    # against np.average: 1e-12 relative is the order-of-summation bound -- np.average adds the ~10^3 terms in another order (each
    # order is good to n 2^-53 of sum |u x|, a few times |mean| here), and posterior()'s weights are already normalised by a
    # different sum than the W the kernels divide by
    np.testing.assert_allclose(got["mean"], np.average(x, axis=0, weights=w), rtol=1e-12, atol=0.0)
    assert abs(got["mean"][0] - 0.5) < 0.2 and abs(got["mean"][1] + 1.0) < 0.2 and np.all(np.abs(got["var"] - 0.49) < 0.2)
    assert got["ess"] == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-12)
    from tempest_amd.marginals import hpd_levels
    lv = hpd_levels(got["counts_2d"][0])
    assert lv[0] >= lv[1] > 0
    # the untrimmed selection, and a derived= NumPy function on torch callbacks (the host route: evaluated on the host, uploaded)
    s2 = gauss2(tp, derived=lambda x: np.stack([x[:, 0] + x[:, 1], x[:, 0] * x[:, 1]], axis=1) if isinstance(x, np.ndarray)
                else torch.stack([x[:, 0] + x[:, 1], x[:, 0] * x[:, 1]], dim=1))
    for trim in (True, False):
        x, w, _, blobs = s2.posterior(return_blobs=True, trim_importance_weights=trim)
        got = s2.marginals(bins=32, trim_importance_weights=trim)
        assert got["n_dim"] == 2 and got["n_derived"] == 2 and got["counts"].shape == (4, 32)
        full = np.concatenate([x, blobs], axis=1)
        check(got, restate(full, w, 32), full, 32, 32)
        plain = s2.marginals(bins=32, derived=False, trim_importance_weights=trim)
        assert plain["n_derived"] == 0 and plain["counts"].shape == (2, 32)
        np.testing.assert_array_equal(plain["counts"], got["counts"][:2])


@pytest.mark.gpu
@needs_hipcc
def test_sampler_marginals_with_hipcallbacks_and_numpy_derived():
    import tempest_amd as tp
    need_gpu()
    d, k = 4, 2
    cb = tp.HipCallbacks(BASE + ARITH, d, n_derived=k)
    s = tp.Sampler(cb.prior_transform, cb.log_likelihood, d, n_particles=512, vectorize=True, clustering=False, random_state=4)
    s.run(n_total=2048, progress=False)
    x, w, _, blobs = s.posterior(return_blobs=True)
    got = s.marginals(pairs=[(0, 5), (4, 1)], bins_2d=16)
    assert got["n_dim"] == d and got["n_derived"] == k and got["mean"].shape == (d + k,)
    np.testing.assert_array_equal(blobs, f_arith(x, k))
    full = np.concatenate([x, blobs], axis=1)
    check(got, restate(full, w, pairs=[(0, 5), (4, 1)], bins_2d=16), full, 64, 16)
    plain = s.marginals(derived=False)
    assert plain["n_derived"] == 0 and plain["counts"].shape == (d, 64)
    np.testing.assert_array_equal(plain["counts"], got["counts"][:d])
    with pytest.raises(ValueError):
        s.marginals(pairs=[(0, d + k)])
    # NumPy callbacks and a NumPy derived function
    mh = np.linspace(-1, 1, d)
    s2 = tp.Sampler(lambda u: 10 * u - 5, lambda x: -0.5 * ((x - mh) ** 2).sum(axis=1), d, n_particles=256, vectorize=True,
                    clustering=False, random_state=2, backend="numpy", derived=lambda x: f_arith(x, 2))
    s2.run(n_total=512, progress=False)
    x, w, _, blobs = s2.posterior(return_blobs=True)
    got = s2.marginals(bins=16)
    full = np.concatenate([x, blobs], axis=1)
    assert got["n_derived"] == 2
    check(got, restate(full, w, 16), full, 16, 32)

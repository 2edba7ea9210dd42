"""Posterior marginals: the host pieces of `HipContext.marginals` / `Sampler.marginals` -- the validation of
a request, the NumPy restatement of the bin rule, and the contour heights of a corner plot.  Nothing here needs a GPU.

The constants are design constants of csrc/marginals.hip (`tph_marginals_layout` answers the same numbers)."""
from fractions import Fraction

import numpy as np

from ._lib import CONSTANTS

# the order of every floating-point sum over rows: chunks of 64 consecutive rows by the halving tree v[:h] + v[h:2h], blocks of 16
# chunk sums in chunk order, block sums in block order, every level from +0.0 (PREDICT_SUM_LAYOUT's order)
MARGINAL_SUM_LAYOUT = (64, 16)
MAX_MARGINAL_COLUMNS = 128
MAX_MARGINAL_BINS = 1024
MAX_MARGINAL_BINS_2D = 128
MAX_QUANTILES = 8
MARGINAL_SCRATCH_WORDS = 1 << 23   # 64 MiB of batch scratch at most: more columns than fit go through in batches
# the geometry a call may pin (HipContext.marginals_tile: a dict of some of these; 0 / absent = the library's rule), in the order of
# tph_marginals' tiles_host: columns per workgroup of the moment sweeps (<= 16), of the 1-D histogram (<= 8, tile x (bins + 1) <=
# 4100), rows per workgroup of the 1-D histogram and the select (a multiple of 256), columns per workgroup of the select (tile x
# n_q <= 16), the 2-D table (1 = global atomics, 2 = LDS, bins_2d <= 64), rows per workgroup of the 2-D histogram, words of batch scratch
MARGINAL_TILE_KEYS = ("sweep_cols", "hist_cols", "hist_rows", "select_cols", "table_2d", "rows_2d", "batch_words")
assert len(MARGINAL_TILE_KEYS) == CONSTANTS["TPH_MARGINALS_TILES"]
DEFAULT_QUANTILES = (0.025, 0.16, 0.5, 0.84, 0.975)


def plan(c, bins=64, range=None, quantiles=DEFAULT_QUANTILES, pairs=None, bins_2d=32):
    """Every check of a marginals request, before anything is launched: ValueError, or a dict with `c`, `bins`, `bins_2d`, `range`
    (None, or a (c, 2) float64 array), `quantiles` (float64 array) and `pairs` ((P, 2) int32 array; "all" = every a < b)."""
    def as_int(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"marginals: {what} must be an int, got {v!r}")
        return int(v)
    c = as_int(c, "the number of columns")
    if not 1 <= c <= MAX_MARGINAL_COLUMNS:
        raise ValueError(f"marginals: 1 .. {MAX_MARGINAL_COLUMNS} columns, got {c}")
    bins = as_int(bins, "bins")
    if not 1 <= bins <= MAX_MARGINAL_BINS:
        raise ValueError(f"marginals: bins must be 1 .. {MAX_MARGINAL_BINS}, got {bins}")
    bins_2d = as_int(bins_2d, "bins_2d")
    if not 1 <= bins_2d <= MAX_MARGINAL_BINS_2D:
        raise ValueError(f"marginals: bins_2d must be 1 .. {MAX_MARGINAL_BINS_2D}, got {bins_2d}")
    if range is not None:
        r = np.asarray(range, dtype=np.float64)
        if r.shape == (2,):
            r = np.tile(r, (c, 1))
        if r.shape != (c, 2):
            raise ValueError(f"marginals: range must be (lo, hi) or a ({c}, 2) array, got shape {r.shape}")
        with np.errstate(over="ignore", invalid="ignore"):
            ok = np.isfinite(r).all() and (r[:, 0] < r[:, 1]).all() and np.isfinite(r[:, 1] - r[:, 0]).all()
        if not ok:
            raise ValueError("marginals: every range must be finite with lo < hi (and a finite width)")
        range = np.ascontiguousarray(r)
    qs = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if qs.ndim != 1 or len(qs) > MAX_QUANTILES or not np.all((qs >= 0.0) & (qs <= 1.0)):
        raise ValueError(f"marginals: quantiles must be at most {MAX_QUANTILES} numbers in [0, 1], got {quantiles!r}")
    if pairs is None:
        pr = np.empty((0, 2), dtype=np.int32)
    elif isinstance(pairs, str):
        if pairs != "all":
            raise ValueError(f"marginals: pairs must be None, \"all\" or a sequence of index pairs, got {pairs!r}")
        pr = np.array([(a, b) for a in np.arange(c) for b in np.arange(a + 1, c)], dtype=np.int32).reshape(-1, 2)
    else:
        try:
            pa = np.asarray(pairs)
        except ValueError:
            pa = None
        if pa is not None and pa.size == 0:
            pa = np.empty((0, 2), dtype=np.int64)
        if pa is None or pa.ndim != 2 or pa.shape[1] != 2 or pa.dtype.kind not in "iu":
            raise ValueError(f"marginals: pairs must be a sequence of (a, b) column indices, got {pairs!r}")
        if pa.size and (pa.min() < 0 or pa.max() >= c or np.any(pa[:, 0] == pa[:, 1])):
            raise ValueError(f"marginals: every pair must be two different columns in 0 .. {c - 1}, got {pairs!r}")
        pr = np.ascontiguousarray(pa, dtype=np.int32)
    if len(pr) > 65535:
        raise ValueError(f"marginals: at most 65535 pairs, got {len(pr)}")
    return {"c": c, "bins": bins, "bins_2d": bins_2d, "range": range, "quantiles": qs, "pairs": pr}


def bin_index(v, lo, hi, B):
    """The bin rule of the histograms, restated: t = (v - lo) * inv with inv = B / (hi - lo), two separately rounded operations, b =
    (int64) t truncated; v == hi and a b that reaches B go to the last bin; v < lo, v > hi, NaN and +-inf give -1 (outside).
    v, lo, hi broadcast against each other."""
    v = np.asarray(v, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        inv = np.float64(B) / (hi - lo)
        inside = (v >= lo) & (v <= hi)
        t = (v - lo) * inv
        low = inside & (t < B)
        b = np.where(low, t, 0.0).astype(np.int64)
    b = np.where(low & (v != hi), b, B - 1)
    return np.where(inside, b, -1).astype(np.int64)


def edges(range_, B):
    """edges[j] = lo + (hi - lo) * arange(B + 1) / B per column: for plotting (the bin rule is bin_index)."""
    r = np.asarray(range_, dtype=np.float64).reshape(-1, 2)
    return r[:, :1] + (r[:, 1:] - r[:, :1]) * np.arange(B + 1, dtype=np.float64)[None, :] / B


def hpd_levels(counts, levels=(0.68, 0.95)):
    """The contour heights of a corner plot from a table of integer counts (1-D or 2-D): for each level the largest count threshold t,
    at most the table's largest count, such that the bins with count >= t hold at least `level` of the table's (in-range) mass.
    Integer arithmetic on the counts, the level taken as the exact rational of its float.  An empty table gives 0."""
    cnt = np.asarray(counts)
    if cnt.dtype.kind not in "iu":
        raise ValueError("hpd_levels: integer counts expected")
    flat = np.sort(cnt.reshape(-1).astype(np.int64))[::-1]
    if flat.size and flat[-1] < 0:
        raise ValueError("hpd_levels: negative count")
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError(f"hpd_levels: levels must lie in [0, 1], got {levels!r}")
    total = int(flat.sum()) if flat.size else 0
    out = np.zeros(len(lv), dtype=np.int64)
    if total == 0:
        return out
    vals, first = np.unique(-flat, return_index=True)        # distinct counts, largest first; where each starts in `flat`
    vals = -vals
    cum = np.cumsum(flat)
    upto = np.append(first[1:], flat.size) - 1               # the last cell with count >= vals[i]
    held = [int(cum[u]) for u in upto]                       # mass of the bins with count >= vals[i]
    for n, level in enumerate(lv):
        fr = Fraction(float(level))
        for t, h in zip(vals, held):
            if t > 0 and h * fr.denominator >= fr.numerator * total:
                out[n] = int(t)
                break
    return out

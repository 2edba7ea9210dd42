"""Inputs and exact references for the weighted sums and second moments of csrc/modes.hip: k_wsum, k_wsum_final, k_colsum2,
k_colsum2_wide, k_fold_cols, k_mean_from_sums, k_wcov_small, k_wcov, k_wcov_tiled, k_wcov_mfma, k_wmom_small, k_wmom_finish,
k_cov_finish and k_cv_sum.  CPU only, NumPy only: shared by tests/test_moment_cases.py (which checks the references against
independent formulations and the claims below) and tests/test_moments_gpu.py (which holds the device to them bit for bit).

Why the comparison needs no tolerance.  These kernels only add products.  The inputs sit on dyadic lattices chosen so that every
product and every partial sum, in ANY order, is an integer multiple of one unit and smaller than 2^53 units: then no operation
rounds, with or without FMA, on the vector units or the matrix cores, for any number of blocks, slices or shards, and the result
is the exact sum.  Each reference states its unit, computes in integers (or in float64 under the same asserted budget, where it
is exact for the same reason) and asserts its BIT BUDGET: the sum of the ABSOLUTE terms in units -- an upper bound on every
partial sum of every order -- stays below 2^53, and so do the exact operations that follow (the divisions by a power of two,
the fit's v + v / n, the shifted form's S2 / S0 - (S1 / S0)^2).

Lattices.
  u        multiples of 2^-B in [0, 1]; weighted rows use 2 .. 2^B - 2, so that rows 1 and 2 (all coordinates 1 / 2^B and
           (2^B - 1) / 2^B) lie beyond them: with weight zero they must not show in the range output of tph_x_weighted_sums.
  weights  k / 16 with k in 0 .. 15 (counts: small integers); about 30 % zero; row 0 and every row of the last tile of 64 rows
           carry weight, so dropping, repeating or mis-weighting one (row, a, b) term changes that entry.
  centres  odd multiples of 2^-(B+1): a centred coordinate is never zero.
  device mean (tph_weighted_moments, _shifted, tph_fit_modes): the integer weights sum to 2^P (per label for the fit), so the
           mean S1 / S0 is a multiple of 2^-(B+P) and the normalisations are exact.
"""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
LIMIT = 1 << 53
TILE = 64                       # COV_ROWS: rows of one staged tile of k_wcov / k_wcov_tiled / k_wcov_mfma, lanes of k_cv_sum

B = 8                           # u lattice of the sums and the centred second moments
B_FIT = 4                       # ... of the proposal fit (its diagonal v + v / n needs bits(v) + log2 n <= 53)
P_FIT = 10                      # the fit's counts sum to 2^10 per label
B_CV = 2                        # ... of the tph_cv_sum cases
WDEN = 16                       # real weights are k / 16

# ------------------------------------------------------------------------------------------------- dimensions and rows
# Each with the branch it pins (read from modes.hip, not measured).
D_SMALL = tuple(range(1, 17))   # 1..12: k_wcov_small<WT, D> and k_wmom_small<D>, one instantiation each; 13, 14, 15: k_wcov,
#                                 a pair per thread, cov_slices(npl) = 2 row slices (npl = 91, 105, 120); 16: the tiled / MFMA pair
D_SLICES = (17, 20,             # cov_tile_slices (tile_slices below): 5 block rows of 4, 15 block pairs -> 16 row slices, as at 16
            21, 24, 25, 28,     # 6 | 7 block rows, 21 | 28 pairs -> 8 slices (first and last d of each block row count)
            29, 32,             # 8 block rows, 36 pairs -> 4 slices; 32 is the last d of the NV = 8 fill (next tile in registers)
            33, 40,             # 9 .. 10 block rows -> 4 slices; the NV = 0 fill (tile by tile) begins at 33
            41, 60,             # 11 .. 15 block rows, 66 .. 120 pairs -> 2 slices
            61, 64,             # 16 block rows, 136 pairs -> 1 slice: no LDS triangle, every thread stores its own block
            65, 88,             # up to 22 block rows, 253 pairs: the last d with one item per thread
            89)                 # 23 block rows, 276 pairs: a thread owns two block pairs
TILE_SLICES = {16: 16, 17: 16, 20: 16, 21: 8, 24: 8, 25: 8, 28: 8, 29: 4, 32: 4, 33: 4, 40: 4, 41: 2, 60: 2, 61: 1, 64: 1,
               65: 1, 88: 1, 89: 1, 100: 1}
D_WIDE = (22, 23)               # npl = 253 | 276: k_colsum2 | k_colsum2_wide (ncol > 256 and <= 256 partial rows)
D_LIMIT = (97, 99, 100)         # 25 block rows with 1, 3 and 4 live rows in the last; 100 is the largest n_dim served
D_MFMA = (31, 47, 48, 49, 80, 81, 96)   # 16-blocks of k_wcov_mfma: 2 | 3 | 3 | 4 | 5 | 6 | 6 block rows, full and ragged
ALL_D = tuple(sorted(set(D_SMALL + D_SLICES + D_WIDE + D_LIMIT + D_MFMA)))

SMALL_N = (1, 63, 64, 65, 2397)          # one row | one ragged tile | one full tile | a tile and one row | 37 tiles + 29 rows
LARGE_N = {131137: (13, 16, 23, 33, 100),   # 2050 tiles over 2048 blocks: two blocks take a second tile, the last is ragged (1 row);
           #                                  2048 partial rows and more: k_colsum2 also where ncol > 256
           393221: (1, 7, 12),              # > 2 * 768 * 256 rows: second trip of k_wcov_small's two-rows-in-flight loop at its cap
           524291: (1, 3)}                  # > 4 * 512 * 256 rows: second trip of k_wsum's four-rows-in-flight loop at its cap
MOMENT_N = SMALL_N                          # device-mean entry points: the budget 3 P + 2 B < 53 ends at P = 12 (see pow2_weights)
FIT_D = (5, 12, 13, 15, 16, 21, 29, 41, 61, 89, 100)
FIT_N = 2397
CV_D = (1, 2, 13, 16, 64, 100)
CV_LARGE_N = {262149: (2,)}                 # 4097 tiles over k_cv_sum's 4096 blocks: block 0 takes a second tile, ragged (5 rows)
MAX_D = 100


def pair_slices(d):
    """cov_slices(npl) of modes.hip, restated: row slices of k_wcov (13 <= d <= 15)."""
    npl, s = d * (d + 1) // 2, 1
    while s < 16 and npl * s * 2 <= 256:
        s *= 2
    return s


def tile_slices(d):
    """cov_tile_slices of modes.hip, restated."""
    nbk = (d + 3) // 4
    pairs, sl = nbk * (nbk + 1) // 2, 1
    while sl < 16 and pairs * sl * 2 <= 256:
        sl *= 2
    return sl


def rows_for(d):
    return SMALL_N + tuple(n for n, ds in sorted(LARGE_N.items()) if d in ds)


def cv_rows_for(d):
    return SMALL_N + tuple(n for n, ds in sorted(CV_LARGE_N.items()) if d in ds)


def forced_rows(n):
    """Rows that must carry weight: row 0 and the rows of the last tile."""
    f = np.zeros(n, dtype=bool)
    f[0] = True
    f[TILE * ((n - 1) // TILE):] = True
    return f


# ------------------------------------------------------------------------------------------------------ inputs
Lattice = namedtuple("Lattice", "d b k c2")      # k[n][d] integers: u = k / 2^b;  c2[d] odd: centre = c2 / 2^(b+1)


@functools.lru_cache(maxsize=4)
def lattice(d, n, b=B, seed=0):
    """n rows of the lattice for dimension d (the longest row count of d; shorter cases use its first rows)."""
    rs = np.random.RandomState(1000 * d + b + seed)
    top = 1 << b
    k = rs.randint(2, top - 1, size=(n, d)).astype(np.int64) if top > 4 else rs.randint(0, top + 1, size=(n, d)).astype(np.int64)
    if top > 4 and n > 2:
        k[1], k[2] = 1, top - 1
    c2 = 2 * rs.randint(3 * top // 8, 5 * top // 8 + (top <= 4), size=d).astype(np.int64) + 1
    k.setflags(write=False)
    c2.setflags(write=False)
    return Lattice(d, b, k, c2)


def u_of(lat, n=None):
    return lat.k[:n].astype(np.float64) / float(1 << lat.b)


def centre_of(lat):
    return lat.c2.astype(np.float64) / float(1 << (lat.b + 1))


def weights(d, n, kmax=15, seed=0):
    """Integer weights 0 .. kmax, about 30 % zero, none zero on forced_rows(n); rows 1 and 2 (the range rows) zero where allowed."""
    rs = np.random.RandomState(7919 * d + n % 100003 + seed)
    kw = rs.randint(1, kmax + 1, size=n).astype(np.int64)
    zero = rs.rand(n) < 0.3
    zero[1:3] = True
    kw[zero & ~forced_rows(n)] = 0
    return kw


def pow2_weights(d, n, seed=0, labels=None, K=1, P=None, kmax=3):
    """Integer weights as weights(), raised so that they sum to a power of two 2^P (per label): -> (kw, P).  The deficit is
    spread over the rows that already carry weight, so zero rows stay zero."""
    kw = weights(d, n, kmax=kmax, seed=seed + 1)
    labels = np.zeros(n, dtype=np.int32) if labels is None else labels
    Ps = []
    for lab in range(K):
        idx = np.flatnonzero((labels == lab) & (kw > 0))
        s = int(kw[idx].sum())
        p = max(int(s - 1).bit_length(), 0) if P is None else P
        deficit = (1 << p) - s
        assert idx.size > 0 and deficit >= 0, (lab, s, p)
        kw[idx] += deficit // idx.size
        kw[idx[:deficit % idx.size]] += 1
        assert int(kw[idx].sum()) == 1 << p
        Ps.append(p)
    assert len(set(Ps)) == 1 or P is None
    return kw, (Ps[0] if K == 1 else Ps)


def fit_counts(d, K):
    """Counts and labels of the fit cases (FIT_N rows, per-label totals 2^P_FIT).  K = 3: label 2 owns no row of the last tile."""
    n = FIT_N
    rs = np.random.RandomState(31 * d + K)
    labels = rs.randint(0, K, size=n).astype(np.int32)
    if K > 1:
        last = np.arange(TILE * ((n - 1) // TILE), n)
        labels[last] = rs.randint(0, K - 1, size=last.size)
        labels[0] = K - 1
    kw = weights(d, n, kmax=1, seed=K)                 # ones and zeros, raised to the total below
    keep = forced_rows(n)
    for lab in range(K):
        idx = np.flatnonzero((labels == lab) & (kw > 0))
        spare = idx[~keep[idx]]
        kw[spare[3 << (P_FIT - 2):]] = 0                # at most 3/4 of the total in rows of count one, the rest in twos
        idx = np.flatnonzero((labels == lab) & (kw > 0))
        deficit = (1 << P_FIT) - idx.size
        assert 0 <= deficit, (lab, idx.size)
        kw[idx] += deficit // idx.size
        kw[idx[:deficit % idx.size]] += 1
        assert int(kw[labels == lab].sum()) == 1 << P_FIT
    return kw.astype(np.int32), labels


# ---------------------------------------------------------------------------------------------------- references
def sums_ref(lat, kw):
    """(sums[1 + d], range[2 d]) of tph_weighted_sums / tph_x_weighted_sums under w = kw / WDEN.  Unit 2^-b / WDEN; budget: the
    terms are non-negative, so the result itself bounds every partial sum."""
    n = kw.size
    k = lat.k[:n]
    s1 = kw @ k                                              # int64, exact
    s0 = int(kw.sum())
    assert s0 < LIMIT and int(s1.max(initial=0)) < LIMIT
    sums = np.concatenate([[s0 / WDEN], s1.astype(np.float64) / float(WDEN << lat.b)])
    on = kw > 0
    rng = np.empty(2 * lat.d)
    rng[0::2] = k[on].min(axis=0) / float(1 << lat.b)
    rng[1::2] = k[on].max(axis=0) / float(1 << lat.b)
    return sums, rng


def centred(lat, n):
    """Centred coordinates about the lattice's centre in units of 2^-(b+1): odd integers, never zero."""
    return 2 * lat.k[:n] - lat.c2


def cov_budget(kw, xc):
    """Sum of |w x_a x_b| over the rows, bounded entry by entry by sum(kw) max|xc|^2 (Python integers)."""
    return int(kw.sum()) * int(np.abs(xc).max()) ** 2


def cov_ref(lat, kw, exact_int=False):
    """sum_i w_i (u_ia - c_a)(u_ib - c_b), full d x d, about the lattice's centre: what tph_weighted_cov_centered and
    tph_x_weighted_cov return (no normalisation).  Unit 2^-(2 b + 2) / WDEN.  exact_int: the int64 product; else the float64
    BLAS product of the same integers, exact under the asserted budget (test_moment_cases.py compares the two)."""
    n = kw.size
    xc = centred(lat, n)
    assert cov_budget(kw, xc) < LIMIT
    scale = float(WDEN << (2 * lat.b + 2))
    if exact_int:
        return ((xc * kw[:, None]).T @ xc).astype(np.float64) / scale
    xf = xc.astype(np.float64)
    return ((xf * kw[:, None].astype(np.float64)).T @ xf) / scale


Moments = namedtuple("Moments", "s0 mean cov")


def moments_ref(lat, kw, P, labels=None, label=0):
    """Weighted mean and covariance sum_i w_i (u_i - mean)(u_i - mean)^T / sum_i w_i with the device's own mean, for integer
    weights that sum to 2^P (over the rows of `label`).  mean = S1 / 2^(b+P) exactly; centred coordinates in units of
    g = 2^-(b+P); cov = C / 2^P in units g^2.  Budget: 2^P max|xc|^2 < 2^53 bounds every partial sum of every entry."""
    n = kw.size
    sel = np.ones(n, dtype=bool) if labels is None else labels[:n] == label
    kk = np.where(sel, kw, 0).astype(np.int64)
    assert int(kk.sum()) == 1 << P
    k = lat.k[:n]
    s1 = kk @ k
    xc = (k << P) - s1
    assert cov_budget(kk, xc) < LIMIT
    xf = xc.astype(np.float64)
    c = (xf * kk[:, None].astype(np.float64)).T @ xf         # exact under the budget
    return Moments(float(1 << P), np.ldexp(s1.astype(np.float64), -(lat.b + P)), np.ldexp(c, -(3 * P + 2 * lat.b)))


def moments_ref_int(lat, kw, P):
    """The same covariance from the int64 product, in units of 2^-(3 P + 2 b)."""
    k = lat.k[:kw.size]
    xc = (k << P) - kw @ k
    return (xc * kw[:, None]).T @ xc


def shifted_budget_bits(lat, P):
    """tph_weighted_moments_shifted: da = S1 / S0 is a multiple of 2^-(b+1+P) below 1, da * db needs twice those bits, and
    S2 / S0 - da db lies on the same grid below 1."""
    return 2 * (lat.b + 1 + P)


def shifted_ref_int(lat, kw, P):
    """cov of the shifted form, S2 / S0 - (S1 / S0)(S1 / S0)^T about the lattice's centre, in units of 2^-2(b+1+P), as integers."""
    xc = centred(lat, kw.size)
    da = kw @ xc
    s2 = (xc * kw[:, None]).T @ xc
    assert int(np.abs(s2).max()) << P < LIMIT and int(np.abs(da).max()) ** 2 < LIMIT
    return (s2 << P) - np.outer(da, da)


def fit_cov_ref(lat, counts, labels, label):
    """covs[label] of tph_fit_modes: Sigma = C / n + diag(C / n) / n with n = 2^P_FIT the label's total count (k_cov_finish,
    student = 1).  The diagonal needs bits(v) + P_FIT <= 53: asserted."""
    m = moments_ref(lat, counts.astype(np.int64), P_FIT, labels, label)
    v = m.cov.copy()
    units = np.ldexp(np.diag(v), 3 * P_FIT + 2 * lat.b)      # the diagonal of C in its integer units
    assert int(units.max()) * ((1 << P_FIT) + 1) < LIMIT
    v[np.diag_indices(lat.d)] = np.diag(v) + np.diag(v) / float(1 << P_FIT)
    return v


# ------------------------------------------------------------------------------------------------------ tph_cv_sum
CvCase = namedtuple("CvCase", "lat kw P shift")


def cv_case(d, n, shift=0):
    """Coarse lattice (b = 2), integer weights 0 .. 3 (0 .. 2 in the clip case), integer banded P of both signs times 2^shift."""
    lat = lattice(d, max(cv_rows_for(d)), b=B_CV, seed=5)
    kw = weights(d, n, kmax=2 if shift else 3, seed=11)
    rs = np.random.RandomState(17 * d + 3)
    Pm = np.zeros((d, d), dtype=np.int64)
    for off in (-2, -1, 0, 1, 2):
        idx = np.arange(max(0, -off), min(d, d - off))
        Pm[idx, idx + off] = rs.randint(-2, 3, size=idx.size)
    Pm[np.diag_indices(d)] = rs.choice([-3, -2, 2, 3], size=d)
    return CvCase(lat, kw, Pm, shift)


def cv_inputs(case):
    return centre_of(case.lat), np.ldexp(case.P.astype(np.float64), case.shift)


def cv_ref(case):
    """sum_i w_i^2 clip(d2_i - d, +-1e6)^2, d2 = (u - c)^T P (u - c).  xc in units 2^-(b+1), d2 in units 2^(shift - 2 b - 2):
    shift = 0 -> everything in units e = 2^-(2 b + 2); shift >= 2 b + 2 -> everything is an integer (e = 1).  Budget: the terms
    are non-negative, so the total bounds every partial sum; the inner sums of d2 are bounded by d max|xc|^2 max_r sum_j |P_rj|.
    -> (value, rows clipped at +1e6, rows clipped at -1e6)"""
    lat, kw, Pm, shift = case
    n, d, fb = kw.size, lat.d, 2 * lat.b + 2
    assert shift == 0 or shift >= fb
    xc = centred(lat, n)
    assert d * int(np.abs(xc).max()) ** 2 * int(np.abs(Pm).sum(axis=1).max()) << max(shift - fb, 0) < LIMIT
    d2 = np.einsum("ia,ab,ib->i", xc, Pm, xc)                # int64, units 2^(shift - fb)
    e = fb if shift == 0 else 0                              # results in units 2^-e
    dev = (d2 << max(shift - fb, 0)) - (d << e)
    lim = 10 ** 6 << e
    hi, lo = int((dev > lim).sum()), int((dev < -lim).sum())
    dev = np.clip(dev, -lim, lim)
    assert int(np.abs(dev).max()) ** 2 * int(kw.max()) ** 2 < (1 << 62) // n
    total = int((kw * kw * dev * dev).sum())
    assert total < LIMIT
    return np.ldexp(float(total), -2 * e), hi, lo


# ------------------------------------------------------------------------------------- non-lattice data and its a-priori bound
def gaussian_case(d, n=2397):
    """Correlated Gaussian clipped to the cube, log-normal weights, Poisson counts: the one non-lattice input."""
    rs = np.random.RandomState(4000 + d)
    A = rs.randn(d, d) * 0.05
    u = np.clip(0.5 + rs.randn(n, d) @ A.T + 0.1 * rs.randn(n, 1), 0.0, 1.0)
    w = np.exp(rs.randn(n))
    counts = rs.poisson(np.exp(rs.randn(n) - 0.5)).astype(np.int32)
    counts[0] = max(counts[0], 1)
    return u, w, counts


def moments_bound(u, w):
    """np.longdouble reference of (mean, cov = sum w (u - m)(u - m)^T / sum w) and the a-priori error bound of ANY float64
    evaluation order, entry by entry, with eps = (n + 4) 2^-53 (n - 1 additions, two subtractions, two products, one division):
        eps T_ab / S0                         T_ab = sum w |xc_a xc_b|: the rounding of the terms and of their sum
      + eps |C_ab| / S0                       the rounding of S0
      + (A_a dm_b + A_b dm_a) / S0            A_a = sum w |xc_a|, dm_j = eps (sum w |u_j| / S0 + |m_j|): the computed mean, whose
                                              relative error is that of S1 and of S0, propagated to first order
    -> (mean, cov, bound_mean, bound_cov)"""
    n = w.size
    eps = LD(n + 4) * LD(2.0) ** -53
    ul, wl = u.astype(LD), w.astype(LD)
    s0 = wl.sum()
    m = (wl[:, None] * ul).sum(axis=0) / s0
    xc = ul - m
    a = np.abs(xc)
    c = np.einsum("i,ia,ib->ab", wl, xc, xc)
    t = np.einsum("i,ia,ib->ab", wl, a, a)
    am = (wl[:, None] * a).sum(axis=0)
    dm = eps * ((wl[:, None] * np.abs(ul)).sum(axis=0) / s0 + np.abs(m))
    bound = (eps * t + eps * np.abs(c) + np.outer(am, dm) + np.outer(dm, am)) / s0
    return m, c / s0, dm, bound

"""What tests/test_lean_math.py (host) and tests/test_lean_math_gpu.py (device) share: fixed, seeded samples for the lean FP64
functions, the generator and the boundary maps of tempest_amd/csrc/common.h, their truth from mpmath at 40 digits, the error helpers,
the derived bounds and the two probe plugins that reach the header's functions through derived().

The probes are the header's code under the library's compiler and flags (build_plugin: -O3 -ffp-contract=on, gfx950); they are not the
instruction sequence inside any particular library kernel.  Integer arguments travel as doubles: counters below 2^32 (and the item
2^32) exactly, a 64-bit seed as its two 32-bit halves."""
import functools
from collections import namedtuple

import numpy as np

from oracle import philox as px

U = 2.0 ** -53                         # unit roundoff; one ulp of relative error is counted as 2 U throughout
SIZES = (1, 63, 64, 65, 1000)          # both sides of a wave; 1000: four workgroups, no multiple of 256
SQRT_HALF = 0.70710678118654752440     # tph_log's mantissa switch
MASK32 = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------ truth and errors
Truth = namedtuple("Truth", "near rem")        # the exact value = near (the nearest double) + rem (a double, |rem| <= ulp / 2)


def _truth(exact):
    import mpmath as mp
    near = np.array([float(v) for v in exact], dtype=np.float64)
    rem = np.array([float(v - mp.mpf(float(n))) for v, n in zip(exact, near)], dtype=np.float64)
    near.setflags(write=False)
    rem.setflags(write=False)
    return Truth(near, rem)


def _mp(fn, *cols):
    """Truth of fn over the rows of the columns, all arguments exact mpf copies of the doubles."""
    import mpmath as mp
    with mp.workdps(40):
        return _truth([fn(*(mp.mpf(float(v)) for v in row)) for row in zip(*cols)])


def abs_error(got, truth):
    """|got - exact|: got - near is exact wherever got is within a factor two of near, and far larger than any bound elsewhere."""
    return np.abs((np.asarray(got, dtype=np.float64) - truth.near) - truth.rem)


def ulp_error(got, truth):
    """|got - exact| in ulps of the exact value's nearest double (5e-324 at zero, so that only an exact zero passes there)."""
    return abs_error(got, truth) / np.spacing(np.abs(truth.near))


def take(truth, idx):
    return Truth(truth.near[idx], truth.rem[idx])


def _rs(k):
    return np.random.RandomState(20250300 + k)


def _around(v, k):
    """The doubles from k below v to k above it."""
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.array(sorted(float(x) for x in out))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------------------- division, reciprocal
# The call sites of tph_div and tph_rcp (grep over tempest_amd/csrc) and the domains of their arguments:
DIV_SITES = (
    ("tph_log: s = f / (2 + f)", "f in [-0.293, 0.414], the reduced mantissa minus one"),
    ("tph_tpcn_factor: m / nu", "nu in [0.1, 1e6], forms m up to 1e300 (beyond: the IEEE division)"),
    ("proposal kernels (mutate.hip, maha_tile.h, propose_blkm.hip, user_plugin.hip.in): 2 / (nu + m)", "nu + m in [0.1, 1e300]"),
    ("tph_log1p_unit: c / u", "u = fl(1 + e) in [1, 2], c = e - (u - 1) the rounding error of that sum: 0, or as small as 5e-324 over u = 1"),
)
RCP_SITES = (
    ("tph_div", "the divisors above"),
    ("tph_gamma_mt, mutate.hip: c = rcp(sqrt(9 d))", "sqrt(9 d) in [1.7, 2200]: shapes up to 5e5"),
    ("proposal kernels: sqrt(rcp(gam))", "gam = Gamma x 2 / (nu + m) in [1e-300, 1e6]"),
)


@functools.lru_cache(maxsize=None)
def sample_div():
    """(a, b): the numerators and divisors of DIV_SITES, then zero numerators and subnormal numerators over 1.0."""
    rs = _rs(1)
    f = rs.uniform(-0.293, 0.414, 3000)
    nu = 10.0 ** rs.uniform(-1.0, 6.0, 3000)
    m = 10.0 ** rs.uniform(-10.0, 300.0, 3000)
    den = 10.0 ** rs.uniform(-1.0, 300.0, 2000)
    e = np.concatenate([rs.uniform(0.0, 1.0, 1500), np.exp(-rs.uniform(0.0, 745.0, 1500)), [5e-324, 1e-310, 2.0 ** -1022, 2.0 ** -54]])
    u = 1.0 + e
    zero_over = np.array([1.0, 1.5, 0.1, 1e6, 1e300, 2.0 - 0.293])
    a = np.concatenate([f, m, np.full(den.size, 2.0), e - (u - 1.0), np.zeros(zero_over.size)])
    b = np.concatenate([2.0 + f, nu, den, u, zero_over])
    return _frozen(a, b)


@functools.lru_cache(maxsize=None)
def sample_rcp():
    rs = _rs(2)
    _, b = sample_div()
    return _frozen(np.concatenate([b, np.sqrt(9.0 * 10.0 ** rs.uniform(0.0, 5.7, 1500)), 10.0 ** rs.uniform(-300.0, 6.0, 2500)]))


@functools.lru_cache(maxsize=None)
def truth_div():
    return _mp(lambda a, b: a / b, *sample_div())


@functools.lru_cache(maxsize=None)
def truth_rcp():
    return _mp(lambda b: 1 / b, sample_rcp())


# ------------------------------------------------------------------------------------------------------------------------ square root
@functools.lru_cache(maxsize=None)
def sample_sqrt():
    """-2 log u1 in [0, 73.5]; 9 d up to 4.5e6 (tph_gamma_mt); 1 - sigma^2; 1 / gam up to 1e300; small normal values; both zeros."""
    rs = _rs(3)
    sig = rs.uniform(0.0, 0.99, 1000)
    return _frozen(np.concatenate([rs.uniform(0.0, 73.5, 4000), 10.0 ** rs.uniform(0.3, 6.654, 2000), 1.0 - sig * sig,
                                   10.0 ** rs.uniform(0.0, 300.0, 1000), 10.0 ** rs.uniform(-300.0, 0.0, 2000),
                                   [2.0 ** -1022, 73.5, 4.5e6, 0.0, -0.0]]))


@functools.lru_cache(maxsize=None)
def truth_sqrt():
    import mpmath as mp
    return _mp(mp.sqrt, np.abs(sample_sqrt()))


# ------------------------------------------------------------------------------------------------------------------------- logarithm
@functools.lru_cache(maxsize=None)
def sample_log():
    """(k + 1) 2^-53 (the radius uniform: random k, k = 0, and k = 2^53 - 1, where the argument is 1); 1 - j 2^-53 and j 2^-53 for
    j <= 2^20; the doubles within 5 ulp of the sqrt(1/2) mantissa switch at several exponents; 1 + m / nu up to 1e300; Marsaglia-
    Tsang's v down to 1e-30; (r + 1) 2^-32 (the acceptance uniform: random r, r = 0, and r = 2^32 - 1, where the argument is 1)."""
    rs = _rs(4)
    k = np.concatenate([rs.randint(0, 2 ** 53, 4000, dtype=np.int64), [0, 2 ** 53 - 1]]).astype(np.float64)
    j = np.concatenate([rs.randint(1, 2 ** 20 + 1, 1500, dtype=np.int64), [1, 2, 2 ** 20]]).astype(np.float64)
    switch = np.concatenate([np.ldexp(_around(SQRT_HALF, 5), e) for e in (-1000, -52, -31, -1, 0, 1, 10, 300, 996)])
    r = np.concatenate([rs.randint(0, 2 ** 32, 2000, dtype=np.int64), [0, 2 ** 32 - 1]]).astype(np.float64)
    return _frozen(np.concatenate([(k + 1.0) * 2.0 ** -53, 1.0 - j * 2.0 ** -53, j * 2.0 ** -53, switch,
                                   1.0 + 10.0 ** rs.uniform(-16.0, 300.0, 2000), 10.0 ** rs.uniform(-30.0, 0.5, 2000),
                                   (r + 1.0) * 2.0 ** -32]))


@functools.lru_cache(maxsize=None)
def truth_log():
    import mpmath as mp
    return _mp(mp.log, sample_log())


# ------------------------------------------------------------------------------------------------------------------------- sincospi
@functools.lru_cache(maxsize=None)
def sample_sincospi():
    """t in [0, 2]: k 2^-52 for random k; the 32-bit angles r 2^-31; the quarter turns and the rint ties j / 4 with the doubles within
    4 ulp of each; 2 - 2^-52."""
    rs = _rs(5)
    k = rs.randint(0, 2 ** 53, 6000, dtype=np.int64).astype(np.float64)
    r = np.concatenate([rs.randint(0, 2 ** 32, 3000, dtype=np.int64), [0, 1, 2 ** 32 - 1]]).astype(np.float64)
    near = np.concatenate([_around(0.25 * j, 4) for j in range(9)])
    t = np.concatenate([k * 2.0 ** -52, r * 2.0 ** -31, near[(near >= 0.0) & (near <= 2.0)], [2.0 - 2.0 ** -52]])
    return _frozen(t)


QUARTERS = _frozen(0.25 * np.arange(9.0))      # even j: a quarter turn (values 0 or +-1); odd j: a tie of rint(2 t)


@functools.lru_cache(maxsize=None)
def truth_sincospi():
    import mpmath as mp
    t = sample_sincospi()
    return _mp(mp.sinpi, t), _mp(mp.cospi, t)


def unit_circle_defect(sn, cs):
    """sn^2 + cs^2 - 1, exactly (the squares of doubles need 106 bits; 40 digits hold 132)."""
    import mpmath as mp
    with mp.workdps(40):
        return np.array([float(mp.mpf(float(s)) ** 2 + mp.mpf(float(c)) ** 2 - 1) for s, c in zip(sn, cs)])


# ----------------------------------------------------------------------------------------------------------- log1p_unit, logaddexp
@functools.lru_cache(maxsize=None)
def sample_log1p():
    rs = _rs(6)
    return _frozen(np.concatenate([rs.uniform(0.0, 1.0, 3000), np.exp(-rs.uniform(0.0, 745.0, 3000)),
                                   [0.0, 1.0, 5e-324, 1e-310, 2.0 ** -1022, 2.0 ** -53, 2.0 ** -52, 1.0 - 2.0 ** -53, 0.5]]))


@functools.lru_cache(maxsize=None)
def truth_log1p():
    import mpmath as mp
    return _mp(mp.log1p, sample_log1p())


def bound_log1p(truth):
    """|error| of tph_log1p_unit(e), 0 <= e <= 1, with L = log1p(e) and u = fl(1 + e): tph_log(u) is within one ulp of log u <= L + U,
    2 U L; c / u <= U with a relative error of 2 U, 2 U^2; the series of log(u + c) cut after c / u, U^2 / 2; the final sum, U L.
    Together 3 U L + 4 U^2."""
    return 3.0 * U * np.abs(truth.near) + 4.0 * U * U


@functools.lru_cache(maxsize=None)
def sample_logaddexp():
    """(x, y) with |x - y| = 10^U(-3, 2.87) <= 742 either way round, at magnitudes from 1e-3 to 1e4 (the log-weights of the mixture)."""
    rs = _rs(7)
    n = 6000
    x = np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 4.0, n)
    y = x + np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 2.87, n)
    x = np.concatenate([x, [0.0, -740.0, 0.0, 1e-300]])
    y = np.concatenate([y, [-740.0, 0.0, 2.0 ** -30, -1e-300]])
    return _frozen(x, y)


@functools.lru_cache(maxsize=None)
def truth_logaddexp():
    """(truth, bound).  The bound, with t = x - y, E = exp(-|t|), q = E / (1 + E), L = log1p(E) and r the result: the rounding of t moves
    E by U |t| relatively and the library exp by one ulp, 2 U, which is U (2 + |t|) q in log1p(E) (d log1p(E) = q dE / E), plus one
    subnormal step where E is subnormal; tph_log1p_unit adds 3 U L + 4 U^2 (bound_log1p); the final sum U |r|."""
    import mpmath as mp
    x, y = sample_logaddexp()
    with mp.workdps(40):
        rows = [(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(x, y)]
        exact = [max(a, b) + mp.log1p(mp.exp(-abs(a - b))) for a, b in rows]
        big_e = np.array([float(mp.exp(-abs(a - b))) for a, b in rows])
    truth = _truth(exact)
    t = np.abs(x - y)
    bound = U * (np.abs(truth.near) + (2.0 + t) * big_e / (1.0 + big_e) + 3.0 * np.log1p(big_e)) + 8.0 * U * U + 5e-324
    return truth, _frozen(bound)


def logaddexp_specials():
    """(x, y) where tph_logaddexp must give np.logaddexp's bits.  Where exp underflows (|x - y| > 745) or is subnormal (about 740) the
    larger argument is of normal size, so that the result does not hang on the last bit of a subnormal exp."""
    inf, nan = np.inf, np.nan
    rows = [(0.0, 0.0), (1.5, 1.5), (-3.25e7, -3.25e7), (1e-300, 1e-300), (inf, inf), (-inf, -inf), (inf, -inf), (-inf, inf),
            (-inf, 2.5), (-inf, -1e300), (3.0, -inf), (-inf, 0.0), (nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (-inf, nan),
            (3.5, 3.5 - 746.0), (3.5 - 746.0, 3.5), (-2000.0, 100.0), (1e5, -1e5), (-1.0, -751.0), (12.0, -733.5),
            (3.5, 3.5 - 740.0), (3.5 - 740.0, 3.5), (-20.25, -760.0), (-760.5, -20.25), (1.0, -739.0), (700.0, -40.0)]
    a = np.array(rows, dtype=np.float64)
    return a[:, 0].copy(), a[:, 1].copy()


# --------------------------------------------------------------------------------------------------------------------- boundary maps
@functools.lru_cache(maxsize=None)
def sample_bc():
    """+-U(0, 3), exact integers, +-0, +-1e-17, +-5e-324, 1 - 2^-53, -2^-53, +-(1e15 + 0.5), 2^53 -- finite; NaN goes by itself."""
    rs = _rs(8)
    v = rs.uniform(0.0, 3.0, 4000)
    ints = np.arange(-6.0, 7.0)
    return _frozen(np.concatenate([v, -v, ints, [0.0, -0.0, 1e-17, -1e-17, 5e-324, -5e-324, 1.0 - 2.0 ** -53, -2.0 ** -53,
                                                 1e15 + 0.5, -(1e15 + 0.5), 2.0 ** 53, -2.0 ** 53, 2.0 ** 53 + 2.0]]))


# ------------------------------------------------------------------------------------------------------------------------------ RNG
# Random123's known-answer vectors for Philox4x32-10 (kat_vectors of the Random123 distribution): counter, key, output
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))

CORNER_ITEMS = (0, 1, 2 ** 32 - 1, 2 ** 32, 3 * 10 ** 9)      # item 2^32 is item 0: the truncation is part of the stream's definition
CORNER_DRAWS = (0, 2 ** 32 - 1)
CORNER_TICKS = (0, 2 ** 32 - 1)
CORNER_TAGS = (1, 2, 3, 4, 5, 6, 7)
CORNER_SEEDS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)
RANDOM_SEEDS = (0x9E3779B97F4A7C15, 0x0123456789ABCDEF, 7, 0xDEADBEEF00000001)

Counters = namedtuple("Counters", "item draw tick tag seed")      # uint64 arrays of one length


def _counters(item, draw, tick, tag, seed):
    return Counters(*(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.uint64), np.shape(item))) for v in (item, draw, tick, tag, seed)))


def _random_counters(rs, n, tag=None, seeds=RANDOM_SEEDS):
    word = lambda: rs.randint(0, 2 ** 32, n, dtype=np.int64).astype(np.uint64)
    tags = rs.randint(1, 8, n).astype(np.uint64) if tag is None else np.full(n, tag, dtype=np.uint64)
    return _counters(word(), word(), word(), tags, np.array(seeds, dtype=np.uint64)[rs.randint(0, len(seeds), n)])


def _concat(*cs):
    return Counters(*(np.concatenate([getattr(c, f) for c in cs]) for f in Counters._fields))


@functools.lru_cache(maxsize=None)
def corner_counters():
    """The three known-answer vectors as (item, draw, tick, tag; seed), the 560 corners, then 4096 random counters."""
    kat = _counters(*(np.array([v[0][i] for v in KAT], dtype=np.uint64) for i in range(4)),
                    np.array([v[1][0] | (v[1][1] << 32) for v in KAT], dtype=np.uint64))
    grid = np.array([(i, d, t, g, s) for i in CORNER_ITEMS for d in CORNER_DRAWS for t in CORNER_TICKS for g in CORNER_TAGS
                     for s in CORNER_SEEDS], dtype=np.uint64)
    return _concat(kat, _counters(*grid.T), _random_counters(_rs(9), 4096))


def by_seed(c, fn, n_out):
    """fn(seed, item, draw, tick, tag) -> n_out arrays, over counters of several seeds (the oracle takes one seed at a time)."""
    out = None
    for s in np.unique(c.seed):
        m = c.seed == s
        vals = fn(int(s), c.item[m], c.draw[m], c.tick[m], c.tag[m])
        if out is None:
            out = [np.empty(c.seed.size, dtype=np.asarray(v).dtype) for v in vals[:n_out]]
        for o, v in zip(out, vals):
            o[m] = v
    return out


def oracle_words(c):
    return by_seed(c, lambda s, i, d, t, g: px.philox4x32(i, d, t, g, s & MASK32, s >> 32), 4)


def probe_rows(c, shape=1.0):
    """The counters as rows of the RNG probe: item, draw, tick, tag, seed's low half, seed's high half, the Gamma shape."""
    lo, hi = c.seed & np.uint64(MASK32), c.seed >> np.uint64(32)
    return np.stack([c.item.astype(np.float64), c.draw.astype(np.float64), c.tick.astype(np.float64), c.tag.astype(np.float64),
                     lo.astype(np.float64), hi.astype(np.float64), np.broadcast_to(np.float64(shape), c.item.shape)], axis=1)


# Box-Muller on extreme blocks: found by a scan of items 0 .. 2^22 - 1 of this (seed, tick, draw) with the oracle
SCAN = dict(seed=7, tick=3, draw=0, items=2 ** 22, keep=32)


@functools.lru_cache(maxsize=None)
def extreme_counters():
    """Of the scanned blocks: the 32 with the smallest u1 and the 32 with the largest, and for every multiple of 1/8 the 32 whose u2
    is closest to it (the quarter turns and the rint ties of the angle 2 u2)."""
    keep, step = SCAN["keep"], 2 ** 16                      # the oracle in cache-sized pieces
    pairs = [px.uniform_pair(SCAN["seed"], np.arange(i, i + step, dtype=np.uint64), SCAN["draw"], SCAN["tick"], px.TAG_NORMAL)
             for i in range(0, SCAN["items"], step)]
    u1, u2 = (np.concatenate([p[k] for p in pairs]) for k in range(2))

    def smallest(key):
        part = np.argpartition(key, keep)[:keep]
        return part[np.argsort(key[part], kind="stable")]

    picks = [smallest(u1), smallest(-u1)] + [smallest(np.abs(u2 - j / 8.0)) for j in range(9)]
    items = np.concatenate(picks).astype(np.uint64)
    return _counters(items, SCAN["draw"], SCAN["tick"], px.TAG_NORMAL, SCAN["seed"])


@functools.lru_cache(maxsize=None)
def normal_counters():
    """2 x 10^4 ordinary counters under TAG_NORMAL, then the extreme blocks."""
    return _concat(_random_counters(_rs(10), 20000, tag=px.TAG_NORMAL), extreme_counters())


def _exact_candidates(r0, r1, r2, r3, pair=True):
    """Exact Box-Muller on Philox words, as mpf: (radius, z0, z1 [53-bit angle]) and (x, logu) of the Gamma candidate [32-bit angle]."""
    import mpmath as mp
    k = ((int(r0) >> 5) << 26) | (int(r1) >> 6)
    rad = mp.sqrt(-2 * mp.log(mp.mpf(k + 1) / 2 ** 53))
    x = rad * mp.cospi(mp.mpf(int(r2)) / 2 ** 31)
    logu = mp.log(mp.mpf(int(r3) + 1) / 2 ** 32)
    if not pair:
        return rad, x, logu
    t = mp.mpf(((int(r2) >> 5) << 26) | (int(r3) >> 6)) / 2 ** 52           # 2 u2
    return rad, rad * mp.cospi(t), rad * mp.sinpi(t), x, logu


NormalTruth = namedtuple("NormalTruth", "rad z0 z1 x logu")


@functools.lru_cache(maxsize=None)
def truth_normals():
    """Over normal_counters(): the radius sqrt(-2 ln u1) (a double, for the bounds), and the truth of normal2's two outputs and of
    gamma_candidate's x and logu at attempt = draw, from mpmath on the oracle's Philox words."""
    import mpmath as mp
    w = oracle_words(normal_counters())
    with mp.workdps(40):
        rows = [_exact_candidates(*r) for r in zip(*w)]
        rad = np.array([float(r[0]) for r in rows])
        cols = [_truth([r[i] for r in rows]) for i in range(1, 5)]
    return NormalTruth(_frozen(rad), *cols)


def bound_normal(rad):
    """|error| of a Box-Muller normal z = rad x trig, rad = sqrt(-2 ln u1): tph_log is within one ulp, 2 U relative, which the square
    root halves to U; tph_sqrt's own ulp adds 2 U: the radius is within 3 U relative.  tph_sincospi is within 2^-52 = 2 U absolute
    on an angle that is exact (2 u2 and r 2^-31 are).  The product's rounding adds U |z| <= U rad.  rad (3 U |trig| + 2 U) + U rad
    <= 6 U rad."""
    return 6.0 * U * rad


def bound_oracle_normal(rad, turn):
    """The same for oracle/philox.py, whose angle is rounded: np.log within one ulp (U after the root) and a correctly rounded sqrt
    (U): the radius within 2 U; theta = fl(fl(2 pi) turn) is off by at most 1.5 U theta (fl(2 pi) by 0.36 U, the product by U) and
    the library cos / sin by one ulp of a value <= 1, 2 U; the product U rad.  rad U (2 + 1.5 theta + 2 + 1)."""
    return U * rad * (5.0 + 1.5 * 2.0 * np.pi * turn)


# ---------------------------------------------------------------------------------------------------------------- Marsaglia-Tsang
GAMMA_SHAPES = (0.3, 0.7, 1.0, 5.5, 50.5, 5e5)      # boosted twice; with nu = 1e6 the tpCN shapes (d + nu) / 2 of d = 2 ...
GAMMA = dict(seed=7, tick=3, items=4000, max_attempts=64)
GammaTruth = namedtuple("GammaTruth", "value bound attempts left_out min_margin")


@functools.lru_cache(maxsize=None)
def truth_gamma():
    """Per shape, over items 0 .. GAMMA['items'] - 1: the value d v [u^(1 / shape)] of the attempt that the EXACT evaluation of
    Marsaglia-Tsang's test accepts first, the bound of the device's value, the accepted attempt, how many items were left out, and the
    smallest acceptance margin relative to d.

    Exact means: on the doubles that the device holds without rounding error -- the Philox words, d = fl(fl(shape [+ 1]) - fl(1/3)),
    for a boosted shape u = k 2^-53 + 2^-53 and the exponent fl(1 / shape) -- with everything else (c = 1 / sqrt(9 d), the candidate,
    w = 1 + c x, v = w^3, the test, the power) in mpmath.

    Bound of the value.  The candidate x is within 6 U rad (bound_normal).  c~ = tph_rcp(tph_sqrt(fl(9 d))) is within 5 U relative
    (U / 2 from the product under the root, one ulp each for root and reciprocal).  So w~ = fl(1 + c~ x~) is within
    dw = U (6 c rad + 6 c |x| + |w|) -- candidate, c~ and the product's rounding, the sum's rounding -- and v = w^3 moves by
    |dv| / v <= 3 dw / |w|; the cube's two products and d v add 3 U; a boosted value's pow (one ulp) and product 3 U more.  Second-order
    terms are covered by the factor 1 + 2^-20.

    Left out.  An item is left out only where, at an attempt up to the accepted one, the exact margin rhs - logu of the test is below
    the rounding bound of the device's inequality, or |w| <= dw (the sign of v uncertain).  The inequality's bound, term by term:
    logu within 2 U |logu|; x^2 / 2 within |x| 6 U rad + 1.5 U x^2; d v within d v (ev + U) and d log v within d (ev + 2 U |log v|)
    with ev = 3 dw / |w| + 2 U; four roundings of sums of terms of size at most S = x^2 / 2 + d + d v + d |log v|, 4 U S."""
    import mpmath as mp
    seed, tick, n = GAMMA["seed"], GAMMA["tick"], GAMMA["items"]
    items = np.arange(n, dtype=np.uint64)
    third = 1.0 / 3.0
    ub = px.uniform_pair(seed, items, 2 * GAMMA["max_attempts"], tick, px.TAG_GAMMA)[0] + 2.0 ** -53
    cand = {}                                           # attempt -> {item: (rad, x, logu)}: shared by the shapes
    out = {}
    with mp.workdps(40):
        u = mp.mpf(U)
        for shape in GAMMA_SHAPES:
            boost = shape < 1.0
            d_f = ((shape + 1.0) if boost else shape) - third
            d = mp.mpf(d_f)
            c = 1 / mp.sqrt(9 * d)
            values, bounds, atts = [None] * n, np.zeros(n), np.full(n, -1)
            left_out, min_margin = 0, np.inf
            todo = list(range(n))
            for att in range(GAMMA["max_attempts"]):
                if not todo:
                    break
                have = cand.setdefault(att, {})
                need = [i for i in todo if i not in have]
                if need:
                    w4 = px.philox4x32(np.array(need, dtype=np.uint64), att, tick, px.TAG_GAMMA, seed & MASK32, seed >> 32)
                    for i, r in zip(need, zip(*w4)):
                        have[i] = _exact_candidates(*r, pair=False)
                still = []
                for i in todo:
                    rad, x, logu = have[i]
                    w = 1 + c * x
                    dw = u * (6 * c * rad + 6 * c * abs(x) + abs(w))
                    if abs(w) <= dw:
                        left_out += 1
                        continue
                    if w < 0:
                        still.append(i)
                        continue
                    v = w ** 3
                    lv = mp.log(v)
                    margin = x * x / 2 + d - d * v + d * lv - logu
                    ev = 3 * dw / w + 2 * u
                    size = x * x / 2 + d + d * v + d * abs(lv)
                    e_ineq = 2 * u * abs(logu) + abs(x) * 6 * u * rad + 1.5 * u * x * x + d * v * (ev + u) + d * (ev + 2 * u * abs(lv)) \
                        + 4 * u * size
                    if abs(margin) < e_ineq:
                        left_out += 1
                        continue
                    min_margin = min(min_margin, float(abs(margin) / d))
                    if margin > 0:
                        rel = (3 * dw / w + 3 * u) * (1 + mp.mpf(2) ** -20)
                        val = d * v
                        if boost:
                            val *= mp.power(mp.mpf(float(ub[i])), mp.mpf(1.0 / shape))
                            rel += 3 * u
                        values[i], bounds[i], atts[i] = val, float(rel * val), att
                    else:
                        still.append(i)
                todo = still
            kept = np.array([v is not None for v in values])
            truth = _truth([v if v is not None else mp.mpf(0) for v in values])
            out[shape] = (GammaTruth(truth, _frozen(bounds), _frozen(atts), left_out + len(todo), min_margin), _frozen(kept))
    return out


def gamma_rows(shape):
    n = GAMMA["items"]
    return probe_rows(_counters(np.arange(n, dtype=np.uint64), 0, GAMMA["tick"], px.TAG_GAMMA, GAMMA["seed"]), shape)


# --------------------------------------------------------------------------------------------------------------------------- probes
_CALLBACKS = '''
__device__ void prior_transform(const double* u, double* x) {
  for (int j = 0; j < N_DIM; ++j) x[j] = u[j];
}
__device__ double log_likelihood(const double* x) { return -0.5 * x[0] * x[0]; }
'''

# x = (a, b): every lean function of a [and b] beside each other; a test reads the columns whose arguments its rows were made for
MATH_COLUMNS = ("rcp", "div", "sqrt", "log", "sinpi", "cospi", "log1p_unit", "logaddexp", "bc_periodic", "bc_reflective", "radius")
MATH_N_DIM = 2
MATH_SOURCE = _CALLBACKS + '''
__device__ void derived(const double* x, double* out) {
  const double a = x[0], b = x[1];
  out[0] = tph_rcp(a);
  out[1] = tph_div(a, b);
  out[2] = tph_sqrt(a);
  out[3] = tph_log(a);
  tph_sincospi(a, out[4], out[5]);
  out[6] = tph_log1p_unit(a);
  out[7] = tph_logaddexp(a, b);
  out[8] = bc_periodic(a);
  out[9] = bc_reflective(a);
  out[10] = tph_sqrt(-2.0 * tph_log(a));      // the Box-Muller radius at u1 = a
}
'''

# x = (item, draw, tick, tag, seed low, seed high, shape)
RNG_COLUMNS = ("w0", "w1", "w2", "w3", "u_a", "u_b", "z0", "z1", "cand_x", "cand_logu", "k53", "gamma")
RNG_N_DIM = 7
RNG_SOURCE = _CALLBACKS + '''
__device__ void derived(const double* x, double* out) {
  const uint64_t item = (uint64_t)x[0];
  const uint32_t draw = (uint32_t)x[1], tick = (uint32_t)x[2], tag = (uint32_t)x[3], k0 = (uint32_t)x[4], k1 = (uint32_t)x[5];
  const uint64_t seed = ((uint64_t)k1 << 32) | (uint64_t)k0;
  const tph_u4 r = tph_philox((uint32_t)item, draw, tick, tag, k0, k1);
  out[0] = (double)r.x;
  out[1] = (double)r.y;
  out[2] = (double)r.z;
  out[3] = (double)r.w;
  const tph_rng g(seed, tick, tag, item);
  g.uniform2(draw, out[4], out[5]);
  g.normal2(draw, out[6], out[7]);
  g.gamma_candidate(draw, out[8], out[9]);
  out[10] = tph_k53((uint32_t)item, draw);
  out[11] = tph_gamma_mt(g, x[6]);
}
'''

PROBES = {"math": (MATH_SOURCE, MATH_N_DIM, len(MATH_COLUMNS)), "rng": (RNG_SOURCE, RNG_N_DIM, len(RNG_COLUMNS))}


def column(names, out, name):
    return np.ascontiguousarray(out[:, names.index(name)])

"""Inputs, references and derived bounds for the log-mixture (K1: k_logmix_append, csrc/ctx.hip), the reweighting pass (K2:
k_reweight_reduce<NB, U>, k_reweight_vshards, k_reweight_fold, csrc/reweight.hip) and the weight kernels (K3: k_weights, k_logw,
k_sum_sq_max, k_sum_sq_max_final).  CPU only, NumPy only: shared by tests/test_reweight_cases.py (which checks the claims made
here) and tests/test_reweight_gpu.py (which holds the device to them).

Three kinds of comparison, none with a fitted tolerance.

EXACT COUNTS (K2).  A history whose iterations all have beta_t = 0, logZ_t = 0 caches one constant C for every finite l.  "On" rows
carry l = 0, "off" rows l = -2^40, trial betas are 0 and dyadic values in [2^-20, 1].  Then beta l is exact, an on row has
v = -C with or without FMA, an off row lies 2^20 or more below it and exp gives exactly 0 -- also in a rescale factor f, when a
lane, block or shard saw only off rows first --, for beta = 0 every row has v = -C, and every partial sum is a small integer:
in any order, on any number of blocks and shards, the triple is (-C, n_on, n_on) bit for bit ((-C, n, n) for beta = 0; (v_off, n, n)
when no row is on).  A dropped or doubled row changes the count; a padding value that is not neutral adds to it.

DERIVED BOUNDS (K1, K2, k_weights).  References in np.longdouble (64-bit mantissa, asserted), bounds summed from the roundings the
kernel commits on its longest path (acc_bound, logmix_bounds, weights_bound say which).  Every rounding the reference commits is
one the device commits too, at 2^-11 of its size (2^-64 against 2^-53), and the pairwise np.sum adds (log2 n + 8) 2^-64 where the
device adds at least eight roundings of 2^-53: the reference's own error is below REF_SHARE = 2^-9 of the bound, which is added.
One ulp of a library function counts as 2 U, as in tests/lean_math_cases.py.

EXACT FORMS (max, k_logw, k_sum_sq_max).  The maximum and beta l - (C - log n) are single expressions: the device must give one of
their two correctly rounded forms (fused, unfused), found with fractions.Fraction.  The weights of the k_sum_sq_max cases are
k 2^-20, k < 1024: sums and sums of squares are exact in any order (bit budget asserted).

Literal -inf log-likelihoods.  A row with l = -inf has C = -inf (every beta_t > 0) or NaN (a beta_t = 0 meets it), so
v = beta l - C is NaN in the reference's arithmetic (NumPy) as on the device: such rows are compared with the reference like any
other (NaN sums).  A row with v = -inf and a finite C -- weight 0, no NaN, and the (-inf, 0, 0) triple k_reweight_fold documents when
every row is one -- needs beta l to overflow: l = -DBL_MAX under a trial beta of 2 (acc_edges: "overflow-...")."""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision long double"
U = 2.0 ** -53
SUBNORMAL = 5e-324
HALF_STEP = LD(2) ** LD(-1075)      # half the smallest subnormal: a smaller exact value rounds to 0
REF_SHARE = 2.0 ** -9
DBL_MAX = np.finfo(np.float64).max
LIMIT = 1 << 53

THREADS = 256                   # TPH_RED_THREADS
RED_BLOCKS = 2048               # TPH_RED_BLOCKS
MAX_NB = 16                     # TPH_MAX_NB
VSHARD_CANDIDATES = (48, 16, 12, 8, 6, 4, 3, 2, 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def unroll(nb):
    """U of launch_reduce<NB>: loads in flight per lane and array."""
    return 8 if nb == 1 else (4 if nb <= 4 else 2)


U_CLASSES = {8: (1,), 4: (2, 3, 4), 2: tuple(range(5, 17))}


# ---------------------------------------------------------------------------------------- geometry (k2_geometry, tph_partition)
Part = namedtuple("Part", "T n_loc vl V nv canonical")
Geom = namedtuple("Geom", "n n_loc nv RB T vl V BPP PPB bv canonical")
Run = namedtuple("Run", "block r0 r1")          # rows [r0, r1) of one piece, read by workgroup `block`


def vshards_for(n_global):
    for c in VSHARD_CANDIDATES:
        if n_global > 0 and n_global % (c * 256) == 0:
            return c
    return 1


def partition(n_t):
    """tph_partition on one GPU (world = 1, n_global_t = n_local_t), restated."""
    n_t = [int(v) for v in n_t]
    n = sum(n_t)
    if any(v != n_t[0] for v in n_t):
        return Part(1, n, 1, 1, n, False)
    nl = n_t[0]
    if nl % 256 == 0:
        V = vshards_for(nl)
        return Part(len(n_t), nl, V, V, nl // V, True)
    return Part(len(n_t), nl, 1, 1, nl, False)


def geometry(n_t, reduce_grid=0):
    """k2_geometry, restated."""
    p = partition(n_t)
    cap = reduce_grid if reduce_grid > 0 else RED_BLOCKS
    bv_max = max(cap // p.V, 1)
    rb = -(-(p.nv * p.T) // bv_max)
    rb = -(-rb // 4096) * 4096
    floor_rows = -(-p.nv // 4096) * 4096 if p.nv < 16384 else 16384
    rb = max(rb, floor_rows)
    if rb >= p.nv:
        ppb = min(rb // p.nv, p.T)
        bpp, bv = 1, -(-p.T // ppb)
    else:
        bpp = -(-p.nv // rb)
        ppb, bv = 1, p.T * bpp
    return Geom(sum(int(v) for v in n_t), p.n_loc, p.nv, rb, p.T, p.vl, p.V, bpp, ppb, bv, p.canonical)


def block_span(g, bb):
    """(t0, t1, q0, q1) of block bb of a shard: pieces [t0, t1), rows [q0, q1) of each."""
    if g.BPP == 1:
        t0 = bb * g.PPB
        return t0, min(t0 + g.PPB, g.T), 0, g.nv
    t0 = bb // g.BPP
    q0 = (bb - t0 * g.BPP) * g.RB
    return t0, t0 + 1, q0, min(q0 + g.RB, g.nv)


def runs(g):
    """Every contiguous row run of the pass, in block order."""
    out = []
    for v in range(g.vl):
        for bb in range(g.bv):
            t0, t1, q0, q1 = block_span(g, bb)
            for t in range(t0, t1):
                r0 = t * g.n_loc + v * g.nv + q0
                out.append(Run(v * g.bv + bb, r0, r0 + (q1 - q0)))
    return out


def split_run(r):
    """-> (odd-end rows taken by thread 0, first and last row of the pair loop) as k_reweight_reduce splits a run."""
    r0, r1, odd = r.r0, r.r1, []
    if (r0 & 1) and r0 < r1:
        odd.append(r0)
        r0 += 1
    if (r1 & 1) and r0 < r1:
        odd.append(r1 - 1)
        r1 -= 1
    return odd, r0, r1


def describe(g):
    """What a geometry reaches, for the assertions of the cases table."""
    rr = runs(g)
    shard0 = [block_span(g, bb) for bb in range(g.bv)]
    splits = [split_run(r) for r in rr]
    return dict(g._asdict(), blocks=g.vl * g.bv,
                pieces=[t1 - t0 for t0, t1, _, _ in shard0], block_rows=[q1 - q0 for _, _, q0, q1 in shard0],
                odd_r0=any(r.r0 & 1 for r in rr), odd_r1=any(r.r1 & 1 for r in rr),
                no_pairs=any(a == b for _, a, b in splits),
                lane_trips=-(-g.bv // 64))


def covers_once(g):
    """Every row of the history lies in exactly one run."""
    cnt = np.zeros(g.n + 1, dtype=np.int64)
    for r in runs(g):
        cnt[r.r0] += 1
        cnt[r.r1] -= 1
    return bool(np.all(np.cumsum(cnt)[:-1] == 1))


def edge_rows(g):
    """First and last row of every run, every odd-end row, and the last pair of every run: where a row is dropped or doubled."""
    e = set()
    for r in runs(g):
        odd, a, b = split_run(r)
        e.update((r.r0, r.r1 - 1))
        e.update(odd)
        if b - a >= 2:
            e.update((b - 2, b - 1))
    return np.array(sorted(e), dtype=np.int64)


def odd_end_rows(g):
    return np.array(sorted({x for r in runs(g) for x in split_run(r)[0]}), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------- exact counts
L_OFF = -2.0 ** 40
COUNT_BETAS = np.array([1.0, 2.0 ** -20, 0.5, 0.75, 2.0 ** -10, 0.0, 3 * 2.0 ** -12, 0.625, 2.0 ** -19, 0.3125, 2.0 ** -5, 0.875,
                        2.0 ** -15, 5 * 2.0 ** -18, 0.09375, 2.0 ** -1 + 2.0 ** -20])
COUNT_BETAS.setflags(write=False)
MAX_SINGLES = 12

CountGeom = namedtuple("CountGeom", "name n_t reduce_grid expect")


def _cg(rows, iters, grid=0, **expect):
    return CountGeom(f"{rows}x{iters}" + (f"-grid{grid}" if grid else ""), (rows,) * iters, grid, expect)


# rows x iterations, with the branch each pins (asserted from the restated geometry by tests/test_reweight_cases.py)
COUNT_GEOMS = (
    _cg(1, 1, canonical=False, blocks=1, no_pairs=True),
    _cg(2, 1, canonical=False, blocks=1, odd_r0=False, odd_r1=False),
    _cg(3, 1, canonical=False, blocks=1, odd_r1=True),
    _cg(777, 9, canonical=False, V=1, PPB=5, bv=2, pieces=[5, 4], odd_r0=True, odd_r1=True),
    _cg(256, 5, canonical=True, V=1, nv=256, PPB=5, bv=1),
    _cg(512, 7, canonical=True, V=2, nv=256), _cg(768, 7, canonical=True, V=3, nv=256),
    _cg(1024, 7, canonical=True, V=4, nv=256), _cg(1536, 7, canonical=True, V=6, nv=256),
    _cg(2048, 7, canonical=True, V=8, nv=256), _cg(3072, 7, canonical=True, V=12, nv=256),
    _cg(4096, 7, canonical=True, V=16, nv=256),
    _cg(4096, 1, canonical=True, V=16, nv=256, T=1, PPB=1, bv=1),
    _cg(12288, 40, canonical=True, V=48, nv=256, PPB=16, bv=3, pieces=[16, 16, 8]),
    _cg(12288, 40, 1, canonical=True, V=48, PPB=40, bv=1, RB=12288),
    _cg(12288, 40, 96, canonical=True, V=48, PPB=32, bv=2, pieces=[32, 8]),
    _cg(12288, 40, 1 << 20, canonical=True, V=48, RB=4096, PPB=16, bv=3),
    _cg(34304, 3, canonical=True, V=2, nv=17152, RB=16384, BPP=2, bv=6, block_rows=[16384, 768] * 3),
    _cg(40001, 3, canonical=False, V=1, BPP=3, bv=9, odd_r0=True, odd_r1=True),
    _cg(1280, 200, canonical=True, V=1, PPB=3, bv=67, lane_trips=2),
    _cg(1064961, 1, canonical=False, BPP=66, bv=66, odd_r1=True, block_rows=[16384] * 65 + [1]),
    CountGeom("4097-unequal", (1365, 1366, 1366), 0, dict(canonical=False, T=1, V=1, nv=4097, blocks=1, odd_r1=True)),
)
COUNT_WIDTH_GEOMS = ("777x9", "34304x3")
COUNT_BY_NAME = {c.name: c for c in COUNT_GEOMS}


def count_history(c, on):
    """(logl, beta_t, logz_t, n_t) of the count history with the rows of the mask `on` switched on."""
    T = len(c.n_t)
    return np.where(on, 0.0, L_OFF), np.zeros(T), np.zeros(T), np.array(c.n_t, dtype=np.int64)


def single_edges(g):
    """At most MAX_SINGLES edge rows for the one-row-on patterns: odd ends first, then the ends of the history, then a spread."""
    e, odd = edge_rows(g), odd_end_rows(g)
    first = [odd[0], odd[-1], odd[len(odd) // 2]] if odd.size else []
    spread = e[np.unique(np.linspace(0, e.size - 1, MAX_SINGLES).astype(np.int64))]
    out = []
    for r in [*first, 0, g.n - 1, *spread]:
        if int(r) not in out:
            out.append(int(r))
    return out[:MAX_SINGLES]


def count_patterns(c):
    """(label, mask of the rows that are on): two random halves, the edges and their complement, single edge rows, no row."""
    g = geometry(c.n_t, c.reduce_grid)
    for seed in (1, 2):
        yield f"half{seed}", np.random.RandomState(seed).rand(g.n) < 0.5
    e = np.zeros(g.n, dtype=bool)
    e[edge_rows(g)] = True
    yield "edges", e
    yield "not-edges", ~e
    for r in single_edges(g):
        m = np.zeros(g.n, dtype=bool)
        m[r] = True
        yield f"row{r}", m
    yield "all-off", np.zeros(g.n, dtype=bool)


def count_expected(C, n, n_on, betas):
    """The triples [(m, s1, s2)] the pass must return, bit for bit, for the cached constant C."""
    out = np.empty((len(betas), 3))
    for i, b in enumerate(betas):
        if b == 0.0:
            out[i] = (-C, n, n)
        elif n_on:
            out[i] = (-C, n_on, n_on)
        else:
            out[i] = (b * L_OFF - C, n, n)          # b * L_OFF is exact: one rounding, fused or not
    return out


# --------------------------------------------------------------------------------- the long-double references of K1 and K2
def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def mixture_terms(logl, bt, zt, nt):
    """a[s][t] = l_s beta_t - logZ_t + log n_t in long double."""
    with np.errstate(invalid="ignore"):
        return _ld(logl)[:, None] * _ld(bt)[None, :] - _ld(zt)[None, :] + np.log(_ld(nt))[None, :]


def lse_rows(a):
    """log sum_t exp(a[s][t]) in long double; -inf where every term is, NaN where one is."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(a, axis=1)
        safe = np.where(np.isfinite(m), m, LD(0))
        out = safe + np.log(np.sum(np.exp(a - safe[:, None]), axis=1))
        return np.where(np.isnan(m), LD(np.nan), np.where(m == -np.inf, LD(-np.inf), out))


def logmix_reference(logl, bt, zt, nt):
    return lse_rows(mixture_terms(logl, bt, zt, nt))


def _term_error(logl, bt, zt, nt):
    """|error| of the device's a[s][t], fused or not: the product, the subtraction, the addition, and log n_t within an ulp."""
    with np.errstate(invalid="ignore"):
        p = _ld(logl)[:, None] * _ld(bt)[None, :]
        q = p - _ld(zt)[None, :]
        ln = np.log(_ld(nt))[None, :]
        return (U * (np.abs(p) + np.abs(q) + np.abs(q + ln)) + 2 * U * np.abs(ln)).astype(np.float64)


def _lae_bound(x, y, r):
    """|error| of tph_logaddexp(x, y) with exact result r on exact arguments, as tests/lean_math_cases.py (truth_logaddexp) derives it:
    U (|r| + (2 + |t|) q + 3 log1p(E)) + 8 U^2 + one subnormal step, t = x - y, E = exp(-|t|), q = E / (1 + E)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.abs(x - y).astype(np.float64)
        E = np.exp(-t)
        return U * (np.abs(r).astype(np.float64) + (2.0 + t) * E / (1.0 + E) + 3.0 * np.log1p(E)) + 8 * U * U + SUBNORMAL


def logmix_bounds(logl, bt, zt, nt, route, entered=None):
    """|error| per row of the cached log-mixture.

    route "load": all T terms by the streaming log-sum-exp of k_logmix_append: with p_t the softmax of the terms, the sum
    sum_t exp(a_t - m) carries, per term, the term's own error and the maximum's, the subtraction U |a_t - M| (telescoped over the
    rescales), the exp (2 U) and, per rescale, an exp and a product (3 U, at most T - 1 of them), and T - 1 additions; the weighted
    mean Y of expm1 of that moves the logarithm by at most Y / (1 - Y); then the library log (2 U |log sum|) and the final sum U |C|.

    route "append": the rows of iteration k enter by the streaming sum over the k + 1 terms known then; every later commit folds one
    term in with tph_logaddexp, which is 1-Lipschitz in the larger error of its arguments and adds its own bound (_lae_bound)."""
    a = mixture_terms(logl, bt, zt, nt)
    err = _term_error(logl, bt, zt, nt)
    T = len(bt)
    if entered is None:         # (given: the iteration each row of a slice of the history entered with)
        entered = np.repeat(np.arange(T), np.asarray(nt, dtype=np.int64)) if route == "append" else np.full(len(logl), T - 1)
    out = np.full(len(logl), np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in np.unique(entered):
            rows = np.flatnonzero(entered == k)
            ak, ek = a[rows, :k + 1], err[rows, :k + 1]
            m = np.max(ak, axis=1)
            c = lse_rows(ak)
            p = np.exp(ak - c[:, None]).astype(np.float64)
            emax = np.take_along_axis(ek, np.argmax(ak, axis=1)[:, None], axis=1)
            theta = ek + emax + U * np.abs(ak - m[:, None]).astype(np.float64) + 2 * U + 3 * U * k + U * k
            Y = np.sum(np.where(p > 0, p * np.expm1(theta), 0.0), axis=1)
            e = Y / (1.0 - Y) + 2 * U * np.abs(c - m).astype(np.float64) + U * np.abs(c).astype(np.float64)
            for t in range(k + 1, T):
                c_new = lse_rows(a[rows, :t + 1])
                e = np.maximum(e, err[rows, t]) + _lae_bound(c, a[rows, t], c_new)
                c = c_new
            out[rows] = e * (1.0 + REF_SHARE)
    return out


# ---------------------------------------------------------------------------------------------- K2: reference and bound
Triple = namedtuple("Triple", "m s1 s2 v")          # long double; v[n] the exact v_s = beta l_s - C_s


def acc_reference(logl, C, beta):
    """(max v, sum e^(v - max), sum e^(2 (v - max))) in long double for the given cached C.  NaN rows make NaN sums; the maximum is
    taken over the other rows, as fmax does."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = LD(beta) * _ld(logl) - _ld(C)
        ok = ~np.isnan(v)
        m = np.max(v[ok]) if ok.any() else LD(-np.inf)
        if m == -np.inf:
            return Triple(m, LD(np.nan) if not ok.all() else LD(0), LD(np.nan) if not ok.all() else LD(0), v)
        e = np.exp(v - m)
        return Triple(m, np.sum(e), np.sum(e * e), v)


def path_counts(g, nb):
    """(R, A): rescales and additions on the longest path of one term through the pass.
    Lane: one rescale and one accumulation per 4-row chunk (U / 2 chunks per trip) and per odd-end row, two additions inside the
    chunk; block: one rescale, 6 shuffle levels and the 4 wave sums; shard: one rescale per partial, ceil(bv / 64) additions per lane
    and 6 shuffle levels; fold: V - 1 merges of one rescale and one addition each."""
    u = unroll(nb)
    per_block = {}
    for r in runs(g):
        odd, a, b = split_run(r)
        per_block[r.block] = per_block.get(r.block, 0) + len(odd) + -(-((b - a) // 2) // (THREADS * u)) * (u // 2)
    chunks = max(per_block.values())
    return chunks + 2 + (g.V - 1), (chunks + 2) + (6 + 4) + (-(-g.bv // 64) + 6) + (g.V - 1)


AccBound = namedtuple("AccBound", "m s1 s2 logz ess")


def _v_rounding(logl, beta, ref):
    """(U (|beta l| + |v|) per row in float64, rows whose v is a finite double on the device)."""
    with np.errstate(invalid="ignore", over="ignore"):
        blx = np.abs(LD(beta) * _ld(logl))
        ok = np.isfinite(ref.v) & (blx <= DBL_MAX)      # beyond: the device's product overflows, v = -inf, the term is exactly 0
        return U * np.where(ok, blx, 0).astype(np.float64) + U * np.where(ok, np.abs(ref.v), 0).astype(np.float64), ok


def max_bound(logl, beta, ref):
    """|m - max v|: the largest rounding of v among the rows that can be the maximum."""
    ev, ok = _v_rounding(logl, beta, ref)
    if not ok.any():
        return 0.0
    v = np.where(ok, ref.v, -np.inf).astype(np.float64)
    return float(np.max(ev[v + ev >= float(ref.m) - ev[np.argmax(v)]])) * (1 + REF_SHARE)


def acc_bound(logl, beta, ref, g, nb):
    """Bounds for the triple of one beta against acc_reference, derived from the inputs.

    Per term, the exponent of e = exp(v - m) is off by the rounding of the product and of the subtraction, U (|beta l| + |v|) --
    which covers the fused and the unfused form --, and by the subtractions of the running maxima on its way to the final one, which
    telescope to U |v - M|; the exp costs 2 U; each rescale an exp and a product (3 U; f * f and its product 6 U for s2, whose
    exponent errors double and whose e * e is one more rounding); each addition U.  The sums' relative errors are the means of
    expm1 of that, weighted with the terms themselves (all positive), plus one subnormal step for each of the n terms and at most n
    rescales where a value underflows.  The triples are compared after bringing the device's sums to the reference's maximum
    (exactly, in long double); logZ and ESS follow from the sums' bounds, logZ with the 2^-60 of the comparison's own long-double
    sum.  (The weights of the mean are formed in float64: they move the bound by 1e-13 of itself.)"""
    R, A = path_counts(g, nb)
    n = len(logl)
    ev, ok = _v_rounding(logl, beta, ref)
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.where(ok, ref.m - ref.v, 0).astype(np.float64)
        e = np.where(ok, np.exp(-dist), 0.0)
        p1, p2 = e / float(ref.s1), e * e / float(ref.s2)
        t1 = ev + U * dist + 2 * U + 3 * U * R + U * A
        t2 = 2 * ev + 2 * U * dist + 5 * U + 6 * U * R + U * A
        under = 2.0 * n * SUBNORMAL
        b1 = float(np.sum(np.where(p1 > 0, p1 * np.expm1(t1), 0.0))) * (1 + REF_SHARE) + under / float(ref.s1)
        b2 = float(np.sum(np.where(p2 > 0, p2 * np.expm1(t2), 0.0))) * (1 + REF_SHARE) + under / float(ref.s2)
    return AccBound(max_bound(logl, beta, ref), b1, b2,
                    b1 / (1 - b1) + 2.0 ** -60 * (1 + abs(float(ref.m)) + abs(math.log(float(ref.s1)))), (1 + b1) ** 2 / (1 - b2) - 1)


def acc_errors(got, ref):
    """(|m - m_ref|, rel. error of s1, of s2, |logZ - logZ_ref|, rel. error of ESS) of a device triple, in long double; the sums are
    first brought to the reference's maximum."""
    m, s1, s2 = (LD(float(x)) for x in got)
    sc = np.exp(m - ref.m)
    a1, a2 = s1 * sc, s2 * sc * sc
    lz, lz_ref = m + np.log(s1), ref.m + np.log(ref.s1)
    ess, ess_ref = s1 * s1 / s2, ref.s1 * ref.s1 / ref.s2
    return tuple(float(x) for x in (abs(m - ref.m), abs(a1 - ref.s1) / ref.s1, abs(a2 - ref.s2) / ref.s2, abs(lz - lz_ref),
                                    abs(ess - ess_ref) / ess_ref))


# ----------------------------------------------------------------------------------------------- K2: the realistic histories
ACC_BETAS = np.array([0.0, 1e-4, 0.05, 0.37, 0.9, 1.0, 0.2, 0.21, 0.22, 0.23, 0.5, 0.51, 0.52, 0.53, 0.54, 0.7])
ACC_BETAS.setflags(write=False)
ACC_LIMIT = 1e-12               # the realistic inputs are chosen so that every bound stays below this (checked on the CPU)
ACC_GEOMS = ((777, 9), (12288, 40), (34304, 3), (1064961, 1))
History = namedtuple("History", "logl bt zt nt")


def schedule(T):
    """beta_t rising from 0 with two leading zeros (one where T < 3), logZ_t falling."""
    bt = np.concatenate([np.zeros(min(2, T)), np.linspace(0.0, 0.6, max(T - 1, 1))[1:][:max(T - 2, 0)]])
    return bt, -1.5 * np.arange(T, dtype=np.float64)


@functools.lru_cache(maxsize=8)
def realistic(rows, T, seed=0):
    rs = np.random.RandomState(7000 + 13 * T + seed)
    logl = -rs.chisquare(10, size=rows * T) * 1.5
    bt, zt = schedule(T)
    logl.setflags(write=False)
    return History(logl, bt, zt, np.full(T, rows, dtype=np.int64))


def exact_case():
    """4099 rows in three unequal iterations (the one-piece geometry, an odd end): the case of the exact maximum and of k_logw."""
    rs = np.random.RandomState(4099)
    nt = np.array([1366, 1366, 1367], dtype=np.int64)
    return History(-rs.chisquare(10, size=4099) * 1.5, np.array([0.0, 0.0, 0.3]), np.array([0.0, -1.5, -3.0]), nt)


EXACT_BETAS = (0.37, 1.0, 0.05, 1.0 / 3.0)


def _round(fr):
    return float(fr)                                 # int / int true division: correctly rounded


def two_forms(beta, logl, sub):
    """(fused, unfused): fl(beta l - sub) and fl(fl(beta l) - sub), each correctly rounded, per row."""
    fb = Fraction(float(beta))
    fused = np.array([_round(fb * Fraction(float(x)) - Fraction(float(c))) for x, c in zip(logl, sub)])
    unfused = np.asarray(beta * np.asarray(logl, dtype=np.float64), dtype=np.float64) - np.asarray(sub, dtype=np.float64)
    return fused, unfused


def log_nh(n):
    """log((double) n) as the host library forms it for k_logw (the C library's log, which math.log calls)."""
    return math.log(float(n))


# --------------------------------------------------------------------------------------------------- K2: edges of the range
def acc_edges():
    """name -> (History, trial betas, note).  Geometries: 777 x 9 (odd piece starts and ends) and 34 304 x 3 (two shards of two
    blocks per piece)."""
    out = {}
    h = realistic(777, 9)
    hi = (0.7, 0.9, 1.0)                             # above every beta_t: v rises with l
    out["ascending"] = (h._replace(logl=np.sort(h.logl)), hi, "v ascending along the history: a rescale at every chunk")
    l = h.logl.copy()
    l[-1] = l.max() + 5.0
    out["max-last-row"] = (h._replace(logl=l), hi, "the maximum in the very last row (an odd-end row of the last piece)")
    l = h.logl.copy()
    l[777] = l.max() + 5.0
    out["max-odd-start"] = (h._replace(logl=l), hi, "the maximum in the odd first row of piece 1")
    l = h.logl.copy()
    l[5::7] -= 400.0
    l[3::11] -= 2000.0
    out["spread"] = (h._replace(logl=l), (1.0, 0.9), "terms 400 below the maximum (e^2 underflows) and 2000 below (e underflows)")
    # v = -inf with a finite C: l = -DBL_MAX under beta = 2 (beta l overflows); under beta <= 1 the same rows are finite and far away
    h2 = realistic(34304, 3)
    pos = History(h2.logl, np.array([0.25, 0.5, 0.75]), h2.zt, h2.nt)
    g = geometry(pos.nt)
    l = pos.logl.copy()
    l[16384:17152] = -DBL_MAX                       # piece (0, 0), second block: a whole block
    out["overflow-block"] = (pos._replace(logl=l), (2.0, 1.0, 0.875), "a whole block of v = -inf rows among finite ones")
    l = pos.logl.copy()
    for t in range(3):
        l[t * g.n_loc + g.nv:(t + 1) * g.n_loc] = -DBL_MAX
    out["overflow-shard"] = (pos._replace(logl=l), (2.0, 1.0, 0.875), "a whole virtual shard of v = -inf rows")
    out["overflow-all"] = (pos._replace(logl=np.full(pos.logl.size, -DBL_MAX)), (2.0, 1.5), "every row v = -inf: (-inf, 0, 0)")
    # literal -inf and NaN: NaN sums, on the device as in the reference
    l = pos.logl.copy()
    l[100:200] = -np.inf
    out["neg-inf"] = (pos._replace(logl=l), (1.0, 0.875), "l = -inf with every beta_t > 0: C = -inf, v = NaN")
    l = pos.logl.copy()
    l[16385] = np.nan
    out["nan-row"] = (pos._replace(logl=l), (1.0, 0.875), "a NaN row: NaN sums, the maximum of the others")
    return out


# ------------------------------------------------------------------------------------------------------------------ K1 cases
def logmix_cases():
    """name -> History for the two routes (history_load; one history_append per iteration)."""
    out = {}
    T = 40
    rs = np.random.RandomState(40)
    bt, zt = schedule(T)
    out["T40"] = History(-rs.chisquare(10, size=97 * T) * 1.5, bt, zt, np.full(T, 97, dtype=np.int64))
    nt = np.array([33, 64, 65, 1, 200, 255, 257], dtype=np.int64)
    out["ragged"] = History(-rs.chisquare(4, size=int(nt.sum())) * 20.0, np.array([0, 0, 0.01, 0.05, 0.2, 0.5, 0.9]),
                            -np.array([0, 0.5, 3.0, 9.0, 20.0, 31.0, 40.0]), nt)
    # equal terms: iterations 0/1 and 2/3 are the same (beta, logZ, n): a == m in the streaming sum, x == y in tph_logaddexp
    out["equal"] = History(-rs.chisquare(10, size=4 * 130), np.array([0.0, 0.0, 0.5, 0.5]), np.array([0.0, 0.0, -2.0, -2.0]),
                           np.full(4, 130, dtype=np.int64))
    l = -rs.chisquare(10, size=5 * 100)
    l[7::13] = -np.inf
    out["neg-inf"] = History(l, np.array([0.1, 0.2, 0.3, 0.4, 0.5]), -np.arange(5.0), np.full(5, 100, dtype=np.int64))
    out["nan"] = History(l, np.array([0.1, 0.2, 0.0, 0.4, 0.5]), -np.arange(5.0), np.full(5, 100, dtype=np.int64))
    return out


# size_old, rows appended: the capped grid of k_logmix_append (2048 x 256 threads) and its two-pairs-in-flight loop
APPEND_LARGE = ((1048579, 7), (3145731, 600001))
APPEND_STRIDE = RED_BLOCKS * 256


def append_large(size_old, n_new):
    rs = np.random.RandomState(size_old % 1000)
    logl = -rs.chisquare(10, size=size_old + n_new) * 1.5
    return History(logl, np.array([0.0, 0.4]), np.array([0.0, -2.5]), np.array([size_old, n_new], dtype=np.int64))


def append_loop_shape(size_old, size_new):
    """k_logmix_append's loops, restated for threads 0 and 1: grid, (trips of the two-in-flight body, remainder taken) of each, and
    whether the last old row is odd and falls to the scalar tail."""
    grid = min(max(-(-size_new // 256), 1), RED_BLOCKS)
    stride, pairs = grid * 256, size_old >> 1
    out = {"grid": grid, "odd_tail": bool(size_old & 1)}
    for tid in (0, 1):
        p, body = tid, 0
        while p + stride < pairs:
            body, p = body + 1, p + 2 * stride
        out[tid] = (body, p < pairs)
    return out


# ------------------------------------------------------------------------------------------------------------------ K3 cases
SSM_SIZES = (1, 255, 1025, 263169, 2098177)
SSM_UNIT = 2.0 ** -20


def ssm_grid(n):
    """Blocks of k_sum_sq_max: tph_grid_for(n, 256, 4)."""
    return min(max(-(-n // 1024), 1), RED_BLOCKS)


def ssm_max_rows(n):
    """Rows for the unique maximum: the last row (the last, ragged grid-stride trip), the last row of the last block's first trip,
    and row 0."""
    last_block = min((ssm_grid(n) - 1) * 256 + 255, n - 1)
    return sorted({n - 1, last_block, 0})


def ssm_weights(n, max_row, seed=0):
    """(k, w = k 2^-20): k < 1023, about a third zero, and 1023 in max_row alone."""
    rs = np.random.RandomState(900 + seed + n % 997)
    k = rs.randint(0, 1023, size=n).astype(np.int64)
    k[rs.rand(n) < 1.0 / 3.0] = 0
    k[max_row] = 1023
    return k, k.astype(np.float64) * SSM_UNIT


def ssm_expected(k):
    """(sum, sum of squares, max), exact: the absolute terms stay below 2^53 units of 2^-20 and 2^-40 (asserted)."""
    s, q = int(k.sum()), int((k * k).sum())
    assert s < LIMIT and q < LIMIT
    return np.array([s * SSM_UNIT, q * SSM_UNIT * SSM_UNIT, int(k.max()) * SSM_UNIT])


def weights_reference(logl, C, beta, vmax, s1):
    """w = exp(beta l - C - vmax) / s1 in long double, for the (vmax, s1) handed to k_weights."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = LD(beta) * _ld(logl) - _ld(C)
        e = np.exp(v - LD(vmax))
        return e / LD(s1), v, e


def weights_bound(logl, beta, v, vmax, w):
    """(relative, absolute) error bound per row of k_weights: the exponent's roundings U (|beta l| + |v| + |v - vmax|), the exp
    (2 U) and the division (U); one subnormal step where the weight is not a normal number.  Rows whose exact weight lies below half
    the smallest subnormal must come out as exactly 0 (their bound is 0 + one step, and the device value is compared with 0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        th = U * (np.abs(LD(beta) * _ld(logl)) + np.abs(v) + np.abs(v - LD(vmax))).astype(np.float64) + 3 * U
        return np.expm1(th) * (1 + REF_SHARE), np.where(np.asarray(w, dtype=np.float64) < 2.0 ** -1021, SUBNORMAL, 0.0)


def ssm_additions(n):
    """Additions on the longest path of k_sum_sq_max + k_sum_sq_max_final: grid-stride trips, 6 + 6 shuffle levels, twice."""
    g = ssm_grid(n)
    return -(-n // (g * 256)) + 12 + -(-g // 256) + 12

"""References and input sets for the Metropolis accept, its canonical sums and the step adaptation (csrc/mutate.hip: k_accept,
k_accept_sums, k_adapt; csrc/common.h: tph_tpcn_factor, tph_block_sum, tph_adapt_scalar).  CPU only, NumPy only: shared by
tests/test_accept_ref.py (which checks these helpers against independent formulations) and tests/test_accept_adapt_gpu.py (which
holds the device to them).

Two kinds of reference live here.  `alpha_ref` evaluates the FORMULA at higher precision and comes with an error bound; the sums
(`block_partials_ref`, `sums_ref`) and the adaptation (`adapt_ref`) restate the device's ORDER OF OPERATIONS in float64, so the
comparison is bit for bit."""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53

# ------------------------------------------------------------------------------------------------ per-row tolerance
# The device's alpha is held to  C_DEVICE * b_i  relative, b_i from alpha_ref.  ORACLE_WORST_RATIO is the largest error of the
# float64 oracle (oracle.mcmc.accept: NumPy's log and exp on the same doubles) in units of b_i over every committed input set
# (tests/test_accept_ref.py measures it: 0.6727, at tpCN d = 100, beta = 0.6, rounded up here, and asserts that the measurement
# stays between half this constant and this constant); the factor 4 is for tph_log (< 1 ulp), tph_div and the contracted
# beta * dl + factor rounding differently from libm.  Measured against the reference, never fitted to the device: the worst DEVICE
# ratio of the MI355X run that went with this file was 0.6727 as well (tpCN, d = 100, beta = 0.6, the same row: at large forms the
# rounding of 1 + m / nu dominates, and that operation is IEEE on both sides); RWM: 0.43 (test_alpha_per_row_within_the_bound
# prints the worst row of every case).
ORACLE_WORST_RATIO = 0.7
C_DEVICE = 4.0 * ORACLE_WORST_RATIO

KERNELS = ("tpcn", "rwm")
BETAS = (0.0, 0.6, 1.0)
DOFS4 = (0.7, 4.0, 25.0, 1e6)          # per-row dof of the per-row alpha test (K = n)
DOFS3 = (1e6, 4.0, 25.0)               # the three clusters of the K = 3 calls
ALPHA_DIMS = (1, 10, 16, 50, 100)
ALPHA_N = 4096
SEED, TICK, ITEM0 = 0x5EEDACCE97, 23, 1_000_003

# ---------------------------------------------------------------------------------------------------- case tables
X = "x"        # a finite form of ordinary size (the dimension d)
INF, NAN = float("inf"), float("nan")
# (logl, logl'): finite / +-inf / NaN pairs (forms finite)
LIKELIHOOD_PAIRS = [(-3.5, INF), (-3.5, -INF), (-INF, -INF), (INF, INF), (-INF, -2.25), (NAN, -2.25), (-3.5, NAN),
                    (0.0, -800.0),        # exp underflows to exactly 0 at beta = 1, a normal 1e-209 at beta = 0.6
                    (0.0, -1300.0),       # exactly 0 at beta = 0.6 too
                    (0.0, 800.0),         # exp overflows: alpha = 1
                    (-3.0, -3.0)]         # with equal forms the exponent is exactly 0
# (m, m'): Mahalanobis forms 0, +inf, NaN on either side and on both (likelihoods finite)
FORM_PAIRS = [(0.0, X), (X, 0.0), (0.0, 0.0), (INF, X), (X, INF), (INF, INF), (NAN, X), (X, NAN), (NAN, NAN), (INF, NAN),
              (NAN, INF), (0.0, INF), (INF, 0.0), (X, X)]
# 1 + m / nu just below / above the 1e300 at which tph_tpcn_factor leaves the lean log: (side of m, side of m'); the two forms
# are exp(+-0.7 / (0.5 (d + nu))) apart, so the factor itself is +-0.7 or +-1.4 and alpha is an ordinary number
BIG_FORM_SIDES = [(-2, -1), (-1, 1), (1, -1), (1, 2), (-1, -2), (2, 1)]
BIG_LIKELIHOOD = (-3.0, -4.5)

Rows = namedtuple("Rows", "kernel d n dofs cluster nu logl loglp maha_u maha_up")


def edge_rows(d, dofs):
    """The edge table as rows (logl, logl', m, m', index into dofs)."""
    out = []
    x = float(d)
    for j, nu in enumerate(dofs):
        for l0, l1 in LIKELIHOOD_PAIRS:
            same = l0 == l1 == -3.0
            out.append((l0, l1, 0.9 * x, 0.9 * x if same else 1.1 * x, j))
        for m0, m1 in FORM_PAIRS:
            out.append((-3.5, -3.0, x if m0 == X else m0, x if m1 == X else m1, j))
        r = math.exp(0.7 / (0.5 * (d + nu)))
        for s0, s1 in BIG_FORM_SIDES:
            out.append((BIG_LIKELIHOOD[0], BIG_LIKELIHOOD[1], 1e300 * nu * r ** s0, 1e300 * nu * r ** s1, j))
    return out


@functools.lru_cache(maxsize=None)
def rows(kernel, d, n, dofs, seed, edges=True):
    """One committed input set: the edge table first (cut to n rows), then random rows -- forms 1e-3 ... 1e4 times a chi^2_d
    draw at u; at u' either a factor of ordinary size (so that alpha is spread over (0, 1)) or an unrelated form."""
    rs = np.random.RandomState(seed)
    E = edge_rows(d, dofs) if edges else []
    E = E[:n]
    m = n - len(E)
    cl = rs.randint(len(dofs), size=m)
    nu = np.asarray(dofs)[cl]
    mu = 10.0 ** rs.uniform(-3, 4, size=m) * rs.chisquare(d, size=m)
    t = 1.5 * rs.randn(m)
    targeted = nu * ((1.0 + mu / nu) * np.exp(t / (0.5 * (d + nu))) - 1.0)
    loose = mu * np.exp(rs.choice([1e-3, 0.1, 1.0, 5.0], size=m) * rs.randn(m))
    mup = np.where((rs.rand(m) < 0.6) & (targeted > 0), targeted, loose)
    logl = -10.0 * rs.rand(m) - 0.5 * rs.chisquare(d, size=m)
    loglp = logl + 2.0 * rs.randn(m)
    # no random row in the subnormal range of exp (-745 ... -708), where a relative bound says nothing: such a row proposes its
    # own form instead (the range itself is probed by the edge table, from either side)
    fac = 0.5 * (d + nu) * (np.log1p(mup / nu) - np.log1p(mu / nu))
    for beta in BETAS:
        e = beta * (loglp - logl) + fac
        mup = np.where((e > -780) & (e < -680), mu, mup)
    col = lambda k, tail: np.concatenate([np.array([e[k] for e in E], dtype=tail.dtype), tail])  # noqa: E731
    cluster = col(4, cl.astype(np.int64)).astype(np.int32)
    out = Rows(kernel, d, n, dofs, cluster, np.asarray(dofs)[cluster], col(0, logl), col(1, loglp), col(2, mu), col(3, mup))
    for a in out[4:]:
        a.setflags(write=False)
    return out


def alpha_rows(kernel, d):
    """Input set of the per-row alpha test: 4096 rows, per-row dof from DOFS4."""
    return rows(kernel, d, ALPHA_N, DOFS4, 1000 + d)


def decision_rows(kernel, n, K):
    """Input sets of the decision / write tests and of the block partials (d = 10): K = 3 clusters with DOFS3, or one."""
    return rows(kernel, 10, n, DOFS3 if K == 3 else (4.0,), 2000 + n + K)


def sum_rows(kernel, n, K):
    """Input sets of the canonical-sum tests: random rows only, K clusters with the dofs of DOFS4 in turn."""
    return rows(kernel, 3, n, tuple(DOFS4[k % 4] for k in range(K)), 3000 + n % 9973 + K, edges=False)


def uniforms(n, tick=TICK):
    from oracle import philox as px
    return px.uniform1(SEED, np.arange(n, dtype=np.uint64) + np.uint64(ITEM0), tick, px.TAG_ACCEPT)


# --------------------------------------------------------------------------------------------------- alpha, per row
def exponent_ref(kernel, beta, logl, loglp, maha_u, maha_up, nu, d):
    """The argument of exp in the Metropolis probability and the (d + nu)(2 + log au + log ap) term of its bound, long double."""
    with np.errstate(all="ignore"):
        arg = LD(beta) * (np.asarray(loglp, dtype=LD) - np.asarray(logl, dtype=LD))
        spread = np.zeros(arg.shape, dtype=LD)
        if kernel == "tpcn":
            nu = np.asarray(nu, dtype=LD)
            la = np.log(1 + np.asarray(maha_u, dtype=LD) / nu)
            lp = np.log(1 + np.asarray(maha_up, dtype=LD) / nu)
            arg = arg + LD(0.5) * (d + nu) * (lp - la)
            spread = (d + nu) * (2 + la + lp)
    return arg, spread


def alpha_ref(kernel, beta, logl, loglp, maha_u, maha_up, nu, d):
    """min(1, exp(beta (l' - l) + 1/2 (d + nu)(log(1 + m'/nu) - log(1 + m/nu)))), NaN -> 0: the formula of oracle.mcmc.accept on
    the same doubles in long double, rounded to float64.  Also returns the per-row RELATIVE error bound
    b_i = 2^-53 (4 + 2 |arg_i| + (d + nu_i)(2 + log au_i + log ap_i)): four roundings of ordinary operations, the exponent's own
    rounding (an absolute error of the exponent is a relative error of alpha) and the 2^-53 absolute loss of 1 + m / nu, which
    the log turns into at most 2^-53 and the factor multiplies by (d + nu) / 2, at either point."""
    arg, spread = exponent_ref(kernel, beta, logl, loglp, maha_u, maha_up, nu, d)
    with np.errstate(all="ignore"):
        a = np.where(np.isnan(arg), LD(0), np.minimum(LD(1), np.exp(arg)))
        b = EPS * (4 + 2 * np.abs(arg) + spread)
    return a.astype(np.float64), np.where(np.isfinite(b), b, 0).astype(np.float64)


def alpha_ratio(got, ref, bound):
    """|got - ref| in units of bound * ref per row; rows whose reference is exactly 0 or exactly 1 must be hit exactly (inf if
    not).  A reference within its bound of 1 may thus read 1, nothing may exceed 1."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    inner = (ref > 0) & (ref < 1)
    with np.errstate(all="ignore"):
        r = np.where(inner, np.abs(got - ref) / (bound * ref), np.where(got == ref, 0.0, np.inf))
    return np.where((got >= 0) & (got <= 1), r, np.inf)


def undecidable_rows(kernel, beta, r, c=C_DEVICE):
    """Rows of an input set on which a device inside its tolerance could still differ from the reference in KIND -- none may
    exist in a committed set: an exponent in (0, c b] (reference exactly 1, device below), and an exponent in the subnormal
    range of exp (the relative bound means nothing there)."""
    arg, _ = exponent_ref(kernel, beta, r.logl, r.loglp, r.maha_u, r.maha_up, r.nu, r.d)
    _, b = alpha_ref(kernel, beta, r.logl, r.loglp, r.maha_u, r.maha_up, r.nu, r.d)
    with np.errstate(invalid="ignore"):
        return np.nonzero(((arg > 0) & (arg <= c * b)) | ((arg > -746) & (arg < -707)))[0]


def ambiguous_decisions(alpha, bound, U, c=C_DEVICE):
    """Rows whose uniform lies within the device's tolerance of alpha: their decision could fall either way."""
    return np.nonzero(np.abs(U - alpha) <= c * bound * alpha)[0]


# ------------------------------------------------------------------------------------------- block partials, bit for bit
def _wave_tree(v):
    """tph_wave_sum, lane 0: __shfl_down offsets 32, 16, ..., 1 over the last axis (64 lanes)."""
    v = np.array(v, dtype=np.float64)
    o = 32
    while o:
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    return v[..., 0]


def block_partials_ref(alpha, accepted, assign, K):
    """What k_accept leaves in partials[block][1 + K]: column 0 the accepted rows, column 1 + k the alphas of cluster k, each
    by tph_block_sum over 256 threads -- the shuffle tree per wave, then the same tree over the four wave sums padded with
    zeros, i.e. (w0 + w2) + (w1 + w3).  Plain float64 additions in that order."""
    alpha = np.asarray(alpha, dtype=np.float64)
    n = alpha.size
    assign = np.zeros(n, dtype=np.int64) if assign is None else np.asarray(assign)
    nb = (n + 255) // 256
    cols = np.zeros((nb * 256, 1 + K))
    cols[:n, 0] = np.asarray(accepted, dtype=np.float64)
    ok = (assign >= 0) & (assign < K)
    cols[np.nonzero(ok)[0], 1 + assign[ok]] = alpha[ok]
    w = _wave_tree(cols.reshape(nb, 4, 64, 1 + K).transpose(0, 3, 1, 2))        # [block][col][wave]
    return (w[..., 0] + w[..., 2]) + (w[..., 1] + w[..., 3])


# ----------------------------------------------------------------------------------------- canonical sums, bit for bit
def partition_ref(n, world=1):
    """active_partition for a rank of `world` holding n / world of the n particles: (vl, V)."""
    from tempest_amd.device import vshards_for
    if n % 256 == 0:
        V = vshards_for(n)
        if V % world == 0:
            return V // world, V
    return 1, world


def sums_ref(partials, n, K, world=1):
    """(#accepted, sum alpha_c) of n particles from the block partials [block][1 + K] of `world` ranks in rank order (n / world
    particles each), as active_partition + vshard_colsums + vshard_fold form them: a rank's blocks are cut into its vl virtual
    shards of mper = nblocks / vl blocks; per (shard, column) one wave -- lane l adds blocks l, l + 64, ... in order from 0.0,
    then the shuffle tree --; the V shard sums of the run are folded left to right.  n % 256 != 0: one shard per rank."""
    ncol = 1 + K
    assert n % world == 0
    nb = (n // world + 255) // 256
    P = np.asarray(partials, dtype=np.float64).reshape(world, nb, ncol)
    vl, V = partition_ref(n, world)
    mper = nb // vl
    shard = []
    for r in range(world):
        for v in range(vl):
            src = P[r, v * mper:(v + 1) * mper]
            lanes = np.zeros((64, ncol))
            for b in range(0, mper, 64):
                chunk = src[b:b + 64]
                lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
            shard.append(_wave_tree(lanes.T))
    assert len(shard) == V
    out = shard[0]
    for v in range(1, V):
        out = out + shard[v]
    return out


def fsum_columns(partials, K):
    P = np.asarray(partials, dtype=np.float64).reshape(-1, 1 + K)
    return np.array([math.fsum(P[:, c]) for c in range(1 + K)])


# ----------------------------------------------------------------------------------------------- adaptation, bit for bit
def _fma(a, b, c):
    """a * b + c with one rounding (finite arguments; exact rational arithmetic, float() rounds to nearest even)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def adapt_ref(kernel, sums, counts, K, sigmas, steps_done, n_global, d, n_steps, n_max, contract=True, trace=None):
    """tph_adapt_scalar (csrc/common.h) in float64 Python, operation by operation: -> (sigmas, state[0..5]).

    Takes `counts` and `sums` where oracle.mcmc.adapt takes `assign` and `alpha`, so that empty clusters and n_global != n can
    be expressed.  `contract`: the library is compiled with -ffp-contract=on, under which the two multiply-adds of the function
    that stand in ONE expression -- sigma + rate * (mean - 0.234) and wsig += sigma_q * count_c -- are single fused operations
    (one rounding); contract=False rounds the product first, which is NumPy's arithmetic: that form equals oracle.mcmc.adapt
    exactly (tests/test_accept_ref.py), and the two forms differ by one rounding of a product in sigma and the weighted sigma."""
    mad = _fma if contract else (lambda a, b, c: a * b + c)
    sums = [float(v) for v in sums]
    counts = [float(v) for v in counts]
    sigmas = [float(v) for v in sigmas]
    iteration = int(steps_done) + 1
    sigma_0 = 2.38 / math.sqrt(float(d))
    rate = 1.0 / float(iteration + 1)
    alpha_tot = 0.0
    for c in range(K):
        alpha_tot += sums[1 + c]
        if counts[c] > 0.0:
            mean_accept = sums[1 + c] / counts[c]
            s = mad(rate, mean_accept - 0.234, sigmas[c])
            if kernel == "tpcn":
                s = min(max(s, 0.0), min(sigma_0, 0.99))
            sigmas[c] = s
    acc = sums[0] / float(n_global)
    wsum = wsig = smean = 0.0
    q = 0
    for c in range(K):
        smean += sigmas[c]
        if counts[c] > 0.0:
            wsig = mad(sigmas[q], counts[c], wsig)          # sigmas[:n_nonempty] with the non-empty sizes (mcmc.py:107-117)
            wsum += counts[c]
            q += 1
    weighted_sigma = wsig / wsum
    n_min = float(n_steps) * d
    ratio = sigma_0 / max(1e-6, weighted_sigma)
    n_adapt = float(n_steps) * d * (0.234 / max(0.01, acc)) * (ratio * ratio)
    n_final = min(max(n_min, n_adapt), float(n_max) * d)
    n_int = int(n_final)
    state = [float(iteration), 1.0 if iteration >= n_int else 0.0, acc, alpha_tot / float(n_global), (smean / K) / sigma_0,
             float(n_int)]
    if trace is not None:       # which branch each case takes (the CPU test checks that the grid reaches all of them)
        trace.update(n_min=n_min, n_adapt=n_adapt, cap=float(n_max) * d, weighted_sigma=weighted_sigma, acc=acc, sigmas=sigmas,
                     sigma_top=min(sigma_0, 0.99), done=iteration >= n_int, iteration=iteration, n_int=n_int)
    return np.array(sigmas), np.array(state)


AdaptCase = namedtuple("AdaptCase", "label kernel d K counts sums sigmas steps_done n_global n_steps n_max")


def _adapt_case(label, kernel, d, counts, means, acc, sigmas, steps_done, n_steps, n_max, n_scale=1):
    counts = [float(c) for c in counts]
    n = sum(counts)
    sums = [acc * n * n_scale] + [m * c for m, c in zip(means, counts)]
    return AdaptCase(label, kernel, d, len(counts), tuple(counts), tuple(sums), tuple(sigmas), steps_done, n * n_scale, n_steps,
                     n_max)


def adapt_cases(kernel):
    """The adaptation grid as data: d in {1, 10, 50} x K in {1, 3, 5} x {no / first / middle / last cluster empty} x
    steps done in {0, 4, 999}, the remaining parameters taken in turn from the lists below, then the named corners."""
    out = []
    means_pool = [0.0, 0.005, 0.234, 0.31, 0.77, 1.0, 0.1234567]
    acc_pool = [0.0, 0.005, 0.234, 1.0, 0.1875, 0.5]
    steps_pool = [(2, 40), (1, 1), (5, 3), (3, 100000), (100, 1000), (7, 11)]
    i = 0
    for d in (1, 10, 50):
        s0 = 2.38 / math.sqrt(d)
        for K in (1, 3, 5):
            for empty in ([None] if K == 1 else [None, 0, K // 2, K - 1]):
                for steps_done in (0, 4, 999):
                    counts = [100 + 37 * ((i + c) % 5) + c for c in range(K)]
                    if empty is not None:
                        counts[empty] = 0
                    means = [means_pool[(i + 3 * c) % len(means_pool)] for c in range(K)]
                    sig = [min(s0, 0.99) * (0.15 + 0.17 * ((i + 2 * c) % 6)) for c in range(K)]
                    n_steps, n_max = steps_pool[i % len(steps_pool)]
                    out.append(_adapt_case(f"grid d={d} K={K} empty={empty} done={steps_done}", kernel, d, counts, means,
                                           acc_pool[i % len(acc_pool)], sig, steps_done, n_steps, n_max, n_scale=1 + i % 2))
                    i += 1
    for d in (1, 10, 50):
        top = min(2.38 / math.sqrt(d), 0.99)
        # sigma driven below 0 and above min(sigma_0, 0.99) (tpCN clamps at both ends, RWM does not); one cluster empty
        out.append(_adapt_case(f"clamp low d={d}", kernel, d, [300, 0, 700], [0.0, 0.5, 0.001], 0.0, [0.05, 0.4, 0.01], 0, 2, 40))
        out.append(_adapt_case(f"clamp high d={d}", kernel, d, [300, 700, 0], [1.0, 0.999, 0.5], 1.0, [top, 0.9 * top, 0.3], 0, 2, 40))
        # the floors max(0.01, acc) and max(1e-6, sigma), and which of n_min, n_adapt, n_max d wins
        for acc in (0.0, 0.005, 0.234, 1.0):
            out.append(_adapt_case(f"acc={acc} d={d} n_adapt wins", kernel, d, [1000], [acc], acc, [0.4 * top], 4, 2, 1000000))
            out.append(_adapt_case(f"acc={acc} d={d} cap wins", kernel, d, [1000], [acc], acc, [0.01 * top], 4, 2, 3))
            out.append(_adapt_case(f"acc={acc} d={d} n_min wins", kernel, d, [1000], [acc], acc, [40.0 * top], 4, 2, 40))
        out.append(_adapt_case(f"sigma floor d={d}", kernel, d, [400, 600], [0.234, 0.234], 0.234, [1e-7, 3e-7], 4, 2, 2 ** 31 - 1))
        out.append(_adapt_case(f"sigma zero d={d}", kernel, d, [400, 600], [0.0, 0.0], 0.0, [1e-9, 0.0], 0, 2, 2 ** 31 - 1))
        out.append(_adapt_case(f"cap below n_min d={d}", kernel, d, [1000], [0.3], 0.3, [0.5 * top], 4, 5, 3))
        # the stopping rule at equality and one step before it
        out.append(_adapt_case(f"stop at equality d={d}", kernel, d, [1000], [1.0], 1.0, [40.0 * top], 2 * d - 1, 2, 40))
        out.append(_adapt_case(f"one before the stop d={d}", kernel, d, [1000], [1.0], 1.0, [40.0 * top], 2 * d - 2, 2, 40))
        # n_global = 2 n: the acceptance rates are over the run's particles, the cluster means over this rank's
        out.append(_adapt_case(f"n_global=2n d={d}", kernel, d, [100, 0, 250, 650, 0], [0.3, 0.9, 0.2, 0.25, 0.9], 0.27,
                               [0.2, 0.3, 0.25, 0.35, 0.1], 4, 2, 40, n_scale=2))
    return out

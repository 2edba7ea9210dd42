"""The references of tests/accept_cases.py against independent formulations, on the CPU: what tests/test_accept_adapt_gpu.py
holds the device to has to stand on something itself.  Also the conditions on the committed input sets that let the GPU tests
compare whole masks and hit exact zeros and ones without exclusions."""
import math

import numpy as np
import pytest

from oracle import mcmc as omc
from tests import accept_cases as ac


def _alpha_sets():
    """(name, rows) of every input set whose alphas or decisions a GPU test compares with alpha_ref."""
    for kernel in ac.KERNELS:
        for d in ac.ALPHA_DIMS:
            yield f"alpha {kernel} d={d}", ac.alpha_rows(kernel, d)
        for n in (1, 255, 256, 257, 1000, 4096):
            for K in (1, 3):
                yield f"decision {kernel} n={n} K={K}", ac.decision_rows(kernel, n, K)


def _oracle_alpha(beta, r):
    dof, assign = np.asarray(r.dofs), r.cluster
    with np.errstate(all="ignore"):
        return omc.accept(r.kernel, beta, r.logl, r.loglp, r.maha_u, r.maha_up, dof, assign, r.d, ac.SEED, ac.TICK, ac.ITEM0)


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


# ------------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("n,K", [(1, 1), (255, 3), (256, 1), (1000, 3), (4096, 3), (4096, 64), (12288, 1), (266240, 3),
                                 (266241, 1), (5000, 3)])
def test_block_partials_and_sums_agree_with_fsum(n, K):
    rs = np.random.RandomState(n + K)
    alpha, acc = rs.rand(n), rs.rand(n) < 0.3
    assign = rs.randint(K, size=n)
    P = ac.block_partials_ref(alpha, acc, assign, K)
    assert P.shape == ((n + 255) // 256, 1 + K)
    want = [float(acc.sum())] + [math.fsum(alpha[assign == k]) for k in range(K)]
    # a block's partial against fsum of its 256 rows, then the step's sums against fsum of everything
    for blk in (0, P.shape[0] - 1):
        sl = slice(256 * blk, min(n, 256 * (blk + 1)))
        for k in range(K):
            ref = math.fsum(alpha[sl][assign[sl] == k])
            assert abs(P[blk, 1 + k] - ref) <= 255 * ac.EPS * ref
    S = ac.sums_ref(P, n, K)
    assert S[0] == want[0]
    np.testing.assert_allclose(S[1:], want[1:], rtol=n * ac.EPS, atol=0)
    np.testing.assert_allclose(S, ac.fsum_columns(P, K), rtol=n * ac.EPS, atol=0)


def test_block_partials_order_is_the_shuffle_tree():
    """Values that round away unless added in the device's order: lane l + lane l + 32 first, (w0 + w2) + (w1 + w3) last."""
    t, none = 2.0 ** -53, np.zeros(256)

    def block(**at):
        a = np.zeros(256)
        for k, v in at.items():
            a[int(k[1:])] = v
        return ac.block_partials_ref(a, none, None, 1)[0, 1]
    assert block(i0=1.0, i32=t, i1=t) == 1.0                        # (1 + t) = 1 (tie to even), then 1 + t = 1; t + t first: 1 + 2t
    assert block(i0=1.0, i1=t, i33=t) == 1.0 + 2 * t                # lane 1 gathers 2t before it meets lane 0
    assert block(i0=1.0, i128=t, i64=t, i192=t) == 1.0 + 2 * t      # (w0 + w2) + (w1 + w3) = (1 + t) + 2t; left to right: 1
    assert block(i0=t, i64=1.0, i128=t) == 1.0 + 2 * t              # (t + t) + (1 + 0); (w0 + w1) + (w2 + w3) would give 1
    assert block(i0=t, i64=t, i128=1.0) == 1.0                      # (t + 1) + (t + 0)


def test_sums_order_is_lanes_then_tree_then_shards():
    """sums_ref on partials built so that every other order gives another double."""
    t = 2.0 ** -53
    # one shard (n % 256 != 0), 130 blocks: lane 0 adds blocks 0, 64, 128 in order: (1 + t) + t = 1, not 1 + 2t
    n = 130 * 256 - 1
    P = np.zeros((130, 2))
    P[0, 1], P[64, 1], P[128, 1] = 1.0, t, t
    assert ac.sums_ref(P, n, 1)[1] == 1.0
    P[0, 1], P[64, 1], P[128, 1] = t, t, 1.0
    assert ac.sums_ref(P, n, 1)[1] == 1.0 + 2 * t
    # V = 3 shards of one block: ((s0 + s1) + s2)
    P = np.zeros((3, 2))
    P[:, 1] = [1.0, t, t]
    assert ac.sums_ref(P, 768, 1)[1] == 1.0
    P[:, 1] = [t, t, 1.0]
    assert ac.sums_ref(P, 768, 1)[1] == 1.0 + 2 * t
    # n = 1024: V = 4 shards, NOT one wave over four blocks: (((s0 + s1) + s2) + s3)
    P = np.zeros((4, 2))
    P[:, 1] = [1.0, t, t, 0.0]
    assert ac.sums_ref(P, 1024, 1)[1] == 1.0              # the wave tree (b0 + b2) + (b1 + b3) would also give 1 ...
    P[:, 1] = [t, 1.0, t, 0.0]
    assert ac.sums_ref(P, 1024, 1)[1] == 1.0              # ... but here it gives 1 + 2t; the fold (t + 1) + t = 1
    assert ac.partition_ref(1024) == (4, 4) and ac.partition_ref(1023) == (1, 1) and ac.partition_ref(12288) == (48, 48)
    assert ac.partition_ref(266240) == (16, 16) and ac.partition_ref(266241) == (1, 1)


@pytest.mark.parametrize("n", [256, 512, 768, 1024, 1536, 2048, 3072, 4096, 12288, 266240])
def test_sums_do_not_depend_on_the_number_of_ranks(n):
    """A property of the restated tree: every world in {1, 2, 3, 4} that divides V gives the same doubles."""
    rs = np.random.RandomState(n)
    K = 3
    P = rs.rand(n // 256, 1 + K) * 10.0 ** rs.uniform(-8, 8, size=(n // 256, 1))
    one = ac.sums_ref(P, n, K)
    V = ac.partition_ref(n)[1]
    seen = 0
    for world in (2, 3, 4):
        if V % world == 0:
            np.testing.assert_array_equal(ac.sums_ref(P, n, K, world), one)
            seen += 1
    assert seen or V == 1


# ------------------------------------------------------------------------------------------------ adaptation
@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_adapt_ref_equals_the_oracle(kernel):
    """Every case of the grid that oracle.mcmc.adapt can express (n_global = n; the cluster means as means of 0/1 alphas, whose
    sums NumPy forms exactly) -- the product-rounded form of adapt_ref, exactly."""
    checked = 0
    for case in ac.adapt_cases(kernel):
        n = int(sum(case.counts))
        if case.n_global != n:
            continue
        # alphas of 0 and 1: cluster c gets round(mean * count) ones, the mask sums[0] ones
        assign = np.repeat(np.arange(case.K), np.asarray(case.counts, dtype=int))
        alpha = np.zeros(n)
        sums = [0.0] * (1 + case.K)
        for c in range(case.K):
            ones = int(round(case.sums[1 + c]))
            alpha[np.nonzero(assign == c)[0][:ones]] = 1.0
            sums[1 + c] = float(ones)
        mask = np.arange(n) < int(round(case.sums[0]))
        sums[0] = float(mask.sum())
        sig = np.array(case.sigmas)
        ws, done, acc, target = omc.adapt(kernel, alpha, mask, assign, case.K, sig, case.steps_done + 1, case.d,
                                          case.n_steps, case.n_max)
        got_s, st = ac.adapt_ref(kernel, sums, case.counts, case.K, sig, case.steps_done, n, case.d, case.n_steps,
                                 case.n_max, contract=False)
        np.testing.assert_array_equal(got_s, ws, err_msg=case.label)
        assert (st[0], bool(st[1]), st[2], st[5]) == (case.steps_done + 1, bool(done), acc, target), case.label
        # the fused form the library is compiled to: one rounding of a product apart, per multiply-add
        fs, fst = ac.adapt_ref(kernel, sums, case.counts, case.K, sig, case.steps_done, n, case.d, case.n_steps, case.n_max)
        np.testing.assert_allclose(fs, ws, rtol=4 * ac.EPS, atol=4 * ac.EPS, err_msg=case.label)
        assert abs(fst[5] - target) <= max(1.0, 1e-12 * target), case.label
        checked += 1
    assert checked >= 90


@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_adapt_grid_reaches_every_branch(kernel):
    seen = set()
    for case in ac.adapt_cases(kernel):
        t = {}
        s, st = ac.adapt_ref(kernel, case.sums, case.counts, case.K, case.sigmas, case.steps_done, case.n_global, case.d,
                             case.n_steps, case.n_max, trace=t)
        for c in range(case.K):
            if case.counts[c] == 0:
                assert s[c] == case.sigmas[c]             # an empty cluster keeps its sigma
                seen.add("empty first" if c == 0 else "empty last" if c == case.K - 1 else "empty middle")
        plain = sum(v * c for v, c in zip(s, case.counts)) / sum(case.counts)
        if abs(plain - t["weighted_sigma"]) > 1e-3 * abs(plain):
            seen.add("quirk matters")
        lo, hi = t["n_min"], t["cap"]
        seen.add("n_min wins" if t["n_adapt"] <= lo <= hi else "cap wins" if max(lo, t["n_adapt"]) >= hi else "n_adapt wins")
        if lo < t["n_adapt"] < hi and t["n_adapt"] != int(t["n_adapt"]):
            seen.add("truncation")
        if t["acc"] < 0.01:
            seen.add("acc floor")
        if t["weighted_sigma"] < 1e-6:
            seen.add("sigma floor")
        if kernel == "tpcn":
            seen.update("clamp low" for v, c in zip(s, case.counts) if c and v == 0.0)
            seen.update("clamp high" for v, c in zip(s, case.counts) if c and v == t["sigma_top"])
        else:
            seen.update("clamp low" for v in s if v < 0.0)
            seen.update("clamp high" for v in s if v > t["sigma_top"])
        seen.add("done" if t["done"] else "not done")
        if t["iteration"] == t["n_int"]:
            seen.add("stop at equality")
        if case.n_global != sum(case.counts):
            seen.add("n_global")
        seen.add(f"steps {case.steps_done}")
    want = {"empty first", "empty middle", "empty last", "quirk matters", "n_min wins", "cap wins", "n_adapt wins", "truncation",
            "acc floor", "sigma floor", "clamp low", "clamp high", "done", "not done", "stop at equality", "n_global", "steps 0",
            "steps 4", "steps 999"}
    assert want <= seen, want - seen


# --------------------------------------------------------------------------------------------------- alpha
def test_alpha_ref_equals_mpmath_on_the_edge_table():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50

    def exact(beta, l0, l1, m0, m1, nu, d, kernel):
        f = mp.mpf                      # mpmath's own inf / nan arithmetic: inf - inf and 0 * inf are nan
        arg = f(beta) * (f(l1) - f(l0))
        if kernel == "tpcn":
            arg += (f(d) + f(nu)) / 2 * (mp.log(1 + f(m1) / f(nu)) - mp.log(1 + f(m0) / f(nu)))
        if mp.isnan(arg):
            return 0.0
        return 1.0 if arg >= 0 else float(mp.exp(arg))
    for kernel in ac.KERNELS:
        for d in (1, 16, 100):
            E = ac.edge_rows(d, ac.DOFS4)
            cols = [np.array([e[k] for e in E]) for k in range(4)]
            nu = np.asarray(ac.DOFS4)[[e[4] for e in E]]
            for beta in ac.BETAS:
                a, b = ac.alpha_ref(kernel, beta, cols[0], cols[1], cols[2], cols[3], nu, d)
                for i, e in enumerate(E):
                    want = exact(beta, e[0], e[1], e[2], e[3], nu[i], d, kernel)
                    if want in (0.0, 1.0):
                        assert a[i] == want, (kernel, d, beta, e, a[i])
                    else:                     # long double carries 11 bits more than the bound's unit
                        assert abs(a[i] - want) <= (2.0 ** -52 + b[i] / 256) * want, (kernel, d, beta, e, a[i], want)


def test_oracle_lies_inside_the_bound_and_no_row_is_undecidable():
    """The two conditions on the references alone, for every input set the GPU tests use: the float64 oracle's error is at most
    ORACLE_WORST_RATIO bounds (the device gets four times that), and no row's kind or decision depends on the device's
    rounding -- no exponent in (0, c b], none in exp's subnormal range, no uniform within c b alpha of alpha."""
    worst, where, inner = 0.0, None, 0
    for name, r in _alpha_sets():
        U = ac.uniforms(r.n)
        for beta in ac.BETAS:
            a, b = ac.alpha_ref(r.kernel, beta, r.logl, r.loglp, r.maha_u, r.maha_up, r.nu, r.d)
            got, mask = _oracle_alpha(beta, r)
            ratio = ac.alpha_ratio(got, a, b)
            assert np.isfinite(ratio).all(), (name, beta, np.nonzero(~np.isfinite(ratio))[0][:5])
            if ratio.max() > worst:
                worst, where = float(ratio.max()), (name, beta)
            assert ac.undecidable_rows(r.kernel, beta, r).size == 0, (name, beta)
            assert ac.ambiguous_decisions(a, b, U).size == 0, (name, beta)
            np.testing.assert_array_equal(mask, U < a)
            inner += int(((a > 0) & (a < 1)).sum())
            if r.n >= 256 and beta > 0:
                assert 0.15 < np.mean((a > 0) & (a < 1)), (name, beta)       # the sets are not all zeros and ones
    print(f"oracle worst ratio {worst:.4f} at {where}; {inner} alphas strictly inside (0, 1)")
    assert 0.5 * ac.ORACLE_WORST_RATIO <= worst <= ac.ORACLE_WORST_RATIO, (worst, where)
    assert ac.C_DEVICE == 4.0 * ac.ORACLE_WORST_RATIO

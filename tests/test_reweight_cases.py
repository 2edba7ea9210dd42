"""The cases of tests/reweight_cases.py are the specification of tests/test_reweight_gpu.py; this file checks them without a GPU:
every geometry reaches the branch its table entry names (asserted from the restated k2_geometry / tph_partition), the premises of
the exact counts hold in float64, the long-double references agree with mpmath at 40 digits, the derived bounds stay below
ACC_LIMIT on the realistic inputs (their values are printed), hold for an honest float64 evaluation in another order and are
broken by one dropped row, and the lattice of the k_sum_sq_max cases is exact in any order."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import reweight_cases as rc

LD = rc.LD


def _c64(h):
    """The cached log-mixture as a correctly rounded double (the device's differs within logmix_bounds)."""
    return rc.logmix_reference(*h).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("c", rc.COUNT_GEOMS, ids=lambda c: c.name)
def test_geometry_reaches_the_branch_its_entry_names(c):
    g = rc.geometry(c.n_t, c.reduce_grid)
    d = rc.describe(g)
    for key, want in c.expect.items():
        assert d[key] == want, (c.name, key, d[key], want)
    assert rc.covers_once(g) and g.n <= 1_070_000
    assert g.V <= 48 and 3 * g.V <= 48 * 3                      # k_reweight_fold parks V <= 48 triples in LDS
    e, odd = rc.edge_rows(g), rc.odd_end_rows(g)
    assert e[0] == 0 and e[-1] == g.n - 1 and set(odd) <= set(e)
    assert bool(odd.size) == (d["odd_r0"] or d["odd_r1"])
    singles = rc.single_edges(g)
    assert 1 <= len(singles) <= rc.MAX_SINGLES and set(singles) <= set(e) and len(set(singles)) == len(singles)
    if odd.size:
        assert odd[0] in singles and odd[-1] in singles


def test_the_table_covers_every_shard_count_and_both_block_forms():
    canon = {rc.geometry(c.n_t, c.reduce_grid).V for c in rc.COUNT_GEOMS if rc.describe(rc.geometry(c.n_t, c.reduce_grid))["canonical"]}
    assert canon == {1, 2, 3, 4, 6, 8, 12, 16, 48}
    d = {c.name: rc.describe(rc.geometry(c.n_t, c.reduce_grid)) for c in rc.COUNT_GEOMS}
    assert d["12288x40-grid1"]["pieces"] == [40] and d["12288x40-grid1048576"]["RB"] == d["12288x40"]["RB"] == 4096
    assert d["34304x3"]["BPP"] == 2 and d["34304x3"]["V"] == 2             # a block cut inside a piece together with V > 1
    assert d["1280x200"]["bv"] == 67 > 64                                    # second trip of vshard_triple's lane loops
    assert d["1064961x1"]["no_pairs"] and d["1064961x1"]["bv"] == 66
    assert d["40001x3"]["block_rows"][:3] == [16384, 16384, 7233]
    assert all(n in d for n in rc.COUNT_WIDTH_GEOMS)
    # the unroll classes: every width, three factors
    assert sorted(nb for v in rc.U_CLASSES.values() for nb in v) == list(range(1, 17))
    assert all(rc.unroll(nb) == u for u, nbs in rc.U_CLASSES.items() for nb in nbs)


# ------------------------------------------------------------------------------------------------------------ exact counts
def test_premises_of_the_exact_counts():
    assert np.exp(0.0) == 1.0 and np.exp(-2.0 ** 20) == 0.0
    b = rc.COUNT_BETAS
    assert b.size == rc.MAX_NB and (b == 0).sum() == 1 and np.all((b == 0) | ((b >= 2.0 ** -20) & (b <= 1.0)))
    for x in b:
        assert Fraction(float(x)) * Fraction(rc.L_OFF) == Fraction(float(x * rc.L_OFF))       # the product is exact
        assert Fraction(float(x)) * 0 == 0
    for c in rc.COUNT_GEOMS:
        n, T = sum(c.n_t), len(c.n_t)
        assert n < rc.LIMIT
        C = float(_c64(rc.History(np.array([0.0, rc.L_OFF]), np.zeros(T), np.zeros(T), np.array(c.n_t)))[0])
        assert 0.0 <= C <= math.log(n * T) + 1e-9
        for x in b[b > 0]:
            v_off = x * rc.L_OFF - C
            assert v_off - (-C) <= -2.0 ** 19 and np.exp(v_off - (-C)) == 0.0                 # as a term and as a rescale factor
        assert 0.0 * rc.L_OFF - C == -C and 1.0 * 0.0 - C == -C


@pytest.mark.parametrize("name", ["3x1", "777x9", "512x7", "4097-unequal"])
def test_count_expected_is_what_float64_gives_in_any_order(name):
    c = rc.COUNT_BY_NAME[name]
    for label, on in rc.count_patterns(c):
        logl, bt, zt, nt = rc.count_history(c, on)
        cm = _c64(rc.History(logl, bt, zt, nt))
        assert np.all(rc.bits(cm) == rc.bits(cm)[0]), label
        want = rc.count_expected(cm[0], on.size, int(on.sum()), rc.COUNT_BETAS)
        p = np.random.RandomState(5).permutation(on.size)
        for i, beta in enumerate(rc.COUNT_BETAS):
            v = beta * logl[p] - cm[p]
            e = np.exp(v - v.max())
            got = np.array([v.max(), np.add.reduce(e[::-1]), (e * e).sum()])
            np.testing.assert_array_equal(got, want[i], err_msg=f"{name} {label} beta {beta}")
    labels = [lb for lb, _ in rc.count_patterns(c)]
    assert labels[:4] == ["half1", "half2", "edges", "not-edges"] and labels[-1] == "all-off" and len(labels) <= 5 + rc.MAX_SINGLES


def test_all_off_history_has_its_own_form():
    C = math.log(7.0)
    got = rc.count_expected(C, 9, 0, rc.COUNT_BETAS)
    assert np.all(got[:, 1:] == 9)
    assert got[5, 0] == -C and got[0, 0] == rc.L_OFF - C and got[1, 0] == -2.0 ** 20 - C


# ---------------------------------------------------------------------------------------------- references against mpmath
def test_references_against_mpmath_at_40_digits():
    mp = pytest.importorskip("mpmath")
    h = rc.realistic(777, 9)
    rows = np.random.RandomState(1).choice(h.logl.size, 400, replace=False)
    ref = rc.logmix_reference(*h)
    with mp.workdps(40):
        for s in rows:
            terms = [mp.mpf(float(h.logl[s])) * mp.mpf(float(b)) - mp.mpf(float(z)) + mp.log(int(n)) for b, z, n in zip(h.bt, h.zt, h.nt)]
            exact = mp.log(mp.fsum(mp.exp(t) for t in terms))
            assert abs(mp.mpf(float(ref[s])) + mp.mpf(float(ref[s] - LD(float(ref[s])))) - exact) <= abs(exact) * mp.mpf(2) ** -61
        C = ref.astype(np.float64)
        for beta in (1.0, 0.37):
            t = rc.acc_reference(h.logl, C, beta)
            v = [mp.mpf(float(beta)) * mp.mpf(float(l)) - mp.mpf(float(c)) for l, c in zip(h.logl, C)]
            m = max(v)
            s1, s2 = mp.fsum(mp.exp(x - m) for x in v), mp.fsum(mp.exp(2 * (x - m)) for x in v)
            for got, exact in ((t.m, m), (t.s1, s1), (t.s2, s2)):
                hi = float(got)
                assert abs(mp.mpf(hi) + mp.mpf(float(got - LD(hi))) - exact) <= abs(exact) * mp.mpf(2) ** -58


# ---------------------------------------------------------------------------------------------------- K2: derived bounds
def _plain64(logl, C, beta):
    """An honest float64 evaluation in another order (NumPy's pairwise sums), with its own maximum."""
    v = beta * logl - C
    e = np.exp(v - v.max())
    return v.max(), e.sum(), (e * e).sum()


@pytest.mark.parametrize("rows,T", rc.ACC_GEOMS)
def test_bounds_of_the_realistic_cases_stay_below_the_limit(rows, T):
    h = rc.realistic(rows, T)
    assert h.bt[0] == 0 and (T < 2 or h.bt[1] == 0) and np.all(np.diff(h.bt) >= 0) and np.all(np.diff(h.zt) <= 0)
    g, C = rc.geometry(h.nt), _c64(h)
    worst = 0.0
    for i, beta in enumerate(rc.ACC_BETAS):
        ref = rc.acc_reference(h.logl, C, beta)
        for nb in ((16, 1, 4) if beta == 1.0 else (16,)):
            b = rc.acc_bound(h.logl, beta, ref, g, nb)
            worst = max(worst, b.s1, b.s2, b.logz, b.ess)
            assert 0 < b.s1 <= b.s2 <= rc.ACC_LIMIT and b.logz <= rc.ACC_LIMIT and b.ess <= rc.ACC_LIMIT and b.m <= rc.ACC_LIMIT, (beta, nb, b)
        err = rc.acc_errors(_plain64(h.logl, C, beta), ref)
        assert all(e <= x for e, x in zip(err, b)), (beta, err, b)
    print(f"{rows} x {T}: largest bound {worst:.3e}, path (rescales, additions) at nb = 16: {rc.path_counts(g, 16)}")


def test_the_bound_is_broken_by_one_dropped_or_doubled_row():
    h = rc.realistic(777, 9)
    g, C = rc.geometry(h.nt), _c64(h)
    for beta in (1.0, 0.37, 0.0):
        ref = rc.acc_reference(h.logl, C, beta)
        b = rc.acc_bound(h.logl, beta, ref, g, 16)
        p = np.exp(ref.v - ref.m) / ref.s1
        row = int(np.argsort(p)[p.size // 2])                       # a row of median weight
        assert p[row] > 100 * b.s1
        for keep in (np.delete(np.arange(p.size), row), np.append(np.arange(p.size), row)):
            err = rc.acc_errors(_plain64(h.logl[keep], C[keep], beta), ref)
            assert err[1] > b.s1 and err[3] > b.logz


def test_edges_of_the_range_are_what_their_names_say():
    ed = rc.acc_edges()
    h, betas, _ = ed["ascending"]
    C = _c64(h)
    for beta in betas:
        assert np.all(np.diff(beta * h.logl - C) >= 0)
    g = rc.geometry(h.nt)
    assert g.n - 1 in rc.odd_end_rows(g) and 777 in rc.odd_end_rows(g)
    for name, row in (("max-last-row", g.n - 1), ("max-odd-start", 777)):
        h, betas, _ = ed[name]
        assert all(np.argmax(rc.acc_reference(h.logl, _c64(h), b).v) == row for b in betas)
    h, betas, _ = ed["spread"]
    ref = rc.acc_reference(h.logl, _c64(h), 1.0)
    d = (ref.v - ref.m).astype(np.float64)
    assert (d < -745.2).any() and ((d > -420) & (d < -372.6)).any()        # e = 0 | e^2 = 0 < e in float64
    assert np.exp(-745.2) == 0.0 and np.exp(-372.6) ** 2 == 0.0 < np.exp(-420.0)
    for name in ("overflow-block", "overflow-shard", "overflow-all"):
        h, betas, _ = ed[name]
        C = _c64(h)
        g2 = rc.geometry(h.nt)
        assert np.all(np.isfinite(C)) and g2.V == 2 and g2.BPP == 2
        big = h.logl == -rc.DBL_MAX
        with np.errstate(over="ignore"):
            assert np.all(2.0 * h.logl[big] - C[big] == -np.inf) and np.all(np.isfinite(1.0 * h.logl[big] - C[big]))
        if name == "overflow-block":
            r = [x for x in rc.runs(g2) if x.block == 1]
            assert len(r) == 1 and np.all(big[r[0].r0:r[0].r1]) and big.sum() == r[0].r1 - r[0].r0
        if name == "overflow-shard":
            mine = np.zeros(g2.n, dtype=bool)
            for x in rc.runs(g2):
                if x.block >= g2.bv:
                    mine[x.r0:x.r1] = True
            assert np.array_equal(mine, big)
        if name == "overflow-all":
            assert big.all()
    h, betas, _ = ed["neg-inf"]
    assert np.all(h.bt > 0)
    C = _c64(h)
    assert np.all(C[np.isinf(h.logl)] == -np.inf) and np.isnan(rc.acc_reference(h.logl, C, 1.0).s1)
    h, betas, _ = ed["nan-row"]
    t = rc.acc_reference(h.logl, _c64(h), 1.0)
    assert np.isnan(t.s1) and np.isnan(t.s2) and np.isfinite(t.m)


def test_the_two_rounded_forms():
    h = rc.exact_case()
    assert h.logl.size == 4099 and rc.geometry(h.nt).T == 1
    C = _c64(h)
    differ = 0
    for beta in rc.EXACT_BETAS:
        fused, unfused = rc.two_forms(beta, h.logl, C)
        exact = LD(beta) * h.logl.astype(LD) - C.astype(LD)
        assert np.all(np.abs(fused.astype(LD) - exact) <= np.spacing(np.abs(fused)) * 0.5 * (1 + 2.0 ** -9))
        assert np.all(np.abs(unfused - fused) <= np.spacing(np.abs(fused)))
        differ += int((fused != unfused).sum())
    assert differ > 0                                   # the two forms are not the same array: the test tells them apart
    assert rc.log_nh(4099) == math.log(4099.0)


# ------------------------------------------------------------------------------------------------------------------------ K1
def _stream64(a):
    """k_logmix_append's streaming log-sum-exp in float64."""
    m, s = a[:, 0].copy(), np.ones(a.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, a.shape[1]):
            x = a[:, t]
            up = x > m
            s = np.where(up, s * np.exp(m - x) + 1.0, s + np.where(x == m, 1.0, np.exp(x - m)))
            m = np.where(up, x, m)
        return m + np.log(s)


@pytest.mark.parametrize("name", sorted(rc.logmix_cases()))
def test_logmix_bounds_hold_for_float64_by_both_routes(name):
    h = rc.logmix_cases()[name]
    assert len(h.bt) <= 40 and h.logl.size == h.nt.sum()
    ref = rc.logmix_reference(*h)
    with np.errstate(invalid="ignore"):
        a = h.logl[:, None] * h.bt[None, :] - h.zt[None, :] + np.log(h.nt.astype(np.float64))[None, :]
    entered = np.repeat(np.arange(len(h.bt)), h.nt)
    load = _stream64(a)
    app = np.empty_like(load)
    for k in range(len(h.bt)):
        rows = entered == k
        c = _stream64(a[rows, :k + 1])
        for t in range(k + 1, len(h.bt)):
            with np.errstate(invalid="ignore"):
                c = np.logaddexp(c, a[rows, t])
        app[rows] = c
    fin = np.isfinite(ref)
    for route, got in (("load", load), ("append", app)):
        b = rc.logmix_bounds(*h, route)
        assert np.all(b[fin] > 0) and np.all(b[fin] < 1e-12 * np.maximum(1.0, np.abs(ref[fin]).astype(np.float64)))
        assert np.all(np.abs(got[fin].astype(LD) - ref[fin]) <= b[fin]), (name, route)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)].astype(np.float64))
    if name == "neg-inf":
        assert np.all(ref[np.isinf(h.logl)] == -np.inf) and not np.isnan(ref).any()
    if name == "nan":
        assert np.isnan(ref[np.isinf(h.logl)]).all() and (h.bt == 0).any()
    if name == "equal":
        assert np.all(a[:, 0] == a[:, 1]) and np.all(a[:, 2] == a[:, 3])


def test_the_large_appends_reach_the_pair_loop():
    (o1, n1), (o2, n2) = rc.APPEND_LARGE
    s1, s2 = rc.append_loop_shape(o1, o1 + n1), rc.append_loop_shape(o2, o2 + n2)
    assert s1 == {"grid": 2048, "odd_tail": True, 0: (1, False), 1: (0, True)}       # one lane in the body; the others the remainder
    assert s2 == {"grid": 2048, "odd_tail": True, 0: (2, False), 1: (1, True)}       # a second trip; the remainder behind a trip
    assert rc.append_loop_shape(777 * 8, 777 * 9)[0] == (0, True)                     # what the earlier test reaches
    assert max(o1 + n1, o2 + n2) <= 3_800_000
    h = rc.append_large(o1, n1)
    assert len(h.bt) == 2 and h.nt.tolist() == [o1, n1]


# ------------------------------------------------------------------------------------------------------------------------ K3
@pytest.mark.parametrize("n", rc.SSM_SIZES)
def test_sum_sq_max_lattice_is_exact_in_any_order(n):
    assert rc.ssm_grid(263169) > 256 and 2098177 > rc.RED_BLOCKS * 1024 and rc.ssm_grid(2098177) == rc.RED_BLOCKS
    for row in rc.ssm_max_rows(n):
        k, w = rc.ssm_weights(n, row)
        want = rc.ssm_expected(k)
        assert (k == 1023).sum() == 1 and k[row] == 1023 and k.max() < 1024
        if n > 1000:
            assert 0.3 < (k == 0).mean() < 0.37
        p = np.random.RandomState(n % 91).permutation(n)
        for order in (w, w[::-1], w[p]):
            np.testing.assert_array_equal([order.sum(), (order * order).sum(), order.max()], want)
            np.testing.assert_array_equal([np.add.reduce(order[:, None], axis=0)[0], np.cumsum(order * order)[-1]], want[:2])


def test_weights_bound_holds_for_float64_and_sees_a_wrong_scale():
    h, _, _ = rc.acc_edges()["spread"]
    C = _c64(h)
    beta = 1.0
    m, s1, _ = _plain64(h.logl, C, beta)
    w, v, e = rc.weights_reference(h.logl, C, beta, m, s1)
    rel, ab = rc.weights_bound(h.logl, beta, v, m, w)
    got = np.exp(beta * h.logl - C - m) / s1
    assert np.all(np.abs(got.astype(LD) - w) <= w * rel + ab)
    assert (e.astype(np.float64) == 0).any() and (e * (1 + rel) < rc.HALF_STEP).any() and np.all(got[e * (1 + rel) < rc.HALF_STEP] == 0.0)
    wrong = got * (1 + 2.0 ** -40)
    assert not np.all(np.abs(wrong.astype(LD) - w) <= w * rel + ab)
    assert rc.ssm_additions(h.logl.size) < 64

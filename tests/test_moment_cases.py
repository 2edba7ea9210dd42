"""The cases of tests/moment_cases.py are the specification of tests/test_moments_gpu.py; this file checks them without a GPU:
every bit budget holds, the float64 evaluation of each reference in several summation orders (BLAS, permuted rows, chunked
accumulation) equals the integer reference bit for bit -- the property that lets the device be compared without a tolerance --
and every row of the last tile matters to every entry."""
import numpy as np
import pytest

from tests import moment_cases as mc

INT_PRODUCT_MAX = 40_000_000     # rows x pairs up to which the int64 matrix product is taken in full (it has no BLAS)


def _orders(xc, kw, rs):
    """sum_i kw_i xc_i xc_i^T in float64: BLAS on the rows as they are, BLAS on permuted rows, chunks of another permutation
    accumulated one after the other."""
    xf, wf = xc.astype(np.float64), kw.astype(np.float64)
    yield (xf * wf[:, None]).T @ xf
    p = rs.permutation(kw.size)
    yield (xf[p] * wf[p, None]).T @ xf[p]
    p = rs.permutation(kw.size)
    acc = np.zeros((xc.shape[1],) * 2)
    for s in range(0, kw.size, 997):
        q = p[s:s + 997]
        acc += np.einsum("i,ia,ib->ab", wf[q], xf[q], xf[q])
    yield acc


def _int_product(xc, kw, rs):
    """-> (index arrays a, b; int64 values): the whole product, or 256 sampled entries plus the diagonal where it is too slow."""
    n, d = xc.shape
    if n * d * (d + 1) // 2 <= INT_PRODUCT_MAX:
        a, b = np.indices((d, d))
        return a.ravel(), b.ravel(), ((xc * kw[:, None]).T @ xc).ravel()
    a = np.concatenate([rs.randint(0, d, 256), np.arange(d)])
    b = np.concatenate([rs.randint(0, d, 256), np.arange(d)])
    return a, b, np.array([int((kw * xc[:, i] * xc[:, j]).sum()) for i, j in zip(a, b)], dtype=np.int64)


def test_the_dimension_lists_pin_the_branches_they_name():
    assert mc.ALL_D[0] == 1 and mc.ALL_D[-1] == mc.MAX_D and set(range(1, 17)) <= set(mc.ALL_D)
    for d, sl in mc.TILE_SLICES.items():
        assert mc.tile_slices(d) == sl, d
    # every change of the slice count, and the step to two block pairs per thread, has both neighbours in the list
    for d in range(17, 101):
        if mc.tile_slices(d) != mc.tile_slices(d - 1):
            assert d in mc.ALL_D and d - 1 in mc.ALL_D, d
    pairs = lambda d: ((d + 3) // 4) * ((d + 3) // 4 + 1) // 2      # noqa: E731
    assert pairs(88) <= 256 < pairs(89) and pairs(60) * 2 <= 256 < pairs(61) * 2
    npl = lambda d: d * (d + 1) // 2                                  # noqa: E731
    assert npl(22) <= 256 < npl(23)                                   # k_colsum2_wide needs ncol > 256 ...
    assert all(-(-n // 64) <= 256 for n in mc.SMALL_N) and -(-131137 // 64) > 2048      # ... and <= 256 partial rows
    assert 131137 % 64 == 1 and 393221 > 2 * 768 * 256 and 524291 > 4 * 512 * 256 and -(-262149 // 64) == 4097
    assert [mc.pair_slices(d) for d in (13, 14, 15)] == [2, 2, 2]     # k_wcov: two row slices of 32 rows per pair
    for n in mc.SMALL_N:
        f = mc.forced_rows(n)
        assert f[0] and f[-1] and f.sum() == min(n, 1 + (n - 1) % 64 + (n > 64))


@pytest.mark.parametrize("d", mc.ALL_D)
def test_sums_and_centred_second_moments(d):
    rs = np.random.RandomState(d)
    lat = mc.lattice(d, max(mc.rows_for(d)))
    assert lat.k.min() >= 1 and lat.k.max() <= (1 << mc.B) - 1 and np.all(lat.c2 % 2 == 1)
    for n in mc.rows_for(d):
        kw = mc.weights(d, n)
        f = mc.forced_rows(n)
        assert np.all(kw[f] > 0) and (n <= 64 or abs((kw == 0).mean() - 0.3) < 0.15)
        xc, k = mc.centred(lat, n), lat.k[:n]
        # first moments: two orders in float64 against the integers
        sums, rng = mc.sums_ref(lat, kw)
        u, w = mc.u_of(lat, n), kw / 16.0
        p = rs.permutation(n)
        for got in (w @ u, w[p] @ u[p], np.add.reduce(w[:, None] * u, axis=0)):
            np.testing.assert_array_equal(got, sums[1:])
        assert sums[0] == w.sum() == w[p].sum()
        if n > 64:                                       # the range rows lie beyond the weighted rows and carry no weight
            assert kw[1] == kw[2] == 0 and np.all(rng[0::2] > u[1]) and np.all(rng[1::2] < u[2])
        # second moments
        ref = mc.cov_ref(lat, kw)
        np.testing.assert_array_equal(ref, ref.T)
        for got in _orders(xc, kw, rs):
            np.testing.assert_array_equal(got / float(16 << (2 * mc.B + 2)), ref)
        a, b, val = _int_product(xc, kw, rs)
        np.testing.assert_array_equal(val.astype(np.float64) / float(16 << (2 * mc.B + 2)), ref[a, b])
        if n * d * d <= INT_PRODUCT_MAX:
            np.testing.assert_array_equal(mc.cov_ref(lat, kw, exact_int=True), ref)
        # sensitivity: the term of every (forced row, a, b) and (forced row, j) is non-zero, so the reference without that row
        # differs in every entry
        assert np.all(kw[f, None] * k[f] != 0)
        assert np.all(kw[f, None, None] * xc[f, :, None] * xc[f, None, :] != 0)


@pytest.mark.parametrize("d", mc.ALL_D)
def test_moments_about_the_device_mean(d):
    rs = np.random.RandomState(100 + d)
    lat = mc.lattice(d, max(mc.rows_for(d)))
    for n in mc.MOMENT_N:
        kw, P = mc.pow2_weights(d, n)
        f = mc.forced_rows(n)
        assert np.all(kw[f] > 0) and 3 * P + 2 * mc.B < 53
        m = mc.moments_ref(lat, kw, P)
        c_int = mc.moments_ref_int(lat, kw, P)
        np.testing.assert_array_equal(np.ldexp(c_int.astype(np.float64), -(3 * P + 2 * mc.B)), m.cov)
        xc = (lat.k[:n] << P) - kw @ lat.k[:n]
        for got in _orders(xc, kw, rs):
            np.testing.assert_array_equal(np.ldexp(got, -(3 * P + 2 * mc.B)), m.cov)
        # float64 as the device forms it: mean = S1 / S0, centred coordinates, products, division by S0
        u, w = mc.u_of(lat, n), kw / 16.0
        mean = (w @ u) / w.sum()
        np.testing.assert_array_equal(mean, m.mean)
        np.testing.assert_array_equal(((u - mean) * w[:, None]).T @ (u - mean) / w.sum(), m.cov)
        if n > 1:
            # (the device's mean can fall on a lattice point, so here a centred coordinate may vanish: rarely.  The guarantee
            # that EVERY term counts belongs to the supplied-centre cases above, which run the same kernels)
            assert (xc[f] == 0).mean() < 0.01
        if d <= 12:
            # the shifted one-pass form about the half-lattice centre gives the same numbers, within its own budget
            assert mc.shifted_budget_bits(lat, P) <= 53
            s_int = mc.shifted_ref_int(lat, kw, P)
            np.testing.assert_array_equal(s_int << P, 4 * c_int)
            c, xs = mc.centre_of(lat), u - mc.centre_of(lat)
            da = (w @ xs) / w.sum()
            np.testing.assert_array_equal(c + da, m.mean)
            np.testing.assert_array_equal((xs * w[:, None]).T @ xs / w.sum() - np.outer(da, da), m.cov)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("d", mc.FIT_D)
def test_fit_cases(d, K):
    lat = mc.lattice(d, mc.FIT_N, b=mc.B_FIT)
    counts, labels = mc.fit_counts(d, K)
    last = np.arange(64 * ((mc.FIT_N - 1) // 64), mc.FIT_N)
    assert np.all(counts[last] > 0) and counts[0] > 0 and counts.min() >= 0
    if K == 3:
        assert not np.any(labels[last] == 2) and set(labels[last]) == {0, 1}
    for lab in range(K):
        assert counts[labels == lab].sum() == 1 << mc.P_FIT
        ref = mc.fit_cov_ref(lat, counts, labels, lab)
        np.testing.assert_array_equal(ref, ref.T)
        assert np.linalg.eigvalsh(ref).min() > 0.01      # the Cholesky behind the fit succeeds: covs comes back unridged
        kk = np.where(labels == lab, counts, 0).astype(np.int64)
        c_int = mc.moments_ref_int(lat, kk, mc.P_FIT).astype(np.float64)
        v = np.ldexp(c_int, -(3 * mc.P_FIT + 2 * mc.B_FIT))
        v[np.diag_indices(d)] *= 1.0 + 2.0 ** -mc.P_FIT
        np.testing.assert_array_equal(v, ref)
        # as np.cov has it, in float64: exact too
        u = mc.u_of(lat)
        mean = (kk @ u) / kk.sum()
        c = ((u - mean) * kk[:, None]).T @ (u - mean) / kk.sum()
        np.testing.assert_array_equal(c + np.diag(np.diag(c)) / kk.sum(), ref)


@pytest.mark.parametrize("d", mc.CV_D)
def test_cv_sum_cases(d):
    rs = np.random.RandomState(d)
    cases = [mc.cv_case(d, n) for n in mc.cv_rows_for(d)] + ([mc.cv_case(d, 2397, shift=20)] if d == 13 else [])
    for case in cases:
        ref, hi, lo = mc.cv_ref(case)
        n = case.kw.size
        if case.shift:
            assert hi > 100 and lo > 100 and n - hi - lo > 100         # both clips, and rows inside them
        else:
            assert hi == lo == 0
        mean, P = mc.cv_inputs(case)
        xc = mc.u_of(case.lat, n) - mean
        d2 = np.einsum("ia,ab,ib->i", xc, P, xc)
        if d > 1 and n > 1:
            assert (d2 < 0).any() and (d2 > 0).any() and (d2 < d).any()     # forms of both signs, negative deviations
        t = case.kw.astype(np.float64) ** 2 * np.clip(d2 - d, -1e6, 1e6) ** 2
        p = rs.permutation(n)
        assert ref == t.sum() == t[p].sum() == np.add.reduce(t[::-1])
        f = mc.forced_rows(n)
        assert np.all(t[f] != 0)                         # every row of the last tile contributes


@pytest.mark.parametrize("d", [5, 14, 50])
def test_the_non_lattice_bound_holds_for_float64_numpy(d):
    """The a-priori bound of moments_bound is for any float64 order: NumPy's own must sit inside it (far inside)."""
    u, w, counts = mc.gaussian_case(d)
    for wt in (w, counts.astype(np.float64)):
        m, c, bm, bc = mc.moments_bound(u, wt)
        mean = (wt @ u) / wt.sum()
        cov = ((u - mean) * wt[:, None]).T @ (u - mean) / wt.sum()
        assert np.all(np.abs(mean - m) <= bm) and np.all(np.abs(cov - c) <= bc)
        assert float((np.abs(cov - c) / bc).max()) < 0.1

"""The weighted sums and second-moment kernels of csrc/modes.hip (k_wsum, k_wsum_final, k_colsum2, k_colsum2_wide, k_fold_cols,
k_mean_from_sums, k_wcov_small, k_wcov, k_wcov_tiled, k_wcov_mfma, k_wmom_small, k_wmom_finish, k_cov_finish, k_cv_sum) through
every entry point that launches them, against the exact references of tests/moment_cases.py (checked on the CPU by
tests/test_moment_cases.py).

Tolerances: none.  On the lattice inputs no operation of these kernels rounds, whatever the order (moment_cases.py states and
asserts the bit budget of every case), so every comparison is assert_array_equal: a dropped, repeated or mis-weighted row, a
wrong lane of the last 4 x 4 or 16 x 16 block, a slice merged twice or a partial row left out changes the bits.  The one
exception is test_non_lattice_data_within_the_a_priori_bound, which says where its bound comes from.

One context per n_dim, its history loaded once at the longest row count of that n_dim; the shorter cases pass shorter weight
vectors.  The x-array pair is called as student.py calls it, on one device array with ld > n whose base is offset by one double
and whose padding is NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import moment_cases as mc  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for c, _ in _CTX.values():
        c.close()
    _CTX.clear()


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def H(t):
    return t.cpu().numpy()


def new_ctx(d, u):
    """A context of n_dim d whose history holds the rows of u (n, d)."""
    from tempest_amd.device import HipContext
    c = HipContext(d, 0)
    n = u.shape[0]
    c.history_load(np.ascontiguousarray(u.T), None, np.zeros(n), [0.0], [0.0], [n], soa=True)
    return c


class XArray:
    """u as an explicit SoA array x[j * ld + i] with ld = n + 3, one double into its allocation, NaN wherever no row lives."""

    def __init__(self, u):
        n, d = u.shape
        self.ld = n + 3
        self.flat = torch.full((1 + d * self.ld,), float("nan"), dtype=torch.float64, device="cuda")
        self.flat[1:].view(d, self.ld)[:, :n] = T(u.T)
        self.ptr = self.flat.data_ptr() + 8


_CTX = {}


def ctx(d):
    """(context, x array) of the B-bit lattice of n_dim d."""
    if d not in _CTX:
        u = mc.u_of(mc.lattice(d, max(mc.rows_for(d))))
        _CTX[d] = (new_ctx(d, u), XArray(u))
    return _CTX[d]


def cov_modes(c, d):
    """The settings of OPT_COV_KERNEL that pick different kernels at this n_dim: 1 register blocks | 2 matrix cores (d >= 16)."""
    from tempest_amd.device import OPT_COV_KERNEL
    for mode in ((1, 2) if d >= 16 else (0,)):
        c.set_option(OPT_COV_KERNEL, mode)
        yield mode
    c.set_option(OPT_COV_KERNEL, 0)


def x_sums(c, x, n, w):
    from tempest_amd._lib import check
    sums, rng = c.empty(1 + c.n_dim), c.empty(2 * c.n_dim)
    check(c.lib.tph_x_weighted_sums(c._ctx, x.ptr, x.ld, n, w.data_ptr(), sums.data_ptr(), rng.data_ptr()), "tph_x_weighted_sums")
    return H(sums), H(rng)


def x_cov(c, x, n, w, mean):
    from tempest_amd._lib import check
    cov = c.empty(c.n_dim * c.n_dim)
    check(c.lib.tph_x_weighted_cov(c._ctx, x.ptr, x.ld, n, w.data_ptr(), mean.data_ptr(), cov.data_ptr()), "tph_x_weighted_cov")
    return H(cov)


@pytest.mark.parametrize("d", mc.ALL_D)
def test_weighted_sums_exact(d):
    """tph_weighted_sums on the history and tph_x_weighted_sums on the x array: sum w, sum w u_j, and (x form) the range of u_j
    over the rows WITH weight -- rows 1 and 2 lie beyond it and carry none."""
    c, x = ctx(d)
    lat = mc.lattice(d, max(mc.rows_for(d)))
    for n in mc.rows_for(d):
        kw = mc.weights(d, n)
        sums, rng = mc.sums_ref(lat, kw)
        w = T(kw / 16.0)
        np.testing.assert_array_equal(H(c.weighted_sums(w)), sums, err_msg=f"tph_weighted_sums d={d} n={n}")
        got, got_rng = x_sums(c, x, n, w)
        np.testing.assert_array_equal(got, sums, err_msg=f"tph_x_weighted_sums d={d} n={n}")
        np.testing.assert_array_equal(got_rng, rng, err_msg=f"tph_x_weighted_sums range d={d} n={n}")


@pytest.mark.parametrize("d", mc.ALL_D)
def test_centred_second_moments_exact(d):
    """tph_weighted_cov_centered and tph_x_weighted_cov about a supplied half-lattice centre: every d x d entry, both kernels at
    d >= 16."""
    c, x = ctx(d)
    lat = mc.lattice(d, max(mc.rows_for(d)))
    centre = T(mc.centre_of(lat))
    for n in mc.rows_for(d):
        kw = mc.weights(d, n)
        ref = mc.cov_ref(lat, kw)
        w = T(kw / 16.0)
        for mode in cov_modes(c, d):
            got = H(c.weighted_cov_centered(w, centre)).reshape(d, d)
            np.testing.assert_array_equal(got, ref, err_msg=f"tph_weighted_cov_centered d={d} n={n} cov_kernel={mode}")
            np.testing.assert_array_equal(got, got.T)
            got = x_cov(c, x, n, w, centre).reshape(d, d)
            np.testing.assert_array_equal(got, ref, err_msg=f"tph_x_weighted_cov d={d} n={n} cov_kernel={mode}")
            np.testing.assert_array_equal(got, got.T)


@pytest.mark.parametrize("d", mc.ALL_D)
def test_weighted_moments_exact(d):
    """tph_weighted_moments: weights that sum to a power of two, so the device's own mean S1 / S0 and cov = C / S0 are exact."""
    c, _ = ctx(d)
    lat = mc.lattice(d, max(mc.rows_for(d)))
    for n in mc.MOMENT_N:
        kw, P = mc.pow2_weights(d, n)
        ref = mc.moments_ref(lat, kw, P)
        w = T(kw / 16.0)
        for mode in cov_modes(c, d):
            out = H(c.weighted_moments(w))
            np.testing.assert_array_equal(out[:d], ref.mean, err_msg=f"tph_weighted_moments mean d={d} n={n}")
            np.testing.assert_array_equal(out[d:].reshape(d, d), ref.cov,
                                          err_msg=f"tph_weighted_moments cov d={d} n={n} cov_kernel={mode}")


@pytest.mark.parametrize("d", range(1, 13))
def test_shifted_moments_exact(d):
    """tph_weighted_moments_shifted (k_wmom_small<d>, k_wmom_finish): S0, mean = c + S1 / S0, cov = S2 / S0 - (S1 / S0)^2 about
    a half-lattice centre."""
    c, _ = ctx(d)
    lat = mc.lattice(d, max(mc.rows_for(d)))
    centre = T(mc.centre_of(lat))
    for n in mc.MOMENT_N:
        kw, P = mc.pow2_weights(d, n)
        assert mc.shifted_budget_bits(lat, P) <= 53
        ref = mc.moments_ref(lat, kw, P)
        out = H(c.weighted_moments_shifted(T(kw / 16.0), centre))
        assert out[0] == ref.s0 / 16.0, (d, n)
        np.testing.assert_array_equal(out[1:1 + d], ref.mean, err_msg=f"tph_weighted_moments_shifted mean d={d} n={n}")
        np.testing.assert_array_equal(out[1 + d:].reshape(d, d), ref.cov, err_msg=f"tph_weighted_moments_shifted cov d={d} n={n}")


def test_shifted_moments_refuse_13_dimensions():
    from tempest_amd._lib import TempestHipError
    c, _ = ctx(13)
    with pytest.raises(TempestHipError, match=r"n_dim=13 > 12"):
        c.weighted_moments_shifted(T(np.ones(64)), T(np.full(13, 0.5)))


@pytest.mark.parametrize("d", mc.FIT_D)
def test_fit_covs_exact(d):
    """covs of tph_fit_modes (k_wsum<int>, k_wsum_final, k_fold_cols, k_mean_from_sums, the second-moment kernel with integer
    counts and a label filter, k_colsum2 / _wide, k_cov_finish student = 1) against C / n + diag(C / n) / n: K = 1, and K = 3 with
    a label that owns no row of the last tile; per-label totals 2^10."""
    lat = mc.lattice(d, mc.FIT_N, b=mc.B_FIT)
    c = new_ctx(d, mc.u_of(lat))
    for K in (1, 3):
        counts, labels = mc.fit_counts(d, K)
        ct, lt = T(counts, np.int32), (T(labels, np.int32) if K > 1 else None)
        for mode in cov_modes(c, d):
            covs = H(c.fit_modes(ct, lt, K, mc.FIT_N)[1])
            for lab in range(K):
                np.testing.assert_array_equal(covs[lab], mc.fit_cov_ref(lat, counts, labels, lab),
                                              err_msg=f"tph_fit_modes covs d={d} K={K} label={lab} cov_kernel={mode}")
    c.close()


@pytest.mark.parametrize("d", mc.CV_D)
def test_cv_sum_exact(d):
    """tph_cv_sum: sum w^2 clip(d2 - d, +-1e6)^2 with an indefinite integer banded P; at d = 13 also with P scaled so that rows
    clip on both sides."""
    lat = mc.lattice(d, max(mc.cv_rows_for(d)), b=mc.B_CV, seed=5)
    c = new_ctx(d, mc.u_of(lat))
    cases = [mc.cv_case(d, n) for n in mc.cv_rows_for(d)] + ([mc.cv_case(d, 2397, shift=20)] if d == 13 else [])
    for case in cases:
        ref, hi, lo = mc.cv_ref(case)
        mean, P = mc.cv_inputs(case)
        got = H(c.cv_sum(T(case.kw.astype(np.float64)), T(mean), T(P)))[0]
        assert got == ref, (d, case.kw.size, case.shift, hi, lo, got, ref)
    c.close()


def test_more_than_100_dimensions_are_refused():
    from tempest_amd._lib import TempestHipError
    d, n = 101, 65
    u = mc.u_of(mc.lattice(d, n))
    c, x = new_ctx(d, u), XArray(u)
    w, mean, msg = T(np.ones(n)), T(np.full(d, 0.5)), r"covariance kernel supports n_dim <= 100 \(got 101\)"
    with pytest.raises(TempestHipError, match=msg):
        c.weighted_cov_centered(w, mean)
    with pytest.raises(TempestHipError, match=msg):
        x_cov(c, x, n, w, mean)
    with pytest.raises(TempestHipError, match=msg):
        c.weighted_moments(w)
    with pytest.raises(TempestHipError, match=msg):
        c.fit_modes(T(np.ones(n), np.int32), None, 1, n)
    c.close()


@pytest.mark.parametrize("d", [5, 14, 50])
def test_non_lattice_data_within_the_a_priori_bound(d, capsys):
    """The one comparison with a tolerance: correlated Gaussian data clipped to the cube, log-normal weights
    (tph_weighted_moments) and Poisson counts (covs of tph_fit_modes), against np.longdouble.  The bound is moment_cases.
    moments_bound: per entry (n + 4) 2^-53 times the sum of the absolute terms, plus the rounding of S0 and the error of the
    computed mean propagated to first order -- what ANY summation order satisfies, derived, not fitted to the device.  The
    largest ratio error / bound is printed.  Measured on the MI355X (n = 2397), largest over the entries: mean 2.7e-4 | 6.2e-4 |
    4.0e-4 at d = 5 | 14 | 50; cov 5.8e-5 | 1.1e-4 | 1.2e-4 (matrix cores at d = 50: 9.1e-5); fit covs 9.3e-5 | 1.1e-4 | 1.8e-4
    (matrix cores: 1.5e-4).  Rounding errors add like a random walk, the bound adds their moduli: three to four decimal orders
    of room are what a correct kernel shows, and the bound stays where the derivation puts it."""
    u, w, counts = mc.gaussian_case(d)
    n = w.size
    c = new_ctx(d, u)
    worst = {}
    m, cov, bm, bc = mc.moments_bound(u, w)
    nf = float(counts.sum())
    mf, cf, _, bf = mc.moments_bound(u, counts.astype(np.float64))
    fit_ref = cf + np.diag(np.diag(cf)) / nf
    fit_bound = bf * (1.0 + 1.0 / nf) + 2.0 ** -52 * np.abs(fit_ref)       # the finish: one division and one addition more
    for mode in cov_modes(c, d):
        out = H(c.weighted_moments(T(w)))
        worst["mean", mode] = float((np.abs(out[:d] - m) / bm).max())
        worst["cov", mode] = float((np.abs(out[d:].reshape(d, d) - cov) / bc).max())
        covs = H(c.fit_modes(T(counts, np.int32), None, 1, n)[1])[0]
        worst["fit", mode] = float((np.abs(covs - fit_ref) / fit_bound).max())
    c.close()
    with capsys.disabled():
        print(f"\n[moments] non-lattice d={d} n={n}: error / a-priori bound = "
              + ", ".join(f"{k[0]}(cov_kernel={k[1]}) {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst

"""csrc/quantile.h on the device: tphu_ndtri / tphu_erfinv through a traced derived() against mpmath on the fixed sample of
tests/quantile_cases.py, tempest_amd.Prior traced and hand-assembled giving the same bits, and a whole run under Normal priors
against its closed form.  One plugin each, shared by the tests of this module."""
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import quantile_cases as Q

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")]

SIZES = (1, 63, 64, 65, 1000)          # both sides of a wave; 1000: four workgroups, no multiple of 256


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------ device values
def prior_pair(u):
    return torch.stack([u[:, 0], 2.0 * u[:, 1] - 1.0], dim=1)


def like_pair(x):
    return -0.5 * (x * x).sum(dim=1)


def derived_pair(x):
    return torch.stack([torch.special.ndtri(x[:, 0]), torch.erfinv(x[:, 1])], dim=1)


@pytest.fixture(scope="module")
def pair():
    import tempest_amd as tp
    return tp.trace_callbacks(prior_pair, like_pair, 2, derived=derived_pair, check=True)


def rows():
    """(n, 2) arguments -- the special values first, then the fixed samples (the shorter one repeated) -- and the index of every row
    in its sample (-1: a special value)."""
    p, y = Q.sample_p(), Q.sample_y()
    n = max(p.size, y.size)
    ip, iy = np.arange(n) % p.size, np.arange(n) % y.size
    x = np.stack([np.concatenate([Q.SPECIAL_P, p[ip]]), np.concatenate([Q.SPECIAL_Y, y[iy]])], axis=1)
    pad = np.full(Q.SPECIAL_P.size, -1)
    return x, np.concatenate([pad, ip]), np.concatenate([pad, iy])


def test_device_values_against_mpmath(pair):
    """Every finite value within the host-measured bound plus 2 ulp of the truth; the non-finite ones where the replay has them."""
    from tempest_amd.trace import erfinv_host, ndtri_host
    x, ip, iy = rows()
    assert Q.SPECIAL_P.size == Q.SPECIAL_Y.size and x.shape[0] > 19000
    # the whole sample in batches of 1000 rows, on the torch entry ...
    got = np.concatenate([pair.derived(torch.from_numpy(x[i:i + 1000]).cuda()).cpu().numpy() for i in range(0, x.shape[0], 1000)])
    # ... and every launch shape from the first row on, special values included, on the NumPy entry: the same bits
    for n in SIZES:
        np.testing.assert_array_equal(bits(pair.derived(x[:n])), bits(got[:n]), err_msg=f"n = {n}")
    for c, (name, host, truth, idx, bound) in enumerate((("tphu_ndtri", ndtri_host, Q.truth_ndtri(), ip, Q.NDTRI_HOST_ULP),
                                                         ("tphu_erfinv", erfinv_host, Q.truth_erfinv(), iy, Q.ERFINV_HOST_ULP))):
        want = host(x[:, c])
        for kind in (np.isnan, np.isposinf, np.isneginf):
            np.testing.assert_array_equal(kind(got[:, c]), kind(want), err_msg=f"{name}: {kind.__name__}")
        assert np.isnan(want).sum() >= 6 and np.isinf(want).sum() >= 2
        sampled = idx >= 0
        assert np.all(np.isfinite(got[sampled, c]))
        err = Q.ulp_error(got[sampled, c], (truth[0][idx[sampled]], truth[1][idx[sampled]]))
        print(f"{name} on the device: largest error {err.max():.3f} ulp, mean {err.mean():.3f} ulp over {err.size} values; "
              f"{int((bits(got[sampled, c]) != bits(want[sampled])).sum())} differ from the replay")
        assert err.max() <= bound + Q.DEVICE_EXTRA_ULP, (name, float(err.max()))
        special = ~sampled & np.isfinite(want)
        np.testing.assert_array_equal(bits(got[special, c]), bits(want[special]), err_msg=f"{name}: zeros and their signs")


# ------------------------------------------------------------------------------------------------------- two spellings, same bits
LIKE7 = "__device__ double log_likelihood(const double* x) { return -0.5 * (x[0] * x[0] + x[1] * x[1]); }\n"


def like7(x):
    return -0.5 * (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])


def seven():
    import tempest_amd as tp
    P = tp.priors
    return tp.Prior([P.Uniform(-5, 5), P.Normal(0.0, 2.0), P.LogNormal(0.0, 0.5), P.HalfNormal(1.0),
                     P.TruncatedNormal(0.0, 1.0, lo=-1.0, hi=3.0), P.LogUniform(1e-3, 1e2), P.Exponential(2.0)])


@pytest.fixture(scope="module")
def spellings():
    import tempest_amd as tp
    prior = seven()
    return prior, tp.trace_callbacks(prior.transform, like7, 7, check=True), tp.HipCallbacks(prior.hip_source() + LIKE7, 7)


def test_traced_and_hand_assembled_prior_give_the_same_bits(spellings):
    from tempest_amd import trace as T
    prior, cb_traced, cb_hand = spellings
    assert cb_traced.trace_report["probe"]["prior_transform"]["nonfinite_agree"]
    for n in (1, 64, 1000):
        u = np.random.RandomState(n).uniform(size=(n, 7))
        u[0, :] = (0.5, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)[:7]                 # the ends of the unit interval: infinite parameters
        a, b = cb_traced.prior_transform(u), cb_hand.prior_transform(u)
        assert isinstance(a, np.ndarray) and a.shape == (n, 7)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"NumPy entry, n = {n}")
        ut = torch.from_numpy(u).cuda()
        at, bt = cb_traced.prior_transform(ut), cb_hand.prior_transform(ut)
        assert isinstance(at, torch.Tensor) and at.is_cuda
        np.testing.assert_array_equal(bits(at.cpu().numpy()), bits(bt.cpu().numpy()), err_msg=f"torch entry, n = {n}")
        np.testing.assert_array_equal(bits(at.cpu().numpy()), bits(a))
        # And they are the replay's values up to the device's own log and exp.  The widest column is the log-normal one: ndtri within
        # 2 ulp of the replay's (DEVICE_EXTRA_ULP), at |ndtri| < 4 and s = 0.5 an absolute 2 ulp(2) x 0.5 = 2 ulp(1) in the argument of
        # exp, which is up to 4 ulp of a result whose mantissa is next to 1; one more for the device's exp, one for the rounding.
        want = T.replay(cb_traced.trace_graphs["prior_transform"], u)
        for kind in (np.isnan, np.isposinf, np.isneginf):
            np.testing.assert_array_equal(kind(a), kind(want))
        fin = np.isfinite(want)
        assert T._ulps(a[fin], want[fin]).max() <= 6.0


# ------------------------------------------------------------------------------------------------------------------- a whole run
Y, SIGMA = (0.7, -0.4, 1.0), 0.5


def like_run(x):
    """Gaussian data y_j ~ N(x_j, sigma^2): normalised in the two columns under Normal priors, the bare exponential in the third, so
    that the evidence is  sum_{j<2} log N(y_j; 0, 1 + sigma^2) + log(sigma sqrt(2 pi) / 20)."""
    z0, z1, z2 = (x[:, 0] - Y[0]) / SIGMA, (x[:, 1] - Y[1]) / SIGMA, (x[:, 2] - Y[2]) / SIGMA
    return -0.5 * (z0 * z0 + z1 * z1 + z2 * z2) - 2.0 * math.log(SIGMA * math.sqrt(2.0 * math.pi))


def test_a_whole_run_under_normal_priors():
    import tempest_amd as tp
    P = tp.priors
    prior = tp.Prior([P.Normal(0.0, 1.0)] * 2 + [P.Uniform(-10.0, 10.0)])
    cb = tp.trace_callbacks(prior.transform, like_run, prior.n_dim, check=True)
    v = 1.0 + SIGMA ** 2
    truth = sum(-0.5 * y * y / v - 0.5 * math.log(2.0 * math.pi * v) for y in Y[:2]) + math.log(SIGMA * math.sqrt(2.0 * math.pi) / 20.0)
    out = []
    for _ in range(2):
        s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=128, vectorize=True, clustering=False, random_state=4,
                       batch_prior=True)
        s.run(n_total=512, progress=False)
        x, w, _ = s.posterior()
        out.append((s.evidence()[0], np.average(x, weights=w, axis=0)))
    (z, mean), (z2, _) = out
    print(f"logZ = {z:.4f} (closed form {truth:.4f}); posterior mean {mean[:2]} (closed form {[y / v for y in Y[:2]]})")
    assert abs(z - truth) < 0.5, (z, truth)
    np.testing.assert_allclose(mean[:2], [y / v for y in Y[:2]], atol=0.1)
    assert bits(np.array([z]))[0] == bits(np.array([z2]))[0]

"""One row selection behind every result method: on the state file the reference wrote (tests/golden/ref_state_small.state), the rows
and weights the device-side outputs reduce over are the `x` and `weights` of `posterior()`, bit for bit and in order; the resampled
posterior is `x[idx]` of the systematic draw at the same uniform; derived blobs are the function's values on the returned rows;
`marginals()` counts the same rows -- with the default trim, without trimming, and with another (ess, bins) setting."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(__file__), "golden")
SETTINGS = {"trim": dict(trim_importance_weights=True),
            "full": dict(trim_importance_weights=False),
            "trim90": dict(trim_importance_weights=True, ess_trim=0.9, bins_trim=50)}
each_setting = pytest.mark.parametrize("tag", list(SETTINGS))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def load(**kw):
    import tempest_amd as tp
    g = np.load(os.path.join(G, "ref_state_small.npz"))
    d, n = int(g["n_dim"]), int(g["n_particles"])
    mean = torch.tensor(g["mean"], dtype=torch.float64, device="cuda:0")

    def like(x):
        return -0.5 * ((x - mean) ** 2).sum(dim=1) - 0.5 * d * float(np.log(2 * np.pi))
    s = tp.Sampler(lambda u: 20 * u - 10, like, d, n_particles=n, vectorize=True, clustering=False, random_state=7, **kw)
    s.load_state(os.path.join(G, "ref_state_small.state"))
    return s


@pytest.fixture(scope="module")
def sampler():
    return load()


@pytest.fixture(scope="module")
def posterior(sampler):
    """(x, weights, logl) of the unresampled posterior() per setting: computed once, left unchanged."""
    return {tag: sampler.posterior(**kw) for tag, kw in SETTINGS.items()}


def test_the_trim_drops_rows_on_this_state(posterior):
    n = {tag: len(p[0]) for tag, p in posterior.items()}
    assert 0 < n["trim"] < n["full"] and 0 < n["trim90"] < n["full"], n


@each_setting
def test_weighted_rows_are_the_posterior_rows(sampler, posterior, tag):
    kw = dict(dict(trim_importance_weights=True, ess_trim=0.99, bins_trim=1000), **SETTINGS[tag])
    x_dev, w_sel = sampler._core._weighted_rows("marginals", "", kw["trim_importance_weights"], kw["ess_trim"], kw["bins_trim"])
    x, w, _ = posterior[tag]
    assert x_dev.is_cuda and w_sel.is_cuda
    np.testing.assert_array_equal(x_dev.cpu().numpy(), x)
    np.testing.assert_array_equal(w_sel.cpu().numpy(), w)


@each_setting
@pytest.mark.parametrize("k", [0, 11])
def test_resampled_posterior_is_the_systematic_draw_of_the_rows(sampler, posterior, tag, k):
    from tempest_amd.tools import systematic_resample
    x, w, logl = posterior[tag]
    np.random.seed(k)
    xr, wr, lr = sampler.posterior(resample=True, **SETTINGS[tag])
    idx = systematic_resample(len(w), w, random_state=k)          # seeds NumPy's stream with k: the same uniform
    assert idx.shape == (len(w),) and len(np.unique(idx)) > 1
    np.testing.assert_array_equal(xr, x[idx])
    np.testing.assert_array_equal(lr, logl[idx])
    np.testing.assert_array_equal(wr, np.ones(len(w)) / len(w))


@each_setting
def test_derived_blobs_are_the_function_on_the_returned_rows(posterior, tag):
    two = lambda x: x[:, 0:2] * x[:, 1:3]                          # noqa: E731  (one IEEE product: the same bits on either side)
    one = lambda x: x[:, 0] * x[:, 1]                              # noqa: E731
    x0, w0, _ = posterior[tag]
    for fn, shape in ((two, (len(x0), 2)), (one, (len(x0),))):
        s = load(derived=fn)
        x, w, _, blobs = s.posterior(return_blobs=True, **SETTINGS[tag])
        np.testing.assert_array_equal(x, x0)
        np.testing.assert_array_equal(w, w0)
        assert blobs.shape == shape and blobs.dtype == np.float64
        np.testing.assert_array_equal(blobs, fn(x))
        np.random.seed(5)
        xr, _, _, br = s.posterior(return_blobs=True, resample=True, **SETTINGS[tag])
        assert br.shape == shape
        np.testing.assert_array_equal(br, fn(xr))


@each_setting
def test_marginals_count_the_posterior_rows(sampler, posterior, tag):
    assert sampler.marginals(**SETTINGS[tag])["n_rows"] == len(posterior[tag][0])

"""tempest_amd.trace_callbacks on the device: the compiled traces against the eager torch callbacks on the same GPU, against the
replay of their graphs, the probe, and a whole run.  One plugin per n_dim, shared by every test of this module."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")]

EPS = float(np.finfo(np.float64).eps)
SIZES = (1, 63, 64, 65, 1000)          # both sides of a wave; 1000: four workgroups, no multiple of 256


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------------------------------- exact operations, d = 2 and 3
def prior_assigned(u):
    x = torch.empty_like(u)
    x[:, 0] = 10.0 * u[:, 0] - 5.0
    x[:, 1:] = 8.0 * u[:, 1:] - 3.0
    return x


def like2(x):
    a = x[:, 0] ** 2 - x[:, 1]
    s = 1.0 + x[:, 0] * x[:, 0]
    # 0.3 / s, -0.7 / (2 s): number / tensor through the operator, which torch computes as reciprocal() * number
    return -(10.0 * a ** 2 + (x[:, 0] - 1.0) ** 2) - torch.sqrt(torch.abs(x[:, 1])) / s + 0.3 / s - 0.7 / (2.0 * s) + x[:, 1] / 3.0


def derived2(x):
    return torch.stack([x[:, 0] * x[:, 1], torch.maximum(x[:, 0], x[:, 1]) - x[:, 0] ** 3], dim=1)


def like3(x):
    """-inf outside a box (where), exact operations inside."""
    r = torch.abs(x[:, 0]) + torch.minimum(x[:, 1], x[:, 2] ** 3) / (2.0 + torch.sqrt(torch.abs(x[:, 1] - x[..., -1])))
    inside = (x[:, 0] > -4.0) & (x[:, 0] < 3.5) & ~(x[:, 2] >= 4.0)
    return torch.where(inside, -(r * r) - torch.clamp(x[:, 1], -1.0, 2.0), -np.inf)


# one column per transcendental (against eager torch on the same GPU), and NaN from the log of a negative number in the last
TRANSCENDENTALS = ("exp", "log", "log1p", "sin", "tanh", "erf", "lgamma", "logsumexp")


def derived3(x):
    pos = torch.abs(x[:, 1]) + 0.125
    return torch.stack([torch.exp(x[:, 0]), torch.log(pos), torch.log1p(pos), torch.sin(x[:, 2]), torch.tanh(x[:, 0]), torch.erf(x[:, 1]),
                        torch.lgamma(pos), torch.logsumexp(x[:, :2], dim=1), torch.log(x[:, 0])], dim=-1)


# ------------------------------------------------------------------------------------------------------------------ reductions
def prior20(u):
    return 20 * u - 10


def rosenbrock(x):
    return -(10.0 * (x[:, ::2] ** 2.0 - x[:, 1::2]) ** 2.0 + (x[:, ::2] - 1.0) ** 2.0).sum(dim=1)


A5 = np.random.RandomState(11).uniform(-2.0, 2.0, size=(5, 5))


def prior_matmul(u):
    return u @ torch.as_tensor(A5, device=u.device)


def like_sum(x):
    return x.sum(dim=1)


CASES = {2: (prior_assigned, like2, derived2), 3: (prior_assigned, like3, derived3), 5: (prior_matmul, like_sum, None),
         10: (prior20, rosenbrock, None), 16: (prior20, rosenbrock, None)}


@pytest.fixture(scope="module")
def plugins():
    import tempest_amd as tp
    made = {}

    def get(d):
        need_gpu()
        if d not in made:
            pt, ll, dv = CASES[d]
            made[d] = tp.trace_callbacks(pt, ll, d, derived=dv, check=True)
        return made[d]
    return get


def unit(n, d, seed=0):
    return np.random.RandomState(seed + n).uniform(size=(n, d))


def same(got, want, msg=""):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=msg)


@pytest.mark.parametrize("d", [2, 3])
def test_exact_operations_equal_eager_torch_bit_for_bit(plugins, d):
    cb = plugins(d)
    pt, ll, _ = CASES[d]
    for n in SIZES:
        u = unit(n, d)
        ut = torch.from_numpy(u).cuda()
        xt = pt(ut)
        got = cb.prior_transform(ut)                                  # the torch-tensor entry
        assert isinstance(got, torch.Tensor) and got.is_cuda
        same(got.cpu(), xt.cpu(), f"prior n={n}")
        same(cb.log_likelihood(xt).cpu(), ll(xt).cpu(), f"like n={n}")
        x = xt.cpu().numpy()
        got = cb.prior_transform(u)                                   # the NumPy entry
        assert isinstance(got, np.ndarray)
        same(got, x, f"prior numpy n={n}")
        same(cb.log_likelihood(x), ll(xt).cpu().numpy(), f"like numpy n={n}")


def test_derived_of_exact_operations_equals_eager_torch(plugins):
    cb = plugins(2)
    xt = prior_assigned(torch.from_numpy(unit(1000, 2)).cuda())
    same(cb.derived(xt).cpu(), derived2(xt).cpu())


@pytest.mark.parametrize("d", [10, 16])
def test_rosenbrock_equals_replay_and_is_within_the_summation_bound_of_eager(plugins, d):
    from tempest_amd import trace as T
    cb = plugins(d)
    u = unit(1000, d)
    ut = torch.from_numpy(u).cuda()
    xt = prior20(ut)
    same(cb.prior_transform(ut).cpu(), xt.cpu())
    x = xt.cpu().numpy()
    got = cb.log_likelihood(xt).cpu().numpy()
    same(got, T.replay(cb.trace_graphs["log_likelihood"], x))
    eager = rosenbrock(xt).cpu().numpy()
    k = d // 2                                                        # terms of one sign: sum |terms| = |logl|
    err = np.abs(got - eager)
    print(f"d={d}: largest |traced - eager| / (eps |logl|) = {np.max(err / (EPS * np.abs(eager))):.3g}, bound {2 * (k - 1)}")
    assert np.all(err <= 2 * (k - 1) * EPS * np.abs(eager))


def test_matmul_equals_replay_and_is_within_the_summation_bound_of_eager(plugins):
    from tempest_amd import trace as T
    cb = plugins(5)
    u = unit(1000, 5)
    ut = torch.from_numpy(u).cuda()
    got = cb.prior_transform(ut).cpu().numpy()
    same(got, T.replay(cb.trace_graphs["prior_transform"], u))
    want = np.zeros((1000, 5))
    for i in range(5):                                                # the stated order: products in index order, added left to right
        want = u[:, i:i + 1] * A5[i] if i == 0 else want + u[:, i:i + 1] * A5[i]
    same(got, want)
    eager = prior_matmul(ut).cpu().numpy()
    k, terms = 5, np.abs(u) @ np.abs(A5)
    print(f"matmul: largest |traced - eager| / (eps sum|terms|) = {np.max(np.abs(got - eager) / (EPS * terms)):.3g}, bound {2 * (k - 1)}")
    assert np.all(np.abs(got - eager) <= 2 * (k - 1) * EPS * terms)
    xt = torch.from_numpy(got).cuda()
    ll = cb.log_likelihood(xt).cpu().numpy()
    same(ll, T.replay(cb.trace_graphs["log_likelihood"], got))
    assert np.all(np.abs(ll - like_sum(xt).cpu().numpy()) <= 2 * (k - 1) * EPS * np.abs(got).sum(axis=1))


def test_transcendentals_equal_eager_torch_on_the_same_gpu(plugins):
    """Both sides call the same device math library: 0 ulp expected, equality asserted (the figures are printed first)."""
    from tempest_amd.trace import _ulps
    cb = plugins(3)
    xt = prior_assigned(torch.from_numpy(unit(1000, 3, seed=7)).cuda())
    got, want = cb.derived(xt).cpu().numpy(), derived3(xt).cpu().numpy()
    ulps = {}
    for c, name in enumerate(TRANSCENDENTALS):
        assert np.all(np.isfinite(want[:, c])), name
        ulps[name] = float(_ulps(got[:, c], want[:, c]).max()) if np.all(np.isfinite(got[:, c])) else float("inf")
    print("largest difference from eager torch in ulp:", ulps)
    for c, name in enumerate(TRANSCENDENTALS):
        same(got[:, c], want[:, c], name)


def test_non_finite_values_fall_on_eagers_rows(plugins):
    cb = plugins(3)
    xt = prior_assigned(torch.from_numpy(unit(1000, 3, seed=9)).cuda())
    want = like3(xt).cpu().numpy()
    got = cb.log_likelihood(xt).cpu().numpy()
    assert 0 < np.isneginf(want).sum() < 1000
    same(np.isneginf(got), np.isneginf(want))
    same(got, want)
    nan_got, nan_want = cb.derived(xt).cpu().numpy()[:, -1], derived3(xt).cpu().numpy()[:, -1]
    assert 0 < np.isnan(nan_want).sum() < 1000                        # log of a negative number
    same(np.isnan(nan_got), np.isnan(nan_want))
    same(nan_got, nan_want)


def test_probe_passes_and_fills_the_report(plugins):
    for d, (_, _, dv) in CASES.items():
        rep = plugins(d).trace_report
        assert rep["n_ops"] > 0 and rep["widest"] >= d and rep["constants"] and rep["probe"]["against"] == "compiled plugin on the device"
        assert set(rep["probe"]["eager_on"].values()) == {"device"}
        for name in ("prior_transform", "log_likelihood") + (("derived",) if dv else ()):
            p = rep["probe"][name]
            assert p["nonfinite_agree"] and np.isfinite(p["max_abs_diff"]) and np.isfinite(p["max_ulps"])
        assert rep["ops"]["log_likelihood"] == plugins(d).trace_graphs["log_likelihood"].n_ops()


def test_probe_refuses_a_trace_of_another_function(plugins):
    from tempest_amd import trace as T
    cb = plugins(2)
    with pytest.raises(T.TraceError, match="log_likelihood: differs from the eager function") as e:
        T.probe(cb, prior_assigned, lambda x: like2(x) + 1e-3, derived2)
    assert e.value.source == cb.source and "log_likelihood" in e.value.report
    with pytest.raises(T.TraceError, match="prior_transform: the non-finite values"):
        T.probe(cb, lambda u: torch.log(prior_assigned(u)), like2, derived2)


def run(tp, pt, ll, seed=5):
    # batch_prior=True: the prior is written for (n, d) batches (column assignment), as traced callbacks are; no row-by-row probe
    s = tp.Sampler(pt, ll, 2, n_particles=1024, vectorize=True, clustering=False, random_state=seed, batch_prior=True)
    s.run(n_total=2048, progress=False)
    np.random.seed(3)
    return s, s.posterior(), s.evidence()


def test_whole_run_is_the_eager_run_bit_for_bit(plugins):
    import tempest_amd as tp
    fused = plugins(2)
    assert fused.fused
    unfused = tp.trace_callbacks(prior_assigned, like2, 2, derived=derived2, check=False, fused=False)      # the same plugin file
    assert unfused.path == fused.path and not unfused.fused
    _, post_e, z_e = run(tp, prior_assigned, like2)
    _, post_u, z_u = run(tp, unfused.prior_transform, unfused.log_likelihood)
    s, post_f, z_f = run(tp, fused.prior_transform, fused.log_likelihood)
    assert s._core.callbacks.hip_plugin is fused
    for a, b in zip(post_u, post_e):
        same(a, b, "fused=False against the eager callbacks")
    assert z_u == z_e
    for a, b in zip(post_f, post_u):
        same(a, b, "fused=True against fused=False")
    assert z_f == z_u
    np.random.seed(3)
    x, w, logl, blobs = s.posterior(return_blobs=True)
    same(x, post_f[0])
    assert blobs.shape == (len(x), 2)
    same(blobs, derived2(torch.from_numpy(np.ascontiguousarray(x)).cuda()).cpu().numpy())
    assert s.marginals()["n_derived"] == 2

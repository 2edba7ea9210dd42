"""tempest_amd.trace_callbacks(replicate=, discrepancy=) on the device: the traced torch restatements of BERN and GAUSS against the
hand-written sources of test_hipcallbacks_replicate.py -- equal bits expected in every output of cb.replicated: the same operations in
the same order, contraction off around user code, the same kernels --, the traced Bernoulli against the host's y_rep matrix, the probe
against the compiled plugin, draws and seeds, update_data on the observed entry, and a Sampler run.  Rows 1, 63, 700 and n_replicate
1, 64, 65, 130: the smallest shapes that cross one wave, one 64-row tile and the 64 / 16 sum layout.

The objects are built once per module: a plugin file per source text (data sets of the same names share it), an object per data set."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

from tests.test_hipcallbacks_replicate import BERN, GAUSS, KEYS, QS, bern_case, gauss_data, gauss_rows, make, same_bits
from tests.test_trace_replicate import gauss_discrepancy, gauss_prior, gauss_replicate, gauss_term, traced_bern, traced_gauss

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")]

ROWS = (1, 63, 700)
N_REPLICATE = (1, 64, 65, 130)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def gauss_pair(R):
    """(traced, hand-written, data) of the linear Gaussian at R observations."""
    import tempest_amd as tp
    D = gauss_data(R, seed=R)
    return traced_gauss(tp, D), make(tp, GAUSS, 2, D, n_terms="t"), D


@functools.lru_cache(maxsize=None)
def bern_pair(R):
    import tempest_amd as tp
    D = bern_case(1, R, 3)[2]                       # the data depend on R alone
    return traced_bern(tp, D), make(tp, BERN, 3, D), D


@pytest.mark.parametrize("R", N_REPLICATE)
def test_traced_gauss_equals_the_hand_written_source(R):
    need_gpu()
    traced, hand, D = gauss_pair(R)
    assert traced.path != hand.path and traced.n_replicate == hand.n_replicate == R
    for n in ROWS:
        x, w = gauss_rows(n, seed=n)
        xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
        a, b = traced.replicated(xt, wt, quantiles=QS, seed=n + 1), hand.replicated(xt, wt, quantiles=QS, seed=n + 1)
        assert set(a) == set(b) and set(KEYS) <= set(a)
        same_bits(a, b, msg=f"n={n} R={R}: traced against hand-written")
        assert np.all(np.isfinite(a["mean"])) and np.isfinite(a["t_rep_mean"])


@pytest.mark.parametrize("R", N_REPLICATE)
def test_traced_bern_equals_the_hand_written_source_and_the_host_matrix(R):
    need_gpu()
    traced, hand, _ = bern_pair(R)
    for n in ROWS:
        x, w, D, seed, ref = bern_case(n, R, 3)
        xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
        a, b = traced.replicated(xt, wt, quantiles=QS, seed=seed), hand.replicated(xt, wt, quantiles=QS, seed=seed)
        same_bits(a, b, msg=f"n={n} R={R}: traced against hand-written")
        same_bits(a, ref, msg=f"n={n} R={R}: traced against the host's y_rep matrix")


def test_the_probe_ran_the_compiled_plugin_and_holds_replicate_and_discrepancy():
    need_gpu()
    for cb in (gauss_pair(65)[0], bern_pair(65)[0]):
        probe = cb.trace_report["probe"]
        assert probe["against"] == "compiled plugin on the device"
        for name in ("replicate", "discrepancy"):
            print(name, probe[name])                 # (the probe raises beyond SQRTEPS (1 + |eager|): an entry is within the rule)
            assert probe[name]["nonfinite_agree"] and np.isfinite(probe[name]["max_abs_diff"]), (name, probe[name])
        assert probe["eager_on"]["replicate"] == "device"
    # the uniforms are the device's bits and BERN's operations are exact: nothing may differ; GAUSS's normals agree to rounding
    for name in ("replicate", "discrepancy"):
        assert bern_pair(65)[0].trace_report["probe"][name]["max_abs_diff"] == 0.0
    assert gauss_pair(65)[0].trace_report["probe"]["replicate"]["max_abs_diff"] <= 1e-12


def test_a_wrong_trace_is_caught_by_the_probe_on_the_device():
    import tempest_amd as tp
    from tempest_amd.trace import TV, TraceError
    need_gpu()
    D = gauss_data(65, seed=65)

    def hidden_branch(x, D, g):                     # Python control flow on a value the tracer cannot see: one branch is traced
        return gauss_replicate(x, D, g) if isinstance(x, TV) else gauss_replicate(x, D, g) + 1e-3

    def hidden_branch_disc(x, y, D):
        return gauss_discrepancy(x, y, D) if isinstance(x, TV) else gauss_discrepancy(x, y, D) * 1.001
    with pytest.raises(TraceError, match="replicate: differs from the eager function") as e:
        tp.trace_callbacks(gauss_prior, gauss_term, 2, data=D, n_terms="t", replicate=hidden_branch, n_replicate="t", observed="y",
                           discrepancy=gauss_discrepancy)
    assert "double replicate(" in e.value.source and "compiled plugin on the device" in str(e.value)
    with pytest.raises(TraceError, match="discrepancy: differs from the eager function") as e:
        tp.trace_callbacks(gauss_prior, gauss_term, 2, data=D, n_terms="t", replicate=gauss_replicate, n_replicate="t", observed="y",
                           discrepancy=hidden_branch_disc)
    assert "double discrepancy(" in e.value.source


def test_draws_differ_by_k_and_by_seed_and_repeat_with_the_seed():
    import tempest_amd as tp
    from tempest_amd.trace import Noise
    need_gpu()
    R, n = 65, 63
    D = gauss_data(R, seed=R)

    def by_k(k):
        return tp.trace_callbacks(gauss_prior, gauss_term, 2, data=D, n_terms="t", n_replicate="t",
                                  replicate=lambda x, D, g: 0.0 * x[:, 0:1] + (D["s"] - D["s"]) + g.uniform(k))
    x, w = gauss_rows(n, seed=1)
    one = np.zeros(n)
    one[5] = 1.0                                                     # row 5 alone has weight: mean[r] is ITS draw at r, item 5
    out = {k: by_k(k).replicated(x, one, quantiles=(0.5,), seed=3)["mean"] for k in (1, 2)}      # lane 1 of draw 0, lane 0 of draw 1
    for k in (1, 2):
        np.testing.assert_array_equal(out[k], Noise(3, [5], R).uniform(k).numpy()[0], err_msg=f"k={k}: the host twin's bits")
    assert np.all(out[1] != out[2])
    cb = gauss_pair(R)[0]
    a, again, b = (cb.replicated(x, w, quantiles=QS, seed=s) for s in (3, 3, 4))
    same_bits(a, again, msg="the same seed")
    assert np.all(a["mean"] != b["mean"]) and np.any(a["quantiles"] != b["quantiles"]) and a["t_rep_mean"] != b["t_rep_mean"]
    assert a["t_obs_mean"] == b["t_obs_mean"]                        # the observed side draws nothing


def test_update_data_on_the_observed_entry_moves_pit_and_not_the_bands():
    import tempest_amd as tp
    need_gpu()
    R, n = 64, 700
    D = gauss_data(R, seed=7)
    traced, hand = traced_gauss(tp, D), make(tp, GAUSS, 2, D, n_terms="t")
    x, w = gauss_rows(n, seed=2)
    before = traced.replicated(x, w, quantiles=QS, seed=5)
    y2 = D["y"] + 0.05
    traced.update_data("y", y2)
    hand.update_data("y", y2)
    after = traced.replicated(x, w, quantiles=QS, seed=5)
    same_bits(after, before, keys=("mean", "var", "quantiles", "t_rep_mean"))
    assert np.any(after["pit"] != before["pit"]) and after["t_obs_mean"] != before["t_obs_mean"]
    same_bits(after, hand.replicated(x, w, quantiles=QS, seed=5), msg="after update_data: traced against hand-written")


def test_through_the_sampler():
    import tempest_amd as tp
    need_gpu()
    D = gauss_data(40, seed=40)
    cb = traced_gauss(tp, D)
    s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 2, n_particles=512, vectorize=True, clustering=False, random_state=11)
    s.run(n_total=1024, progress=False)
    assert s._core.callbacks.hip_plugin is cb
    x, w, _ = s.posterior()
    got, direct = s.replicated(seed=3), cb.replicated(x, w, seed=3)
    assert got["n_rows"] == len(x) and got["seed"] == 3
    same_bits(got, direct)
    assert np.all((got["pit"] >= 0.0) & (got["pit"] <= 1.0)) and 0.0 <= got["p_value"] <= 1.0

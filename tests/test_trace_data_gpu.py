"""tempest_amd.trace_callbacks with observed data on the device: traced torch term functions against the hand-written sources they
restate (REG, POIS of test_hipcallbacks_data.py; QUAD + QUAD_PRED of test_hipcallbacks_predict.py) -- equal bits expected: the same
operations in the same order, contraction off around user code, one sum layout -- and against the NumPy restatements, at the edges of
the sum layout (256-term chunks, 64-chunk blocks) and on both likelihood paths; predictive and pointwise key by key; a design matrix
and a mixture against the replay of their graphs; update_data, eagerly and under a captured graph; whole runs."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests.test_hipcallbacks_data import POIS, REG, layered_sum, particles, pois_data, reference_loglike, reg_data, reg_terms
from tests.test_hipcallbacks_predict import QUAD, QUAD_PRED
from tests.test_trace_data import data_of, design_term, mixture_term, pois_term, prior, quad_model, quad_term, reg_term

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")]

N_TERMS = (1, 255, 256, 257, 16_385)          # one term; either side of a chunk; one past a block of 64 chunks
N_PARTICLES = (1, 63, 700)
QS = (0.025, 0.5, 0.975)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same(got, want, msg=""):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=msg)


def both_paths(cb, xt):
    out = {}
    for path in ("lane", "split"):
        cb.data_like = path
        out[path] = cb.log_likelihood(xt).cpu().numpy()
    cb.data_like = None
    return out


def quad_data(n_terms):
    return {k: v for k, v in reg_data(n_terms).items() if k != "c"}


@pytest.mark.parametrize("n_terms", N_TERMS)
def test_traced_reg_equals_the_hand_written_source_and_the_restatement(n_terms):
    import tempest_amd as tp
    need_gpu()
    D = reg_data(n_terms)
    traced = tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms="t")
    hand = tp.HipCallbacks(REG, 3, data=D, n_terms="t")
    assert traced.trace_report["probe"]["against"] == "compiled plugin on the device" and traced.path != hand.path
    for n in N_PARTICLES:
        x = particles(n, seed=n)
        want = reference_loglike(x, D, reg_terms, traced.sum_layout)
        xt = torch.from_numpy(x).cuda()
        got, ref = both_paths(traced, xt), both_paths(hand, xt)
        for path in ("lane", "split"):
            same(got[path], ref[path], f"{path} n={n} n_terms={n_terms}: traced against hand-written")
            same(got[path], want, f"{path} n={n} n_terms={n_terms}: traced against the restatement")
    u = np.random.RandomState(2).uniform(size=(65, 3))
    same(traced.prior_transform(u), hand.prior_transform(u))
    same(traced.prior_transform(u), 10.0 * u - 5.0)


@pytest.mark.parametrize("n_terms", N_TERMS)
def test_traced_pois_equals_the_hand_written_source(n_terms):
    """The same device exp / log on the same arguments: equal bits against the hand-written POIS.  Against the eager torch terms
    (torch's own exp / log kernels) summed by layered_sum only the probe's tolerance is asserted; the largest difference in ulps
    is printed (recorded in DESIGN.md section 11t)."""
    import tempest_amd as tp
    from tempest_amd.tools import SQRTEPS
    from tempest_amd.trace import _ulps
    need_gpu()
    D = pois_data(n_terms)
    traced = tp.trace_callbacks(prior, pois_term, 3, data=D, n_terms=n_terms)
    hand = tp.HipCallbacks(POIS, 3, data=D, n_terms=n_terms)
    Dt = {k: torch.from_numpy(v).cuda() for k, v in D.items()}
    worst = 0.0
    for n in N_PARTICLES:
        x = particles(n, seed=100 + n)
        xt = torch.from_numpy(x).cuda()
        got, ref = both_paths(traced, xt), both_paths(hand, xt)
        for path in ("lane", "split"):
            same(got[path], ref[path], f"{path} n={n} n_terms={n_terms}")
        eager = layered_sum(pois_term(xt, Dt).cpu().numpy(), *traced.sum_layout)
        worst = max(worst, float(_ulps(got["lane"], eager).max()))
        assert np.all(np.abs(got["lane"] - eager) <= SQRTEPS * (1.0 + np.abs(eager))), (n, n_terms)
    print(f"n_terms={n_terms}: traced POIS against eager torch terms summed by layered_sum: at most {worst:.0f} ulp")


@pytest.mark.parametrize("n_terms", [7, 257])
def test_predictive_and_pointwise_equal_the_hand_written_objects(n_terms):
    import tempest_amd as tp
    need_gpu()
    D = quad_data(n_terms)
    traced = tp.trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", predict=quad_model, n_predict="t", pointwise=True)
    hand = tp.HipCallbacks(QUAD + QUAD_PRED, 3, data=D, n_terms="t", n_predict="t", pointwise=True)
    probe = traced.trace_report["probe"]
    assert probe["predict"]["max_ulps"] == 0.0 and probe["predict"]["nonfinite_agree"]          # exact operations: predict exactly
    for n in (1, 65, 3001):
        rng = np.random.RandomState(n + n_terms)
        x = particles(n, seed=n) * 0.2 + np.array([0.7, 1.9, -1.1])
        w = rng.uniform(0.1, 1.0, n)
        xt, wt = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
        a, b = traced.predictive(xt, wt, quantiles=QS), hand.predictive(xt, wt, quantiles=QS)
        assert set(a) == set(b) == {"mean", "var", "quantiles", "n_rows", "ess"}
        for k in a:
            same(a[k], b[k], f"predictive {k} n={n}")
        a, b = traced.pointwise(xt, wt), hand.pointwise(xt, wt)
        assert set(a) == set(b)
        for k in a:
            if k == "totals":
                assert a[k].keys() == b[k].keys()
                for kk in a[k]:
                    same(a[k][kk], b[k][kk], f"pointwise totals {kk} n={n}")
            else:
                same(a[k], b[k], f"pointwise {k} n={n}")
        same(traced.log_likelihood(xt).cpu(), hand.log_likelihood(xt).cpu())


def test_design_matrix_and_mixture_equal_the_summed_replay():
    """x @ D["X"].T (k = 3): products and sums in column order, every one rounded -- the device equals layered_sum of the replayed
    terms.  The mixture's exp / log are the device's: the probe's tolerance."""
    import tempest_amd as tp
    from tempest_amd import trace as T
    from tempest_amd.tools import SQRTEPS
    need_gpu()
    D = data_of(257)
    x = particles(700, seed=9)
    xt = torch.from_numpy(x).cuda()
    cb = tp.trace_callbacks(prior, design_term(3), 3, data=D, n_terms="y")
    want = layered_sum(T.replay(cb.trace_graphs["log_likelihood_term"], x, D), *cb.sum_layout)
    for path, got in both_paths(cb, xt).items():
        same(got, want, f"design matrix, {path}")
    assert cb.trace_report["reads"]["log_likelihood_term"]["X"] == ["column 0", "column 1", "column 2"]
    cb = tp.trace_callbacks(prior, mixture_term, 3, data=D, n_terms="y")
    want = layered_sum(T.replay(cb.trace_graphs["log_likelihood_term"], x, D), *cb.sum_layout)
    got = both_paths(cb, xt)
    same(got["lane"], got["split"])
    print(f"mixture: at most {T._ulps(got['lane'], want).max():.0f} ulp from the summed replay")
    assert np.all(np.abs(got["lane"] - want) <= SQRTEPS * (1.0 + np.abs(want)))


@pytest.mark.parametrize("path", ["lane", "split"])
def test_update_data_reaches_the_traced_likelihood_and_a_captured_graph(path):
    import tempest_amd as tp
    need_gpu()
    D = reg_data(20_000)
    cb = tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms="t")
    cb.data_like = path
    x = particles(300)
    xt = torch.from_numpy(x).cuda()
    same(cb.log_likelihood(xt).cpu(), reference_loglike(x, D, reg_terms, cb.sum_layout))      # tables uploaded, scratch sized
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = cb.log_likelihood(xt)
    g.replay()
    torch.cuda.synchronize()
    same(out.cpu(), reference_loglike(x, D, reg_terms, cb.sum_layout))
    D2 = dict(D, y=D["y"] + 0.25)
    cb.update_data("y", D2["y"])
    want = reference_loglike(x, D2, reg_terms, cb.sum_layout)
    same(cb.log_likelihood(xt).cpu(), want, "eagerly, after update_data")
    g.replay()
    torch.cuda.synchronize()
    same(out.cpu(), want, "the captured graph, after update_data")


@pytest.mark.parametrize("graph", [False, True])
def test_whole_run_equals_the_hand_written_run(graph):
    import tempest_amd as tp
    need_gpu()
    D = quad_data(257)
    traced = tp.trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", predict=quad_model, n_predict="t", pointwise=True)
    hand = tp.HipCallbacks(QUAD + QUAD_PRED, 3, data=D, n_terms="t", n_predict="t", pointwise=True)
    out = []
    for cb in (traced, hand):
        s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=2048, vectorize=True, clustering=False, random_state=4,
                       graph=graph)
        s.run(n_total=4096, progress=False)
        assert s._core.callbacks.hip_plugin is cb
        np.random.seed(3)
        post = s.posterior()
        out.append((post, s.evidence()[0], s.predictive(), s.pointwise()))
    (pa, za, qa, wa), (pb, zb, qb, wb) = out
    for a, b, name in zip(pa, pb, ("rows", "weights", "log-likelihoods")):
        same(a, b, name)
    assert za == zb and np.isfinite(za)
    for k in qa:
        same(qa[k], qb[k], f"predictive {k}")
    for k in wa:
        if k == "totals":
            assert wa[k] == wb[k]
        else:
            same(wa[k], wb[k], f"pointwise {k}")

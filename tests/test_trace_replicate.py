"""tempest_amd.trace_callbacks(replicate=, n_replicate=, observed=, discrepancy=) without a GPU: the torch restatements of BERN and
GAUSS of test_hipcallbacks_replicate.py traced into `replicate(x, r, g, D)` / `discrepancy(x, r, y, D)`; the argument rules and the
refusals, all before the compiler runs; trace.Noise against oracle/philox.py; the replay of the graphs against the eager functions
on the same Noise, to the bit; the CPU side of the probe; and traced sources without replicate= keep the text they had."""
import os
import shutil
import types

import numpy as np
import pytest
import torch

from oracle import philox
from tests.test_hipcallbacks_replicate import TAG_NORMAL, TAG_UNIFORM, bern_data, bern_rows, gauss_data, gauss_rows

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


# ------------------------------------------------------------------------------------------- the torch functions under trace
def gauss_prior(u):
    return 4.0 * u - 1.0


def gauss_term(x, D):
    z = (D["y"] - (x[:, 0:1] + x[:, 1:2] * D["t"])) / D["s"]
    return -0.5 * z * z


def gauss_replicate(x, D, g):
    """GAUSS_REP of test_hipcallbacks_replicate.py, operation by operation."""
    return (x[:, 0:1] + x[:, 1:2] * D["t"]) + D["s"] * g.normal(0)


def gauss_discrepancy(x, y, D):
    z = (y - (x[:, 0:1] + x[:, 1:2] * D["t"])) / D["s"]
    return z * z


def bern_prior(u):
    return u.clone()


def bern_like(x, D):
    return 0.0 * x[:, 0]


def bern_replicate(x, D, g):
    """BERN of test_hipcallbacks_replicate.py: a Bernoulli through compare and where."""
    p = 0.25 + 0.5 * x[:, 0:1] * D["t"]
    return torch.where(g.uniform(0) < p, torch.ones_like(p), torch.zeros_like(p))


def bern_discrepancy(x, y, D):
    p = 0.25 + 0.5 * x[:, 0:1] * D["t"]
    d = y - p
    return d * d


def traced_gauss(tp, D, **kw):
    return tp.trace_callbacks(gauss_prior, gauss_term, 2, data=D, n_terms="t", replicate=gauss_replicate, n_replicate="t",
                              observed="y", discrepancy=gauss_discrepancy, **kw)


def traced_bern(tp, D, n_dim=3, **kw):
    return tp.trace_callbacks(bern_prior, bern_like, n_dim, data=D, replicate=bern_replicate, n_replicate="t", observed="y",
                              discrepancy=bern_discrepancy, **kw)


def spec_of(D):
    from tempest_amd.hipcallbacks import _table_spec
    tables, host = _table_spec(D)
    return (tables, {k: (host[k].shape, True) for k, _ in tables}), host


def graphs_of(rep, disc, n_dim, D):
    from tempest_amd import trace as T
    spec, _ = spec_of(D)
    extent = (len(D["t"]), "n_replicate")
    return (T.trace_function(rep, n_dim, None, "replicate", spec, extent, noise=True),
            T.trace_function(disc, n_dim, None, "discrepancy", spec, extent, yarg=True))


def tensors(D):
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)) for k, v in D.items()}


# ----------------------------------------------------------------------------------------------------------------- it builds
@needs_hipcc
def test_the_traced_replicate_and_discrepancy_build_with_the_hand_written_signatures():
    import tempest_amd as tp
    D = gauss_data(37, seed=1)
    cb = traced_gauss(tp, D)
    assert cb.n_replicate == 37 and cb.observed == "y" and cb.has_discrepancy and cb.term and cb.n_terms == 37
    src = cb.source
    assert "__device__ double replicate(const double* x, int64_t r, const tphu_noise& g, const tphu_data& D) {" in src
    assert "__device__ double discrepancy(const double* x, int64_t r, double y, const tphu_data& D) {" in src
    assert src.count("g.normal(0)") == 1 and "g.uniform" not in src and " = y;" in src
    for sym in ("tphu_replicated", "tphu_replicate_layout"):
        assert hasattr(cb.lib, sym)
    rep = cb.trace_report
    assert rep["draws"] == {"replicate": {"normal": [0], "uniform": []}}
    assert rep["reads"]["replicate"] == {"t": ["per-term"], "s": ["per-term"]}
    assert rep["reads"]["discrepancy"] == {"t": ["per-term"], "s": ["per-term"]}            # y arrives as the argument, not from D
    assert set(rep["probe"]) >= {"prior_transform", "log_likelihood", "replicate", "discrepancy"}
    if not torch.cuda.is_available():
        assert "NOT run" in rep["probe"]["against"]
        for name in ("replicate", "discrepancy"):
            assert rep["probe"][name]["max_ulps"] == 0.0 and rep["probe"][name]["nonfinite_agree"]
    b = traced_bern(tp, bern_data(5, seed=5))
    assert b.trace_report["draws"] == {"replicate": {"normal": [], "uniform": [0]}} and b.source.count("g.uniform(0)") == 1
    assert b.n_replicate == 5 and b.has_discrepancy and not b.term


@needs_hipcc
def test_a_replicate_that_never_draws_is_allowed_and_reported():
    import tempest_amd as tp
    D = gauss_data(5, seed=1)
    cb = tp.trace_callbacks(gauss_prior, gauss_term, 2, data=D, n_terms="t", n_replicate="t",
                            replicate=lambda x, D, g: x[:, 0:1] + x[:, 1:2] * D["t"])
    assert cb.trace_report["draws"] == {"replicate": {"normal": [], "uniform": []}} and "g." not in cb.source.replace("& g", "")
    assert cb.n_replicate == 5 and cb.observed is None and not cb.has_discrepancy
    assert "discrepancy" not in cb.trace_report["probe"] and "replicate" in cb.trace_report["probe"]


# ------------------------------------------------------------------------------------------------ rules and refusals
def test_argument_rules_raise_before_the_compiler_runs(monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    D = gauss_data(5, seed=1)
    base = dict(data=D, n_terms="t")
    for kw, match in (
            (dict(replicate=gauss_replicate, n_replicate=5), "replicate= without data="),
            (dict(base, replicate=gauss_replicate), "replicate= needs n_replicate="),
            (dict(base, n_replicate="t"), "n_replicate= goes with replicate="),
            (dict(base, discrepancy=gauss_discrepancy, observed="y"), "discrepancy= goes with replicate="),
            (dict(base, replicate=gauss_replicate, n_replicate="t", discrepancy=gauss_discrepancy), "discrepancy= needs observed="),
            (dict(base, observed="y"), "observed= goes with replicate="),
            (dict(base, replicate=gauss_replicate, n_replicate="nope"), "n_replicate='nope' names no data entry"),
            (dict(base, replicate=gauss_replicate, n_replicate=0), "n_replicate must be a positive int"),
            (dict(base, replicate=gauss_replicate, n_replicate=True), "n_replicate must be a positive int"),
            (dict(base, replicate=gauss_replicate, n_replicate="t", observed="nope"), "observed='nope' names no data entry")):
        like = gauss_term if "n_terms" in kw else (lambda x: x.sum(dim=1))
        with pytest.raises(ValueError, match=match):
            tp.trace_callbacks(gauss_prior, like, 2, **kw)


def _k_float(x, D, g):
    return x[:, 0:1] + D["s"] * g.normal(0.0)


def _k_negative(x, D, g):
    return x[:, 0:1] + D["s"] * g.uniform(-1)


def _k_bool(x, D, g):
    return x[:, 0:1] + D["s"] * g.normal(True)


def _k_large(x, D, g):
    return x[:, 0:1] + D["s"] * g.normal(2 ** 31)


def _k_traced(x, D, g):
    return x[:, 0:1] + D["s"] * g.normal(x[:, 0])


def _sum_r(x, D, g):
    return (x[:, 0:1] + D["s"] * g.normal(0)).sum(dim=-1, keepdim=True) + 0.0 * D["t"]


def _cumsum_r(x, D, g):
    return torch.cumsum(x[:, 0:1] + D["s"] * g.normal(0), dim=-1)


def _index_r(x, D, g):
    return x[:, 0:1] + g.normal(0)[:, 0:1] * D["s"]


def _no_axis(x, D, g):
    return x[:, 0:1] + x[:, 1:2]


def _extra_axis(x, D, g):
    a = x[:, 0:1] + D["s"] * g.normal(0)
    return torch.stack([a, a], dim=1)


def _bool_result(x, D, g):
    return g.uniform(0) < x[:, 0:1] * D["t"]


def _other_method(x, D, g):
    return x[:, 0:1] + D["s"] * g.poisson(0)


def _disc_sum(x, y, D):
    return ((y - x[:, 0:1]) ** 2).sum(dim=1)


def _disc_index(x, y, D):
    return (y[:, 0:1] - x[:, 0:1]) * D["s"]


def _disc_bool(x, y, D):
    return y > x[:, 0:1]


def _disc_no_axis(x, y, D):
    return x[:, 0:1] * x[:, 1:2]


SUM = r"the library owns the sum over observations"


@pytest.mark.parametrize("rep,disc,names", [
    (_k_float, None, (r"g\.normal\(0\.0\)", "constant", r"g\.normal\(0\), g\.normal\(1\)")),
    (_k_negative, None, (r"g\.uniform\(-1\)", "0 <= k < 2\\^31")),
    (_k_bool, None, (r"g\.normal\(True\)", "Python int")),
    (_k_large, None, (r"g\.normal\(2147483648\)", "0 <= k < 2\\^31")),
    (_k_traced, None, (r"g\.normal\(", "a traced value")),
    (_other_method, None, (r"g\.poisson", r"g\.normal\(k\) and g\.uniform\(k\)", r"torch\.where\(g\.uniform\(k\) < p")),
    (_sum_r, None, ("sum along the term axis", SUM)),
    (_cumsum_r, None, ("cumsum along the term axis", SUM)),
    (_index_r, None, ("at the term axis", SUM)),
    (_no_axis, None, ("replicate returned", r"expected \(n, n_replicate\)", "no term axis of its own", "def _no_axis")),
    (_extra_axis, None, ("replicate returned", r"expected \(n, n_replicate\)", "reduce the other", "def _extra_axis")),
    (_bool_result, None, ("a bool result of replicate", r"torch\.where\(condition, 1\.0, 0\.0\)", "def _bool_result")),
    (gauss_replicate, _disc_sum, ("sum along the term axis", SUM)),
    (gauss_replicate, _disc_index, ("at the term axis", SUM)),
    (gauss_replicate, _disc_bool, ("a bool result of discrepancy", "def _disc_bool")),
    (gauss_replicate, _disc_no_axis, ("discrepancy returned", r"expected \(n, n_replicate\)", "def _disc_no_axis")),
], ids=["k-float", "k-negative", "k-bool", "k-large", "k-traced", "other-method", "sum-r", "cumsum-r", "index-r", "no-axis", "extra-axis",
        "bool", "disc-sum", "disc-index", "disc-bool", "disc-no-axis"])
def test_refusals_name_the_operation_and_the_line_before_the_compiler_runs(rep, disc, names, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    from tempest_amd.trace import TraceError
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    kw = {} if disc is None else {"observed": "y", "discrepancy": disc}
    with pytest.raises(TraceError) as e:
        tp.trace_callbacks(gauss_prior, gauss_term, 2, data=gauss_data(5, seed=1), n_terms="t", replicate=rep, n_replicate="t", **kw)
    import re
    for name in names:
        assert re.search(name, str(e.value)), (name, str(e.value))
    assert os.path.basename(__file__) in str(e.value)                                   # the line to change is named


def test_one_node_per_distinct_draw():
    from tempest_amd import trace as T

    def rep(x, D, g):
        a = g.normal(3) + g.normal(3) * g.uniform(3)
        return x[:, 0:1] * a + D["s"] * g.normal(2) + g.uniform(np.int64(0))
    spec, _ = spec_of(gauss_data(5, seed=1))
    graph = T.trace_function(rep, 2, None, "replicate", spec, (5, "n_replicate"), noise=True)
    draws = sorted(graph.nodes[i] for i in graph.live() if graph.nodes[i][0].startswith("noise_"))
    assert draws == [("noise_normal", 2), ("noise_normal", 3), ("noise_uniform", 0), ("noise_uniform", 3)]
    text = T.emit(graph, "__device__ double replicate(const double* x, int64_t r, const tphu_noise& g, const tphu_data& D)", "x",
                  lambda k, t: f"return {t};")
    assert text.count("g.normal(3)") == 1 and text.count("g.uniform(3)") == 1 and text.count("g.normal(2)") == 1


# ------------------------------------------------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("R", [1, 65])
@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_noise_is_the_oracle_philox_at_the_documented_counters(k, R):
    """item = the row's index, tick = r, draw = k >> 1, lane k & 1; tags 10 / 11.  Uniforms bit-equal; the normals too here, as both
    sides are NumPy (the device's log / cos / sin are its own: rounding only, see the class)."""
    from tempest_amd.trace import Noise
    items = np.array([0, 1, 2 ** 32 - 1], dtype=np.int64)
    for seed in (0, 3, 2 ** 64 - 1, 0x123456789ABCDEF):
        g = Noise(seed, items, R)
        u = philox.uniform_pair(seed, items[:, None], k >> 1, np.arange(R)[None, :], TAG_UNIFORM)[k & 1]
        z = philox.normal_pair(seed, items[:, None], k >> 1, np.arange(R)[None, :], TAG_NORMAL)[k & 1]
        for got, want in ((g.uniform(k), u), (g.normal(k), z)):
            assert got.dtype == torch.float64 and tuple(got.shape) == (3, R)
            np.testing.assert_array_equal(got.numpy().view(np.int64), want.view(np.int64))
        assert g.uniform(k) is g.uniform(k) and g.normal(k) is g.normal(k)                # the same k asked twice
        assert float(g.uniform(k).min()) >= 0.0 and float(g.uniform(k).max()) < 1.0


def test_noise_refuses_what_the_device_cannot_count():
    from tempest_amd.trace import Noise
    for bad in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(n_replicate=0), dict(n_replicate=2 ** 31),
                dict(items=[-1]), dict(items=[2 ** 32]), dict(items=[[0]]), dict(items=[0.5])):
        with pytest.raises(ValueError, match="Noise"):
            Noise(**dict(dict(seed=1, items=[0], n_replicate=2), **bad))
    g = Noise(1, [0], 2)
    for bad in (-1, 2 ** 31, 1.0, True):
        with pytest.raises(ValueError, match="k must be an int"):
            g.normal(bad)
    import tempest_amd as tp
    assert tp.Noise is Noise and "Noise" in tp.__all__


# ------------------------------------------------------------------------------------------------------ replay against eager
@pytest.mark.parametrize("R", [1, 65])
def test_replay_with_noise_is_bit_equal_to_the_eager_functions(R):
    from tempest_amd import trace as T
    n, seed = 33, 9
    for rep, disc, d, (x, _), D in ((gauss_replicate, gauss_discrepancy, 2, gauss_rows(n, seed=R), gauss_data(R, seed=R)),
                                    (bern_replicate, bern_discrepancy, 3, bern_rows(n, 3, seed=R), bern_data(R, seed=R))):
        g_rep, g_disc = graphs_of(rep, disc, d, D)
        items = np.arange(n)
        xt, Dt = torch.from_numpy(x), tensors(D)
        want = rep(xt, Dt, T.Noise(seed, items, R)).numpy()
        got = T.replay(g_rep, x, D, noise=T.Noise(seed, items, R))
        assert got.shape == want.shape == (n, R)
        np.testing.assert_array_equal(got, want)
        if rep is bern_replicate:
            assert set(np.unique(got)) <= {0.0, 1.0}
        for y in (D["y"], got):                                     # the observed row for all, and the replicated matrix
            yt = torch.from_numpy(np.broadcast_to(y, (n, R)).copy())
            np.testing.assert_array_equal(T.replay(g_disc, x, D, y=y), disc(xt, yt, Dt).numpy())
        with pytest.raises(ValueError, match="noise="):
            T.replay(g_rep, x, D)
        with pytest.raises(ValueError, match="y="):
            T.replay(g_disc, x, D)
        with pytest.raises(ValueError, match="shape"):
            T.replay(g_rep, x, D, noise=T.Noise(seed, items[:-1], R))


def test_probe_without_a_device_checks_replicate_and_discrepancy(monkeypatch):
    from tempest_amd import trace as T
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # the CPU side of the probe, on any machine
    D = gauss_data(130, seed=2)
    spec, host = spec_of(D)
    g_rep, g_disc = graphs_of(gauss_replicate, gauss_discrepancy, 2, D)
    graphs = {"prior_transform": T.trace_function(gauss_prior, 2, 2, "prior_transform", spec, pass_data=False),
              "log_likelihood_term": T.trace_function(gauss_term, 2, None, "log_likelihood_term", spec, (130, "n_terms")),
              "replicate": g_rep, "discrepancy": g_disc}
    cb = types.SimpleNamespace(trace_graphs=graphs, n_dim=2, _host=host, tables=spec[0], n_terms=130, n_predict=0, n_replicate=130,
                               observed="y", device=None, source="the text")
    rep = T.probe(cb, gauss_prior, gauss_term, None, None, gauss_replicate, gauss_discrepancy)
    for name in ("replicate", "discrepancy"):
        assert rep[name]["nonfinite_agree"] and rep[name]["max_ulps"] == 0.0, (name, rep[name])

    def hidden_branch(x, D, g):                     # Python control flow on a value the tracer cannot see: one branch was traced
        return gauss_replicate(x, D, g) + (0.0 if isinstance(x, T.TV) else 1e-3)
    with pytest.raises(T.TraceError, match="replicate: differs from the eager function") as e:
        T.probe(cb, gauss_prior, gauss_term, None, None, hidden_branch, gauss_discrepancy)
    assert e.value.source == "the text"
    with pytest.raises(T.TraceError, match="discrepancy: differs from the eager function"):
        T.probe(cb, gauss_prior, gauss_term, None, None, gauss_replicate, lambda x, y, D: gauss_discrepancy(x, y, D) * 1.001)


# ------------------------------------------------------------------------------------- sources without replicate= are as before
@needs_hipcc
def test_traced_sources_without_replicate_emit_the_text_they_had():
    import tempest_amd as tp
    from tempest_amd import trace as T
    D = gauss_data(37, seed=1)
    cb = tp.trace_callbacks(gauss_prior, gauss_term, 2, data=D, n_terms="t", check=False)
    assert cb.source == T.emit_source(cb.trace_graphs, cb.tables) and set(cb.trace_graphs) == {"prior_transform", "log_likelihood_term"}
    for word in ("tphu_noise", "replicate", "discrepancy", "double y"):
        assert word not in cb.source, word
    assert cb.n_replicate == 0 and cb.observed is None and "draws" not in cb.trace_report
    with_rep = traced_gauss(tp, D, check=False)
    assert with_rep.source.startswith(cb.source) and with_rep.path != cb.path             # the two functions are appended, nothing moved

"""tempest_amd.trace_callbacks with observed data, without a GPU: torch term functions of (x, D) traced per term -- the replay of
their graphs against the eager functions on the CPU, the refusals, the emitted sources through hipcc and the HipCallbacks
constructor, and the report.  The hand-written sources and NumPy restatements are those of test_hipcallbacks_data.py."""
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

from tests.test_hipcallbacks_data import REG, layered_sum, particles, pois_data, reference_loglike, reg_data, reg_terms

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

EPS = float(np.finfo(np.float64).eps)
N_ROWS = 33
N_TERMS = (1, 5, 257)


# ------------------------------------------------------------------------------------------- the torch functions under trace
def prior(u):
    return 10.0 * u - 5.0


def reg_term(x, D):
    """REG of test_hipcallbacks_data.py, operation by operation."""
    m = x[:, 0:1] + x[:, 1:2] * D["t"] + x[:, 2:3] * D["t"] * D["t"]
    z = (D["y"] - m) / D["s"]
    return -0.5 * z * z - D["c"]


def pois_term(x, D):
    """POIS of test_hipcallbacks_data.py."""
    lam = torch.exp(0.1 * x[:, 0:1] + 0.1 * x[:, 1:2] * D["t"]) + (x[:, 2:3] + 6.0)
    return D["k"] * torch.log(lam) - lam - D["c"]


def quad_term(x, D):
    """QUAD of test_hipcallbacks_predict.py (the README's example)."""
    m = x[:, 0:1] + x[:, 1:2] * D["t"] + x[:, 2:3] * D["t"] * D["t"]
    z = (D["y"] - m) / D["s"]
    return -0.5 * z * z


def quad_model(x, D):
    return x[:, 0:1] + x[:, 1:2] * D["t"] + x[:, 2:3] * D["t"] * D["t"]


def design_term(k):
    def term(x, D):
        z = (D["y"] - x[:, :k] @ D["X"].T) / D["s"]
        return -0.5 * z * z
    return term


def design_term_linear(x, D):
    z = (D["y"] - torch.nn.functional.linear(x, D["X"])) / D["s"]
    return -0.5 * z * z


LOG_W = torch.tensor([[math.log(0.3)], [math.log(0.7)]], dtype=torch.float64)


def mixture_term(x, D):
    """Two Gaussian components with means x0, x1 and a common width |x2| + 0.5: (n, 2, 1) against (T,) gives (n, 2, T)."""
    mu = x[:, 0:2].unsqueeze(-1)
    z = (D["y"][None, :] - mu) / (torch.abs(x[:, 2:3]) + 0.5).unsqueeze(-1)
    return torch.logsumexp(-0.5 * z * z + LOG_W.to(x.device), dim=1)


def hyper_term(x, D):
    z = (D["y"] - x[:, 0:1] * D["h"][0] - x[:, 1:2] * D["X"][0, 1]) / D["h"][2]
    return -0.5 * z * z - D["h"][-2] * x[:, 2:3] * D["X"][:, 1]


def data_of(n_terms, seed=5):
    rng = np.random.RandomState(seed + n_terms)
    D = reg_data(n_terms)
    D["X"] = rng.uniform(-1.0, 1.0, size=(n_terms, 3))
    D["h"] = np.array([1.25, -0.75, 2.5])
    return D


def spec_of(D):
    from tempest_amd.hipcallbacks import _table_spec
    tables, host = _table_spec(D)
    return (tables, {k: (host[k].shape, np.asarray(D[k]).dtype == np.float64) for k, _ in tables})


def trace_term(fn, D, n_terms=None, name="log_likelihood_term"):
    from tempest_amd import trace as T
    return T.trace_function(fn, 3, None, name, spec_of(D), (len(D["t"]) if n_terms is None else n_terms, "n_terms"))


def tensors(D):
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)) for k, v in D.items()}


# ------------------------------------------------------------------------------------------------------ replay against eager
@pytest.mark.parametrize("n_terms", N_TERMS)
@pytest.mark.parametrize("fn", [reg_term, pois_term, quad_term, quad_model, mixture_term, hyper_term],
                         ids=["reg", "pois", "quad", "quad_model", "mixture", "hyper"])
def test_replay_is_bit_equal_to_the_eager_term_function_on_the_cpu(fn, n_terms):
    from tempest_amd import trace as T
    D = dict(data_of(n_terms), **(pois_data(n_terms) if fn is pois_term else {}))
    x = particles(N_ROWS, seed=n_terms)
    got = T.replay(trace_term(fn, D), x, D)
    want = fn(torch.from_numpy(x), tensors(D)).numpy()
    assert got.shape == want.shape == (N_ROWS, n_terms)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("n_terms", N_TERMS)
def test_replayed_reg_terms_sum_to_the_reference_loglike(n_terms):
    from tempest_amd import trace as T
    from tempest_amd.hipcallbacks import SUM_LAYOUT
    D = reg_data(n_terms)
    x = particles(N_ROWS, seed=3)
    terms = T.replay(trace_term(reg_term, D), x, D)
    np.testing.assert_array_equal(terms, reg_terms(x, D))
    want = reference_loglike(x, D, reg_terms, SUM_LAYOUT)
    np.testing.assert_array_equal(layered_sum(terms, *SUM_LAYOUT), want)
    np.testing.assert_array_equal(T.layered_sum(terms, *SUM_LAYOUT), want)               # the probe's restatement of the same rule


@pytest.mark.parametrize("n_terms", N_TERMS)
@pytest.mark.parametrize("k", [1, 3])
def test_design_matrix_is_within_the_summation_bound_of_eager_and_in_column_order(k, n_terms):
    """x[:, :k] @ D["X"].T: bit-equal to the column-order NumPy form (every product and sum rounded, left to right); against eager,
    whose BLAS fuses and reorders, the bound of test_matmul_with_any_constant_is_within_one_fused_rounding_of_eager: 2 (k - 1) eps
    sum|products|, carried through the division by s and the square (k = 1: no sum, equality)."""
    from tempest_amd import trace as T
    D = data_of(n_terms)
    D["X"] = np.ascontiguousarray(D["X"][:, :k])
    x = particles(N_ROWS, seed=n_terms + k)
    got = T.replay(trace_term(design_term(k), D), x, D)
    X = D["X"]
    inner = x[:, 0:1] * X[None, :, 0]
    for j in range(1, k):
        inner = inner + x[:, j:j + 1] * X[None, :, j]
    z = (D["y"][None, :] - inner) / D["s"][None, :]
    np.testing.assert_array_equal(got, (-0.5 * z) * z)
    if k == 3:
        np.testing.assert_array_equal(T.replay(trace_term(design_term_linear, D), x, D), got)       # F.linear: the same graph
    eager = design_term(k)(torch.from_numpy(x), tensors(D)).numpy()
    if k == 1:
        np.testing.assert_array_equal(got, eager)
        return
    d_inner = 2 * (k - 1) * EPS * (np.abs(x[:, :k]) @ np.abs(X).T)
    # -z^2 / 2 with z = (y - inner) / s: |d term| <= |z| |dz| + dz^2 / 2, |dz| <= d_inner / s (1 + a few eps for the later roundings)
    dz = d_inner / D["s"][None, :] * (1 + 8 * EPS) + 4 * EPS * np.abs(z)
    assert np.all(np.abs(got - eager) <= np.abs(z) * dz + 0.5 * dz * dz + 4 * EPS * np.abs(got))


def test_data_values_alone_stay_data_values_and_every_elementwise_operation_applies():
    from tempest_amd import trace as T

    def term(x, D):
        w = torch.log(D["s"]) + (D["y"] - D["t"]).unsqueeze(0)                      # data alone
        a = torch.where(D["t"] > 0.0, x[:, 0:1], x[:, 1:2] * D["X"][:, 0])
        b = torch.clamp(x[:, 2:3] * D["t"], -0.5, 0.5) ** 2 + torch.maximum(D["y"], x[:, 0:1])
        return torch.stack([a, b], dim=1).sum(dim=1) - w
    for n_terms in N_TERMS:
        D = data_of(n_terms)
        x = particles(N_ROWS)
        g = trace_term(term, D)
        np.testing.assert_array_equal(T.replay(g, x, D), term(torch.from_numpy(x), tensors(D)).numpy())
        assert g.reads == {"s": {"per-term"}, "y": {"per-term"}, "t": {"per-term"}, "X": {"column 0"}}


def test_shape_shows_the_term_axis_as_a_name():
    seen = {}

    def term(x, D):
        seen["t"], seen["X"], seen["h"] = D["t"].shape, D["X"].shape, D["h"].shape
        y = x[:, 0:1] * D["t"]
        seen["y"], seen["k"] = y.shape, (x[:, 0:2].unsqueeze(-1) * D["t"]).shape
        return y
    trace_term(term, data_of(5))
    assert [repr(v) for v in seen["y"]] == ["n", "n_terms"] and [repr(v) for v in seen["k"]] == ["n", "2", "n_terms"]
    assert repr(seen["t"][0]) == "n_terms" and seen["X"][1] == 3 and repr(seen["X"][0]) == "n_terms" and seen["h"] == (3,)


# ----------------------------------------------------------------------------------------------------------------- refusals
def _mask(x, D):
    y = x[:, 0:1] * D["t"]
    return y[:, [True, False, True, False, True]]


def _arange(x, D):
    return x[:, 0:1] * torch.arange(D["t"].shape[0])


def _range(x, D):
    return sum(x[:, 0:1] * D["t"][i] for i in range(len(D["t"])))


def _arange_constant(x, D):
    return x[:, 0:1] * D["t"] + torch.arange(5, dtype=torch.float64)


SUM = r"the library owns the sum over observations(.|\n)*return the \(n, n_terms\) terms"


@pytest.mark.parametrize("fn,names", [
    (lambda x, D: (x[:, 0:1] * D["t"]).sum(dim=1), r"sum along the term axis(.|\n)*" + SUM),
    (lambda x, D: (x[:, 0:1] * D["t"]).sum(dim=-1, keepdim=True) + D["y"], r"sum along the term axis(.|\n)*" + SUM),
    (lambda x, D: torch.logsumexp(x[:, 0:2].unsqueeze(-1) * D["t"], dim=2), r"logsumexp along the term axis(.|\n)*" + SUM),
    (lambda x, D: D["y"].sum() + x[:, 0:1] * D["t"], r"sum of a data value(.|\n)*" + SUM),
    (lambda x, D: torch.cumsum(x[:, 0:1] * D["t"], dim=1), r"cumsum along the term axis(.|\n)*" + SUM),
    (lambda x, D: (x[:, 0:1] * D["t"])[:, 0:1] + D["y"], r"an index, slice, mask or new axis at the term axis(.|\n)*" + SUM),
    (lambda x, D: (x[:, 0:1] * D["t"])[..., 0].unsqueeze(-1) + D["y"], r"at the term axis(.|\n)*" + SUM),
    (_mask, r"at the term axis(.|\n)*" + SUM),
    (lambda x, D: x[:, 0:1] * D["t"][1:], r"D\['t'\]\[.*\]: an index, slice or mask along the observations(.|\n)*" + SUM),
    (lambda x, D: x[:, 0:1] * D["X"][0:2, 1], r"along the observations(.|\n)*" + SUM),
    (lambda x, D: x[:, 0:1] * D["h"] + D["t"], r"D\['h'\], a 1-D entry of length 3, used whole(.|\n)*index it: D\['h'\]\[j\]"),
    (lambda x, D: x[:, 0:1] * D["X"] + D["t"], r"D\['X'\], a 2-D entry, used whole(.|\n)*D\['X'\]\[:, j\]"),
    (_arange, r"the extent of the term axis(.|\n)*put it into a data entry"),
    (_range, r"the extent of the term axis(.|\n)*put it into a data entry"),
    (_arange_constant, r"a captured array of shape \(5,\) against a value with a term axis(.|\n)*put it into a data entry"),
    (lambda x, D: x[:, 0:1] * D["t"] + D["h"][x[:, 0]], r"with a traced index(.|\n)*a traced index into a table"),
    (lambda x, D: x * D["t"], r"broadcasting \(n,3\) against a term axis"),
    (lambda x, D: x[:, 0] * D["t"], r"broadcasting \(n,\) against a term axis"),
    (lambda x, D: x[:, 0:1] * D["h"][3] + D["t"], r"D\['h'\]\[\.\.\.\] with index 3(.|\n)*extent 3"),
    (lambda x, D: x[:, 0:1] * D["X"][5, 0] + D["t"], r"D\['X'\]\[\.\.\.\] with index 5(.|\n)*extent 5"),
    (lambda x, D: x @ D["X"], r"x @ D\[name\](.|\n)*x @ D\[name\]\.T"),
    (lambda x, D: x[:, 0:1] * D["ki"], r"D\['ki'\], given as an integer or float32 array, in arithmetic(.|\n)*float64"),
    (lambda x, D: x[:, 0:1] * D["kf"][0] + D["t"], r"D\['kf'\], given as an integer or float32 array"),
    (lambda x, D: x[:, 0:1] * D["nope"], r"D\['nope'\](.|\n)*no such data entry"),
], ids=["sum", "sum_keepdim", "logsumexp_terms", "sum_of_data", "cumsum", "slice", "ellipsis_index", "mask", "entry_slice", "row_slice",
        "other_length_whole", "matrix_whole", "arange", "range_len", "arange_constant", "traced_index", "n3_against_T", "n_against_T",
        "element_out_of_range", "row_out_of_range", "untransposed", "integer_entry", "float32_entry", "unknown_entry"])
def test_refusals_name_the_operation(fn, names):
    from tempest_amd.trace import TraceError
    D = data_of(5)
    D["ki"] = np.arange(5)
    D["kf"] = np.ones(5, dtype=np.float32)
    with pytest.raises(TraceError, match=names) as e:
        trace_term(fn, D)
    assert "instead:" in str(e.value) and "test_trace_data.py" in str(e.value)      # what to do, and the user's line


def test_a_cast_entry_is_traced():
    from tempest_amd import trace as T
    D = data_of(5)
    D["ki"] = np.arange(5)
    g = trace_term(lambda x, D: x[:, 0:1] * D["ki"].double() + D["ki"].to(torch.float64)[2], D)
    x = particles(N_ROWS)
    np.testing.assert_array_equal(T.replay(g, x, D), x[:, 0:1] * np.arange(5.0)[None, :] + 2.0)


def test_results_with_and_without_a_term_axis_are_held_to_their_place():
    from tempest_amd import trace as T
    D = data_of(5)
    with pytest.raises(T.TraceError, match=r"log_likelihood_term returned \('?n'?,\)(.|\n)*no term axis"):
        trace_term(lambda x, D: x[:, 0] * D["h"][0], D)
    with pytest.raises(T.TraceError, match=r"returned \(n, 2, n_terms\), expected \(n, n_terms\)"):
        trace_term(lambda x, D: x[:, 0:2].unsqueeze(-1) * D["t"], D)
    with pytest.raises(T.TraceError, match="returned a data value"):
        trace_term(lambda x, D: D["t"] * 2.0, D)
    # prior_transform, derived and a whole log_likelihood have no term axis: a per-observation value cannot arise in them
    for name, width in (("prior_transform", 3), ("derived", None), ("log_likelihood", ())):
        with pytest.raises(T.TraceError, match=r"D\['t'\], a 1-D entry of length 5, used whole(.|\n)*has no term axis(.|\n)*index it"):
            T.trace_function(lambda x, D: x[:, 0:1] * D["t"], 3, width, name, spec_of(D))
        with pytest.raises(T.TraceError, match=r"D\['X'\]\[:, j\](.|\n)*has no term axis"):
            T.trace_function(lambda x, D: x[:, 0:1] * D["X"][:, 0], 3, width, name, spec_of(D))


def test_the_old_refusals_keep_their_words():
    from tempest_amd import trace as T
    with pytest.raises(T.TraceError, match=r"an intermediate of 65 columns(.|\n)*data="):
        T.trace_function(lambda x: torch.cat([x] * 13, dim=1).sum(dim=1), 5, ())
    with pytest.raises(T.TraceError, match=r"more than 4096 embedded constants(.|\n)*data=(.|\n)*trace_callbacks"):
        T.trace_function(lambda x: (x @ torch.arange(4100, dtype=torch.float64).reshape(5, 820))[:, 0], 5, ())
    with pytest.raises(T.TraceError, match=r"sum\(\) over all axes"):
        T.trace_function(lambda x: x.sum(), 5, ())


def test_argument_rules(monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    D = reg_data(5)
    like = lambda x: x.sum(dim=1)                                                             # noqa: E731
    with pytest.raises(ValueError, match="n_terms=.*data="):
        tp.trace_callbacks(prior, reg_term, 3, n_terms=5)
    with pytest.raises(ValueError, match="names no data entry"):
        tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms="nope")
    with pytest.raises(ValueError, match="n_terms=4 is the length"):
        tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms=4)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_terms must be a positive int"):
            tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms=bad)
    with pytest.raises(ValueError, match="predict= without data="):
        tp.trace_callbacks(prior, like, 3, predict=lambda x: x, n_predict=3)
    with pytest.raises(ValueError, match="predict= needs n_predict="):
        tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms="t", predict=quad_model)
    with pytest.raises(ValueError, match="n_predict= goes with predict="):
        tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms="t", n_predict="t")
    with pytest.raises(ValueError, match="pointwise=True goes with n_terms="):
        tp.trace_callbacks(prior, like, 3, data=D, pointwise=True)
    with pytest.raises(ValueError, match="n_derived="):
        tp.trace_callbacks(prior, like, 3, n_derived=2)


# ----------------------------------------------------------------------------------------------------------------- emission
def no_data_literal(source, own):
    """Every literal of the text is one of the functions' own constants: no data value was copied into it."""
    lits = set(re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", source))
    assert lits == {float.hex(v) for v in own}, lits


@needs_hipcc
def test_term_form_compiles_and_reads_the_tables():
    import tempest_amd as tp
    D = data_of(257)
    cb = tp.trace_callbacks(prior, hyper_term, 3, data=D, n_terms="t")
    src = cb.source
    assert cb.term and cb.n_terms == 257 and cb.tables == (("t", 1), ("y", 1), ("s", 1), ("c", 1), ("X", 2), ("h", 1))
    assert "__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {" in src
    assert "__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {" in src
    assert not re.search(r"\blog_likelihood\s*\(", src) and "predict" not in src and "derived" not in src.split("\n", 1)[1]
    for read in ("D.y[r]", "D.X[r * D.X_cols + 1]", "D.h[2]", "D.h[0]", "D.h[1]", "D.X[0 * D.X_cols + 1]"):
        assert read in src, read
    assert "D.t[r]" not in src                                                     # hyper_term does not read t
    assert "D.t[r]" in tp.trace_callbacks(prior, reg_term, 3, data=D, n_terms="t", check=False).source
    no_data_literal(src, (10.0, 5.0, -0.5))
    rep = cb.trace_report
    assert rep["reads"]["log_likelihood_term"] == {"y": ["per-term"], "h": ["element [0]", "element [1]", "element [2]"],
                                                   "X": ["column 1", "element [0, 1]"]}
    assert rep["reads"]["prior_transform"] == {}
    assert rep["probe"]["rows"] == 4096
    if not torch.cuda.is_available():
        assert rep["probe"]["against"].startswith("replay on the CPU") and "NOT run" in rep["probe"]["against"]
        assert rep["probe"]["log_likelihood"]["max_ulps"] == 0.0 and rep["probe"]["eager_on"]["log_likelihood"] == "cpu"


@needs_hipcc
def test_two_data_sets_of_the_same_names_and_ranks_share_the_plugin():
    import tempest_amd as tp
    a = tp.trace_callbacks(prior, reg_term, 3, data=reg_data(100), n_terms="t")
    b = tp.trace_callbacks(prior, reg_term, 3, data=reg_data(777, seed=3), n_terms=777)
    assert a.source == b.source and a.path == b.path
    assert a.trace_report["probe"]["rows"] == 4096 and b.trace_report["probe"]["rows"] == 4096
    hand = tp.HipCallbacks(REG, 3, data=reg_data(100), n_terms="t")
    assert hand.path != a.path                                                     # the hand-written text keeps its own file


@needs_hipcc
def test_term_predict_and_pointwise_compile_together():
    import tempest_amd as tp
    D = {k: v for k, v in reg_data(257).items() if k != "c"}
    cb = tp.trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", predict=quad_model, n_predict="t", pointwise=True)
    src = cb.source
    assert cb.n_predict == 257 and cb.pointwise_enabled and cb.term
    assert len(re.findall(r"\bdouble\s+predict\s*\(", src)) == 1 and not re.search(r"\blog_likelihood\s*\(", src)
    assert "__device__ double predict(const double* x, int64_t r, const tphu_data& D) {" in src
    for sym in ("tphu_predictive", "tphu_pointwise", "tphu_like_split"):
        assert hasattr(cb.lib, sym)
    no_data_literal(src, (10.0, 5.0, -0.5))
    assert cb.trace_report["reads"]["predict"] == {"t": ["per-term"]}
    assert set(cb.trace_report["probe"]) >= {"prior_transform", "log_likelihood", "predict"}


def whole_like(x, D):
    z = (x[:, 0] - D["h"][0]) / D["h"][2]
    return -0.5 * z * z - (x[:, 1] * D["X"][1, 2]) ** 2 - x[:, 2] ** 2


def prior_with_data(u, D):
    return D["h"][2] * u - D["h"][0]


def derived_with_data(x, D):
    return torch.stack([x[:, 0] * D["h"][1], x.sum(dim=1)], dim=1)


@needs_hipcc
def test_whole_likelihood_prior_and_derived_read_elements():
    import tempest_amd as tp
    D = {"h": np.array([1.25, -0.75, 2.5]), "X": np.arange(6.0).reshape(2, 3) + 0.5}
    cb = tp.trace_callbacks(prior_with_data, whole_like, 3, derived=derived_with_data, data=D)
    src = cb.source
    assert not cb.term and cb.n_derived == 2
    for sig in ("__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {",
                "__device__ double log_likelihood(const double* x, const tphu_data& D) {",
                "__device__ void derived(const double* x, double* out, const tphu_data& D) {"):
        assert sig in src, sig
    assert "D.h[2]" in src and "D.X[1 * D.X_cols + 2]" in src and "[r" not in src
    no_data_literal(src, (-0.5,))
    assert cb.trace_report["reads"] == {"prior_transform": {"h": ["element [0]", "element [2]"]},
                                        "log_likelihood": {"h": ["element [0]", "element [2]"], "X": ["element [1, 2]"]},
                                        "derived": {"h": ["element [1]"]}}
    assert set(cb.trace_report["probe"]) >= {"prior_transform", "log_likelihood", "derived"}
    plain = tp.trace_callbacks(prior, whole_like, 3, derived=lambda x: x[:, 0], data=D, check=False)      # one parameter: no D handed over
    assert plain.trace_report["reads"]["prior_transform"] == {} and "const tphu_data& D" in plain.source


def test_probe_without_a_device_holds_the_replay_against_eager(monkeypatch):
    """The probe's CPU side needs no compiler: the summed replayed terms against the eager terms summed in SUM_LAYOUT order, predict
    against its replay, in row chunks; a trace of another function is refused."""
    import types
    from tempest_amd import trace as T
    from tempest_amd.hipcallbacks import _table_spec
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # the CPU side of the probe, on any machine
    D = {k: v for k, v in reg_data(5000).items() if k != "c"}
    tables, host = _table_spec(D)
    spec = (tables, {k: (host[k].shape, True) for k in host})
    graphs = {"prior_transform": T.trace_function(prior, 3, 3, "prior_transform", spec, pass_data=False),
              "log_likelihood_term": T.trace_function(quad_term, 3, None, "log_likelihood_term", spec, (5000, "n_terms")),
              "predict": T.trace_function(quad_model, 3, None, "predict", spec, (5000, "n_predict"))}
    cb = types.SimpleNamespace(trace_graphs=graphs, n_dim=3, _host=host, tables=tables, n_terms=5000, n_predict=5000, device=None,
                               source="")
    rep = T.probe(cb, prior, quad_term, None, quad_model)
    assert rep["rows"] == 2 ** 22 // 5000 and "NOT run" in rep["against"]
    for name in ("prior_transform", "log_likelihood", "predict"):
        assert rep[name]["nonfinite_agree"] and rep[name]["max_ulps"] == 0.0, (name, rep[name])
    with pytest.raises(T.TraceError, match="log_likelihood: differs from the eager function"):
        T.probe(cb, prior, lambda x, D: quad_term(x, D) + 1e-3, None, quad_model)
    with pytest.raises(T.TraceError, match="predict: differs from the eager function"):
        T.probe(cb, prior, quad_term, None, lambda x, D: quad_model(x, D) * 1.001)

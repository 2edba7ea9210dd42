"""The tracer decides which plugin is built: the emitted text is what the cache key hashes.  CPU only, no compiler: the corpus of
oracle/make_trace_texts.py gives the texts, graphs, replay values, reports, refusals and keyword errors recorded in
tests/golden/trace_texts.json (written by that script on the commit before the tracer became a package with one table of operations,
one registration of torch names and one table of callback kinds), and the tables agree with themselves."""
import json

import numpy as np
import pytest

from oracle import make_trace_texts as M


@pytest.fixture(scope="module")
def recorded():
    """(the record of the code as it stands, the golden record); the replay hashes, which depend on the host's vector libraries
    (oracle.make_trace_texts.merged), are taken out of both and compared by the test below."""
    rec, gold = json.loads(json.dumps(M.record())), json.load(open(M.GOLDEN))
    return rec, gold, M.replays(rec, dict.fromkeys(M.replays(rec))), M.replays(gold, dict.fromkeys(M.replays(gold)))


def test_every_replay_reproduces_a_recorded_one_to_the_bit(recorded):
    mine, theirs = recorded[2], recorded[3]
    assert set(mine) == set(theirs) and all(1 <= len(h) <= 2 for h in theirs.values())
    assert {k: (h, theirs[k]) for k, h in mine.items() if h not in theirs[k]} == {}
    exact = {k for k, h in theirs.items() if len(h) == 1}               # graphs of exact operations: one hash on every host
    assert {("bools", "log_likelihood"), ("shapes", "derived"), ("products", "log_likelihood"), ("elements", "log_likelihood")} <= exact


@pytest.mark.parametrize("part", ["cases", "refusals", "keywords", "torch_names", "tv_attributes", "tv_dunders", "prior_hip_source",
                                  "trace_loaded_by_sampler"])
def test_the_tracer_reproduces_the_record(recorded, part):
    rec, gold = recorded[:2]
    assert set(rec) == set(gold)
    if isinstance(gold[part], dict):
        assert set(rec[part]) == set(gold[part])
        assert {k: (rec[part][k], v) for k, v in gold[part].items() if rec[part][k] != v} == {}
    else:
        assert rec[part] == gold[part]


def test_the_record_holds_cases_refusals_and_keyword_errors_without_paths(recorded):
    gold = recorded[1]
    assert len(gold["cases"]) >= 16 and len(gold["refusals"]) >= 30 and len(gold["keywords"]) >= 12
    assert gold["trace_loaded_by_sampler"] is False
    assert all("/" not in m.split("\n  at ")[1].split(": ")[0] for m in gold["refusals"].values() if "\n  at " in m)


def test_every_operation_has_an_emit_form_and_a_replay_form():
    """One table: what `emit` writes, what `replay` computes, whether the result is a bool, whether the node is a leaf."""
    from tempest_amd import trace as T
    assert set(T.OPS) == set(M.ALL_OPS)
    for name, op in T.OPS.items():
        assert isinstance(op.c, str) and op.c and callable(op.host), name
        assert isinstance(op.is_bool, bool) and isinstance(op.leaf, bool) and not (op.leaf and op.is_bool), name
    g = T.Graph(2, tables=(("t", 1), ("m", 2)), n_term=3)
    a, b = g.add("in", 1), g.const(0.75)
    ids = {"in": a, "const": b, "dterm": g.add("dterm", 1, 0), "delem": g.add("delem", 0, 2, -1), "yarg": g.add("yarg"),
           "noise_normal": g.add("noise_normal", 4), "noise_uniform": g.add("noise_uniform", 5)}
    assert set(ids) == {k for k, op in T.OPS.items() if op.leaf}
    for name, op in T.OPS.items():
        if not op.leaf:
            first = g.add("gt", a, b) if name in ("and", "or", "not", "where") else a
            second = g.add("lt", a, b) if name in ("and", "or") else b
            ids[name] = g.add(name, *(first, second, a)[:op.c.count("{")])
    data = {"t": np.arange(3.0), "m": np.arange(6.0).reshape(3, 2)}
    for name, i in ids.items():                                     # every operation alone: emitted and replayed
        g.outputs = (i,) if not T.OPS[name].is_bool else (g.add("where", i, a, b),)
        text = T.emit(g, "__device__ double f(const double* x, int64_t r, double y, const tphu_noise& g, const tphu_data& D)", "x",
                      lambda k, t: f"return {t};")
        assert f"t{i} = " in text and "{" not in text.split("{", 1)[1], (name, text)
        out = T.replay(g, np.full((4, 2), 0.5), data, noise=T.Noise(1, np.arange(4), 3), y=np.ones(3))
        assert out.shape == (4, 3), name


def test_the_callback_table_is_the_order_of_emission():
    from tempest_amd import trace as T
    assert list(T.CALLBACKS) == ["prior_transform", "log_likelihood_term", "log_likelihood", "predict", "derived", "replicate",
                                 "discrepancy"]
    g = T.trace_function(lambda u: 2.0 * u, 2, 2, "prior_transform")
    text = T.emit_function(g, "prior_transform")
    assert text.startswith("__device__ void prior_transform(const double* u, double* x) {") and "x[1] = " in text
    assert T.emit_function(g, "prior_transform", (("t", 1),)).startswith(
        "__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {")

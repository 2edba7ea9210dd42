"""The host layer of HipCallbacks decides which plugin is built: the translation unit, the -D list and the cache key.  CPU only, no
compiler: every valid combination of a plugin's optional parts generates the text and the key recorded in
tests/golden/plugin_texts.json (oracle/make_plugin_texts.py, run on the commit before the parts became one record), and the
constructor hands build_plugin exactly the combination its arguments imply."""
import inspect
import json

import numpy as np
import pytest

from oracle import make_plugin_texts as M

PRIOR = "__device__ void prior_transform(const double* u, double* x) { for (int j = 0; j < N_DIM; ++j) x[j] = u[j]; }\n"
LIKE = "__device__ double log_likelihood(const double* x) { return -x[0] * x[0]; }\n"
LIKE_D = "__device__ double log_likelihood(const double* x, const tphu_data& D) { return -x[0] * D.t[0]; }\n"
TERM = "__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) { return -x[0] * x[0]; }\n"
DERIVED = "__device__ void derived(const double* x, double* out, const tphu_data& D) { out[0] = x[0]; out[1] = x[1]; }\n"
PREDICT = "__device__ double predict(const double* x, int64_t r, const tphu_data& D) { return x[0] * D.t[r]; }\n"
REPLICATE = "__device__ double replicate(const double* x, int64_t r, const tphu_noise& g, const tphu_data& D) { return x[0] + g.normal(0); }\n"
DISCREPANCY = "__device__ double discrepancy(const double* x, int64_t r, double y, const tphu_data& D) { return (y - x[0]) * (y - x[0]); }\n"
TRACED = "__device__ double widest(const double* x) { return tphu_tr_min(x[0], x[1]); }\n"
T4 = {"t": np.arange(4.0), "y": np.ones(4)}
T4M = {"t": np.arange(4.0), "y": np.ones(4), "m": np.ones((4, 2))}
SPEC4 = (("t", 1), ("y", 1))

PLAIN = dict(tables=None, term=False, n_derived=0, predict=False, pointwise=False, replicate=False, discrepancy=False)
CONSTRUCTIONS = {
    "plain": (PRIOR + LIKE, {}, {}),
    "data": (PRIOR + LIKE_D, {"data": T4}, {"tables": SPEC4}),
    "term_without_data": (PRIOR + TERM, {"n_terms": 5}, {"tables": (), "term": True}),
    "term_pointwise": (PRIOR + TERM, {"data": T4, "n_terms": "t", "pointwise": True}, {"tables": SPEC4, "term": True, "pointwise": True}),
    "derived": (PRIOR + LIKE + DERIVED, {"n_derived": 2}, {"n_derived": 2}),
    "predict": (PRIOR + LIKE_D + PREDICT, {"data": T4, "n_predict": "t"}, {"tables": SPEC4, "predict": True}),
    "predict_int": (PRIOR + LIKE + PREDICT, {"n_predict": 7}, {"predict": True}),
    "replicate": (PRIOR + LIKE_D + REPLICATE, {"data": T4, "n_replicate": 4, "observed": "y"}, {"tables": SPEC4, "replicate": True}),
    "replicate_discrepancy": (PRIOR + LIKE_D + REPLICATE + DISCREPANCY, {"data": T4, "n_replicate": "t", "observed": "y"},
                              {"tables": SPEC4, "replicate": True, "discrepancy": True}),
    "everything": (PRIOR + TERM + DERIVED + PREDICT + REPLICATE + DISCREPANCY + TRACED,
                   {"data": T4M, "n_terms": "t", "pointwise": True, "n_derived": 2, "n_predict": "m", "n_replicate": "t", "observed": "y"},
                   {"tables": SPEC4 + (("m", 2),), "term": True, "pointwise": True, "n_derived": 2, "predict": True, "replicate": True,
                    "discrepancy": True}),
}


def test_every_combination_generates_the_recorded_text_and_key():
    gold = json.load(open(M.GOLDEN))["cases"]
    rec = M.record()
    assert len(gold) == 216 and set(rec) == set(gold)
    assert [cid for cid in gold if rec[cid] != gold[cid]] == []


@pytest.mark.parametrize("name", list(CONSTRUCTIONS))
def test_the_constructor_asks_for_the_plugin_its_arguments_imply(name, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks as H
    source, kw, parts = CONSTRUCTIONS[name]
    signature = inspect.signature(H.build_plugin)

    class Captured(Exception):
        pass

    def capture(*a, **k):
        raise Captured(signature.bind(*a, **k))
    monkeypatch.setattr(H, "build_plugin", capture)
    with pytest.raises(Captured) as e:
        tp.HipCallbacks(source, 3, **kw)
    bound = e.value.args[0]
    bound.apply_defaults()
    assert bound.arguments == dict(source=source, n_dim=3, verbose=False, **{**PLAIN, **parts})


def test_the_compiler_flags_of_every_part():
    """-DN_DIM always, one -D per optional part and only with it, in the order the cache has always seen."""
    from tempest_amd import hipcallbacks as H

    def defs(**kw):
        return H._Parts.of(PRIOR + LIKE, **kw).defines(3)
    assert defs() == defs(tables=SPEC4) == defs(term=True) == ["-DN_DIM=3"]
    assert defs(n_derived=5) == ["-DN_DIM=3", "-DN_DERIVED=5"]
    assert defs(predict=True) == ["-DN_DIM=3", "-DTPHU_PREDICT"]
    assert defs(term=True, pointwise=True) == ["-DN_DIM=3", "-DTPHU_POINTWISE"]
    assert defs(replicate=True) == ["-DN_DIM=3", "-DTPHU_REPLICATE"]
    assert defs(discrepancy=True) == ["-DN_DIM=3"]                    # discrepancy() without replicate() is no part
    assert defs(term=True, n_derived=2, predict=True, pointwise=True, replicate=True, discrepancy=True) == [
        "-DN_DIM=3", "-DN_DERIVED=2", "-DTPHU_PREDICT", "-DTPHU_POINTWISE", "-DTPHU_REPLICATE", "-DTPHU_DISCREPANCY"]


def test_scratch_sizes_and_tiles_follow_the_row_block_rule():
    """The sizing functions against their formulas written out with the literal layout (64 x 16 rows per block)."""
    from tempest_amd import hipcallbacks as H
    assert H.PREDICT_SUM_LAYOUT == (64, 16) and H.PREDICT_SCRATCH_WORDS == H.POINTWISE_SCRATCH_WORDS == 1 << 23
    for n in (1, 63, 64, 1023, 1024, 1025, 5000, 1 << 20, (1 << 31) + 5):
        nb = -(-n // 1024)
        for r in (1, 7, 64, 1000, 100_000):
            per_w = 4 * nb + 2
            assert H.pointwise_scratch_words(n, r) == 1 + nb + per_w * min(r, max(1, (1 << 23) // per_w))
            tile = 64
            while tile > 1 and nb * -(-r // tile) < 1024:
                tile //= 2
            assert H.pointwise_tiles(n, r) == tile
            for nq in (0, 1, 3, 8):
                per = nb + 258 * nq + 1
                batch = min(r, max(1, (1 << 23) // per))
                assert H.predict_scratch_words(n, r, nq) == 1 + nb + per * batch
                assert H.replicate_scratch_words(n, r, nq) == 3 + 3 * nb + 3 * r + 2 * -(-n // 64) + per * batch
                assert H.predict_tiles(n, r, nq)[0] == tile

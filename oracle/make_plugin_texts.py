"""Record what hipcallbacks.plugin_source and plugin_key generate for every valid combination of a plugin's optional parts
(tests/golden/plugin_texts.json; tests/test_plugin_texts.py regenerates and compares).  Only the two public signatures are used, so the
same script runs before and after a change of the host layer: the translation unit and the cache key of a plugin decide which shared
library is built and loaded, and a refactor of the host must move neither.

    python -m oracle.make_plugin_texts          # rewrites the golden file

Per case: a compact id, the first 16 hex digits of the SHA-256 of the text, and the key with the toolchain string replaced by
{toolchain}."""
import hashlib
import itertools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plugin_texts.json")

N_DIM, N_DERIVED = 3, 2
TABLES = (None, (("t", 1),), (("t", 1), ("obs", 2)))
# the text is pasted, not compiled: what matters is whether it calls tphu_tr_max( -- the helpers of a traced source come with it
SOURCE = """__device__ void prior_transform(const double* u, double* x) { for (int j = 0; j < N_DIM; ++j) x[j] = 2.0 * u[j] - 1.0; }
__device__ double log_likelihood(const double* x) { return -0.5 * x[0] * x[0]; }
"""
SOURCES = (SOURCE, SOURCE + "__device__ double widest(const double* x) { return tphu_tr_max(x[0], x[1]); }\n")


def cases():
    """(id, arguments of plugin_source, arguments of plugin_key) of every valid combination."""
    for (ti, tables), term, derived, predict, replicate, pointwise, discrepancy, (si, source) in itertools.product(
            enumerate(TABLES), (False, True), (False, True), (False, True), (False, True), (False, True), (False, True), enumerate(SOURCES)):
        if (pointwise and not term) or (discrepancy and not replicate):
            continue
        flags = "".join(c for c, on in zip("TXPWYZ", (term, derived, predict, pointwise, replicate, discrepancy)) if on)
        yield (f"d{ti}-{flags or '0'}-s{si}",
               ((source, tables, term), dict(derived=derived, predict=predict, pointwise=pointwise, replicate=replicate)),
               ((N_DIM,), dict(n_derived=N_DERIVED if derived else 0, predict=predict, pointwise=pointwise, replicate=replicate,
                               discrepancy=discrepancy)))


def record():
    """{id: [text hash, key]} of the code as it stands."""
    from tempest_amd import hipcallbacks as H
    out = {}
    for cid, (sa, skw), (ka, kkw) in cases():
        text = H.plugin_source(*sa, **skw)
        out[cid] = [hashlib.sha256(text.encode()).hexdigest()[:16], H.plugin_key(*ka, **kkw).replace(H._toolchain_id(), "{toolchain}")]
    return out


if __name__ == "__main__":
    rec = record()
    with open(GOLDEN, "w") as f:
        json.dump({"n_dim": N_DIM, "n_derived": N_DERIVED, "cases": rec}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases -> {GOLDEN}")

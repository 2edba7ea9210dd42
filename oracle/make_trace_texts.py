"""Record what tempest_amd.trace makes of a corpus of small torch callbacks (tests/golden/trace_texts.json; tests/test_trace_texts.py
regenerates and compares): the emitted HIP text, the graph, the replay, the report, the wording of every refusal and keyword error,
the torch names the tracer answers to and the public attributes of its symbolic value.  Only names that a caller of the tracer may
use are touched (trace_callbacks, trace_function, emit_source, replay, probe_batch, Noise, TV, _TORCH, TraceError), so the same script
runs before and after a change of the tracer's insides: the plugin cache key hashes the emitted text, and a refactor must move none of it.

    python -m oracle.make_trace_texts           # rewrites the golden file

Hashes, not texts: the first 16 hex digits of a SHA-256.  No plugin is built -- the HipCallbacks constructor is replaced by a recorder.
Run again on another kind of host, the script adds that host's replay hashes to the file and changes nothing else (`merged`)."""
import hashlib
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trace_texts.json")
ROWS = 64

# every operation of the graph: the corpus below must bring each into a live node
ALL_OPS = ("in const dterm delem yarg noise_normal noise_uniform add sub mul div pow max min abs sqrt rsqrt exp expm1 log log1p sin cos tan "
           "tanh atan erf erfc lgamma ndtri erfinv neg gt lt ge le eq ne and or not where").split()

A33 = np.array([[1.0, -2.0, 0.5], [0.25, 3.0, -1.0], [2.0, 0.0, 1.5]])
W23 = torch.tensor([[0.5, -1.0, 2.0], [1.5, 0.25, -0.75]], dtype=torch.float64)
B2 = torch.tensor([0.125, -3.0], dtype=torch.float64)
DATA = {"t": np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5]), "y": np.array([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0]),
        "m": np.arange(21.0).reshape(7, 3) * 0.125 - 1.0, "c": np.array([0.75, -0.5, 2.0]), "q": np.array([[1.0, 2.0], [3.0, 4.0]])}


def _sha(b):
    return hashlib.sha256(b if isinstance(b, bytes) else b.encode()).hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------- the corpus
def unit(u):
    return 2.0 * u - 1.0


def quantiles(u):
    y = torch.empty_like(u)
    y[:, 0] = 2.0 * u[:, 0] - 1.0
    y[:, 1] = torch.exp(u[:, 1])
    y[:, 2] = torch.special.ndtri(u[:, 2])
    y[:, 3] = torch.erfinv(2.0 * u[:, 3] - 1.0)
    y[:, 4] = u[:, 4] ** 2
    return y


def unaries(x):
    a = torch.abs(x[:, 0]) + torch.sqrt(x[:, 1]) + torch.rsqrt(x[:, 2]) + torch.exp(x[:, 3]) + torch.expm1(x[:, 4])
    b = torch.log(x[:, 0]) + torch.log1p(x[:, 1]) + torch.sin(x[:, 2]) + torch.cos(x[:, 3]) + torch.tan(x[:, 4])
    c = torch.tanh(x[:, 0]) + torch.atan(x[:, 1]) + torch.erf(x[:, 2]) + torch.erfc(x[:, 3]) + torch.lgamma(x[:, 4])
    return a - b * c + (-x).arctan().sum(dim=1) + x.negative().absolute().mean(dim=1)


def powers(x):
    a = x[:, 0]
    return torch.stack([a ** 0, a ** 1, a ** 2, a ** 3, a ** 0.5, a ** -0.5, a ** -1, a ** -2, a ** 2.5, a ** x[:, 1], 2.0 ** a,
                        torch.square(a), torch.reciprocal(a), torch.pow(a, 3.0), (a > 0.5) ** 2], dim=1)


def divisions(x):
    a, b = x[:, 0], x[:, 1]
    s = 3.0 / a + a / 3.0 + a / 0.0 + torch.div(a, b) + a / b + torch.div(torch.tensor(2.0, dtype=torch.float64), a) + 1 / b
    s = s + torch.sigmoid(a) + b.sigmoid() + torch.clamp(a, min=0.25, max=0.75) + b.clip(max=0.5) + torch.clamp(a, min=b)
    s = s + torch.minimum(a, b) + torch.maximum(a, b) + torch.add(a, b, alpha=2) + torch.sub(a, b, alpha=0.5) + torch.rsub(a, 1.0)
    return s + (1.0 - a) + a.mul(b).subtract(a).true_divide(b)


def bools(x):
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    m = ((a > b) & (b >= c)) | ~((a < c) | (b <= 0.5)) | (a == b) & (b != c)
    n = torch.logical_and(a.gt(0.25), torch.logical_or(b.lt(0.75), torch.logical_not(c.ge(0.5))))
    s = torch.where(m, a, b) + torch.where(n, 1.0, c) + (a > 0.5) + (b > 0.5) * c + (a.le(b) + a.eq(b)) - a.ne(c)
    return s + torch.where(a > b, b > c, a > c) * 2.0


def reductions(x):
    s = x.sum(dim=1) + x.mean(dim=-1) + x.prod(dim=1) + x.amax(dim=1) + x.amin(dim=1) + torch.logsumexp(x, dim=1)
    k = torch.sum(x, dim=1, keepdim=True)
    return s + (x / k).sum(dim=(1,)) + x.reshape(-1, 2, 2).sum(dim=2).amax(dim=1) + torch.mean(x[:, 1:3], 1)


def shapes(x):
    a = x.reshape(x.shape[0], 2, 2)
    b = torch.cat([a[:, 0], x[:, 0:1], x[..., 3].unsqueeze(-1)], dim=1)
    z, o = torch.zeros_like(x), torch.ones_like(x)
    y = x.clone()
    y[:, 1:3] = b[:, 0:2] * 2.0
    c = torch.stack([x[:, 0], y[:, 1]], dim=-1).squeeze(-1)
    return torch.cat([b, c, (z + o)[:, 0:1], a.view(-1, 4)[:, None, 2], x.double().contiguous().to(torch.float64)[:, 3:]], dim=1)


def products(x):
    return (x @ A33 + torch.matmul(x, torch.from_numpy(A33)) + x.matmul(A33.T)).sum(dim=1) \
        + torch.nn.functional.linear(x, W23, B2).sum(dim=1) + torch.nn.functional.linear(x, W23)[:, 0] + (x * A33[0]).sum(dim=1) \
        + (x + np.array([[1.0, 2.0, 3.0]])).prod(dim=1)


def prior_with_data(u, D):
    return D["c"][0] + (D["c"][2] - D["c"][0]) * u


def like_elements(x, D):
    return -0.5 * ((x[:, 0] - D["q"][0, 1]) ** 2 + (x[:, 1] - D["q"][-1, -1]) ** 2) * D["c"][1] + D["t"][6] * x[:, 2]


def derived_with_data(x, D):
    return torch.stack([x[:, 0] * D["c"][1], x.sum(dim=1)], dim=1)


def term_reads(x, D):
    mu = x[:, 0:1] + x[:, 1:2] * D["t"] + D["m"][:, 2] * D["c"][0] + x @ D["m"].T
    return -0.5 * (D["y"][None, :] - mu) ** 2 - torch.log(x[:, 2:3])


def term_linear(x, D):
    return torch.nn.functional.linear(x, D["m"]) - D["t"].unsqueeze(0) * x[:, 0].unsqueeze(-1)


def predict_band(x, D):
    return x[:, 0:1] + x[:, 1:2] * D["t"]


def replicate_normal(x, D, g):
    return x[:, 0:1] + x[:, 1:2] * D["t"] + torch.exp(x[:, 2:3]) * (g.normal(0) + 0.5 * g.normal(3))


def replicate_uniform(x, D, g):
    return torch.where(g.uniform(1) < torch.sigmoid(x[:, 0:1] * D["t"]), 1.0, 0.0) + 0.0 * g.uniform(4) * g.normal(1) + g.uniform(0) * 0.0


def discrepancy_square(x, y, D):
    return (y - x[:, 0:1] - x[:, 1:2] * D["t"]) ** 2


def discrepancy_abs(x, y, D):
    return torch.abs(y - D["y"]) * x[:, 0:1]


def _prior():
    import tempest_amd as tp
    return tp.Prior([tp.priors.Uniform(-5.0, 5.0), tp.priors.Normal(0.5, 2.0), tp.priors.LogNormal(0.0, 0.5)])


def _prior_uniform():
    import tempest_amd as tp
    return tp.Prior([tp.priors.Uniform(-5.0, 5.0), tp.priors.Uniform(0.0, 2.0)])


def cases():
    """(id, positional arguments of trace_callbacks, keywords) of every case."""
    d = DATA
    return [
        ("unaries", (quantiles, unaries, 5), {}),
        ("powers", (unit, lambda x: x.sum(dim=1), 2), dict(derived=powers)),
        ("divisions", (lambda u: 0.25 + 0.5 * u, divisions, 2), {}),
        ("bools", (unit, bools, 3), dict(derived=lambda x: (x > 0.0) + 0.0)),
        ("reductions", (lambda u: u + 0.5, reductions, 4), dict(derived=lambda x: x.sum(dim=1))),
        ("shapes", (unit, lambda x: shapes(x).sum(dim=1), 4), dict(derived=shapes)),
        ("products", (unit, products, 3), {}),
        ("elements", (prior_with_data, like_elements, 3), dict(data=d, derived=derived_with_data)),
        ("elements-plain-prior", (unit, like_elements, 3), dict(data=d, derived=lambda x: x[:, 0] * 2.0)),
        ("terms", (lambda u: u + 0.5, term_reads, 3), dict(data=d, n_terms="t", pointwise=True, predict=predict_band, n_predict=7)),
        ("terms-linear", (unit, term_linear, 3), dict(data=d, n_terms=7, derived=derived_with_data)),
        ("replicate-normal", (unit, term_reads, 3), dict(data=d, n_terms="y", replicate=replicate_normal, n_replicate="t", observed="y",
                                                          discrepancy=discrepancy_square)),
        ("replicate-uniform", (prior_with_data, like_elements, 3), dict(data=d, replicate=replicate_uniform, n_replicate=7, observed="y",
                                                                       discrepancy=discrepancy_abs, predict=predict_band, n_predict="m")),
        ("replicate-alone", (unit, like_elements, 3), dict(data=d, replicate=replicate_normal, n_replicate="t")),
        ("prior-normal", (_prior().transform, lambda x: -0.5 * (x * x).sum(dim=1), 3), {}),
        ("prior-uniform", (_prior_uniform().transform, lambda x: -0.5 * (x * x).sum(dim=1), 2), {}),
    ]


class _Recorded(Exception):
    pass


def _traced(args, kw):
    """trace_callbacks(*args, **kw) with the constructor of HipCallbacks replaced by a recorder: (cb, source, constructor keywords)."""
    from tempest_amd import hipcallbacks as H
    from tempest_amd import trace as T
    seen, real = {}, H.HipCallbacks

    def recorder(source, n_dim, **k):
        seen.update(source=source, n_dim=n_dim, kw=k)
        return types.SimpleNamespace(source=source, n_dim=n_dim)
    H.HipCallbacks = recorder
    try:
        cb = T.trace_callbacks(*args, check=False, **kw)
    finally:
        H.HipCallbacks = real
    return cb, seen


def _graph_record(T, g, n_dim, data, y):
    u = T.probe_batch(n_dim, ROWS)
    kinds = {g.nodes[i][0] for i in g.live()}
    extra = {}
    if kinds & {"noise_normal", "noise_uniform"}:
        extra["noise"] = T.Noise(T.PROBE_SEED, np.arange(ROWS), g.n_term)
    if "yarg" in kinds:
        extra["y"] = y
    out = T.replay(g, u, data, **extra) if data is not None else T.replay(g, u)
    return {"graph": _sha(repr(g.nodes) + repr(g.outputs) + repr(g.out_shape)), "widest": g.widest, "captured": len(g.captured),
            "reads": {k: sorted(v) for k, v in sorted(g.reads.items())}, "n_ops": g.n_ops(),
            "replay": _sha(np.ascontiguousarray(out, dtype=np.float64).tobytes()), "shape": list(out.shape)}, kinds


def record_cases():
    from tempest_amd import hipcallbacks as H
    from tempest_amd import trace as T
    out, covered = {}, set()
    for cid, args, kw in cases():
        cb, seen = _traced(args, kw)
        data = kw.get("data")
        tables = None if data is None else H._table_spec(data)[0]
        assert seen["source"] == T.emit_source(cb.trace_graphs, tables), cid
        ckw = {k: (sorted(v) if k == "data" else v) for k, v in seen["kw"].items()}
        report = dict(cb.trace_report, constants=[len(cb.trace_report["constants"]), _sha(repr(cb.trace_report["constants"]))])
        rec = {"source": _sha(seen["source"]), "constructor": ckw, "report": report, "graphs": {}}
        for name, g in cb.trace_graphs.items():
            rec["graphs"][name], kinds = _graph_record(T, g, args[2], data, None if data is None else data["y"])
            covered |= kinds
        out[cid] = rec
    missing = set(ALL_OPS) - covered
    assert not missing, f"the corpus has no live node of {sorted(missing)}"
    return out


# --------------------------------------------------------------------------------------------------------------- the refusals
def _spec(data):
    from tempest_amd.hipcallbacks import _table_spec
    tables, host = _table_spec(data)
    return tables, {k: (host[k].shape, np.asarray(data[k]).dtype == np.float64) for k, _ in tables}


def _unassigned(x):
    y = torch.empty_like(x)
    y[:, 0] = x[:, 0]
    return y * 2.0


def _stale_view(x):
    y = x.clone()
    v = y[:, 0]
    y[:, 0] = 1.0
    return v + y[:, 1]


def _through_view(x):
    y = x.clone()
    v = y[:, 0:2]
    v[:, 0] = 1.0
    return y


def _on_input(x):
    x[:, 0] = 1.0
    return x


def _inplace(x):
    y = x * 2.0
    y += 1.0
    return y


def _branch(x):
    if x[:, 0] > 0:
        return x
    return -x


def _loop(x):
    return sum(r for r in x)


def _arange_terms(x, D):
    return x[:, 0:1] * torch.arange(D["t"].shape[0])


def refusals():
    """(id, arguments of trace_function) of calls the tracer refuses."""
    DI = dict(DATA, k=np.arange(7))
    plain = [
        ("batch-extent", lambda x: x * x.shape[0]),
        ("too-wide", lambda x: torch.cat([x] * 22, dim=1)),
        ("stale-view", _stale_view),
        ("through-view", _through_view),
        ("on-input", _on_input),
        ("inplace", _inplace),
        ("iteration", _loop),
        ("branch", _branch),
        ("float", lambda x: x * float(x[:, 0])),
        ("attribute", lambda x: x.flip(1)),
        ("float32", lambda x: x.float()),
        ("to-float32", lambda x: x.to(torch.float32)),
        ("first-index", lambda x: x[0]),
        ("traced-index", lambda x: x[:, x[:, 0]]),
        ("too-many-indices", lambda x: x[:, 0, 0]),
        ("index-outside", lambda x: x[:, 9]),
        ("unsqueeze-0", lambda x: x.unsqueeze(0)),
        ("squeeze-all", lambda x: x.squeeze()),
        ("reshape", lambda x: x.reshape(2, -1)),
        ("sum-all", lambda x: x.sum()),
        ("sum-particles", lambda x: x.sum(dim=0)),
        ("sum-dtype", lambda x: x.sum(dim=1, dtype=torch.float32)),
        ("rmatmul", lambda x: A33 @ x),
        ("matmul-traced", lambda x: x @ x),
        ("matmul-extent", lambda x: x @ np.ones((2, 2))),
        ("cumsum", lambda x: torch.cumsum(x, dim=1)),
        ("floor", lambda x: torch.floor(x)),
        ("where-one", lambda x: torch.where(x > 0)),
        ("and-of-doubles", lambda x: x & x),
        ("captured-float32", lambda x: x + torch.ones(3, dtype=torch.float32)),
        ("captured-leading", lambda x: x + np.ones((2, 3))),
        ("broadcast-particles", lambda x: x + x[:, 0]),
        ("unassigned", _unassigned),
        ("clamp-none", lambda x: torch.clamp(x)),
        ("stack-0", lambda x: torch.stack([x, x], dim=0)),
        ("cat-0", lambda x: torch.cat([x, x])),
        ("ndtr", lambda x: torch.special.ndtr(x)),
        ("ndtri-out", lambda x: torch.special.ndtri(x, out=None) + torch.erfinv(x, out=x)),
        ("div-rounding", lambda x: torch.div(x, 2.0, rounding_mode="floor")),
        ("returns-number", lambda x: 1.0),
        ("returns-matrix", lambda x: x.reshape(-1, 3, 1).unsqueeze(-1)),
    ]
    out = [(cid, (fn, 3, None, "derived"), {}) for cid, fn in plain]
    out.append(("width", (lambda x: x[:, 0:2], 3, 3, "prior_transform"), {}))
    out.append(("not-a-vector", (lambda x: x, 3, (), "log_likelihood"), {}))
    spec, term = _spec(DI), (7, "n_terms")
    with_data = [
        ("no-entry", lambda x, D: x * D["nope"][0], None),
        ("matrix-whole", lambda x, D: x[:, 0:1] * D["m"], term),
        ("short-entry-whole", lambda x, D: x[:, 0:1] * D["c"], term),
        ("entry-whole-no-terms", lambda x, D: x[:, 0] * D["t"], None),
        ("column-no-terms", lambda x, D: x[:, 0] * D["m"][:, 0], None),
        ("entry-slice", lambda x, D: x[:, 0:1] * D["t"][1:3], term),
        ("entry-traced-index", lambda x, D: x[:, 0:1] * D["t"][x[:, 0]], term),
        ("entry-outside", lambda x, D: x[:, 0] * D["c"][3], None),
        ("integer-entry", lambda x, D: x[:, 0:1] * D["k"], term),
        ("sum-terms", lambda x, D: (x[:, 0:1] * D["t"]).sum(dim=-1), term),
        ("index-terms", lambda x, D: (x[:, 0:1] * D["t"])[:, 0], term),
        ("term-extent", _arange_terms, term),
        ("len-terms", lambda x, D: x[:, 0:1] * len(D["t"]), term),
        ("untransposed", lambda x, D: x @ D["m"], term),
        ("transpose-attribute", lambda x, D: x @ D["m"].T.contiguous(), term),
        ("data-reduced", lambda x, D: x[:, 0:1] * D["t"].sum(), term),
        ("no-term-axis", lambda x, D: x[:, 0:1] * 2.0, term),
        ("extra-axis", lambda x, D: x[:, :, None] * D["t"], term),
        ("returns-data", lambda x, D: D["t"], term),
        ("captured-along-terms", lambda x, D: x[:, 0:1] * D["t"] + np.ones(7), term),
    ]
    out += [(cid, (fn, 3, None, "log_likelihood_term" if t else "log_likelihood", spec, t), {}) for cid, fn, t in with_data]
    rep = (7, "n_replicate")
    out += [
        ("draw-float", (lambda x, D, g: x[:, 0:1] + g.normal(0.0) * D["t"], 3, None, "replicate", spec, rep), dict(noise=True)),
        ("draw-negative", (lambda x, D, g: x[:, 0:1] + g.uniform(-1) * D["t"], 3, None, "replicate", spec, rep), dict(noise=True)),
        ("draw-other", (lambda x, D, g: x[:, 0:1] + g.poisson(0) * D["t"], 3, None, "replicate", spec, rep), dict(noise=True)),
        ("replicate-bool", (lambda x, D, g: g.uniform(0) < x[:, 0:1] * D["t"], 3, None, "replicate", spec, rep), dict(noise=True)),
        ("replicate-no-axis", (lambda x, D, g: x[:, 0:1] * 2.0, 3, None, "replicate", spec, rep), dict(noise=True)),
        ("discrepancy-bool", (lambda x, y, D: y > x[:, 0:1], 3, None, "discrepancy", spec, rep), dict(yarg=True)),
        ("discrepancy-sum", (lambda x, y, D: ((y - x[:, 0:1]) ** 2).sum(dim=1), 3, None, "discrepancy", spec, rep), dict(yarg=True)),
        ("noise-without-data", (lambda x, D, g: x, 3, None, "replicate"), dict(noise=True)),
        ("not-callable", (3, 3), {}),
    ]
    return out


def keyword_errors():
    """(id, keywords of trace_callbacks) of every argument rule, in the order trace_callbacks checks them."""
    d = DATA
    return [
        ("n_dim", dict(n_dim=0)),
        ("n_derived", dict(n_derived=2)),
        ("too-wide", dict(n_dim=65)),
        ("n_predict-alone", dict(data=d, n_predict=7)),
        ("predict-without-data", dict(predict=predict_band, n_predict=7)),
        ("predict-without-n_predict", dict(data=d, predict=predict_band)),
        ("pointwise-without-n_terms", dict(data=d, pointwise=True)),
        ("n_replicate-alone", dict(data=d, n_replicate=7)),
        ("discrepancy-alone", dict(data=d, discrepancy=discrepancy_square, observed="y")),
        ("observed-alone", dict(data=d, observed="y")),
        ("replicate-without-data", dict(replicate=replicate_normal, n_replicate=7)),
        ("replicate-without-n_replicate", dict(data=d, replicate=replicate_normal)),
        ("discrepancy-without-observed", dict(data=d, replicate=replicate_normal, n_replicate=7, discrepancy=discrepancy_square)),
        ("n_terms-without-data", dict(n_terms=7)),
        ("n_terms-of-no-entry", dict(data=d, n_terms=5)),
        ("n_predict-names-nothing", dict(data=d, predict=predict_band, n_predict="nope")),
        # several rules broken at once: the first in the order of the checks is the one reported
        ("first-of-many", dict(n_predict=7, pointwise=True, n_replicate=7, discrepancy=discrepancy_square, observed="y")),
        ("first-of-replicate", dict(replicate=replicate_normal, discrepancy=discrepancy_square)),
        ("first-of-predict", dict(predict=predict_band, pointwise=True, replicate=replicate_normal)),
    ]


def _message(e):
    """type: text, every `at path:line:` reduced to the file's base name."""
    return type(e).__name__ + ": " + re.sub(r"at [^\n]*?([^/\\\n]+?):(\d+): ", r"at \1:\2: ", str(e))


def record_errors():
    from tempest_amd import trace as T
    out, accepted = {"refusals": {}, "keywords": {}}, []
    for cid, args, kw in refusals():
        try:
            T.trace_function(*args, **kw)
            accepted.append(cid)
        except (T.TraceError, TypeError, ValueError) as e:
            out["refusals"][cid] = _message(e)
    for cid, kw in keyword_errors():
        kw = dict(kw)
        n_dim = kw.pop("n_dim", 3)
        try:
            _traced((unit, lambda x, *D: x.sum(dim=1), n_dim), kw)
            accepted.append(cid)
        except (T.TraceError, ValueError) as e:
            out["keywords"][cid] = _message(e)
    assert not accepted, f"traced, but meant to be refused: {accepted}"
    return out


def record_names():
    from tempest_amd import trace as T
    lazy = subprocess.run([sys.executable, "-c", "import sys, tempest_amd, tempest_amd.sampler; "
                           "print(any(m == 'tempest_amd.trace' or m.startswith('tempest_amd.trace.') for m in sys.modules))"],
                          cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    return {"torch_names": sorted(T._TORCH), "tv_attributes": sorted(n for n in dir(T.TV) if not n.startswith("_")),
            "tv_dunders": sorted(n for n in vars(T.TV) if n.startswith("__") and callable(vars(T.TV)[n])),
            "prior_hip_source": {"normal": _sha(_prior().hip_source()), "uniform": _sha(_prior_uniform().hip_source())},
            "trace_loaded_by_sampler": lazy == "True"}


def record():
    return {"cases": record_cases(), **record_errors(), **record_names()}


def replays(rec, replace=None):
    """{(case, graph): the replay entry} of a record; replace: {(case, graph): entry} to put in their place."""
    out = {}
    for cid, case in rec["cases"].items():
        for name, g in case["graphs"].items():
            out[cid, name] = g["replay"]
            if replace is not None:
                g["replay"] = replace[cid, name]
    return out


def merged(rec, gold):
    """The golden record with this host's replay hashes added.  The transcendentals of a replay come from torch and NumPy on the
    CPU, whose vector libraries choose their code by the processor: the bits of exp or log differ from one kind of host to another
    by an ulp, for every commit alike.  So the golden holds, per graph, the replay hash of every kind of host it was recorded on
    (a graph of exact operations has one), and a replay must reproduce one of them.  Everything else is the same on every host:
    where it differs from `gold` (or there is none), the record starts afresh."""
    mine = replays(rec)
    new = json.loads(json.dumps(rec))
    replays(new, {k: [h] for k, h in mine.items()})
    if gold is not None:
        theirs = replays(gold)
        if set(theirs) == set(mine):
            a, b = json.loads(json.dumps(gold)), json.loads(json.dumps(new))
            replays(a, dict.fromkeys(mine))
            replays(b, dict.fromkeys(mine))
            if a == b:
                replays(new, {k: sorted(set(theirs[k]) | {mine[k]}) for k in mine})
    return new


if __name__ == "__main__":
    rec = json.loads(json.dumps(record()))
    gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None
    new = merged(rec, gold)
    with open(GOLDEN, "w") as f:
        json.dump(new, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['cases'])} cases, {len(rec['refusals'])} refusals, {len(rec['keywords'])} keyword errors -> {GOLDEN}; graphs whose "
          f"replay has more than one recorded hash: {sum(len(h) > 1 for h in replays(new).values())} of {len(replays(new))}")

"""Vectorised torch callbacks compiled into the fused step by tracing.

    cb = tempest_amd.trace_callbacks(prior_transform, log_likelihood, n_dim)
    sampler = tempest_amd.Sampler(cb.prior_transform, cb.log_likelihood, n_dim, vectorize=True, ...)

The user's two functions -- (n, d) float64 -> (n, d) and (n, d) -> (n,), written with torch operations -- are run ONCE on a symbolic
input that records what is done to it.  The record is a small SSA graph of scalar operations per particle (the leading axis is
the particle axis and stays symbolic, every trailing shape is static); it is written out as the two HIP device functions
`hipcallbacks.HipCallbacks` compiles into the Metropolis kernel, one statement per node, and the result is an ordinary
HipCallbacks object.  Hand-written code generation: no Triton, no inductor, no torch.fx.

What the emitted code computes is specified by `replay` (the graph in NumPy float64, node by node): a statement per operation
and contraction off, so no multiply-add is fused that eager torch's separate kernels would not fuse; sums, products, means,
maxima and inner products over the column axis run LEFT TO RIGHT IN COLUMN ORDER.  Where one torch-ROCm device kernel does not
compute the textbook form, the graph records what that kernel computes: `x / c` with a Python number c is x * (1 / c), `c / x` is (1 / x) * c, `mean` is
sum * (1 / k), `x ** 2` is x * x.  Everything outside the supported list is refused with a TraceError that
names the operation, the user's source line and what to write instead.

torch.special.ndtri and torch.erfinv are the exception to "what the eager kernel computes": they are emitted as calls of
csrc/quantile.h (Wichura's AS241, its text pasted in front of the source), and `ndtri_host` / `erfinv_host` restate that
header operation by operation -- the replay of these two nodes is their specification, a few ulp from eager torch's other algorithm.

Likelihoods over observed data (`data=`, `n_terms=`, `predict=`): the callbacks take the entries as a second argument D; the term
function (x, D) -> (n, n_terms) returns one column per observation and is emitted as `log_likelihood_term(x, r, D)`, the column at
the term index r -- the library owns the sum.  Under the tracer an entry has no particle axis: one as long as the term axis is a
value per term (`D.t[r]`), so is a column of a 2-D entry and `xs @ D["X"].T`; constant integer indices read one element.

Replicated data (`replicate=`, `n_replicate=`, `observed=`, `discrepancy=`): replicate (x, D, g) -> (n, n_replicate) draws its noise
from g.normal(k) / g.uniform(k), leaf nodes emitted as the calls of the plugin's `tphu_noise`; discrepancy (x, y, D) -> (n,
n_replicate) gets the term-valued y.  `Noise` is the host twin of the device's counter-based stream, for the eager side of the probe
and for `replay(..., noise=, y=)`.

The modules, each importing only those before it: graph, noise, value, probe; here the table of the callback kinds and the entry
points.
"""
import linecache
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from .graph import OPS, Graph, emit, erfinv_host, ndtri_host, quantile_header, replay
from .noise import MAX_DRAW, Noise
from .probe import PROBE_ROWS, PROBE_SEED, _ulps, compare, layered_sum, probe, probe_batch
from .value import (_POINT_TO_DATA, _TORCH, MAX_CONSTANTS, MAX_WIDTH, TV, TraceError, _call, _Data, _Entry, _map, _NoiseArg, _refuse,
                    _TermExtent, _wants_data)

# A callback kind, in the order of emission.  signature: up to the data argument; inp: the name of the input array; store: the
# statement that stores output k, held in tN; args: what the function is traced with -- "x, D" takes D whenever there is data,
# "x, D?" only if its signature has a second positional parameter; extent: the keyword that gives the extent of its term axis (it
# returns (n, extent) and is emitted for one index r), or None; width: the trailing shape it must return without one -- "n_dim", ()
# for (n,), None for (n, k) or (n,) as it comes.  Those traced with g or y return doubles: a bool result is refused.
Callback = namedtuple("Callback", "signature inp store args extent width")
CALLBACKS = {
    "prior_transform": Callback("void prior_transform(const double* u, double* x", "u", "x[{k}] = {t};", "x, D?", None, "n_dim"),
    "log_likelihood_term": Callback("double log_likelihood_term(const double* x, int64_t r", "x", "return {t};", "x, D", "n_terms", None),
    "log_likelihood": Callback("double log_likelihood(const double* x", "x", "return {t};", "x, D", None, ()),
    "predict": Callback("double predict(const double* x, int64_t r", "x", "return {t};", "x, D", "n_predict", None),
    "derived": Callback("void derived(const double* x, double* out", "x", "out[{k}] = {t};", "x, D?", None, None),
    "replicate": Callback("double replicate(const double* x, int64_t r, const tphu_noise& g", "x", "return {t};", "x, D, g",
                          "n_replicate", None),
    "discrepancy": Callback("double discrepancy(const double* x, int64_t r, double y", "x", "return {t};", "x, y, D", "n_replicate", None),
}

# the argument rules of trace_callbacks, in the order they are checked: (broken, by the arguments `a`; the ValueError's text)
_RULES = (
    (lambda a: a.predict is None and a.n_predict is not None,
     "trace_callbacks: n_predict= goes with predict= (a function (x, D) -> (n, n_predict))"),
    (lambda a: a.predict is not None and a.data is None,
     "trace_callbacks: predict= without data= is not traced (every column would be an expression of its own): "
     "give what depends on the index as a data entry and n_predict= its name"),
    (lambda a: a.predict is not None and a.n_predict is None,
     "trace_callbacks: predict= needs n_predict= (an int, or the name of a data entry)"),
    (lambda a: a.pointwise and a.n_terms is None, "trace_callbacks: pointwise=True goes with n_terms= (a term function)"),
    (lambda a: a.replicate is None and a.n_replicate is not None,
     "trace_callbacks: n_replicate= goes with replicate= (a function (x, D, g) -> (n, n_replicate))"),
    (lambda a: a.replicate is None and a.discrepancy is not None,
     "trace_callbacks: discrepancy= goes with replicate= (and n_replicate=, observed=)"),
    (lambda a: a.replicate is None and a.observed is not None, "trace_callbacks: observed= goes with replicate= (and n_replicate=)"),
    (lambda a: a.replicate is not None and a.data is None,
     "trace_callbacks: replicate= without data= is not traced (every column would be an expression of its own): "
     "give what depends on the index as a data entry and n_replicate= its name"),
    (lambda a: a.replicate is not None and a.n_replicate is None,
     "trace_callbacks: replicate= needs n_replicate= (an int, or the name of a data entry)"),
    (lambda a: a.discrepancy is not None and a.observed is None,
     "trace_callbacks: discrepancy= needs observed= (the name of the data entry it is compared on)"),
)


def _defined_at(fn):
    c = getattr(fn, "__code__", None)
    return "<unknown>" if c is None else f"{c.co_filename}:{c.co_firstlineno}: {linecache.getline(c.co_filename, c.co_firstlineno).strip()}"


def trace_function(fn, n_in, out_width=None, name=None, data=None, term=None, pass_data=None, noise=False, yarg=False):
    """Run `fn` once on a symbolic (n, n_in) float64 input; returns its Graph.  out_width: an int -> (n, out_width) expected, () ->
    (n,) expected, None -> (n, k) or (n,) as it comes.  data: (((name, rank), ...), {name: (shape, is float64)}) -- the entries fn may
    read through its second argument D (pass_data: hand D over; default: whenever data is given); term: (extent, its name) -- fn
    returns one column per term, (n, extent), and the graph computes the column at the term index r.  noise: fn is a replicate
    (x, D, g) -> (n, extent) and gets the noise object g behind D; yarg: fn is a discrepancy (x, y, D) -> (n, extent) and gets the
    term-valued y before D.  Either returns doubles: a bool result is refused."""
    if not callable(fn):
        raise TypeError(f"trace_callbacks: expected a callable, got {type(fn).__name__}")
    name = name or getattr(fn, "__name__", "callback")
    if (noise or yarg) and (data is None or term is None):
        raise ValueError("trace_function: noise= / yarg= go with data= and term= (replicate and discrepancy read D and return (n, n_replicate))")
    g = Graph(n_in, name, *((data[0],) if data is not None else (None,)), *(term or ()))
    g.term_extent = _TermExtent(g.term_name)
    x = TV(g, [g.add("in", j) for j in range(n_in)], is_input=True)
    args = (x,)
    if data is not None and (pass_data is None or pass_data):
        D = _Data((nm, _Entry(g, pos, nm, *data[1][nm])) for pos, (nm, _) in enumerate(data[0]))
        args = (x, D, _NoiseArg(g)) if noise else (x, TV(g, g.add("yarg"), term=True), D) if yarg else (x, D)
    y = _call(fn, *args)
    if (noise or yarg) and isinstance(y, TV) and y._bool():
        _refuse(f"a bool result of {g.name}", "a replicated observation and a discrepancy are doubles on the device; a comparison is "
                "a condition, not a value", "torch.where(condition, 1.0, 0.0)", at=_defined_at(fn))
    if not isinstance(y, TV) or not y.batch:
        raise TraceError(f"trace_callbacks: {g.name} returned {'a data value' if isinstance(y, TV) else type(y).__name__}, not a value "
                         "computed from its input with the supported torch operations")
    y = y._as_double()
    if term is not None:
        if not y.term or y.ids.ndim:
            raise TraceError((f"trace_callbacks: {g.name} returned {tuple(y.shape)}, expected (n, {g.term_extent!r}): one column per "
                             f"term, the result has no term axis of its own" if not y.term else
                             f"trace_callbacks: {g.name} returned {tuple(y.shape)}, expected (n, {g.term_extent!r}): reduce the other "
                             "axes (dim=1) first") + (f"\n  at {_defined_at(fn)}" if noise or yarg else ""))
    elif y.ids.ndim > 1 or (out_width is not None and y.ids.shape != ((out_width,) if out_width != () else ())):
        want = "(n, k) or (n,)" if out_width is None else f"(n, {out_width})" if out_width != () else "(n,)"
        raise TraceError(f"trace_callbacks: {g.name} returned (n,{','.join(map(str, y.ids.shape))}), expected {want}"
                         + (" (squeeze(-1) a trailing axis of extent 1)" if out_width == () else ""))
    _map(lambda i: i, y.ids)                        # every output column assigned
    g.outputs, g.out_shape = tuple(int(i) for i in y.ids.reshape(-1)), tuple(y.ids.shape)
    return g


def emit_function(graph, name, tables=None):
    """The HIP device function of the callback kind `name` (a key of CALLBACKS) for `graph`, with the signature a hand-written source
    gives it; tables: the data entries -- the signature then carries `const tphu_data& D`."""
    c = CALLBACKS[name]
    return emit(graph, f"__device__ {c.signature}{'' if tables is None else ', const tphu_data& D'})", c.inp,
                lambda k, t: c.store.format(k=k, t=t))


def emit_source(graphs, tables=None):
    """The HipCallbacks source for {"prior_transform": Graph, "log_likelihood" | "log_likelihood_term": Graph[, "predict": Graph]
    [, "derived": Graph][, "replicate": Graph[, "discrepancy": Graph]]}.  tables: the data entries -- every signature then carries
    `const tphu_data& D`, as hand-written ones do.  A draw of replicate is `g.normal(k)` / `g.uniform(k)`, called once per distinct
    (kind, k); discrepancy uses its `y` directly."""
    parts = ["// emitted by tempest_amd.trace_callbacks (DESIGN.md section 11): values live in registers, one statement per graph node"]
    if any(g.needs_quantile_header() for g in graphs.values()):
        parts.insert(0, quantile_header().rstrip("\n"))          # pasted, not #included: build_plugin hashes the text
    parts += [emit_function(graphs[name], name, tables) for name in CALLBACKS
              if name in graphs and not (name == "log_likelihood" and "log_likelihood_term" in graphs)]
    return "\n".join(parts) + "\n"


def _extent(v, what, host):
    """n_terms / n_predict: the name of a data entry (its length, or its rows), or an int that some entry has as that extent."""
    from ..hipcallbacks import _extent as extent
    if host is None:
        raise ValueError(f"trace_callbacks: {what}= goes with data= (the term and predict functions read the observations from D)")
    return extent(v, what, host, "trace_callbacks", of_an_entry=True)


def _is_f64(a):
    return a.dtype == torch.float64 if isinstance(a, torch.Tensor) else np.asarray(a).dtype == np.float64


def trace_callbacks(prior_transform, log_likelihood, n_dim, derived=None, check=True, *, data=None, n_terms=None, predict=None,
                    n_predict=None, pointwise=False, replicate=None, n_replicate=None, observed=None, discrepancy=None,
                    **hipcallbacks_kwargs):
    """The user's vectorised torch callbacks -- (n, d) float64 -> (n, d) and (n, d) -> (n,), unchanged -- as a HipCallbacks object:
    traced, emitted as HIP device functions, compiled by the usual HipCallbacks constructor.  derived: (n, d) -> (n, k) or (n,),
    becomes the source's derived(); check: run the probe (see `probe`).  cb.source holds the emitted text, cb.trace_report the op
    counts, the widest intermediate, the embedded constants, the data entries each callback reads and the probe's figures,
    cb.trace_graphs the graphs (for `replay`).

    data={name: array}, as HipCallbacks takes it: the callbacks get the entries as a dict D of float64 tensors in a second argument
    (prior_transform and derived only if they accept one).  With n_terms= (the name of an entry, or an int some entry has as its
    length or rows) the second callable is the TERM function (x, D) -> (n, n_terms), one column per observation, and the library owns
    the sum; without it, log_likelihood(x, D) -> (n,) may read elements D[name][j] only.  predict= (x, D) -> (n, n_predict) with
    n_predict= becomes the source's predict() (predict= without data= is refused: every column would have to be spelled out); pointwise=
    as in HipCallbacks (True, or "psis" for psis_loo as well).  A 1-D entry as long as the term axis is a value per term, used whole; a 2-D entry (T, k) gives columns
    D[name][:, j] and xs @ D[name].T; constant integer indices read an element of any entry.

    replicate= (x, D, g) -> (n, n_replicate) with n_replicate= (as n_predict=) becomes the source's replicate(): one replicated
    observation per column, its noise from g.normal(k) / g.uniform(k) -- k a constant Python int in [0, 2^31), each call a value per
    (row, column), the draw tphu_noise::normal(k) / uniform(k) of (seed, row, r) on the device, the same k the same value.
    observed= names the 1-D entry the replicates are compared with (PIT), as in HipCallbacks; discrepancy= (x, y, D) -> (n,
    n_replicate), y (n, n_replicate) the observed row broadcast or the replicated matrix, becomes the source's discrepancy(): the
    terms of the statistic, summed by the library in the term order -- no .sum().  replicate= needs data= and n_replicate=,
    discrepancy= needs replicate= and observed=, observed= needs replicate=.  Neither may reduce or index along the replicate axis
    or return a bool (torch.where(c, 1.0, 0.0)).  `Noise` is g on the host; cb.trace_report["draws"] lists the k that are drawn."""
    from ..hipcallbacks import HipCallbacks, _table_spec
    if not isinstance(n_dim, (int, np.integer)) or isinstance(n_dim, bool) or n_dim <= 0:
        raise ValueError(f"n_dim must be a positive int, got {n_dim!r}")
    n_dim = int(n_dim)
    if hipcallbacks_kwargs.get("n_derived"):
        raise ValueError("trace_callbacks: n_derived= belongs to hand-written sources (here it is the width of what derived returns)")
    if n_dim > MAX_WIDTH:
        raise TraceError(f"trace_callbacks: n_dim = {n_dim} is wider than {MAX_WIDTH} columns; {_POINT_TO_DATA}")
    tables, host = (None, None) if data is None else _table_spec(data)
    spec = None if data is None else (tables, {k: (host[k].shape, _is_f64(data[k])) for k, _ in tables})
    given = SimpleNamespace(data=data, n_terms=n_terms, predict=predict, n_predict=n_predict, pointwise=pointwise, replicate=replicate,
                            n_replicate=n_replicate, observed=observed, discrepancy=discrepancy)
    for broken, message in _RULES:
        if broken(given):
            raise ValueError(message)
    fns = {"prior_transform": prior_transform, "log_likelihood" if n_terms is None else "log_likelihood_term": log_likelihood}
    fns.update((k, f) for k, f in (("predict", predict), ("derived", derived), ("replicate", replicate), ("discrepancy", discrepancy))
               if f is not None)
    graphs = {}
    for name, c in CALLBACKS.items():
        if name in fns:
            term = None if c.extent is None else (_extent(getattr(given, c.extent), c.extent, host), c.extent)
            graphs[name] = trace_function(fns[name], n_dim, n_dim if c.width == "n_dim" else c.width, name, spec, term,
                                          pass_data=(data is not None and _wants_data(fns[name])) if c.args == "x, D?" else None,
                                          noise=c.args == "x, D, g", yarg=c.args == "x, y, D")
    source = emit_source(graphs, tables)
    n_derived = max(1, len(graphs["derived"].outputs)) if derived is not None else None
    data_kwargs = {} if data is None else {"data": host, "n_terms": n_terms, "n_predict": n_predict,
                                                 "pointwise": pointwise if isinstance(pointwise, str) else bool(pointwise)}
    if replicate is not None:
        data_kwargs.update(n_replicate=n_replicate, observed=observed)
    try:
        cb = HipCallbacks(source, n_dim, n_derived=n_derived, **data_kwargs, **hipcallbacks_kwargs)
    except Exception as e:
        e.source = source
        raise
    cb.trace_graphs = graphs
    cb.trace_report = {"ops": {k: g.n_ops() for k, g in graphs.items()}, "n_ops": sum(g.n_ops() for g in graphs.values()),
                       "widest": max(g.widest for g in graphs.values()),
                       "constants": sorted({float.hex(c) if math.isfinite(c) else repr(c) for g in graphs.values() for c in g.constants()}),
                       "probe": None}
    if data is not None:
        cb.trace_report["reads"] = {k: {name: sorted(how) for name, how in g.reads.items()} for k, g in graphs.items()}
    if replicate is not None:
        g = graphs["replicate"]
        cb.trace_report["draws"] = {"replicate": {kind: sorted(g.nodes[i][1] for i in g.live() if g.nodes[i][0] == "noise_" + kind)
                                                  for kind in ("normal", "uniform")}}
    if check:
        cb.trace_report["probe"] = probe(cb, prior_transform, log_likelihood, derived, predict, replicate, discrepancy)
    return cb

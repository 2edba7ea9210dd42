"""The graph a traced callback is recorded into, the one table of its operations, and its two interpreters: `emit` writes a HIP
device function, a statement per live node; `replay` evaluates the same nodes in NumPy float64 and is the specification of what
the emitted code computes.  Below them csrc/quantile.h restated for the host (the replay of "ndtri" and "erfinv")."""
import math
import struct
from collections import namedtuple
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

_UNINIT = -1


class Graph:
    """nodes[i] = (op, operands): "in" (column,), "const" (the double's 64 bits,), "dterm" (table, column) -- the data entry at
    position `table` of the spec read at the term index r: D.name[r], or D.name[r * D.name_cols + column] (column -1: a 1-D entry)
    --, "delem" (table, i, j) -- the element D.name[i] (j = -1) or D.name[i * D.name_cols + j] --, "noise_normal" / "noise_uniform" (k,)
    -- the draw g.normal(k) / g.uniform(k) of replicate, a value per (particle, r) --, "yarg" () -- the y of discrepancy, a value per
    (particle, r) --, else indices of earlier nodes.
    outputs: the node of every output value in row-major order of out_shape (the trailing shape: () for one value per particle).
    tables: ((name, rank), ...) of the data entries; n_term: the extent of the term axis (None: a callback without one), term_name
    its name ("n_terms" / "n_predict"), term_extent the symbolic extent the tracer shows in shapes (trace_function sets it);
    reads: {entry: {how it is read}}."""

    def __init__(self, n_in, name="", tables=None, n_term=None, term_name="n_terms"):
        self.n_in, self.name, self.nodes, self._cse = int(n_in), name, [], {}
        self.outputs, self.out_shape = (), ()
        self.widest, self.captured = int(n_in), set()          # captured: the nodes of constants that came from captured arrays
        self.tables, self.n_term, self.reads = tables, n_term, {}
        self.term_name, self.term_extent = term_name, None

    def add(self, op, *args):
        key = (op,) + args
        i = self._cse.get(key)
        if i is None:
            i = self._cse[key] = len(self.nodes)
            self.nodes.append(key)
        return i

    def const(self, v):
        return self.add("const", struct.unpack("<q", struct.pack("<d", float(v)))[0])

    def is_bool(self, i):
        return OPS[self.nodes[i][0]].is_bool

    def value(self, i):
        return struct.unpack("<d", struct.pack("<q", self.nodes[i][1]))[0]

    def live(self):
        """The nodes the outputs need, in emission order (dead nodes dropped)."""
        need, stack = set(), list(self.outputs)
        while stack:
            i = stack.pop()
            if i not in need:
                need.add(i)
                if not OPS[self.nodes[i][0]].leaf:
                    stack.extend(self.nodes[i][1:])
        return sorted(need)

    def n_ops(self):
        return sum(1 for i in self.live() if not OPS[self.nodes[i][0]].leaf)

    def constants(self):
        return [self.value(i) for i in self.live() if self.nodes[i][0] == "const"]

    def needs_quantile_header(self):
        """A live node is emitted as a call of csrc/quantile.h, whose text then goes in front of the source."""
        return any(self.nodes[i][0] in QUANTILE_OPS for i in self.live())


def _literal(v):
    """A double as a C99 hexadecimal floating literal: no decimal round trip can move a bit."""
    if math.isnan(v):
        return '__builtin_nan("")'
    if math.isinf(v):
        return "__builtin_inf()" if v > 0 else "-__builtin_inf()"
    return float.hex(v)


def _data_read(graph, op, args, r="r"):
    """The C expression of a "dterm" / "delem" node."""
    name = graph.tables[args[0]][0]
    if op == "dterm":
        return f"D.{name}[{r}]" if args[1] < 0 else f"D.{name}[{r} * D.{name}_cols + {args[1]}]"
    return f"D.{name}[{args[1]}]" if args[2] < 0 else f"D.{name}[{args[1]} * D.{name}_cols + {args[2]}]"


def quantile_header():
    """The text of csrc/quantile.h: the device functions behind the "ndtri" and "erfinv" nodes."""
    return (Path(__file__).resolve().parent.parent / "csrc" / "quantile.h").read_text()


# csrc/quantile.h restated: Wichura's AS241 (PPND16), the coefficients in the order of the header's argument lists (c0 first)
_AS241 = {
    "A": (3.3871328727963666080, 133.14166789178437745, 1971.5909503065514427, 13731.693765509461125, 45921.953931549871457,
          67265.770927008700853, 33430.575583588128105, 2509.0809287301226727),
    "B": (1.0, 42.313330701600911252, 687.18700749205790830, 5394.1960214247511077, 21213.794301586595867, 39307.895800092710610,
          28729.085735721942674, 5226.4952788528545610),
    "C": (1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504, 1.27045825245236838258,
          0.241780725177450611770, 0.0227238449892691845833, 7.74545014278341407640e-4),
    "D": (1.0, 2.05319162663775882187, 1.67638483018380384940, 0.689767334985100004550, 0.148103976427480074590,
          0.0151986665636164571966, 5.47593808499534494600e-4, 1.05075007164441684324e-9),
    "E": (6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 0.296560571828504891230, 0.0265321895265761230930,
          0.00124266094738807843860, 2.71155556874348757815e-5, 2.01033439929228813265e-7),
    "F": (1.0, 0.599832206555887937690, 0.136929880922735805310, 0.0148753612908506148525, 7.86869131145613259100e-4,
          1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15),
}


def _torch_unary(name):
    fn = getattr(torch, name)
    return lambda a: fn(torch.from_numpy(np.ascontiguousarray(a))).numpy()


_LOG = _torch_unary("log")


def _poly(r, c):
    s = np.full_like(r, c[7])
    for k in range(6, -1, -1):
        s = s * r + c[k]
    return s


def _ndtri_core(q, t):
    """tphu_ndtri_core of csrc/quantile.h in NumPy float64: the same operations in the same order, every region evaluated for every
    element and the element's own one kept (an element's value does not depend on the others).  log comes from torch on the CPU."""
    with np.errstate(all="ignore"):
        r = 0.180625 - q * q
        central = q * _poly(r, _AS241["A"]) / _poly(r, _AS241["B"])
        r = np.sqrt(-_LOG(t))
        near = _poly(r - 1.6, _AS241["C"]) / _poly(r - 1.6, _AS241["D"])
        far = _poly(r - 5.0, _AS241["E"]) / _poly(r - 5.0, _AS241["F"])
        x = np.where(r <= 5.0, near, far)
        x = np.where(t > 0.0, x, np.inf)
        return np.where(np.abs(q) <= 0.425, central, np.where(q < 0.0, -x, x))


def ndtri_host(p):
    """tphu_ndtri of csrc/quantile.h in NumPy: what the device computes for torch.special.ndtri under the tracer."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where((p >= 0.0) & (p <= 1.0), _ndtri_core(p - 0.5, np.fmin(p, 1.0 - p)), np.nan)


def erfinv_host(y):
    """tphu_erfinv of csrc/quantile.h in NumPy: what the device computes for torch.erfinv under the tracer."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.abs(y) <= 1.0, _ndtri_core(0.5 * y, 0.5 * (1.0 - np.abs(y))) * 0.70710678118654752440, np.nan)


# ------------------------------------------------------------------------------------------------- the operation table
def _host_array(v):
    return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)


# the replay of a leaf: (the run `p` -- graph, rows a, their number n, col, tabs, noise, y --, the node's plain-int operands)
def _replay_dterm(p, table, column):
    t = p.tabs[table]
    if p.graph.n_term is None or t.shape[0] != p.graph.n_term:
        raise ValueError(f"replay: data[{p.graph.tables[table][0]!r}] has {t.shape[0]} rows, traced with {p.graph.n_term}")
    return (t if column < 0 else np.ascontiguousarray(t[:, column]))[None, :]


def _replay_noise(kind):
    def draw(p, k):
        if p.noise is None:
            raise ValueError("replay: this graph draws noise: give noise=Noise(seed, items, n_replicate)")
        v = _host_array(getattr(p.noise, kind)(k))
        if v.shape != (p.n, p.graph.n_term):
            raise ValueError(f"replay: noise.{kind}({k}) has shape {v.shape}, expected {(p.n, p.graph.n_term)}")
        return v
    return draw


def _replay_yarg(p):
    if p.y is None:
        raise ValueError("replay: this graph reads y: give y= (n_replicate,) or (n, n_replicate)")
    v = _host_array(p.y)
    if v.shape not in ((p.graph.n_term,), (p.n, p.graph.n_term)):
        raise ValueError(f"replay: y has shape {v.shape}, expected {(p.graph.n_term,)} or {(p.n, p.graph.n_term)}")
    return v[None, :] if v.ndim == 1 else v


# An operation of the graph.  c: how it is written in C, a format over the names of its operands -- the tN of earlier nodes; for a
# leaf, whose operands are plain ints, the ints themselves, {inp} the input array, {value} the literal of a "const", {read} the
# table access of a "dterm" / "delem".  host: what it computes in the replay, on the operands' arrays; for a leaf on (the run, the
# ints).  The transcendentals come from torch on the CPU, as the eager function's do there: NumPy's differ from them by an ulp on some
# hosts, and the replay of a trace is held against eager torch to the bit.
Op = namedtuple("Op", "c host is_bool leaf", defaults=(False, False))
OPS = {
    "in": Op("{inp}[{0}]", lambda p, column: p.col(p.a[:, column]), leaf=True),
    "const": Op("{value}", lambda p, bits: p.col(np.full(p.n, struct.unpack("<d", struct.pack("<q", bits))[0])), leaf=True),
    "dterm": Op("{read}", _replay_dterm, leaf=True),
    "delem": Op("{read}", lambda p, t, i, j: p.col(np.full(p.n, p.tabs[t][i] if j < 0 else p.tabs[t][i, j])), leaf=True),
    "yarg": Op("y", _replay_yarg, leaf=True),
    "noise_normal": Op("g.normal({0})", _replay_noise("normal"), leaf=True),
    "noise_uniform": Op("g.uniform({0})", _replay_noise("uniform"), leaf=True),
    "add": Op("{0} + {1}", np.add),
    "sub": Op("{0} - {1}", np.subtract),
    "mul": Op("{0} * {1}", np.multiply),
    "div": Op("{0} / {1}", np.divide),
    "pow": Op("pow({0}, {1})", np.power),
    "max": Op("tphu_tr_max({0}, {1})", np.maximum),
    "min": Op("tphu_tr_min({0}, {1})", np.minimum),
    "abs": Op("fabs({0})", np.abs),
    "sqrt": Op("sqrt({0})", np.sqrt),
    "rsqrt": Op("rsqrt({0})", lambda v: 1.0 / np.sqrt(v)),
    **{op: Op(op + "({0})", _torch_unary(op)) for op in ("exp", "expm1", "log", "log1p", "sin", "cos", "tan", "tanh", "atan", "erf",
                                                         "erfc", "lgamma")},
    "ndtri": Op("tphu_ndtri({0})", ndtri_host),         # calls of csrc/quantile.h, restated above -- NOT eager torch's algorithm
    "erfinv": Op("tphu_erfinv({0})", erfinv_host),
    "neg": Op("-{0}", np.negative),
    "gt": Op("{0} > {1}", np.greater, is_bool=True),
    "lt": Op("{0} < {1}", np.less, is_bool=True),
    "ge": Op("{0} >= {1}", np.greater_equal, is_bool=True),
    "le": Op("{0} <= {1}", np.less_equal, is_bool=True),
    "eq": Op("{0} == {1}", np.equal, is_bool=True),
    "ne": Op("{0} != {1}", np.not_equal, is_bool=True),
    "and": Op("{0} && {1}", np.logical_and, is_bool=True),
    "or": Op("{0} || {1}", np.logical_or, is_bool=True),
    "not": Op("!{0}", np.logical_not, is_bool=True),
    "where": Op("{0} ? {1} : {2}", np.where),
}
QUANTILE_OPS = ("ndtri", "erfinv")
DATA_OPS = ("dterm", "delem")


def emit(graph, signature, inp, store, r="r"):
    """One HIP device function for `graph`: `signature` { one statement per live node; store(k, "tN") per output }.  r: the name of
    the term index in the signature (graphs that read data entries per term)."""
    lines = [signature + " {",
             "  // traced from " + (graph.name or "a torch callback") + ": one operation per statement, contraction off; sums, products and",
             "  // inner products over the column axis accumulate left to right in column order",
             "#pragma clang fp contract(off)"]
    for i in graph.live():
        op, args = graph.nodes[i][0], graph.nodes[i][1:]
        o = OPS[op]
        special = {"value": _literal(graph.value(i))} if op == "const" else {"read": _data_read(graph, op, args, r)} if op in DATA_OPS else {}
        rhs = o.c.format(*(args if o.leaf else [f"t{a}" for a in args]), inp=inp, **special)
        lines.append(f"  const {'bool' if o.is_bool else 'double'} t{i} = {rhs};")
    lines += ["  " + store(k, f"t{i}") for k, i in enumerate(graph.outputs)]
    lines.append("}")
    return "\n".join(lines)


def replay(graph, array, data=None, noise=None, y=None):
    """The graph evaluated in NumPy float64, node by node in emission order, on the (n, n_in) rows of `array`: what the emitted
    device function computes -- (n,) + graph.out_shape; (n, T) for a term, predict, replicate or discrepancy graph, whose nodes are
    evaluated for every (row, term index) -- the device function is called once per pair.  data: {name: array} for graphs that read
    data entries; noise: a `Noise` over the n rows (anything with .normal(k) / .uniform(k) -> (n, T)) for a replicate graph that
    draws; y: (T,) -- one row for all -- or (n, T), the y of a discrepancy graph.
    exp, log and the other transcendentals, erf, erfc and lgamma come from torch on the CPU; ndtri and erfinv are `ndtri_host` /
    `erfinv_host`, the restatement of csrc/quantile.h -- NOT eager torch's, which computes them with another algorithm."""
    a = np.ascontiguousarray(array, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != graph.n_in:
        raise ValueError(f"replay: expected (n, {graph.n_in}) rows, got {a.shape}")
    n, val = a.shape[0], {}
    per_term, tabs = graph.n_term is not None, None
    if per_term or any(graph.nodes[i][0] in DATA_OPS for i in graph.live()):
        if data is None:
            raise ValueError("replay: this graph reads data entries: give data={name: array}")
        tabs = [np.ascontiguousarray(data[name], dtype=np.float64) for name, _ in graph.tables]
        for t, (name, rank) in zip(tabs, graph.tables):
            if t.ndim != rank:
                raise ValueError(f"replay: data[{name!r}] has {t.ndim} axes, traced with {rank}")
    # a per-term graph: every value is (n, 1), (1, T) or (n, T) -- a column of x, a data entry at every r, what is computed from both
    col = (lambda v: v[:, None]) if per_term else (lambda v: v)
    run = SimpleNamespace(graph=graph, a=a, n=n, col=col, tabs=tabs, noise=noise, y=y)
    with np.errstate(all="ignore"):
        for i in graph.live():
            o, args = OPS[graph.nodes[i][0]], graph.nodes[i][1:]
            val[i] = o.host(run, *args) if o.leaf else o.host(*(val[j] for j in args))
    if per_term:
        return np.array(np.broadcast_to(val[graph.outputs[0]], (n, graph.n_term)), dtype=np.float64)
    out = np.empty((n, len(graph.outputs)))
    for k, i in enumerate(graph.outputs):
        out[:, k] = val[i]
    return out.reshape((n,) + tuple(graph.out_shape))

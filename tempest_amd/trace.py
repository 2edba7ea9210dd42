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
csrc/quantile.h (Wichura's AS241, its text pasted in front of the source), and `ndtri_host` / `erfinv_host` below restate that
header operation by operation -- the replay of these two nodes is their specification, a few ulp from eager torch's other algorithm.

Likelihoods over observed data (`data=`, `n_terms=`, `predict=`): the callbacks take the entries as a second argument D; the term
function (x, D) -> (n, n_terms) returns one column per observation and is emitted as `log_likelihood_term(x, r, D)`, the column at
the term index r -- the library owns the sum.  Under the tracer an entry has no particle axis: one as long as the term axis is a
value per term (`D.t[r]`), so is a column of a 2-D entry and `xs @ D["X"].T`; constant integer indices read one element.

Replicated data (`replicate=`, `n_replicate=`, `observed=`, `discrepancy=`): replicate (x, D, g) -> (n, n_replicate) draws its noise
from g.normal(k) / g.uniform(k), leaf nodes emitted as the calls of the plugin's `tphu_noise`; discrepancy (x, y, D) -> (n,
n_replicate) gets the term-valued y.  `Noise` is the host twin of the device's counter-based stream, for the eager side of the probe
and for `replay(..., noise=, y=)`.
"""
import linecache
import math
import os
import struct
import sys
from pathlib import Path

import numpy as np

from .tools import SQRTEPS

MAX_WIDTH = 64                  # columns of an intermediate: 64 doubles are a quarter of a lane's 512-VGPR budget
MAX_CONSTANTS = 64 * 64         # elements of captured arrays embedded in the source
PROBE_ROWS, PROBE_SEED, _PROBE_TAG = 4096, 20240611, 0x7472

_POINT_TO_DATA = ("straight-line code over that many values is the wrong tool: give the observations as "
                  "HipCallbacks(source, n_dim, data={...}, n_terms=...) and write log_likelihood_term by hand, or as "
                  "trace_callbacks(..., data={...}, n_terms=...) with a term function of (x, D)")
_OWNS_THE_SUM = "the library owns the sum over observations"
_NO_TERM_AXIS = ("this callback (prior_transform, derived, a log_likelihood without n_terms=) has no term axis: only the term "
                 "function (n_terms=) and predict (n_predict=) return one column per observation")
_RETURN_TERMS = "return the (n, n_terms) terms; reduce over the other axes (dim=1) only"


class TraceError(Exception):
    """A callback that cannot be traced, or a trace the probe found wrong.  `.source`: the emitted text, where there is one."""
    source = None


def _where():
    """file:line: text of the innermost frame that is neither this module nor torch: the user's line."""
    here, f = os.path.abspath(__file__), sys._getframe(1)
    while f is not None:
        fn = f.f_code.co_filename
        if os.path.abspath(fn) != here and (os.sep + "torch" + os.sep) not in fn:
            return f"{fn}:{f.f_lineno}: {linecache.getline(fn, f.f_lineno).strip()}"
        f = f.f_back
    return "<unknown>"


def _refuse(op, why, instead, at=None):
    raise TraceError(f"trace_callbacks: {op} cannot be traced: {why}\n  at {at or _where()}\n  instead: {instead}")


def _call(fn, *args):
    """fn(*args); a torch function that rejects the symbolic extent of an axis by its type (torch.arange(n_terms)) before the extent
    could refuse the use itself is refused here, at the user's line of the traceback."""
    try:
        return fn(*args)
    except TypeError as e:
        kinds = [k for k in (_TermExtent, _Batch) if k.__name__ in str(e)]
        if not kinds:
            raise
        here, at, tb = os.path.abspath(__file__), None, e.__traceback__
        while tb is not None:
            fn_ = tb.tb_frame.f_code.co_filename
            if os.path.abspath(fn_) != here and (os.sep + "torch" + os.sep) not in fn_:
                at = f"{fn_}:{tb.tb_lineno}: {linecache.getline(fn_, tb.tb_lineno).strip()}"
            tb = tb.tb_next
        _refuse(*kinds[0]._WHY, at=at)


# ------------------------------------------------------------------------------------------------------ the graph
_BINARY = {"add": "+", "sub": "-", "mul": "*", "div": "/"}
_CALL2 = {"pow": "pow", "max": "tphu_tr_max", "min": "tphu_tr_min"}
_UNARY = {"abs": "fabs", "sqrt": "sqrt", "rsqrt": "rsqrt", "exp": "exp", "expm1": "expm1", "log": "log", "log1p": "log1p",
          "sin": "sin", "cos": "cos", "tan": "tan", "tanh": "tanh", "atan": "atan", "erf": "erf", "erfc": "erfc", "lgamma": "lgamma",
          "ndtri": "tphu_ndtri", "erfinv": "tphu_erfinv"}
_QUANTILE = ("ndtri", "erfinv")                 # emitted as calls of csrc/quantile.h, whose text emit_source pastes in front
_COMPARE = {"gt": ">", "lt": "<", "ge": ">=", "le": "<=", "eq": "==", "ne": "!="}
_BOOL_OPS = set(_COMPARE) | {"and", "or", "not"}
_NOISE = {"noise_normal": "normal", "noise_uniform": "uniform"}
_LEAF = ("in", "const", "dterm", "delem", "yarg") + tuple(_NOISE)    # nodes without operand nodes: what follows the op are plain ints
_UNINIT = -1


class Graph:
    """nodes[i] = (op, operands): "in" (column,), "const" (the double's 64 bits,), "dterm" (table, column) -- the data entry at
    position `table` of the spec read at the term index r: D.name[r], or D.name[r * D.name_cols + column] (column -1: a 1-D entry)
    --, "delem" (table, i, j) -- the element D.name[i] (j = -1) or D.name[i * D.name_cols + j] --, "noise_normal" / "noise_uniform" (k,)
    -- the draw g.normal(k) / g.uniform(k) of replicate, a value per (particle, r) --, "yarg" () -- the y of discrepancy, a value per
    (particle, r) --, else indices of earlier nodes.
    outputs: the node of every output value in row-major order of out_shape (the trailing shape: () for one value per particle).
    tables: ((name, rank), ...) of the data entries; n_term: the extent of the term axis (None: a callback without one), term_name
    its name ("n_terms" / "n_predict"); reads: {entry: {how it is read}}."""

    def __init__(self, n_in, name="", tables=None, n_term=None, term_name="n_terms"):
        self.n_in, self.name, self.nodes, self._cse = int(n_in), name, [], {}
        self.outputs, self.out_shape = (), ()
        self.widest, self.captured = int(n_in), set()          # captured: the nodes of constants that came from captured arrays
        self.tables, self.n_term, self.reads = tables, n_term, {}
        self.term_extent = _TermExtent(term_name)

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
        return self.nodes[i][0] in _BOOL_OPS

    def value(self, i):
        return struct.unpack("<d", struct.pack("<q", self.nodes[i][1]))[0]

    def live(self):
        """The nodes the outputs need, in emission order (dead nodes dropped)."""
        need, stack = set(), list(self.outputs)
        while stack:
            i = stack.pop()
            if i not in need:
                need.add(i)
                if self.nodes[i][0] not in _LEAF:
                    stack.extend(self.nodes[i][1:])
        return sorted(need)

    def n_ops(self):
        return sum(1 for i in self.live() if self.nodes[i][0] not in _LEAF)

    def constants(self):
        return [self.value(i) for i in self.live() if self.nodes[i][0] == "const"]


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


def emit(graph, signature, inp, store, r="r"):
    """One HIP device function for `graph`: `signature` { one statement per live node; store(k, "tN") per output }.  r: the name of
    the term index in the signature (graphs that read data entries per term)."""
    lines = [signature + " {",
             "  // traced from " + (graph.name or "a torch callback") + ": one operation per statement, contraction off; sums, products and",
             "  // inner products over the column axis accumulate left to right in column order",
             "#pragma clang fp contract(off)"]
    for i in graph.live():
        op, args = graph.nodes[i][0], graph.nodes[i][1:]
        t = [f"t{a}" for a in args]
        kind = "bool" if op in _BOOL_OPS else "double"
        if op == "in":
            rhs = f"{inp}[{args[0]}]"
        elif op == "const":
            rhs = _literal(graph.value(i))
        elif op in ("dterm", "delem"):
            rhs = _data_read(graph, op, args, r)
        elif op in _NOISE:
            rhs = f"g.{_NOISE[op]}({args[0]})"
        elif op == "yarg":
            rhs = "y"
        elif op in _BINARY:
            rhs = f"{t[0]} {_BINARY[op]} {t[1]}"
        elif op in _CALL2:
            rhs = f"{_CALL2[op]}({t[0]}, {t[1]})"
        elif op in _UNARY:
            rhs = f"{_UNARY[op]}({t[0]})"
        elif op == "neg":
            rhs = f"-{t[0]}"
        elif op in _COMPARE:
            rhs = f"{t[0]} {_COMPARE[op]} {t[1]}"
        elif op == "and":
            rhs = f"{t[0]} && {t[1]}"
        elif op == "or":
            rhs = f"{t[0]} || {t[1]}"
        elif op == "not":
            rhs = f"!{t[0]}"
        elif op == "where":
            rhs = f"{t[0]} ? {t[1]} : {t[2]}"
        else:                                        # pragma: no cover
            raise TraceError(f"emit: unknown node {op!r}")
        lines.append(f"  const {kind} t{i} = {rhs};")
    lines += ["  " + store(k, f"t{i}") for k, i in enumerate(graph.outputs)]
    lines.append("}")
    return "\n".join(lines)


def _torch_unary(name):
    import torch
    fn = getattr(torch, name)
    return lambda a: fn(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _host_array(v):
    return np.asarray(v.detach().cpu().numpy() if _is_tensor(v) else v, dtype=np.float64)


def quantile_header():
    """The text of csrc/quantile.h: the device functions behind the "ndtri" and "erfinv" nodes."""
    return (Path(__file__).resolve().parent / "csrc" / "quantile.h").read_text()


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
        r = np.sqrt(-_torch_unary("log")(t))
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
    if per_term or any(graph.nodes[i][0] in ("dterm", "delem") for i in graph.live()):
        if data is None:
            raise ValueError("replay: this graph reads data entries: give data={name: array}")
        tabs = [np.ascontiguousarray(data[name], dtype=np.float64) for name, _ in graph.tables]
        for t, (name, rank) in zip(tabs, graph.tables):
            if t.ndim != rank:
                raise ValueError(f"replay: data[{name!r}] has {t.ndim} axes, traced with {rank}")
    # a per-term graph: every value is (n, 1), (1, T) or (n, T) -- a column of x, a data entry at every r, what is computed from both
    col = (lambda v: v[:, None]) if per_term else (lambda v: v)
    # the transcendentals come from torch on the CPU, the library the eager function calls there: NumPy's differ from it by an ulp
    # on some hosts, and the replay of a trace is held against eager torch to the bit
    un = {"abs": np.abs, "sqrt": np.sqrt, "rsqrt": lambda v: 1.0 / np.sqrt(v), "neg": np.negative, "not": np.logical_not}
    un.update({k: _torch_unary(k) for k in ("exp", "expm1", "log", "log1p", "sin", "cos", "tan", "tanh", "atan")})
    bi = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power, "max": np.maximum,
          "min": np.minimum, "gt": np.greater, "lt": np.less, "ge": np.greater_equal, "le": np.less_equal, "eq": np.equal,
          "ne": np.not_equal, "and": np.logical_and, "or": np.logical_or}
    with np.errstate(all="ignore"):
        for i in graph.live():
            op, args = graph.nodes[i][0], graph.nodes[i][1:]
            if op == "in":
                val[i] = col(a[:, args[0]])
            elif op == "const":
                val[i] = col(np.full(n, graph.value(i)))
            elif op == "delem":
                val[i] = col(np.full(n, tabs[args[0]][args[1]] if args[2] < 0 else tabs[args[0]][args[1], args[2]]))
            elif op == "dterm":
                t = tabs[args[0]]
                if not per_term or t.shape[0] != graph.n_term:
                    raise ValueError(f"replay: data[{graph.tables[args[0]][0]!r}] has {t.shape[0]} rows, traced with {graph.n_term}")
                val[i] = (t if args[1] < 0 else np.ascontiguousarray(t[:, args[1]]))[None, :]
            elif op in _NOISE:
                if noise is None:
                    raise ValueError("replay: this graph draws noise: give noise=Noise(seed, items, n_replicate)")
                val[i] = _host_array(getattr(noise, _NOISE[op])(args[0]))
                if val[i].shape != (n, graph.n_term):
                    raise ValueError(f"replay: noise.{_NOISE[op]}({args[0]}) has shape {val[i].shape}, expected {(n, graph.n_term)}")
            elif op == "yarg":
                if y is None:
                    raise ValueError("replay: this graph reads y: give y= (n_replicate,) or (n, n_replicate)")
                val[i] = _host_array(y)
                if val[i].shape not in ((graph.n_term,), (n, graph.n_term)):
                    raise ValueError(f"replay: y has shape {val[i].shape}, expected {(graph.n_term,)} or {(n, graph.n_term)}")
                val[i] = val[i][None, :] if val[i].ndim == 1 else val[i]
            elif op in bi:
                val[i] = bi[op](val[args[0]], val[args[1]])
            elif op in un:
                val[i] = un[op](val[args[0]])
            elif op in ("erf", "erfc", "lgamma"):
                val[i] = _torch_unary(op)(val[args[0]])
            elif op in _QUANTILE:
                val[i] = (ndtri_host if op == "ndtri" else erfinv_host)(val[args[0]])
            elif op == "where":
                val[i] = np.where(val[args[0]], val[args[1]], val[args[2]])
            else:                                    # pragma: no cover
                raise TraceError(f"replay: unknown node {op!r}")
    if per_term:
        return np.array(np.broadcast_to(val[graph.outputs[0]], (n, graph.n_term)), dtype=np.float64)
    out = np.empty((n, len(graph.outputs)))
    for k, i in enumerate(graph.outputs):
        out[:, k] = val[i]
    return out.reshape((n,) + tuple(graph.out_shape))


# ------------------------------------------------------------------------------------------------ the symbolic value
class _Batch:
    """x.shape[0]: usable as the leading extent of a reshape, and as nothing else."""

    _WHY = ("x.shape[0] (the number of particles n)", "the particle axis is symbolic; its extent may not enter the arithmetic, "
            "a loop or an allocation", "write the function per row: reductions over dim=1, no use of n")

    def _no(self, *a, **k):
        _refuse(*self._WHY)
    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __floordiv__ = __rfloordiv__ = _no
    __mod__ = __pow__ = __rpow__ = __neg__ = __index__ = __int__ = __float__ = __bool__ = __lt__ = __le__ = __gt__ = __ge__ = _no
    __hash__ = None

    def __eq__(self, other):
        return self._no()

    def __repr__(self):
        return "n"


_BATCH = _Batch()


class _TermExtent(_Batch):
    """The extent of the term axis (D["t"].shape[0], y.shape[-1]): a name in .shape, and nothing else."""
    _WHY = ("the extent of the term axis (D[...].shape[0], len(D[...]), range / torch.arange over it)", "the term axis is symbolic, "
            "like the particle axis: the emitted function computes ONE term, at the index r the library hands it; the term index "
            "cannot be manufactured", "write the function for all terms at once, (x, D) -> (n, n_terms); an index-dependent value "
            "goes into a data entry: put it into a data entry (data={'i': np.arange(T, dtype=np.float64)})")

    def __init__(self, name):
        self._name = name

    def __repr__(self):
        return self._name


def _is_tensor(v):
    import torch
    return isinstance(v, torch.Tensor)


class TV:
    """A traced (n,) + ids.shape float64 (or bool) value: ids holds the graph node of every element of a row.  base: the value this
    one is a VIEW of in torch (basic indexing, reshape / view, squeeze / unsqueeze) -- the tracer holds a copy of its ids, so a write
    through the view is refused, and so is the use of a view after its base was assigned to (torch would show the change)."""
    __array_ufunc__ = None          # ndarray <op> TV defers to TV's reflected method
    __hash__ = None

    def __init__(self, g, ids, is_input=False, base=None, term=False, batch=True):
        # term: a last axis over the observations follows the axes of ids (symbolic, like the particle axis: every node is then a
        # value per (particle, term)); batch False: a data value, without the particle axis
        ids = np.asarray(ids, dtype=np.int64)
        self.term, self.batch = bool(term), bool(batch)
        if ids.size > MAX_WIDTH:
            _refuse(f"an intermediate of {ids.size} columns", f"at most {MAX_WIDTH} values per particle live in registers", _POINT_TO_DATA)
        g.widest = max(g.widest, int(ids.size))
        self.g, self._ids, self.is_input, self._version = g, ids, is_input, 0
        self._base = None if base is None else (base if base._base is None else base._base)       # the root of a chain of views
        self._base_version = None if base is None else self._base._version

    @property
    def ids(self):
        if self._base is not None and self._base._version != self._base_version:
            _refuse("use of a view after its base was assigned to", "torch would show the new values through the view; the tracer "
                    "holds the old ones", "take the view (y[:, j], y.reshape(...)) after the assignment, or .clone() it before")
        return self._ids

    def _new(self, ids, **kw):
        """A value of this one's kind (term axis, particle axis) with other nodes."""
        return TV(self.g, ids, term=self.term, batch=self.batch, **kw)

    # ---- what a tensor tells about itself
    @property
    def shape(self):
        return ((_BATCH,) if self.batch else ()) + tuple(int(s) for s in self.ids.shape) + ((self.g.term_extent,) if self.term else ())

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return int(self.batch) + self.ids.ndim + int(self.term)

    ndim = property(dim)

    @property
    def dtype(self):
        import torch
        return torch.bool if self._bool() else torch.float64

    @property
    def device(self):
        import torch
        return torch.device("cpu")

    def _bool(self):
        flat = self.ids.ravel()
        return flat.size > 0 and all(i >= 0 and self.g.is_bool(int(i)) for i in flat)

    def __len__(self):
        (_BATCH if self.batch else self.g.term_extent)._no()

    def __iter__(self):
        _refuse("iteration over x", "it walks the particle axis", "index columns: x[:, j]")

    def __bool__(self):
        _refuse("bool() of a traced value (`if`, `while`, `and`, `or`, `assert` on it)", "data-dependent Python control flow takes one "
                "branch for all particles", "torch.where(condition, a, b)")

    def _scalar(self, *a, **k):
        _refuse("float() / int() / .item() / .tolist() / .numpy() of a traced value", "the value exists only on the device, per particle",
                "keep it a tensor expression")
    __float__ = __int__ = __index__ = item = tolist = numpy = _scalar

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        _refuse(f"x.{name}", "it is outside the supported operation list", "see the list in DESIGN.md section 11; anything else: a "
                "hand-written HipCallbacks source")

    # ---- dtype and placement
    def _dtype_refused(self, what):
        _refuse(what, "traced callbacks are float64 throughout", "drop the conversion (float32 is out of scope)")

    def double(self):
        return self

    def float(self):
        self._dtype_refused("x.float()")

    def half(self):
        self._dtype_refused("x.half()")

    def bfloat16(self):
        self._dtype_refused("x.bfloat16()")

    def int(self):
        self._dtype_refused("x.int()")

    def long(self):
        self._dtype_refused("x.long()")

    def to(self, *args, **kwargs):
        import torch
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.dtype) and a != torch.float64:
                self._dtype_refused(f"x.to({a})")
        return self

    type = to

    def cpu(self):
        return self

    cuda = contiguous = detach = cpu

    def clone(self, *a, **k):
        return self._new(self.ids.copy())

    # ---- columns
    def _key(self, key, what):
        if not isinstance(key, tuple):
            key = (key,)
        if not key or not (key[0] is Ellipsis or (isinstance(key[0], slice) and key[0] == slice(None))):
            _refuse(f"{what} with first index {key[0] if key else key!r}", "the first index selects particles; it must be the full slice",
                    "x[:, j], x[:, a:b], x[..., j]")
        rest = []
        for k in key[1:]:
            if isinstance(k, TV):
                _refuse(f"{what} with a traced index or mask", "which column is read would depend on the data", "torch.where")
            if _is_tensor(k):
                k = k.detach().cpu().numpy()
            if isinstance(k, np.ndarray) and k.dtype == bool or isinstance(k, (list, tuple)) and any(isinstance(e, bool) for e in k):
                k = np.asarray(k, dtype=bool)
            rest.append(k)
        n_idx = sum(1 for k in rest if k is not None and k is not Ellipsis)
        # a value with a term axis: an index behind the static axes, or the last one of a key with `...`, meets the term axis
        if self.term and rest and (n_idx > self.ids.ndim or key[0] is Ellipsis or any(k is Ellipsis for k in rest)):
            if not (isinstance(rest[-1], slice) and rest[-1] == slice(None)):
                _refuse(f"{what}: an index, slice, mask or new axis at the term axis", _OWNS_THE_SUM + "; every term is computed alone, "
                        "and the term axis stays the last one", _RETURN_TERMS)
            rest, n_idx = rest[:-1], n_idx - 1
        if n_idx > self.ids.ndim:
            _refuse(what, f"{n_idx} column indices for a value with {self.ids.ndim} trailing axes: the last would index particles",
                    "x[:, j]")
        return (Ellipsis,) + tuple(rest) if key[0] is Ellipsis else tuple(rest)

    def __getitem__(self, key):
        if not self.batch:              # a data value: (T,) -> (1, T) aligns as (T,) does; anything else would index the observations
            ks = key if isinstance(key, tuple) else (key,)
            if all(k is None or k is Ellipsis or (isinstance(k, slice) and k == slice(None)) for k in ks):
                return self
            _refuse("an index, slice or mask into a data value", _OWNS_THE_SUM + " and hands the function one observation at a time",
                    "D[name][j] with constant integers on the entry itself (an element), or " + _RETURN_TERMS)
        try:
            k = self._key(key, "x[...]")
            basic = all(e is None or e is Ellipsis or isinstance(e, (int, np.integer, slice)) for e in k)    # else torch copies
            return self._new(self.ids[k], base=self if basic else None)
        except IndexError as e:
            _refuse("x[...]", str(e), "an index inside the static trailing shape")

    def __setitem__(self, key, value):
        if self.term or not self.batch:
            _refuse("y[...] = ... on a value with a term axis", "column assignment is traced for per-particle values only",
                    "build the value with torch.stack / torch.where")
        if self.is_input:
            _refuse("x[...] = ... on the input", "in-place change of the callback's input", "y = torch.empty_like(x) (or x.clone()) and "
                    "assign whole columns of y")
        if self._base is not None:
            _refuse("y[...] = ... on a view (a value made by indexing, reshape / view, squeeze / unsqueeze)", "torch writes through to "
                    + ("the callback's input: an in-place change of it" if self._base.is_input else "the value the view was taken from")
                    + ", which the tracer holds as a copy", "assign to the base itself: base[:, j] = ..." if not self._base.is_input else
                    "y = x.clone() (or torch.empty_like(x)) and assign whole columns of y")
        k = self._key(key, "y[...] = ...")
        ids = self.ids.copy()
        try:
            ids[k] = _lift(self.g, value, ids[k].shape)
        except (IndexError, ValueError) as e:
            _refuse("y[...] = ...", str(e), "assign whole columns: y[:, j] = ..., y[:, a:b] = ...")
        self._ids = ids
        self._version += 1

    def unsqueeze(self, dim):
        if not self.batch:
            if self.ids.ndim == 0 and ((self.term and dim in (0, -2)) or (not self.term and dim in (0, -1))):
                return self             # (T,) -> (1, T), () -> (1,): aligned against the trailing axes as before
            _refuse(f"unsqueeze({dim}) of a data value", "the term axis must stay the last axis", "D[name][None, :] or unsqueeze(0)")
        full = 1 + self.ids.ndim + int(self.term) + 1
        d = dim + full if dim < 0 else dim
        if d == 0:
            _refuse("unsqueeze(0)", "the particle axis must stay the leading axis", "unsqueeze(-1)")
        if self.term and d == full - 1:
            _refuse(f"unsqueeze({dim}) behind the term axis", "the term axis must stay the last axis", "unsqueeze(1)")
        return self._new(np.expand_dims(self.ids, d - 1), base=self)

    def squeeze(self, dim=None):
        if dim is None:
            _refuse("squeeze() without dim", "it would also drop a particle axis of extent 1", "squeeze(-1)")
        d = self._axis(dim, "squeeze")
        return self._new(np.squeeze(self.ids, d), base=self) if self.ids.shape[d] == 1 else self

    def reshape(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        if self.term or not self.batch:
            _refuse(f"reshape{tuple(shape)} of a value with a term axis", "the term axis is symbolic and stays the last axis",
                    "reshape the per-particle operands before they meet the data")
        if not shape or not (shape[0] is _BATCH or (shape[0] == -1 and -1 not in shape[1:] and
                                                    int(np.prod(shape[1:], dtype=np.int64)) == self.ids.size)):
            _refuse(f"reshape{tuple(shape)}", "it must keep the particle axis as the leading axis", "x.reshape(x.shape[0], ...) or "
                    "x.reshape(-1, k) with k the number of values per particle")
        try:
            return TV(self.g, self.ids.reshape(tuple(int(s) for s in shape[1:])), base=self)
        except ValueError as e:
            _refuse(f"reshape{tuple(shape)}", str(e), "a shape with as many values per particle")

    view = reshape

    def _axis(self, dim, what):
        full = int(self.batch) + self.ids.ndim + int(self.term)
        if not isinstance(dim, (int, np.integer)) or isinstance(dim, bool) or not -full <= dim < full:
            _refuse(f"{what}(dim={dim!r})", "not an axis of this value", "dim=1 or dim=-1")
        d = dim + full if dim < 0 else int(dim)
        if self.term and d == full - 1:
            _refuse(f"{what} along the term axis (dim={dim})", _OWNS_THE_SUM, _RETURN_TERMS)
        if d == 0:
            _refuse(f"{what} over dim 0", "the particle axis is symbolic: every particle is computed alone",
                    "dim=1 / dim=-1 (over the columns)")
        return d - 1

    # ---- arithmetic
    def _as_double(self):
        if not self._bool():
            return self
        one, zero = self.g.const(1.0), self.g.const(0.0)
        return self._new(_map(lambda c: self.g.add("where", c, one, zero), self.ids))

    def __neg__(self):
        return _unary("neg", self)

    def __pos__(self):
        return self

    def __abs__(self):
        return _unary("abs", self)

    def __invert__(self):
        return _logical_not(self)

    def _inplace(self, *a, **k):
        _refuse("in-place arithmetic (+=, -=, *=, /=, add_, mul_, ...)", "it would change " +
                ("the callback's input" if self.is_input else "a value other expressions may share"),
                "y = x + 1 (a new value); column assignment y[:, j] = ... on an empty_like / clone is supported")
    __iadd__ = __isub__ = __imul__ = __itruediv__ = __ipow__ = __imatmul__ = _inplace
    add_ = sub_ = mul_ = div_ = pow_ = clamp_ = exp_ = log_ = neg_ = abs_ = sqrt_ = fill_ = zero_ = copy_ = _inplace

    def __matmul__(self, other):
        return _matmul(self, other)

    def __rmatmul__(self, other):
        _refuse("A @ x", "the particle axis of x must stay the leading axis of the result", "x @ A.T")

    def __pow__(self, e):
        return _pow(self, e)

    def __rpow__(self, b):
        return _pow(b, self)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", str(func))
        h = _TORCH.get(name)
        if h is None:
            _refuse(f"torch.{name}", "it is outside the supported operation list", "see the list in DESIGN.md section 11; anything else: "
                    "a hand-written HipCallbacks source")
        return h(*args, **(kwargs or {}))


def _map(f, *ids):
    """f over broadcast id arrays, element by element in row-major order."""
    bs = np.broadcast_arrays(*ids)
    out = np.empty(bs[0].shape, dtype=np.int64)
    flat = out.reshape(-1)
    its = [b.reshape(-1) for b in bs]
    for k in range(flat.size):
        vs = [int(it[k]) for it in its]
        if min(vs) < 0:
            _refuse("a column of torch.empty_like(...) that was never assigned", "its value is undefined", "assign every column before use")
        flat[k] = f(*vs)
    return out


def _graph_of(*vals):
    for v in vals:
        if isinstance(v, TV):
            return v.g
        if isinstance(v, (list, tuple)):
            for e in v:
                if isinstance(e, TV):
                    return e.g
    raise TraceError("trace_callbacks: no traced value among the operands")


def _lift(g, v, tshape, term=False, ids=None):
    """The node ids of operand `v` against a traced operand of trailing shape `tshape`: a TV (same rank), a Python number, or a
    captured float64 constant of shape (), (k,), (1, k) ... aligned to the trailing axes.  term: the result has a term axis behind
    `tshape`; ids: v's nodes less the extent-1 axis that met it (_operands)."""
    if isinstance(v, TV):
        if v.g is not g:
            _refuse("an operand traced in another callback", "each callback is traced alone", "compute it inside this function")
        ids = v.ids if ids is None else ids
        if v.batch and ids.ndim != len(tshape):
            _refuse(f"broadcasting (n,{','.join(map(str, ids.shape))}) against (n,{','.join(map(str, tshape))})",
                    "it would align the particle axis with a column axis", "unsqueeze(-1) / x[:, j:j+1] on the narrower operand")
        return ids
    if isinstance(v, _Batch):
        v._no()
    if isinstance(v, (bool, int, float, np.floating, np.integer)):
        return np.asarray(g.const(float(v)), dtype=np.int64)
    if _is_tensor(v):
        import torch
        if v.dtype != torch.float64 and v.dim() > 0 or v.is_complex():
            _refuse(f"a captured {v.dtype} tensor", "traced callbacks are float64 throughout", "build the constant with dtype=torch.float64")
        v = v.detach().to("cpu", torch.float64).numpy()
    a = np.asarray(v)
    if a.dtype != np.float64 and a.ndim > 0 or a.dtype == object or a.dtype.kind not in "fiub":
        _refuse(f"a captured {a.dtype} array", "traced callbacks are float64 throughout", "build the constant with dtype=np.float64")
    a = a.astype(np.float64)
    if term and a.ndim:
        if a.shape[-1] != 1:
            _refuse(f"a captured array of shape {a.shape} against a value with a term axis", "its last axis would run along the "
                    "observations", "put it into a data entry (data={...}); constants per column take shape (k, 1)")
        a = a[..., 0]
    while a.ndim > len(tshape) and a.shape[0] == 1:
        a = a[0]
    if a.ndim > len(tshape):
        _refuse(f"a captured constant of shape {np.asarray(v).shape} against (n,{','.join(map(str, tshape))})",
                "its leading axis would align with the particle axis", "constants of shape (), (k,) or (1, k)")
    ids = np.vectorize(g.const, otypes=[np.int64])(a) if a.size else a.astype(np.int64)
    if a.ndim:
        g.captured.update(int(i) for i in ids.reshape(-1))         # equal values are one node, however often they are used
    if len(g.captured) > MAX_CONSTANTS:
        _refuse(f"more than {MAX_CONSTANTS} embedded constants", "every constant becomes a literal of the kernel", _POINT_TO_DATA)
    return ids


def _operands(*vals):
    """(graph, the broadcastable node ids of the operands, the kind of the result: term axis, particle axis)."""
    g = _graph_of(*vals)
    tvs = [v for v in vals if isinstance(v, TV)]
    term, batch = any(v.term for v in tvs), any(v.batch for v in tvs)

    def trailing(v):                    # a per-particle operand meets the term axis with a last axis of extent 1, which goes
        if not (term and v.batch and not v.term):
            return v.ids
        if v.ids.ndim == 0 or v.ids.shape[-1] != 1:
            _refuse(f"broadcasting (n,{','.join(map(str, v.ids.shape))}) against a term axis", "the term axis is the last axis of "
                    "the other operand: it meets a last axis of extent 1 or another term axis, as torch would align it",
                    "x[:, j:j+1] or unsqueeze(-1) on the per-particle operand")
        return v.ids[..., 0]
    mine = [trailing(v) if isinstance(v, TV) else None for v in vals]
    tshape = max((i.shape for v, i in zip(vals, mine) if isinstance(v, TV) and v.batch), key=len, default=())
    try:
        ids = [_lift(g, v, tshape, term, i) for v, i in zip(vals, mine)]
        np.broadcast_shapes(*[i.shape for i in ids])
    except ValueError as e:
        _refuse("broadcasting", str(e), "operands whose column axes match or are 1")
    return g, ids, {"term": term, "batch": batch}


def _dbl(g, v, ids):
    """Bool operands of arithmetic become 1.0 / 0.0 (torch's type promotion)."""
    if isinstance(v, TV) and v._bool():
        one, zero = g.const(1.0), g.const(0.0)
        return _map(lambda c: g.add("where", c, one, zero), ids)
    return ids


def _unary(op, a):
    a = a._as_double()
    return a._new(_map(lambda i: a.g.add(op, i), a.ids))


def _is_number(v):
    if isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool):
        return True
    return (_is_tensor(v) or isinstance(v, np.ndarray)) and v.ndim == 0 and (not _is_tensor(v) or not v.is_cuda)


def _binary(op, a, b, alpha=1, out=None, **kw):
    if out is not None or kw.get("rounding_mode") is not None:
        _refuse(f"torch.{op}(..., out= / rounding_mode=)", "only true elementwise results are traced", "the plain operator")
    if alpha != 1:
        b = b * alpha
    g, (ia, ib), kind = _operands(a, b)
    ia, ib = _dbl(g, a, ia), _dbl(g, b, ib)
    if op == "div" and _is_number(b):
        # torch-ROCm's device kernel for tensor / host scalar multiplies by the reciprocal
        inv = g.const(1.0 / float(b)) if float(b) != 0.0 else g.const(math.copysign(math.inf, float(b)))
        return TV(g, _map(lambda i: g.add("mul", i, inv), ia), **kind)
    return TV(g, _map(lambda i, j: g.add(op, i, j), ia, ib), **kind)


def _compare(op, a, b):
    g, (ia, ib), kind = _operands(a, b)
    return TV(g, _map(lambda i, j: g.add(op, i, j), _dbl(g, a, ia), _dbl(g, b, ib)), **kind)


def _need_bool(v, what):
    if not (isinstance(v, TV) and v._bool()):
        _refuse(what, "its operands must be results of comparisons", "compare first: (x > 0) & (x < 1)")


def _logical(op, a, b):
    _need_bool(a, f"logical_{op}")
    _need_bool(b, f"logical_{op}")
    g, (ia, ib), kind = _operands(a, b)
    return TV(g, _map(lambda i, j: g.add(op, i, j), ia, ib), **kind)


def _logical_not(a):
    _need_bool(a, "logical_not")
    return a._new(_map(lambda i: a.g.add("not", i), a.ids))


def _where3(c, a=None, b=None):
    if a is None or b is None:
        _refuse("torch.where(condition) with one argument", "it returns indices, whose number depends on the data",
                "torch.where(condition, a, b)")
    _need_bool(c, "torch.where")
    g, (ic, ia, ib), kind = _operands(c, a, b)
    return TV(g, _map(lambda k, i, j: g.add("where", k, i, j), ic, _dbl(g, a, ia), _dbl(g, b, ib)), **kind)


def _pow(a, e):
    """Exponents 2, 3, 0.5, -0.5, -1, -2 as torch's own pow kernel computes them; the rest through the device pow()."""
    if isinstance(a, TV) and _is_number(e):
        e = float(e)
        g = a.g
        one = g.const(1.0)
        if e == 0.0:
            return a._new(_map(lambda i: one, a.ids))
        forms = {1.0: lambda i: i, 2.0: lambda i: g.add("mul", i, i), 3.0: lambda i: g.add("mul", g.add("mul", i, i), i),
                 0.5: lambda i: g.add("sqrt", i), -0.5: lambda i: g.add("rsqrt", i), -1.0: lambda i: g.add("div", one, i),
                 -2.0: lambda i: g.add("div", one, g.add("mul", i, i))}
        if e in forms:
            return a._new(_map(forms[e], a._as_double().ids))
    g, (ia, ib), kind = _operands(a, e)
    return TV(g, _map(lambda i, j: g.add("pow", i, j), _dbl(g, a, ia), _dbl(g, e, ib)), **kind)


def _clamp(a, min=None, max=None, **kw):
    if min is None and max is None:
        _refuse("clamp() without bounds", "nothing to do", "clamp(min=..., max=...)")
    if min is not None:
        a = _binary("max", a, min)
    if max is not None:
        a = _binary("min", a, max)
    return a


def _fold(g, op, ids):
    """ids[0] op ids[1] op ... left to right."""
    acc = ids[0]
    for i in ids[1:]:
        acc = g.add(op, acc, i)
    return acc


def _reduce(kind, a, dim=None, keepdim=False, dtype=None, out=None, **kw):
    import torch
    if not isinstance(a, TV):
        _refuse(f"torch.{kind}", "its first operand is not the traced value", "reduce the traced tensor")
    if not a.batch:
        _refuse(f"{kind} of a data value", _OWNS_THE_SUM + ": a data value has no axis but the observations", _RETURN_TERMS)
    if dtype not in (None, torch.float64) or out is not None:
        _refuse(f"{kind}(dtype= / out=)", "traced callbacks are float64 throughout", "drop the argument")
    if "axis" in kw:
        dim = kw.pop("axis")
    if dim is None or (isinstance(dim, (tuple, list)) and len(dim) == 0):
        _refuse(f"{kind}() over all axes", "it would reduce over the particles", f"{kind}(dim=1)")
    a = a._as_double()
    g = a.g
    dims = sorted({a._axis(d, kind) for d in (dim if isinstance(dim, (tuple, list)) else (dim,))})
    if a.ids.size == 0 or any(a.ids.shape[d] == 0 for d in dims):
        _refuse(f"{kind} over no columns", "empty reduction", "reduce at least one column")
    rest = [d for d in range(a.ids.ndim) if d not in dims]
    moved = np.transpose(a.ids, rest + dims)
    lead = moved.shape[:len(rest)]
    rows = moved.reshape(int(np.prod(lead, dtype=np.int64)), -1)          # the reduced columns of an output, in column order
    if (rows < 0).any():
        _map(lambda i: i, rows)                                           # refuses the unassigned column
    k = rows.shape[1]

    def one(ids):
        ids = [int(i) for i in ids]
        if kind in ("sum", "mean"):
            s = _fold(g, "add", ids)
            return s if kind == "sum" else g.add("mul", s, g.const(1.0 / k))      # the device mean kernel scales by 1 / k
        if kind == "prod":
            return _fold(g, "mul", ids)
        if kind in ("amax", "amin"):
            return _fold(g, kind[1:], ids)
        # logsumexp as torch composes it: m = amax, 0 where |m| is infinite; log(sum exp(x - m)) + m
        m = _fold(g, "max", ids)
        m0 = g.add("where", g.add("eq", g.add("abs", m), g.const(math.inf)), g.const(0.0), m)
        return g.add("add", g.add("log", _fold(g, "add", [g.add("exp", g.add("sub", i, m0)) for i in ids])), m0)
    res = np.array([one(r) for r in rows], dtype=np.int64).reshape(lead)
    if keepdim:
        for d in dims:
            res = np.expand_dims(res, d)
    return TV(g, res, term=a.term)


def _cumsum(a, dim=None, **kw):
    if isinstance(a, TV) and (not a.batch or a.term):
        a._axis(dim if a.batch else -1, "cumsum")            # along the term axis: the library owns that sum
    _refuse("torch.cumsum", "it is outside the supported operation list", "see the list in DESIGN.md section 11; anything else: a "
            "hand-written HipCallbacks source")


def _const_matrix(g, A, what):
    if isinstance(A, TV):
        _refuse(what, "both operands are traced", "the second operand must be a captured constant matrix; an inner product of two "
                "traced rows is (a * b).sum(dim=1)")
    ids = _lift(g, A, (0, 0))
    if ids.ndim != 2:
        _refuse(what, f"the constant has shape {ids.shape}", "a 2-D float64 constant")
    return ids


def _matmul(x, A, transposed=False):
    """x (n, k) @ A (k, m): out[:, j] = ((x0 * A0j + x1 * A1j) + x2 * A2j) + ... -- products and sums in index order."""
    if not isinstance(x, TV):
        _refuse("A @ x", "the particle axis of x must stay the leading axis of the result", "x @ A.T")
    x = x._as_double()
    g = x.g
    if x.ids.ndim != 1 or x.term or not x.batch:
        _refuse("matmul", f"the traced operand must be (n, k), got {tuple(x.shape)}", "reshape to (n, k) first")
    if isinstance(A, (_Entry, _EntryT)):
        if isinstance(A, _EntryT) == bool(transposed):
            _refuse("x @ D[name]", "the rows of a design matrix are the observations: the result would have no term axis",
                    "x @ D[name].T, or torch.nn.functional.linear(x, D[name])")
        return (A.entry if isinstance(A, _EntryT) else A)._inner(x)
    a = _const_matrix(g, A, "matmul")
    if transposed:
        a = a.T
    if a.shape[0] != x.ids.shape[0]:
        _refuse("matmul", f"(n, {x.ids.shape[0]}) @ {a.shape}", "matching inner extents")
    _map(lambda i: i, x.ids)
    out = [_fold(g, "add", [g.add("mul", int(x.ids[i]), int(a[i, j])) for i in range(a.shape[0])]) for j in range(a.shape[1])]
    return TV(g, out)


def _linear(x, weight, bias=None):
    y = _matmul(x, weight, transposed=True)
    return y if bias is None else _binary("add", y, bias)


def _seq(tensors, what):
    if not isinstance(tensors, (list, tuple)) or not tensors:
        _refuse(what, "expected a list of tensors", f"{what}([a, b, ...], dim=1)")
    g = _graph_of(tensors)
    ref = next(t for t in tensors if isinstance(t, TV))
    if any(isinstance(t, TV) and (t.term != ref.term or not t.batch) for t in tensors):
        _refuse(what + " of values with and without a term axis", "their shapes differ", "broadcast first: a + 0.0 * b")
    return g, [_lift(g, t, ref.ids.shape, ref.term) if not isinstance(t, TV) else t._as_double().ids if t._bool() else t.ids
               for t in tensors], ref.term


def _stack(tensors, dim=0, out=None):
    g, ids, term = _seq(tensors, "torch.stack")
    full = 2 + ids[0].ndim + int(term)
    d = dim + full if dim < 0 else dim
    if d == 0 or not 0 <= d < full:
        _refuse(f"torch.stack(dim={dim})", "the particle axis must stay the leading axis", "torch.stack([...], dim=1) or dim=-1")
    if term and d == full - 1:
        _refuse(f"torch.stack(dim={dim}) behind the term axis", "the term axis must stay the last axis", "torch.stack([...], dim=1)")
    try:
        return TV(g, np.stack([np.broadcast_to(i, ids[0].shape) if i.ndim == 0 else i for i in ids], axis=d - 1), term=term)
    except ValueError as e:
        _refuse("torch.stack", str(e), "operands of one shape")


def _cat(tensors, dim=0, out=None, **kw):
    dim = kw.get("axis", dim)
    g, ids, term = _seq(tensors, "torch.cat")
    full = 1 + ids[0].ndim + int(term)
    d = dim + full if dim < 0 else dim
    if d == 0 or not 0 <= d < full:
        _refuse(f"torch.cat(dim={dim})", "it would join along the particle axis", "torch.cat([...], dim=1) or dim=-1")
    if term and d == full - 1:
        _refuse(f"torch.cat(dim={dim}) along the term axis", _OWNS_THE_SUM + ": the number of terms is the data's", "torch.cat([...], dim=1)")
    try:
        return TV(g, np.concatenate(ids, axis=d - 1), term=term)
    except ValueError as e:
        _refuse("torch.cat", str(e), "operands that agree in the other axes")


def _like(fill):
    def make(a, dtype=None, **kw):
        import torch
        if dtype not in (None, torch.float64):
            a._dtype_refused(f"*_like(dtype={dtype})")
        ids = np.full(a.ids.shape, _UNINIT if fill is None else a.g.const(fill), dtype=np.int64)
        return a._new(ids)
    return make


def _method(name):
    return lambda self, *a, **k: _TORCH[name](self, *a, **k)


def _sigmoid(a):
    # torch's device kernel: 1 / (1 + exp(-x))
    return _binary("div", 1.0, _binary("add", 1.0, _unary("exp", _unary("neg", a))))


_TORCH = {
    "neg": lambda a: _unary("neg", a), "negative": lambda a: _unary("neg", a), "abs": lambda a: _unary("abs", a),
    "absolute": lambda a: _unary("abs", a), "square": lambda a: _pow(a, 2.0), "reciprocal": lambda a: _pow(a, -1.0),
    "sigmoid": _sigmoid, "minimum": lambda a, b: _binary("min", a, b), "maximum": lambda a, b: _binary("max", a, b),
    "clamp": _clamp, "clip": _clamp, "where": _where3, "pow": _pow, "matmul": _matmul, "linear": _linear,
    "logical_and": lambda a, b: _logical("and", a, b), "logical_or": lambda a, b: _logical("or", a, b), "logical_not": _logical_not,
    "stack": _stack, "cat": _cat, "concat": _cat, "concatenate": _cat,
    "empty_like": _like(None), "zeros_like": _like(0.0), "ones_like": _like(1.0),
    "clone": lambda a, **k: a.clone(), "unsqueeze": lambda a, dim: a.unsqueeze(dim), "squeeze": lambda a, dim=None: a.squeeze(dim),
    "reshape": lambda a, *s: a.reshape(*s),
    "__rpow__": lambda a, b: _pow(b, a), "__pow__": _pow, "__matmul__": _matmul,
    "__rmatmul__": lambda a, b: _matmul(b, a), "cumsum": _cumsum,
}
for _n in _UNARY:
    if _n != "abs" and _n not in _QUANTILE:
        _TORCH[_n] = (lambda op: lambda a: _unary(op, a))(_n)
_TORCH["arctan"] = _TORCH["atan"]


def _quantile(op):
    def handler(a, out=None):
        if out is not None:
            _refuse(f"torch.{op}(..., out=)", "only true elementwise results are traced", f"torch.special.{op}(x)")
        f = sys._getframe(1)
        while f is not None:                         # Normal(...).icdf(u) arrives here as torch.erfinv(2 u - 1)
            if (os.sep + "torch" + os.sep + "distributions" + os.sep) in f.f_code.co_filename:
                _refuse("a torch.distributions object (icdf)", "its methods check and convert their argument as eager tensors, and "
                        "what they compute differs from one torch version to the next", "tempest_amd.Prior([tempest_amd.priors.Normal("
                        "mu, s), ...]).transform, or the transform written out: mu + s * torch.special.ndtri(u)")
            f = f.f_back
        return _unary(op, a)
    return handler


def _not_traced(name, instead):
    def handler(*a, **k):
        _refuse(name, "it is outside the supported operation list: of the normal distribution's functions the tracer has erf, erfc, "
                "torch.special.ndtri and torch.erfinv", instead)
    return handler


for _n in _QUANTILE:
    _TORCH[_n] = _TORCH["special_" + _n] = _quantile(_n)
_REFUSED = {"ndtr": "0.5 * torch.erfc(-x * 0.7071067811865476)",
            "log_ndtr": "torch.log(0.5 * torch.erfc(-x * 0.7071067811865476)) (it loses the far lower tail: keep x above -37)",
            "erfcinv": "-torch.special.ndtri(0.5 * y) * 0.7071067811865476"}
for _n, _instead in _REFUSED.items():
    _TORCH[_n] = _TORCH["special_" + _n] = _not_traced(f"torch.special.{_n}", _instead)
for _n, _alts in (("add", ("__add__", "__radd__")), ("mul", ("multiply", "__mul__", "__rmul__")), ("sub", ("subtract", "__sub__")),
                  ("div", ("divide", "true_divide", "__truediv__"))):
    for _a in (_n,) + _alts:
        _TORCH[_a] = (lambda op: lambda a, b, **k: _binary(op, a, b, **k))(_n)
_TORCH["__rsub__"] = _TORCH["rsub"] = lambda a, b, **k: _binary("sub", b, a, **k)



def _rdiv(a, b):
    """number / x through the operator: torch's Tensor.__rtruediv__ is x.reciprocal() * number, two roundings, on the host and on the
    device (torch.div(c, x) with a 0-d tensor c, and tensor / x, are true divisions)."""
    return _binary("mul", _pow(a, -1.0), b) if isinstance(a, TV) and _is_number(b) and not (_is_tensor(b) or isinstance(b, np.ndarray)) \
        else _binary("div", b, a)


_TORCH["__rtruediv__"] = _TORCH["__rdiv__"] = _rdiv
for _n in _COMPARE:
    for _a in (_n, f"__{_n}__") + {"gt": ("greater",), "lt": ("less",), "ge": ("greater_equal",), "le": ("less_equal",),
                                   "eq": (), "ne": ("not_equal",)}[_n]:
        _TORCH[_a] = (lambda op: lambda a, b: _compare(op, a, b))(_n)
for _n in ("sum", "mean", "prod", "amax", "amin", "logsumexp"):
    _TORCH[_n] = (lambda kind: lambda a, *args, **k: _reduce(kind, a, *args, **k))(_n)
_TORCH["__and__"] = _TORCH["bitwise_and"] = _TORCH["logical_and"]
_TORCH["__or__"] = _TORCH["bitwise_or"] = _TORCH["logical_or"]
_TORCH["__invert__"] = _TORCH["bitwise_not"] = _TORCH["logical_not"]

# the methods of a traced value: the same handlers
for _n in ("neg", "negative", "abs", "absolute", "square", "reciprocal", "sigmoid", "minimum", "maximum", "clamp", "clip", "where", "pow",
           "matmul", "logical_and", "logical_or", "logical_not", "add", "sub", "mul", "div", "subtract", "multiply", "divide",
           "true_divide", "sum", "mean", "prod", "amax", "amin", "logsumexp", "arctan", "gt", "lt", "ge", "le", "eq", "ne") \
        + tuple(n for n in _UNARY if n != "abs"):
    setattr(TV, _n, _method(_n))
for _n in ("add", "mul", "sub", "truediv", "rsub", "rtruediv", "gt", "lt", "ge", "le", "eq", "ne", "and", "or"):
    setattr(TV, f"__{_n}__", _method(f"__{_n}__"))
TV.cumsum = _method("cumsum")
for _n in _REFUSED:
    setattr(TV, _n, _method(_n))
TV.__radd__ = lambda self, o: _binary("add", o, self)
TV.__rmul__ = lambda self, o: _binary("mul", o, self)
TV.__rand__ = lambda self, o: _logical("and", o, self)
TV.__ror__ = lambda self, o: _logical("or", o, self)


# ------------------------------------------------------------------------------------------------------ data entries
class _Entry(TV):
    """D[name] under the tracer: a data entry has no particle axis and its elements are graph nodes.  A 1-D entry whose length is
    the term extent is a per-term value ("dterm": D.name[r]), so is a column D[name][:, j] of a 2-D entry with that many rows, and
    x @ D[name].T their inner product with the columns of x; constant integer indices read one element ("delem")."""

    def __init__(self, g, pos, name, shape, is_f64):
        self.g, self._pos, self._name, self._shape, self._f64 = g, pos, name, tuple(int(v) for v in shape), bool(is_f64)
        self.is_input, self._version, self._base, self._base_version, self._ids = False, 0, None, None, None
        self.term, self.batch = True, False

    def _node(self, op, *args, how):
        if not self._f64:
            _refuse(f"D[{self._name!r}], given as an integer or float32 array, in arithmetic", "the device table is float64 and the "
                    "eager function would compute in another type", f"give it as float64 (np.asarray(..., dtype=np.float64)), or "
                    f"cast it in the function: D[{self._name!r}].double()")
        self.g.reads.setdefault(self._name, set()).add(how)
        return self.g.add(op, self._pos, *args)

    def _per_term(self):
        return self.g.n_term is not None and self._shape[0] == self.g.n_term

    @property
    def ids(self):
        if self._ids is None:
            n = self._name
            if len(self._shape) == 2:
                _refuse(f"D[{n!r}], a 2-D entry, used whole", "its rows are observations and its columns are not an axis of the result",
                        f"a column D[{n!r}][:, j], an element D[{n!r}][i, j], or xs @ D[{n!r}].T")
            if not self._per_term():
                _refuse(f"D[{n!r}], a 1-D entry of length {self._shape[0]}, used whole", "only an entry as long as the term axis ("
                        f"{self.g.term_extent!r} = {self.g.n_term}) is a value per term" if self.g.n_term is not None else _NO_TERM_AXIS,
                        f"index it: D[{n!r}][j]")
            self._ids = np.asarray(self._node("dterm", -1, how="per-term"), dtype=np.int64)
        return self._ids

    @property
    def shape(self):
        return tuple(self.g.term_extent if k == 0 and self._per_term() else v for k, v in enumerate(self._shape))

    def dim(self):
        return len(self._shape)

    ndim = property(dim)

    @property
    def dtype(self):
        import torch
        return torch.float64

    def __len__(self):
        if self._per_term():
            self.g.term_extent._no()
        return self._shape[0]

    def double(self):
        return self if self._f64 else _Entry(self.g, self._pos, self._name, self._shape, True)

    def to(self, *args, **kwargs):
        import torch
        return self.double() if torch.float64 in list(args) + list(kwargs.values()) else TV.to(self, *args, **kwargs)

    def _index(self, k, axis):
        extent = self._shape[axis]
        if not -extent <= k < extent:
            _refuse(f"D[{self._name!r}][...] with index {k}", f"axis {axis} has extent {extent}", "an index inside the entry's shape")
        return int(k) % extent

    def __getitem__(self, key):
        n, ks = self._name, key if isinstance(key, tuple) else (key,)
        whole = slice(None)
        if any(isinstance(k, TV) or _is_tensor(k) or isinstance(k, (np.ndarray, list)) for k in ks):
            _refuse(f"D[{n!r}][...] with a traced index, an index array or a mask", "which element is read would depend on the data: "
                    "a traced index into a table is a gather", "constant integers D[name][j], or a per-term entry prepared on the host")
        is_int = [isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in ks]
        if all(is_int) and len(ks) == len(self._shape):
            i = self._index(ks[0], 0)
            j = self._index(ks[1], 1) if len(ks) == 2 else -1
            return TV(self.g, self._node("delem", i, j, how=f"element [{i}]" if j < 0 else f"element [{i}, {j}]"), batch=False)
        if len(self._shape) == 1 and all(k is None or k is Ellipsis or (isinstance(k, slice) and k == whole) for k in ks):
            self.ids
            return self
        if len(self._shape) == 2 and len(ks) == 2 and isinstance(ks[0], slice) and ks[0] == whole and is_int[1]:
            if not self._per_term():
                _refuse(f"D[{n!r}][:, j]", f"the entry has {self._shape[0]} rows, not one per term" if self.g.n_term is not None else
                        _NO_TERM_AXIS, f"elements D[{n!r}][i, j]")
            j = self._index(ks[1], 1)
            return TV(self.g, self._node("dterm", j, how=f"column {j}"), term=True, batch=False)
        _refuse(f"D[{n!r}][{', '.join(map(str, ks))}]: an index, slice or mask along the observations", _OWNS_THE_SUM + " and hands "
                "the function one observation at a time", f"the entry whole, a column D[{n!r}][:, j], or constant integers; "
                + _RETURN_TERMS)

    def unsqueeze(self, dim):
        if len(self._shape) == 1:
            return TV.unsqueeze(self, dim)
        self.ids

    @property
    def T(self):
        return _EntryT(self) if len(self._shape) == 2 else self

    mT = T

    def t(self):
        return self.T

    def transpose(self, a, b):
        return self.T if len(self._shape) == 2 and sorted((a % 2, b % 2)) == [0, 1] else self

    def _inner(self, x):
        """x (n, k) @ D[name].T, the entry (T, k): the per-term inner product, left to right in column order (_fold, as x @ A)."""
        n = self._name
        if len(self._shape) != 2 or not self._per_term():
            _refuse(f"x @ D[{n!r}].T", f"the entry has shape {self._shape}: it needs one row per term", "a 2-D entry (n_terms, k)")
        k = self._shape[1]
        if k > MAX_WIDTH or x.ids.shape[0] != k:
            _refuse(f"x @ D[{n!r}].T", f"(n, {x.ids.shape[0]}) against {k} columns (at most {MAX_WIDTH})", "matching inner extents")
        _map(lambda i: i, x.ids)
        g = self.g
        return TV(g, _fold(g, "add", [g.add("mul", int(x.ids[i]), self._node("dterm", i, how=f"column {i}")) for i in range(k)]), term=True)


class _EntryT:
    """D[name].T of a 2-D entry: the second operand of x @ D[name].T, and nothing else."""
    __array_ufunc__ = None

    def __init__(self, entry):
        self.entry = entry

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        _refuse(f"D[{self.entry._name!r}].T.{name}", "the transpose of a design matrix is traced as the operand of a product only",
                f"xs @ D[{self.entry._name!r}].T")


class _Data(dict):
    def __missing__(self, name):
        _refuse(f"D[{name!r}]", "no such data entry", f"one of {sorted(self)}")


def _wants_data(fn):
    """prior_transform and derived get D if and only if they accept a second positional parameter."""
    import inspect
    try:
        ps = list(inspect.signature(fn).parameters.values())
    except (TypeError, ValueError):
        return False
    return sum(p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) for p in ps) >= 2


# ------------------------------------------------------------------------------------------------------ noise
MAX_DRAW = 2 ** 31              # k of g.normal(k) / g.uniform(k): the device takes it as an int


def _draw_index(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < MAX_DRAW:
        return None
    return int(k)


class _NoiseArg:
    """The g of replicate(x, D, g) under the tracer: g.normal(k) / g.uniform(k) are leaf nodes, one per distinct (kind, k), each a
    value per (particle, r) -- shape (n, n_replicate)."""

    def __init__(self, g):
        self._g = g

    def _draw(self, kind, k):
        i = _draw_index(k)
        if i is None:
            _refuse(f"g.{kind}({k!r})", "the index of a draw is a constant of the emitted code: a Python int with 0 <= k < 2^31 (the "
                    "draw belongs to (seed, row, r, k); a traced value, a float or a negative number names none)",
                    f"g.{kind}(0), g.{kind}(1), ...: one constant int per independent draw")
        return TV(self._g, self._g.add("noise_" + kind, i), term=True)

    def normal(self, k):
        return self._draw("normal", k)

    def uniform(self, k):
        return self._draw("uniform", k)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        _refuse(f"g.{name}", "the noise object has g.normal(k) and g.uniform(k) and nothing else", "compose the law from them: a "
                "Bernoulli is torch.where(g.uniform(k) < p, 1.0, 0.0)")


class Noise:
    """The host twin of the device's `tphu_noise`: Noise(seed, items, n_replicate).normal(k) / .uniform(k) are (len(items),
    n_replicate) float64 tensors (on `device`; default: the CPU) whose element [i, r] is the draw g.normal(k) / g.uniform(k) the
    device hands replicate(x, r, g) for the row of index items[i] in the x that cb.replicated(x, w, seed=seed) was given.  Philox4x32-10
    with key = seed, counter (item = the row's index, draw = k >> 1, tick = r, tag = 10 for normals, 11 for uniforms), lane k & 1 of
    the pair.

    The uniforms are 53-bit integers scaled by 2^-53: they EQUAL the device's bits.  The normals are Box-Muller on the same two
    uniforms, r = sqrt(-2 log u1), angle 2 pi u2, with NumPy's log / cos / sin where the device has its own lean versions: they agree
    with the device's to rounding, not to the bit.  A function that thresholds a normal (g.normal(k) > c) can therefore differ
    from the device at a tie; one that thresholds a uniform cannot.  The same k asked twice is the same tensor."""

    def __init__(self, seed, items, n_replicate, device=None):
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"Noise: seed must be an int in [0, 2^64), got {seed!r}")
        if isinstance(n_replicate, bool) or not isinstance(n_replicate, (int, np.integer)) or not 0 < int(n_replicate) < 2 ** 31:
            raise ValueError(f"Noise: n_replicate must be an int in (0, 2^31), got {n_replicate!r}")
        items = np.asarray(items)
        if items.ndim != 1 or items.dtype.kind not in "iu" or (items.size and (int(items.min()) < 0 or int(items.max()) >= 2 ** 32)):
            raise ValueError("Noise: items must be a 1-D array of row indices in [0, 2^32)")
        self.seed, self.n_replicate, self.device = int(seed), int(n_replicate), device
        self.items = items.astype(np.uint64)
        self._pairs, self._out = {}, {}

    def _get(self, kind, k):
        import torch
        from ._philox_host import normal_pair, uniform_pair
        from .hipcallbacks import REPLICATE_TAGS
        i = _draw_index(k)
        if i is None:
            raise ValueError(f"Noise.{kind}: k must be an int with 0 <= k < 2^31, got {k!r}")
        if (kind, i) not in self._out:
            if (kind, i >> 1) not in self._pairs:
                pair, tag = (normal_pair, REPLICATE_TAGS[0]) if kind == "normal" else (uniform_pair, REPLICATE_TAGS[1])
                self._pairs[(kind, i >> 1)] = pair(self.seed, self.items[:, None], i >> 1, np.arange(self.n_replicate, dtype=np.uint64)[None, :], tag)
            t = torch.from_numpy(np.ascontiguousarray(self._pairs[(kind, i >> 1)][i & 1]))
            self._out[(kind, i)] = t if self.device is None else t.to(self.device)
        return self._out[(kind, i)]

    def normal(self, k):
        return self._get("normal", k)

    def uniform(self, k):
        return self._get("uniform", k)


# ------------------------------------------------------------------------------------------------------ tracing
def _defined_at(fn):
    code = getattr(fn, "__code__", None)
    if code is None:
        return "<unknown>"
    return f"{code.co_filename}:{code.co_firstlineno}: {linecache.getline(code.co_filename, code.co_firstlineno).strip()}"


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
    x = TV(g, [g.add("in", j) for j in range(n_in)], is_input=True)
    if data is not None and (pass_data is None or pass_data):
        D = _Data((nm, _Entry(g, pos, nm, *data[1][nm])) for pos, (nm, _) in enumerate(data[0]))
        if noise:
            y = _call(fn, x, D, _NoiseArg(g))
        elif yarg:
            y = _call(fn, x, TV(g, g.add("yarg"), term=True), D)
        else:
            y = _call(fn, x, D)
    else:
        y = _call(fn, x)
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


def emit_source(graphs, tables=None):
    """The HipCallbacks source for {"prior_transform": Graph, "log_likelihood" | "log_likelihood_term": Graph[, "predict": Graph]
    [, "derived": Graph][, "replicate": Graph[, "discrepancy": Graph]]}.  tables: the data entries -- every signature then carries
    `const tphu_data& D`, as hand-written ones do.  A draw of replicate is `g.normal(k)` / `g.uniform(k)`, called once per distinct
    (kind, k); discrepancy uses its `y` directly."""
    D = "" if tables is None else ", const tphu_data& D"
    parts = ["// emitted by tempest_amd.trace_callbacks (DESIGN.md section 11): values live in registers, one statement per graph node"]
    if any(g.nodes[i][0] in _QUANTILE for g in graphs.values() for i in g.live()):
        parts.insert(0, quantile_header().rstrip("\n"))          # pasted, not #included: build_plugin hashes the text
    names = ["prior_transform", "log_likelihood_term" if "log_likelihood_term" in graphs else "log_likelihood"]
    for name in names + [n for n in ("predict", "derived", "replicate", "discrepancy") if n in graphs]:
        signature, arg, store = _EMITTED[name]
        parts.append(emit(graphs[name], f"__device__ {signature}{D})", arg, store))
    return "\n".join(parts) + "\n"


def _returned(k, t):
    return f"return {t};"


# graph name -> (signature up to the data argument, input name, the statement that stores output k)
_EMITTED = {
    "prior_transform": ("void prior_transform(const double* u, double* x", "u", lambda k, t: f"x[{k}] = {t};"),
    "log_likelihood_term": ("double log_likelihood_term(const double* x, int64_t r", "x", _returned),
    "log_likelihood": ("double log_likelihood(const double* x", "x", _returned),
    "predict": ("double predict(const double* x, int64_t r", "x", _returned),
    "derived": ("void derived(const double* x, double* out", "x", lambda k, t: f"out[{k}] = {t};"),
    "replicate": ("double replicate(const double* x, int64_t r, const tphu_noise& g", "x", _returned),
    "discrepancy": ("double discrepancy(const double* x, int64_t r, double y", "x", _returned),
}


def probe_batch(n_dim, rows=PROBE_ROWS, seed=PROBE_SEED):
    """(rows, n_dim) uniforms of the package's Philox host twin: item = row, draw = column."""
    from ._philox_host import philox4x32
    item, draw = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(n_dim, dtype=np.uint64), indexing="ij")
    zero = np.zeros_like(item)
    r = philox4x32(item, draw, zero, zero + np.uint64(_PROBE_TAG), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    k = ((r[0] >> np.uint64(5)) << np.uint64(26)) | (r[1] >> np.uint64(6))
    return k.astype(np.float64) * 2.0 ** -53


def _ulps(a, b):
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    ka, kb = key(a), key(b)
    far = (ka < 0) != (kb < 0)
    with np.errstate(over="ignore"):
        d = np.abs(ka - kb).astype(np.float64)
    return np.where(far, np.abs(ka.astype(np.float64) - kb.astype(np.float64)), d)


def compare(eager, traced):
    """(largest |difference|, largest difference in ulps, non-finite patterns agree, within SQRTEPS (1 + |eager|)) of two arrays."""
    e, t = np.asarray(eager, dtype=np.float64), np.asarray(traced, dtype=np.float64)
    if e.shape != t.shape:
        return math.inf, math.inf, False, False
    same = bool(np.array_equal(np.isnan(e), np.isnan(t)) and np.array_equal(np.isposinf(e), np.isposinf(t))
                and np.array_equal(np.isneginf(e), np.isneginf(t)))
    fin = np.isfinite(e) & np.isfinite(t)
    if not fin.any():
        return 0.0, 0.0, same, True
    d = np.abs(e[fin] - t[fin])
    return float(d.max()), float(_ulps(e[fin], t[fin]).max()), same, bool(np.all(d <= SQRTEPS * (1.0 + np.abs(e[fin]))))


def _seq_sum_last(a):
    """The sum along the last axis, sequentially from +0.0 (np.cumsum adds in order)."""
    return np.cumsum(np.concatenate([np.zeros(a.shape[:-1] + (1,)), a], axis=-1), axis=-1)[..., -1]


def layered_sum(terms, chunk, block):
    """The (n, T) terms summed in the order every term-form kernel follows (hipcallbacks.SUM_LAYOUT): chunks of
    `chunk` consecutive terms added in order, blocks of `block` consecutive chunk sums added in order, the block sums added in order;
    every level starts from +0.0."""
    t = np.asarray(terms, dtype=np.float64)
    for width in (chunk, block):
        n, k = t.shape
        pad = np.zeros((n, -(-k // width) * width))
        pad[:, :k] = t
        t = _seq_sum_last(pad.reshape(n, -1, width))
    return _seq_sum_last(t)


def _eager(report, name, dev, run):
    """run(dev), the eager side of the probe where the compiled code runs; run("cpu") without a device (dev None) or where the
    function's constants were captured on the host, and that alone.  report["eager_on"][name] says which."""
    if dev is not None:
        try:
            report["eager_on"][name] = "device"
            return run(dev)
        except RuntimeError as e:
            if "Expected all tensors to be on the same device" not in str(e):
                raise
    report["eager_on"][name] = "cpu"
    return run("cpu")


def _probe_replicate(cb, graphs, data, x, on_device, report, replicate, discrepancy, D_on, chunks):
    """The (name, eager, traced) pairs of replicate and discrepancy (see `probe`)."""
    import torch
    from .hipcallbacks import SUM_LAYOUT
    R = cb.n_replicate
    disc = discrepancy is not None and "discrepancy" in graphs
    obs = data[cb.observed] if disc else None

    def eager_on(dev, xs, items):
        """(eager y_rep (n, R)[, eager T (n, 2)]) on `dev`."""
        D, g, xt = D_on(dev), Noise(PROBE_SEED, items, R, device=dev), torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
        y = torch.as_tensor(replicate(xt, D, g))
        out = [y.detach().cpu().numpy().astype(np.float64)]
        if disc:
            yo = D[cb.observed][None, :].expand(len(xs), R)
            ts = [torch.as_tensor(discrepancy(xt, yy, D)).detach().cpu().numpy() for yy in (yo, y.to(torch.float64))]
            out.append(np.stack([layered_sum(t, *SUM_LAYOUT) if t.shape == (len(xs), R) else np.full(len(xs), np.nan) for t in ts], axis=1))
        return out

    def eager(xs, items):
        return _eager(report, "replicate", (cb.device or "cuda") if on_device else None, lambda dev: eager_on(dev, xs, items))

    ey, et, ty, tt = [], [], [], []
    if on_device:                                    # at most 8 rows, each alone with weight 1: item 0, mean = replicate exactly
        for i in range(min(8, len(x))):
            got = cb.replicated(x[i:i + 1], np.ones(1), quantiles=(0.5,), seed=PROBE_SEED)
            e = eager(x[i:i + 1], np.zeros(1, dtype=np.int64))
            ey.append(e[0])
            ty.append(np.asarray(got["mean"], dtype=np.float64)[None, :])
            if disc:
                et.append(e[1])
                tt.append(np.array([[got["t_obs_mean"], got["t_rep_mean"]]], dtype=np.float64))
    else:
        for c in chunks(R):
            items = np.arange(c.start, c.stop, dtype=np.int64)
            e = eager(x[c], items)
            y = replay(graphs["replicate"], x[c], data, noise=Noise(PROBE_SEED, items, R))
            ey.append(e[0])
            ty.append(y)
            if disc:
                et.append(e[1])
                tt.append(np.stack([layered_sum(replay(graphs["discrepancy"], x[c], data, y=yy), *SUM_LAYOUT) for yy in (obs, y)], axis=1))
    ok = all(a.shape == t.shape for a, t in zip(ey, ty))                                         # a wrong shape fails the comparison
    pairs = [("replicate", np.concatenate(ey) if ok else np.full(1, np.nan), np.concatenate(ty))]
    if disc:
        pairs.append(("discrepancy", np.concatenate(et), np.concatenate(tt)))
    return pairs


def probe(cb, prior_transform, log_likelihood, derived=None, predict=None, replicate=None, discrepancy=None):
    """Compare the eager callables with the compiled plugin `cb` (with a device) or with the replay of its graphs (without) on the
    probe batch; returns the report, raises TraceError (with .source) where they disagree.  With data the eager functions get the
    float64 tensors the device tables hold; a term function's eager columns are summed by `layered_sum` and held against
    cb.log_likelihood (the replayed terms summed alike, without a device), in chunks of rows so that nothing larger than 2^22
    doubles is formed; predict is checked through cb.predictive with one row of weight 1, which returns predict(x, .) exactly.
    replicate and discrepancy are checked through cb.replicated(x_i, [1.0], seed=PROBE_SEED) in the same way, at most 8 rows: "mean"
    is replicate(x_i, r, g) at item 0 exactly, "t_obs_mean" / "t_rep_mean" the layered sums of discrepancy at the observed and at
    the replicated values; the eager functions get Noise(PROBE_SEED, [0], n_replicate).  Without a device the replay runs on
    Noise(PROBE_SEED, the rows' indices, n_replicate), and so does the eager side.  The normals of Noise agree with the device's to
    rounding only, which the tolerance absorbs; a replicate that thresholds a NORMAL could flip an element at a tie and fail the
    probe on a correct trace (thresholding a uniform cannot: those bits are equal) -- the rule is not widened for it."""
    import torch
    from .hipcallbacks import SUM_LAYOUT
    graphs, d = cb.trace_graphs, cb.n_dim
    data = dict(cb._host) if cb.tables is not None else None
    term = "log_likelihood_term" in graphs
    widest = max(cb.n_terms if term else 1, cb.n_predict if "predict" in graphs else 1, cb.n_replicate if "replicate" in graphs else 1)
    rows = PROBE_ROWS if widest == 1 and not term else max(1, min(PROBE_ROWS, 2 ** 22 // widest))
    u = probe_batch(d, rows)
    on_device = torch.cuda.is_available()
    report = {"rows": rows, "seed": PROBE_SEED, "against": "compiled plugin on the device" if on_device else
              "replay on the CPU (no device present: the compiled code was NOT run)"}

    report["eager_on"] = {}
    tensors = {}

    def D_on(dev):
        if dev not in tensors:
            tensors[dev] = {k: torch.from_numpy(v).to(dev) for k, v in data.items()}
        return tensors[dev]

    def eager(name, fn, a, with_data=False):
        def run(dev):
            y = fn(torch.from_numpy(a).to(dev), *((D_on(dev),) if with_data else ()))
            return (torch.as_tensor(y) if dev == "cpu" else y).detach().cpu().numpy()
        return _eager(report, name, (cb.device or "cuda") if on_device else None, run)

    def traced(name, a):
        if on_device:
            return np.asarray(getattr(cb, name)(a))
        return replay(graphs[name], a, data)

    def chunks(n_cols):
        step = max(1, 2 ** 22 // max(1, n_cols))
        return [slice(i, min(rows, i + step)) for i in range(0, rows, step)]

    def summed(terms, n):
        terms = np.asarray(terms)
        return layered_sum(terms, *SUM_LAYOUT) if terms.shape == (n, cb.n_terms) else np.full(n, np.nan)      # a wrong shape fails below
    has = data is not None
    x = eager("prior_transform", prior_transform, u, has and _wants_data(prior_transform))
    pairs = [("prior_transform", x, traced("prior_transform", u))]
    if x.shape == u.shape:
        if term:
            e = np.concatenate([summed(eager("log_likelihood", log_likelihood, x[c], True), len(x[c])) for c in chunks(cb.n_terms)])
            t = traced("log_likelihood", x) if on_device else np.concatenate(
                [layered_sum(replay(graphs["log_likelihood_term"], x[c], data), *SUM_LAYOUT) for c in chunks(cb.n_terms)])
            pairs.append(("log_likelihood", e, t))
        else:
            pairs.append(("log_likelihood", eager("log_likelihood", log_likelihood, x, has), traced("log_likelihood", x)))
        if predict is not None and "predict" in graphs:
            if on_device:                                # at most 8 rows, each alone with weight 1: mean = predict exactly
                xs = x[:8]
                t = np.stack([cb.predictive(xs[i:i + 1], np.ones(1), quantiles=(0.5,))["mean"] for i in range(len(xs))])
            else:
                xs = x
                t = np.concatenate([replay(graphs["predict"], x[c], data) for c in chunks(cb.n_predict)])
            e = np.concatenate([eager("predict", predict, xs[c], True) for c in chunks(cb.n_predict) if len(xs[c])])
            pairs.append(("predict", e, t))
        if replicate is not None and "replicate" in graphs:
            pairs += _probe_replicate(cb, graphs, data, x, on_device, report, replicate, discrepancy, D_on, chunks)
        if derived is not None:
            e = eager("derived", derived, x, has and _wants_data(derived))
            pairs.append(("derived", e, traced("derived", x).reshape(e.shape) if e.size == x.shape[0] * cb.n_derived else None))
    bad = []
    for name, e, t in pairs:
        mx, ul, same, ok = compare(e, t) if t is not None else (math.inf, math.inf, False, False)
        report[name] = {"max_abs_diff": mx, "max_ulps": ul, "nonfinite_agree": same}
        if not same:
            bad.append(f"{name}: the non-finite values (NaN, +inf, -inf) fall on other rows than the eager function's")
        elif not ok:
            bad.append(f"{name}: differs from the eager function by up to {mx:.3g} ({ul:.3g} ulp), beyond SQRTEPS (1 + |eager|)")
    if bad:
        err = TraceError("trace_callbacks: the probe found the traced code wrong on " + report["against"] + ":\n  " + "\n  ".join(bad)
                         + "\n  (a function whose Python control flow depends on values the tracer cannot see? the emitted text is in "
                         "this error's .source)")
        err.source, err.report = cb.source, report
        raise err
    return report


def _extent(v, what, host):
    """n_terms / n_predict: the name of a data entry (its length, or its rows), or an int that some entry has as that extent."""
    from .hipcallbacks import _extent as extent
    if host is None:
        raise ValueError(f"trace_callbacks: {what}= goes with data= (the term and predict functions read the observations from D)")
    return extent(v, what, host, "trace_callbacks", of_an_entry=True)


def _is_f64(a):
    if _is_tensor(a):
        import torch
        return a.dtype == torch.float64
    return np.asarray(a).dtype == np.float64


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
    as in HipCallbacks.  A 1-D entry as long as the term axis is a value per term, used whole; a 2-D entry (T, k) gives columns
    D[name][:, j] and xs @ D[name].T; constant integer indices read an element of any entry.

    replicate= (x, D, g) -> (n, n_replicate) with n_replicate= (as n_predict=) becomes the source's replicate(): one replicated
    observation per column, its noise from g.normal(k) / g.uniform(k) -- k a constant Python int in [0, 2^31), each call a value per
    (row, column), the draw tphu_noise::normal(k) / uniform(k) of (seed, row, r) on the device, the same k the same value.
    observed= names the 1-D entry the replicates are compared with (PIT), as in HipCallbacks; discrepancy= (x, y, D) -> (n,
    n_replicate), y (n, n_replicate) the observed row broadcast or the replicated matrix, becomes the source's discrepancy(): the
    terms of the statistic, summed by the library in the term order -- no .sum().  replicate= needs data= and n_replicate=,
    discrepancy= needs replicate= and observed=, observed= needs replicate=.  Neither may reduce or index along the replicate axis
    or return a bool (torch.where(c, 1.0, 0.0)).  `Noise` is g on the host; cb.trace_report["draws"] lists the k that are drawn."""
    from .hipcallbacks import HipCallbacks, _table_spec
    if not isinstance(n_dim, (int, np.integer)) or isinstance(n_dim, bool) or n_dim <= 0:
        raise ValueError(f"n_dim must be a positive int, got {n_dim!r}")
    n_dim = int(n_dim)
    if hipcallbacks_kwargs.get("n_derived"):
        raise ValueError("trace_callbacks: n_derived= belongs to hand-written sources (here it is the width of what derived returns)")
    if n_dim > MAX_WIDTH:
        raise TraceError(f"trace_callbacks: n_dim = {n_dim} is wider than {MAX_WIDTH} columns; {_POINT_TO_DATA}")
    tables, host = (None, None) if data is None else _table_spec(data)
    spec = None if data is None else (tables, {k: (host[k].shape, _is_f64(data[k])) for k, _ in tables})
    if predict is None and n_predict is not None:
        raise ValueError("trace_callbacks: n_predict= goes with predict= (a function (x, D) -> (n, n_predict))")
    if predict is not None and data is None:
        raise ValueError("trace_callbacks: predict= without data= is not traced (every column would be an expression of its own): "
                         "give what depends on the index as a data entry and n_predict= its name")
    if predict is not None and n_predict is None:
        raise ValueError("trace_callbacks: predict= needs n_predict= (an int, or the name of a data entry)")
    if pointwise and n_terms is None:
        raise ValueError("trace_callbacks: pointwise=True goes with n_terms= (a term function)")
    if replicate is None and n_replicate is not None:
        raise ValueError("trace_callbacks: n_replicate= goes with replicate= (a function (x, D, g) -> (n, n_replicate))")
    if replicate is None and discrepancy is not None:
        raise ValueError("trace_callbacks: discrepancy= goes with replicate= (and n_replicate=, observed=)")
    if replicate is None and observed is not None:
        raise ValueError("trace_callbacks: observed= goes with replicate= (and n_replicate=)")
    if replicate is not None and data is None:
        raise ValueError("trace_callbacks: replicate= without data= is not traced (every column would be an expression of its own): "
                         "give what depends on the index as a data entry and n_replicate= its name")
    if replicate is not None and n_replicate is None:
        raise ValueError("trace_callbacks: replicate= needs n_replicate= (an int, or the name of a data entry)")
    if discrepancy is not None and observed is None:
        raise ValueError("trace_callbacks: discrepancy= needs observed= (the name of the data entry it is compared on)")
    wants = {"prior_transform": data is not None and _wants_data(prior_transform), "derived": data is not None and _wants_data(derived)}
    graphs = {"prior_transform": trace_function(prior_transform, n_dim, n_dim, "prior_transform", spec, pass_data=wants["prior_transform"])}
    if n_terms is not None:
        graphs["log_likelihood_term"] = trace_function(log_likelihood, n_dim, None, "log_likelihood_term", spec,
                                                       (_extent(n_terms, "n_terms", host), "n_terms"))
    else:
        graphs["log_likelihood"] = trace_function(log_likelihood, n_dim, (), "log_likelihood", spec)
    if predict is not None:
        graphs["predict"] = trace_function(predict, n_dim, None, "predict", spec, (_extent(n_predict, "n_predict", host), "n_predict"))
    if derived is not None:
        graphs["derived"] = trace_function(derived, n_dim, None, "derived", spec, pass_data=wants["derived"])
    if replicate is not None:
        extent = (_extent(n_replicate, "n_replicate", host), "n_replicate")
        graphs["replicate"] = trace_function(replicate, n_dim, None, "replicate", spec, extent, noise=True)
        if discrepancy is not None:
            graphs["discrepancy"] = trace_function(discrepancy, n_dim, None, "discrepancy", spec, extent, yarg=True)
    source = emit_source(graphs, tables)
    n_derived = max(1, len(graphs["derived"].outputs)) if derived is not None else None
    data_kwargs = {} if data is None else {"data": host, "n_terms": n_terms, "n_predict": n_predict, "pointwise": bool(pointwise)}
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

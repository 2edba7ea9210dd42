"""The symbolic value a callback is run on: `TV` records every torch operation done to it into a `Graph`, or refuses it with a
TraceError that names the operation, the user's line and what to write instead.  One registration (`_HANDLERS`) gives every
handler its torch names, operator dunders and aliases, and says which of them are also methods of TV.  Below: the data entries
D[name] and the noise object g of replicate as the tracer hands them to a callback."""
import inspect
import linecache
import math
import os
import sys
from functools import partialmethod

import numpy as np
import torch

from .graph import _UNINIT
from .noise import _draw_index

MAX_WIDTH = 64                  # columns of an intermediate: 64 doubles are a quarter of a lane's 512-VGPR budget
MAX_CONSTANTS = 64 * 64         # elements of captured arrays embedded in the source

_POINT_TO_DATA = ("straight-line code over that many values is the wrong tool: give the observations as "
                  "HipCallbacks(source, n_dim, data={...}, n_terms=...) and write log_likelihood_term by hand, or as "
                  "trace_callbacks(..., data={...}, n_terms=...) with a term function of (x, D)")
_OWNS_THE_SUM = "the library owns the sum over observations"
_NO_TERM_AXIS = ("this callback (prior_transform, derived, a log_likelihood without n_terms=) has no term axis: only the term "
                 "function (n_terms=) and predict (n_predict=) return one column per observation")
_RETURN_TERMS = "return the (n, n_terms) terms; reduce over the other axes (dim=1) only"
_OUTSIDE_THE_LIST = ("it is outside the supported operation list", "see the list in DESIGN.md section 11; anything else: a "
                     "hand-written HipCallbacks source")
_PACKAGE = os.path.dirname(os.path.abspath(__file__)) + os.sep


class TraceError(Exception):
    """A callback that cannot be traced, or a trace the probe found wrong.  `.source`: the emitted text, where there is one."""
    source = None


def _user_line(filename, lineno):
    """file:line: text, if the line is the user's: in no file of this package and not in torch; else None."""
    if os.path.abspath(filename).startswith(_PACKAGE) or (os.sep + "torch" + os.sep) in filename:
        return None
    return f"{filename}:{lineno}: {linecache.getline(filename, lineno).strip()}"


def _where():
    """The user's line of the innermost frame that has one."""
    f = sys._getframe(1)
    while f is not None:
        at = _user_line(f.f_code.co_filename, f.f_lineno)
        if at is not None:
            return at
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
        at, tb = None, e.__traceback__
        while tb is not None:
            at = _user_line(tb.tb_frame.f_code.co_filename, tb.tb_lineno) or at
            tb = tb.tb_next
        _refuse(*kinds[0]._WHY, at=at)


# ------------------------------------------------------------------------------------------------ the symbolic value
class _Batch:
    """x.shape[0]: usable as the leading extent of a reshape, and as nothing else."""

    _WHY = ("x.shape[0] (the number of particles n)", "the particle axis is symbolic; its extent may not enter the arithmetic, "
            "a loop or an allocation", "write the function per row: reductions over dim=1, no use of n")

    def _no(self, *a, **k):
        _refuse(*self._WHY)
    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __floordiv__ = __rfloordiv__ = _no
    __mod__ = __pow__ = __rpow__ = __neg__ = __index__ = __int__ = __float__ = __bool__ = __lt__ = __le__ = __gt__ = __ge__ = __eq__ = _no
    __hash__ = None

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
        return torch.bool if self._bool() else torch.float64

    @property
    def device(self):
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
        _refuse(f"x.{name}", *_OUTSIDE_THE_LIST)

    # ---- dtype and placement
    def _dtype_refused(self, what):
        _refuse(what, "traced callbacks are float64 throughout", "drop the conversion (float32 is out of scope)")

    float, half, bfloat16, int, long = ((lambda n: lambda self: self._dtype_refused(f"x.{n}()"))(n)
                                        for n in ("float", "half", "bfloat16", "int", "long"))

    def to(self, *args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.dtype) and a != torch.float64:
                self._dtype_refused(f"x.to({a})")
        return self

    type = to

    def double(self):
        return self

    cpu = cuda = contiguous = detach = __pos__ = double

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

    # ---- arithmetic: the operators and methods that are torch names too come from _HANDLERS below
    def _as_double(self):
        return self._new(_dbl(self.g, self, self.ids)) if self._bool() else self

    def _inplace(self, *a, **k):
        _refuse("in-place arithmetic (+=, -=, *=, /=, add_, mul_, ...)", "it would change " +
                ("the callback's input" if self.is_input else "a value other expressions may share"),
                "y = x + 1 (a new value); column assignment y[:, j] = ... on an empty_like / clone is supported")
    __iadd__ = __isub__ = __imul__ = __itruediv__ = __ipow__ = __imatmul__ = _inplace
    add_ = sub_ = mul_ = div_ = pow_ = clamp_ = exp_ = log_ = neg_ = abs_ = sqrt_ = fill_ = zero_ = copy_ = _inplace

    def __rmatmul__(self, other):
        _refuse("A @ x", "the particle axis of x must stay the leading axis of the result", "x @ A.T")

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", str(func))
        h = _TORCH.get(name)
        if h is None:
            _refuse(f"torch.{name}", *_OUTSIDE_THE_LIST)
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
        for e in v if isinstance(v, (list, tuple)) else (v,):
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
    _refuse("torch.cumsum", *_OUTSIDE_THE_LIST)


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
    if isinstance(A, TV):
        _refuse("matmul", "both operands are traced", "the second operand must be a captured constant matrix; an inner product of two "
                "traced rows is (a * b).sum(dim=1)")
    a = _lift(g, A, (0, 0))
    if a.ndim != 2:
        _refuse("matmul", f"the constant has shape {a.shape}", "a 2-D float64 constant")
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
        if dtype not in (None, torch.float64):
            a._dtype_refused(f"*_like(dtype={dtype})")
        return a._new(np.full(a.ids.shape, _UNINIT if fill is None else a.g.const(fill), dtype=np.int64))
    return make


def _sigmoid(a):
    # torch's device kernel: 1 / (1 + exp(-x))
    return _binary("div", 1.0, _binary("add", 1.0, _unary("exp", _unary("neg", a))))


def _rdiv(a, b):
    """number / x through the operator: torch's Tensor.__rtruediv__ is x.reciprocal() * number, two roundings, on the host and on the
    device (torch.div(c, x) with a 0-d tensor c, and tensor / x, are true divisions)."""
    return _binary("mul", _pow(a, -1.0), b) if isinstance(a, TV) and _is_number(b) and not (_is_tensor(b) or isinstance(b, np.ndarray)) \
        else _binary("div", b, a)


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
        _refuse(f"torch.special.{name}", "it is outside the supported operation list: of the normal distribution's functions the "
                "tracer has erf, erfc, torch.special.ndtri and torch.erfinv", instead)
    return handler


def _op(f, op):
    return lambda a, *b, **k: f(op, a, *b, **k)


# Every handler once: (handler, its names that are torch functions AND attributes of TV -- x.name(...), the operators --, its names
# that are torch functions only: aliases, what TV defines itself, the reflected operators whose operands TV swaps above).
_HANDLERS = (
    (_op(_unary, "neg"), "neg negative", ""),
    (_op(_unary, "abs"), "abs absolute", ""),
    *((_op(_unary, op), op, "") for op in ("sqrt", "rsqrt", "exp", "expm1", "log", "log1p", "sin", "cos", "tan", "tanh", "erf", "erfc",
                                           "lgamma")),
    (_op(_unary, "atan"), "atan arctan", ""),
    (_quantile("ndtri"), "ndtri", "special_ndtri"),
    (_quantile("erfinv"), "erfinv", "special_erfinv"),
    (_not_traced("ndtr", "0.5 * torch.erfc(-x * 0.7071067811865476)"), "ndtr", "special_ndtr"),
    (_not_traced("log_ndtr", "torch.log(0.5 * torch.erfc(-x * 0.7071067811865476)) (it loses the far lower tail: keep x above -37)"),
     "log_ndtr", "special_log_ndtr"),
    (_not_traced("erfcinv", "-torch.special.ndtri(0.5 * y) * 0.7071067811865476"), "erfcinv", "special_erfcinv"),
    (lambda a: _pow(a, 2.0), "square", ""),
    (lambda a: _pow(a, -1.0), "reciprocal", ""),
    (_pow, "pow __pow__", ""),
    (lambda a, b: _pow(b, a), "__rpow__", ""),
    (_sigmoid, "sigmoid", ""),
    (_op(_binary, "add"), "add __add__", "__radd__"),
    (_op(_binary, "mul"), "mul multiply __mul__", "__rmul__"),
    (_op(_binary, "sub"), "sub subtract __sub__", ""),
    (_op(_binary, "div"), "div divide true_divide __truediv__", ""),
    (lambda a, b, **k: _binary("sub", b, a, **k), "__rsub__", "rsub"),
    (_rdiv, "__rtruediv__", "__rdiv__"),
    (lambda a, b: _binary("min", a, b), "minimum", ""),
    (lambda a, b: _binary("max", a, b), "maximum", ""),
    (_clamp, "clamp clip", ""),
    (_where3, "where", ""),
    *((_op(_compare, op), f"{op} __{op}__", alias) for op, alias in (("gt", "greater"), ("lt", "less"), ("ge", "greater_equal"),
                                                                     ("le", "less_equal"), ("eq", ""), ("ne", "not_equal"))),
    (_op(_logical, "and"), "logical_and __and__", "bitwise_and"),
    (_op(_logical, "or"), "logical_or __or__", "bitwise_or"),
    (_logical_not, "logical_not __invert__", "bitwise_not"),
    *((_op(_reduce, kind), kind, "") for kind in ("sum", "mean", "prod", "amax", "amin", "logsumexp")),
    (_cumsum, "cumsum", ""),
    (_matmul, "matmul __matmul__", ""),
    (lambda a, b: _matmul(b, a), "", "__rmatmul__"),
    (_linear, "", "linear"),
    (_stack, "", "stack"),
    (_cat, "", "cat concat concatenate"),
    *((_like(fill), "", name) for fill, name in ((None, "empty_like"), (0.0, "zeros_like"), (1.0, "ones_like"))),
    (lambda a, **k: a.clone(), "", "clone"),
    (lambda a, dim: a.unsqueeze(dim), "", "unsqueeze"),
    (lambda a, dim=None: a.squeeze(dim), "", "squeeze"),
    (lambda a, *s: a.reshape(*s), "", "reshape"),
)
_TORCH = {}
for _handler, _methods, _functions in _HANDLERS:
    for _n in _methods.split():
        setattr(TV, _n, _handler)
    _TORCH.update((_n, _handler) for _n in (_methods + " " + _functions).split())
# the operators that are no torch names: the unary ones, and the reflected ones, whose operands swap
TV.__neg__, TV.__abs__ = _op(_unary, "neg"), _op(_unary, "abs")
TV.__radd__, TV.__rmul__ = (lambda self, o: _binary("add", o, self)), (lambda self, o: _binary("mul", o, self))
TV.__rand__, TV.__ror__ = (lambda self, o: _logical("and", o, self)), (lambda self, o: _logical("or", o, self))


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
        return torch.float64

    def __len__(self):
        if self._per_term():
            self.g.term_extent._no()
        return self._shape[0]

    def double(self):
        return self if self._f64 else _Entry(self.g, self._pos, self._name, self._shape, True)

    def to(self, *args, **kwargs):
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
    try:
        ps = list(inspect.signature(fn).parameters.values())
    except (TypeError, ValueError):
        return False
    return sum(p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) for p in ps) >= 2


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

    normal, uniform = partialmethod(_draw, "normal"), partialmethod(_draw, "uniform")

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        _refuse(f"g.{name}", "the noise object has g.normal(k) and g.uniform(k) and nothing else", "compose the law from them: a "
                "Bernoulli is torch.where(g.uniform(k) < p, 1.0, 0.0)")

"""The probe: the eager callables held against the compiled plugin (or, without a device, against the replay of its graphs) on a
fixed batch of rows."""
import math

import numpy as np
import torch

from .._philox_host import philox4x32
from ..tools import SQRTEPS
from .graph import replay
from .noise import Noise
from .value import TraceError, _wants_data

PROBE_ROWS, PROBE_SEED, _PROBE_TAG = 4096, 20240611, 0x7472


def probe_batch(n_dim, rows=PROBE_ROWS, seed=PROBE_SEED):
    """(rows, n_dim) uniforms of the package's Philox host twin: item = row, draw = column."""
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


class _Probe:
    """What the check of every callback works with: the plugin `cb`, its graphs and host data, the eager callables `fns`, the
    report, whether a device is present, the unit-cube rows u and -- once prior_transform has been checked and returned rows of
    their shape -- the parameters x the other callbacks are run on."""

    def __init__(self, cb, fns):
        from ..hipcallbacks import SUM_LAYOUT
        self.cb, self.fns, self.graphs, self.sum_layout = cb, fns, cb.trace_graphs, SUM_LAYOUT
        self.data = dict(cb._host) if cb.tables is not None else None
        g = self.graphs
        term = "log_likelihood_term" in g
        widest = max(cb.n_terms if term else 1, cb.n_predict if "predict" in g else 1, cb.n_replicate if "replicate" in g else 1)
        self.rows = PROBE_ROWS if widest == 1 and not term else max(1, min(PROBE_ROWS, 2 ** 22 // widest))
        self.u, self.x = probe_batch(cb.n_dim, self.rows), None
        self.on_device = torch.cuda.is_available()
        self.report = {"rows": self.rows, "seed": PROBE_SEED, "against": "compiled plugin on the device" if self.on_device else
                       "replay on the CPU (no device present: the compiled code was NOT run)", "eager_on": {}}
        self._tensors = {}

    def D_on(self, dev):
        if dev not in self._tensors:
            self._tensors[dev] = {k: torch.from_numpy(v).to(dev) for k, v in self.data.items()}
        return self._tensors[dev]

    def run_eager(self, name, run):
        """run(dev), the eager side of the probe where the compiled code runs; run("cpu") without a device or where the function's
        constants were captured on the host, and that alone.  report["eager_on"][name] says which."""
        if self.on_device:
            try:
                self.report["eager_on"][name] = "device"
                return run(self.cb.device or "cuda")
            except RuntimeError as e:
                if "Expected all tensors to be on the same device" not in str(e):
                    raise
        self.report["eager_on"][name] = "cpu"
        return run("cpu")

    def eager(self, name, fn, a, with_data=False):
        def run(dev):
            y = fn(torch.from_numpy(a).to(dev), *((self.D_on(dev),) if with_data else ()))
            return (torch.as_tensor(y) if dev == "cpu" else y).detach().cpu().numpy()
        return self.run_eager(name, run)

    def traced(self, name, a):
        return np.asarray(getattr(self.cb, name)(a)) if self.on_device else replay(self.graphs[name], a, self.data)

    def chunks(self, n_cols):                        # slices of the rows: nothing larger than 2^22 doubles is formed
        step = max(1, 2 ** 22 // max(1, n_cols))
        return [slice(i, min(self.rows, i + step)) for i in range(0, self.rows, step)]


# ---- the (name, eager, traced) pairs of each callback: (the probe, the eager callable)
def _pairs_prior_transform(p, fn):
    x = p.eager("prior_transform", fn, p.u, p.data is not None and _wants_data(fn))
    p.x = x if x.shape == p.u.shape else None
    return [("prior_transform", x, p.traced("prior_transform", p.u))]


def _pairs_log_likelihood(p, fn):
    """The likelihood, or the layered sum of the term function's columns: either is held against cb.log_likelihood."""
    if "log_likelihood_term" not in p.graphs:
        return [("log_likelihood", p.eager("log_likelihood", fn, p.x, p.data is not None), p.traced("log_likelihood", p.x))]
    cb, x, chunks = p.cb, p.x, p.chunks(p.cb.n_terms)

    def summed(terms, n):
        terms = np.asarray(terms)
        return layered_sum(terms, *p.sum_layout) if terms.shape == (n, cb.n_terms) else np.full(n, np.nan)    # a wrong shape fails below
    e = np.concatenate([summed(p.eager("log_likelihood", fn, x[c], True), len(x[c])) for c in chunks])
    t = p.traced("log_likelihood", x) if p.on_device else np.concatenate(
        [layered_sum(replay(p.graphs["log_likelihood_term"], x[c], p.data), *p.sum_layout) for c in chunks])
    return [("log_likelihood", e, t)]


def _pairs_predict(p, fn):
    cb, chunks = p.cb, p.chunks(p.cb.n_predict)
    if p.on_device:                                  # at most 8 rows, each alone with weight 1: mean = predict exactly
        xs = p.x[:8]
        t = np.stack([cb.predictive(xs[i:i + 1], np.ones(1), quantiles=(0.5,))["mean"] for i in range(len(xs))])
    else:
        xs = p.x
        t = np.concatenate([replay(p.graphs["predict"], xs[c], p.data) for c in chunks])
    e = np.concatenate([p.eager("predict", fn, xs[c], True) for c in chunks if len(xs[c])])
    return [("predict", e, t)]


def _pairs_derived(p, fn):
    e = p.eager("derived", fn, p.x, p.data is not None and _wants_data(fn))
    return [("derived", e, p.traced("derived", p.x).reshape(e.shape) if e.size == p.x.shape[0] * p.cb.n_derived else None)]


def _pairs_replicate(p, replicate):
    """replicate and, where there is one, discrepancy, which is run on what replicate returned."""
    cb, graphs, data, x, R = p.cb, p.graphs, p.data, p.x, p.cb.n_replicate
    discrepancy = p.fns.get("discrepancy")
    disc = discrepancy is not None and "discrepancy" in graphs
    obs = data[cb.observed] if disc else None

    def eager_on(dev, xs, items):
        """(eager y_rep (n, R)[, eager T (n, 2)]) on `dev`."""
        D, g, xt = p.D_on(dev), Noise(PROBE_SEED, items, R, device=dev), torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
        y = torch.as_tensor(replicate(xt, D, g))
        out = [y.detach().cpu().numpy().astype(np.float64)]
        if disc:
            yo = D[cb.observed][None, :].expand(len(xs), R)
            ts = [torch.as_tensor(discrepancy(xt, yy, D)).detach().cpu().numpy() for yy in (yo, y.to(torch.float64))]
            out.append(np.stack([layered_sum(t, *p.sum_layout) if t.shape == (len(xs), R) else np.full(len(xs), np.nan) for t in ts], axis=1))
        return out

    ey, et, ty, tt = [], [], [], []
    if p.on_device:                                  # at most 8 rows, each alone with weight 1: item 0, mean = replicate exactly
        for i in range(min(8, len(x))):
            got = cb.replicated(x[i:i + 1], np.ones(1), quantiles=(0.5,), seed=PROBE_SEED)
            e = p.run_eager("replicate", lambda dev: eager_on(dev, x[i:i + 1], np.zeros(1, dtype=np.int64)))
            ey.append(e[0])
            ty.append(np.asarray(got["mean"], dtype=np.float64)[None, :])
            if disc:
                et.append(e[1])
                tt.append(np.array([[got["t_obs_mean"], got["t_rep_mean"]]], dtype=np.float64))
    else:
        for c in p.chunks(R):
            items = np.arange(c.start, c.stop, dtype=np.int64)
            e = p.run_eager("replicate", lambda dev: eager_on(dev, x[c], items))
            y = replay(graphs["replicate"], x[c], data, noise=Noise(PROBE_SEED, items, R))
            ey.append(e[0])
            ty.append(y)
            if disc:
                et.append(e[1])
                tt.append(np.stack([layered_sum(replay(graphs["discrepancy"], x[c], data, y=yy), *p.sum_layout) for yy in (obs, y)], axis=1))
    ok = all(a.shape == t.shape for a, t in zip(ey, ty))                                         # a wrong shape fails the comparison
    pairs = [("replicate", np.concatenate(ey) if ok else np.full(1, np.nan), np.concatenate(ty))]
    if disc:
        pairs.append(("discrepancy", np.concatenate(et), np.concatenate(tt)))
    return pairs


# in the order they are checked and reported; everything behind prior_transform runs on its rows
_PAIRS = {"prior_transform": _pairs_prior_transform, "log_likelihood_term": _pairs_log_likelihood,
          "log_likelihood": _pairs_log_likelihood, "predict": _pairs_predict, "replicate": _pairs_replicate, "derived": _pairs_derived}


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
    like = "log_likelihood_term" if "log_likelihood_term" in cb.trace_graphs else "log_likelihood"
    p = _Probe(cb, {"prior_transform": prior_transform, like: log_likelihood, "predict": predict, "replicate": replicate,
                    "discrepancy": discrepancy, "derived": derived})
    pairs, report = [], p.report
    for name, pairs_of in _PAIRS.items():
        if p.fns.get(name) is not None and name in p.graphs:
            pairs += pairs_of(p, p.fns[name])
            if p.x is None:                          # prior_transform returned rows of another shape: nothing to run the others on
                break
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
